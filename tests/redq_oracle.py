"""A REDQ update in plain torch, written from the spec (oprl_amd/algos/redq.py, DESIGN.md "REDQ"), for the parity
tests of tests/test_gpu_redq.py.  It computes in the dtype of its inputs (float64 in the tests) with autograd for
every gradient, takes its initial parameters from the learner, and borrows only the tanh-Gaussian head and the Adam /
Polyak arithmetic of oracle/oprl_oracle.py.

The knobs after ``subset`` exist so a test can show that the comparison discriminates: ``subset_shift`` draws the
subset of update u + shift, ``use_mean`` replaces the minimum by the mean, ``polyak_on_actor_steps`` moves the targets
only on actor steps."""
from __future__ import annotations

from typing import Callable

import torch as t

from oracle import oprl_oracle as orc


def mlp(p: list[t.Tensor], x: t.Tensor) -> t.Tensor:
    n = len(p) // 2
    for l in range(n):
        x = x @ p[2 * l].t() + p[2 * l + 1]
        if l < n - 1:
            x = t.relu(x)
    return x


class REDQOracle:
    def __init__(self, S: int, A: int, actor: list[t.Tensor], critics: list[list[t.Tensor]],
                 targets: list[list[t.Tensor]], subset: Callable[[int], list[int]], n_min: int, utd_ratio: int,
                 gamma=0.99, tau=5e-3, lr_actor=3e-4, lr_critic=3e-4, lr_alpha=3e-4, alpha_init=1.0, tune_alpha=True,
                 dtype=t.float64, subset_shift: int = 0, use_mean: bool = False, polyak_on_actor_steps: bool = False):
        self.S, self.A, self.N, self.M, self.G = S, A, len(critics), n_min, utd_ratio
        self.gamma, self.tau = gamma, tau
        cp = lambda ps: [x.detach().to(dtype).clone() for x in ps]   # noqa: E731
        self.actor = cp(actor)
        self.critics = [cp(c) for c in critics]
        self.targets = [cp(c) for c in targets]
        self.subset, self.subset_shift = subset, subset_shift
        self.use_mean, self.polyak_on_actor_steps = use_mean, polyak_on_actor_steps
        self.opt_actor, self.opt_critic = orc.Adam(lr_actor), orc.Adam(lr_critic)
        self.tune_alpha = tune_alpha
        self.log_alpha = t.tensor(float(t.tensor(alpha_init, dtype=t.float64).log()), dtype=t.float64)
        self.alpha_init = alpha_init
        self.opt_alpha = orc.Adam(lr_alpha)
        self.target_entropy = -float(A)
        self.update_step = 0
        self.last: dict = {}

    @property
    def alpha(self) -> float:
        return float(self.log_alpha.exp()) if self.tune_alpha else float(self.alpha_init)

    def flat_critics(self) -> list[t.Tensor]:
        return [x for c in self.critics for x in c]

    def update(self, s, a, r, d, s2, e1, e2) -> None:
        u = self.update_step
        B = s.shape[0]
        alpha = self.alpha                       # (the value before this update's temperature step)
        # 1.-4. the TD target on the subset's target critics
        idx = self.subset(u + self.subset_shift)
        with t.no_grad():
            a2, logp2, _ = orc.gaussian_forward(self.actor, s2, e1, self.A)
            qn = t.cat([mlp(self.targets[i], t.cat([s2, a2], 1)) for i in idx], 1)
            q_next = qn.mean(1, keepdim=True) if self.use_mean else qn.min(1, keepdim=True).values
            y = r + (1.0 - d) * self.gamma * (q_next - alpha * logp2)
        # 5. one Adam step over the critic arena on sum_i mean_b (Q_i - y)^2
        params = [x.clone().requires_grad_(True) for x in self.flat_critics()]
        per = len(self.critics[0])
        qs = [mlp(params[i * per:(i + 1) * per], t.cat([s, a], 1)) for i in range(self.N)]
        loss = sum(((q - y) ** 2).mean() for q in qs)
        grads = list(t.autograd.grad(loss, params))
        flat = self.flat_critics()
        self.opt_critic.step(flat, grads)
        # 6. Polyak on all N targets
        actor_step = (u + 1) % self.G == 0
        if actor_step or not self.polyak_on_actor_steps:
            for i in range(self.N):
                orc.polyak(self.targets[i], self.critics[i], self.tau)
        self.last = dict(q=qs[0].detach(), y=y, critic_loss=loss.detach(), subset=idx)
        # 7. the actor step on the updated critics, then the temperature
        if actor_step:
            ap = [x.clone().requires_grad_(True) for x in self.actor]
            out = mlp(ap, s)
            mu, log_std = out[:, :self.A], out[:, self.A:].clamp(orc.LOG_STD_MIN, orc.LOG_STD_MAX)
            std = log_std.exp()
            uu = mu + std * e2
            pi = t.tanh(uu)
            normal_lp = -((uu - mu) ** 2) / (2 * std * std) - log_std - 0.5 * t.log(t.tensor(2 * t.pi, dtype=s.dtype))
            log_det = 2 * t.log(t.tensor(2.0, dtype=s.dtype)) + t.nn.functional.logsigmoid(2 * uu) + t.nn.functional.logsigmoid(-2 * uu)
            logp = (normal_lp - log_det).sum(1, keepdim=True)
            qpi = t.cat([mlp(c, t.cat([s, pi], 1)) for c in self.critics], 1)
            actor_loss = (alpha * logp).mean() - qpi.mean(1).mean()
            g_a = list(t.autograd.grad(actor_loss, ap))
            self.opt_actor.step(self.actor, g_a)
            self.last.update(actor_loss=actor_loss.detach(), logp=logp.detach())
            if self.tune_alpha:
                g_alpha = -(self.target_entropy + logp.detach().mean().to(t.float64))
                la = [self.log_alpha.reshape(1).clone()]
                self.opt_alpha.step(la, [g_alpha.reshape(1)])
                self.log_alpha = la[0].reshape(())
        self.update_step += 1
