"""The one SAC-family update of the test-side oracles in plain torch (not a test), and the pieces every autograd oracle
shares: the MLP with optional layer normalisation, the cast of a learner's parameters, one Adam step on a loss, the
temperature's step.  DESIGN.md section 27 has the table of the steps and hooks, and the rule for the next mode's oracle.

``SoftOracle`` computes in the dtype of its inputs (float64 in the parity tests, float32 in the feasibility checks) with
autograd for every gradient; the tanh-Gaussian head and the Adam / Polyak arithmetic are oracle/oprl_oracle.py's.  One update:

    1. y = r + (1 - d) gamma (reduce_i Qtarget_i(s', a') - alpha log pi(a'|s')) over the target critics ``draw_subset(u)``
    2. one Adam step over [the critics' parameters ..., ln] on ``critic_loss(qs, y, w)``
    3. Polyak on all N targets (and on the LN parameters' target copy) if ``polyak_due``
    4. every ``utd_ratio`` updates: the actor step on ``actor_loss`` through the updated critics, then the temperature

REDQ (tests/redq_oracle.py), LayerNorm and DroQ critics (tests/ln_oracle.py, tests/droq_oracle.py) and prioritized training
(tests/per_train_oracle.py) are this class with a constructor mapping and the hooks their knobs need."""
from __future__ import annotations

from typing import Callable

import numpy as np
import torch as t

from oracle import oprl_oracle as orc

EPS = float(np.float32(1e-5))       # torch's default eps as the float the device holds


def cast(ps: list[t.Tensor], dtype) -> list[t.Tensor]:
    """A learner's (or a fixture's) parameters as the oracle's own copy in ``dtype``."""
    return [x.detach().to(dtype).clone() for x in ps]


def layer_norm(z: t.Tensor, gamma: t.Tensor, beta: t.Tensor, eps: float = EPS):
    """(n, zh, rstd) of section 24's definition: biased variance, two passes."""
    mu = z.mean(1, keepdim=True)
    d = z - mu
    var = (d * d).mean(1, keepdim=True)
    rstd = 1.0 / t.sqrt(var + eps)
    zh = d * rstd
    return gamma * zh + beta, zh, rstd


def ln_mlp(p: list[t.Tensor], ln: t.Tensor | None, x: t.Tensor, eps: float = EPS, keep: dict | None = None) -> t.Tensor:
    """``p`` = [W0, b0, W1, b1, ...] with LN (``ln`` [hidden layers, 2, W]; None: none) between every hidden Linear and
    its ReLU.  ``keep``: receives per hidden layer the lists z, zh, n, x (the tensors of the graph)."""
    n_layers = len(p) // 2
    for l in range(n_layers):
        z = x @ p[2 * l].t() + p[2 * l + 1]
        if l == n_layers - 1:
            return z
        zh = None
        n = z
        if ln is not None:
            n, zh, _ = layer_norm(z, ln[l, 0], ln[l, 1], eps)
        x = t.relu(n)
        if keep is not None:
            for k, v in (("z", z), ("zh", zh), ("n", n), ("x", x)):
                keep.setdefault(k, []).append(v)
    raise AssertionError("unreachable")


def mlp(p: list[t.Tensor], x: t.Tensor) -> t.Tensor:
    """The plain MLP (ReLU hidden, identity output), differentiable in ``p`` and ``x``."""
    return ln_mlp(p, None, x)


def grad_step(opt: orc.Adam, params: list[t.Tensor], loss_of) -> t.Tensor:
    """One Adam step on loss_of(leaf copies of params); returns the loss."""
    leaves = [x.clone().requires_grad_(True) for x in params]
    loss = loss_of(leaves)
    opt.step(params, list(t.autograd.grad(loss, leaves)))
    return loss.detach()


class SoftOracle:
    """SAC (``algo="sac"``: every critic a target critic, the minimum over the critics in the actor loss, an actor step
    every update) or REDQ (``algo="redq"``: ``subset(u)`` draws the target critics of update u, the mean over the
    ensemble in the actor loss, an actor step every ``utd_ratio`` updates).  ``ln`` / ``ln_target`` [N, hidden layers, 2, W]:
    the critics' LN parameters (None: plain critics).  With them the critic optimiser is ONE Adam over [the critics'
    parameters ..., ln]: gamma / beta step with lr_critic at the critics' step count, and their target copy takes the
    targets' Polyak step.  ``update(..., w)``: per-row weights [B, 1] for ``critic_loss`` / ``actor_loss``; with them
    ``last`` holds |TD| too."""

    def __init__(self, algo: str, S: int, A: int, actor: list[t.Tensor], critics: list[list[t.Tensor]],
                 targets: list[list[t.Tensor]], ln: t.Tensor | None = None, ln_target: t.Tensor | None = None,
                 subset: Callable[[int], list[int]] | None = None, n_min: int = 2, utd_ratio: int = 1,
                 gamma=0.99, tau=5e-3, lr_actor=3e-4, lr_critic=3e-4, lr_alpha=3e-4, alpha_init=1.0, tune_alpha=True,
                 dtype=t.float64, eps: float = EPS):
        assert algo in ("sac", "redq")
        self.algo, self.S, self.A, self.N = algo, S, A, len(critics)
        self.M, self.G = (self.N, 1) if algo == "sac" else (n_min, utd_ratio)
        self.gamma, self.tau, self.eps = gamma, tau, eps
        self.actor = cast(actor, dtype)
        self.critics = [cast(c, dtype) for c in critics]
        self.targets = [cast(c, dtype) for c in targets]
        self.ln = self.ln_target = None
        if ln is not None:
            self.ln, self.ln_target = ln.detach().to(dtype).clone(), ln_target.detach().to(dtype).clone()
        self.subset = subset if subset is not None else (lambda u: list(range(self.N)))
        self.opt_actor, self.opt_critic, self.opt_alpha = orc.Adam(lr_actor), orc.Adam(lr_critic), orc.Adam(lr_alpha)
        self.tune_alpha, self.alpha_init = tune_alpha, alpha_init
        self.log_alpha = t.tensor(float(t.tensor(alpha_init, dtype=t.float64).log()), dtype=t.float64)
        self.target_entropy = -float(A)
        self.update_step = 0
        self.last: dict = {}

    @property
    def alpha(self) -> float:
        return float(self.log_alpha.exp()) if self.tune_alpha else float(self.alpha_init)

    def flat_critics(self) -> list[t.Tensor]:
        return [x for c in self.critics for x in c]

    # ---- the hooks (section 27's table)
    def q(self, params: list[t.Tensor], ln_i: t.Tensor | None, s: t.Tensor, a: t.Tensor) -> t.Tensor:
        """One critic on (s, a).  ``update`` evaluates in a fixed order: the M target critics of the subset, the N
        critics of the critic step, then (on an actor step) the N critics on (s, pi)."""
        return ln_mlp(params, ln_i, t.cat([s, a], 1), self.eps)

    def draw_subset(self, u: int) -> list[int]:
        return self.subset(u)

    def reduce_targets(self, qn: t.Tensor) -> t.Tensor:
        return qn.min(1, keepdim=True).values

    def critic_loss(self, qs: list[t.Tensor], y: t.Tensor, w: t.Tensor | None) -> t.Tensor:
        return sum(((q - y) ** 2).mean() for q in qs)

    def actor_loss(self, alpha: float, logp: t.Tensor, q_row: t.Tensor, w: t.Tensor | None) -> t.Tensor:
        """From log pi [B, 1] and the critics' reduced value of (s, pi) per row, q_row [B]."""
        return (alpha * logp).mean() - q_row.mean()

    def polyak_due(self, actor_step: bool) -> bool:
        return True

    def ln_slot(self, g_ln: t.Tensor) -> tuple[t.Tensor, t.Tensor]:
        """(parameter, gradient) of the LN slot, the last of the critic optimiser."""
        return self.ln, g_ln

    def polyak_ln(self) -> None:
        orc.polyak([self.ln_target], [self.ln], self.tau)

    # ---- the steps
    def temperature_step(self, logp: t.Tensor) -> None:
        g_alpha = -(self.target_entropy + logp.detach().mean().to(t.float64))
        la = [self.log_alpha.reshape(1).clone()]
        self.opt_alpha.step(la, [g_alpha.reshape(1)])
        self.log_alpha = la[0].reshape(())

    def update(self, s, a, r, d, s2, e1, e2, w=None) -> None:
        u = self.update_step
        alpha = self.alpha                       # (the value before this update's temperature step)
        has_ln = self.ln is not None
        idx = self.draw_subset(u)
        with t.no_grad():
            a2, logp2, _ = orc.gaussian_forward(self.actor, s2, e1, self.A)
            qn = t.cat([self.q(self.targets[i], self.ln_target[i] if has_ln else None, s2, a2) for i in idx], 1)
            y = r + (1.0 - d) * self.gamma * (self.reduce_targets(qn) - alpha * logp2)
        # one Adam step over the critic arena and the LN parameters
        params = [x.clone().requires_grad_(True) for x in self.flat_critics()]
        ln = self.ln.clone().requires_grad_(True) if has_ln else None
        per = len(self.critics[0])
        qs = [self.q(params[i * per:(i + 1) * per], ln[i] if has_ln else None, s, a) for i in range(self.N)]
        loss = self.critic_loss(qs, y, w)
        arena = self.flat_critics()
        grads = list(t.autograd.grad(loss, params + [ln] if has_ln else params, allow_unused=True))
        self.last = dict(q=qs[0].detach(), y=y, critic_loss=loss.detach(), subset=idx)
        if has_ln:
            g_ln = grads.pop()
            if g_ln is None:                     # (the loss does not depend on gamma / beta)
                g_ln = t.zeros_like(self.ln)
            p_ln, step_ln = self.ln_slot(g_ln)
            arena, grads = arena + [p_ln], grads + [step_ln]
            self.last["g_ln"] = g_ln.detach()
        if w is not None:                        # (|TD| of the critics as they stood before their step)
            self.last["td_abs"] = sum((q.detach() - y).abs() for q in qs).reshape(-1) / self.N
        self.opt_critic.step(arena, grads)
        actor_step = (u + 1) % self.G == 0
        if self.polyak_due(actor_step):
            for i in range(self.N):
                orc.polyak(self.targets[i], self.critics[i], self.tau)
            if has_ln:
                self.polyak_ln()
        # the actor step on the updated critics (through LN; gamma / beta take no step here), then the temperature
        if actor_step:
            def loss_of(ap):
                pi, logp, _ = orc.gaussian_forward(ap, s, e2, self.A)
                qpi = t.cat([self.q(self.critics[i], self.ln[i] if has_ln else None, s, pi) for i in range(self.N)], 1)
                self.last.update(logp=logp.detach(), qpi=qpi.detach())
                return self.actor_loss(alpha, logp, qpi.min(1).values if self.algo == "sac" else qpi.mean(1), w)
            self.last["actor_loss"] = grad_step(self.opt_actor, self.actor, loss_of)
            if self.tune_alpha:
                self.temperature_step(self.last["logp"])
        self.update_step += 1
