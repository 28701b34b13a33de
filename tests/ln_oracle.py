"""Critics with layer normalisation in plain torch, written from the definitions of DESIGN.md section 24, and SAC / REDQ
updates around them, for tests/test_ln_host.py, tests/test_gpu_ln_slice.py and tests/test_gpu_ln.py (not a test).

A critic MLP(S + A -> 256 -> 256 -> 1) with LN computes per hidden layer l and row, over the columns c,
    z = W x + b;  mu = mean_c z;  var = mean_c (z - mu)^2;  zh = (z - mu) / sqrt(var + eps);  x_l = relu(gamma zh + beta)
and a plain output layer.  Everything computes in the dtype of its inputs (float64 in the parity tests, float32 in the
feasibility check) and autograd supplies every gradient; the tanh-Gaussian head and the Adam / Polyak arithmetic are
oracle/oprl_oracle.py's.  The LN parameters of critic i are ``ln[i]`` [2 hidden layers, 2, W]: [l, 0] gamma, [l, 1] beta.

Three knobs exist only to show that a comparison discriminates: ``no_ln`` (plain critics), ``freeze_ln`` (gamma / beta
never step), ``no_ln_polyak`` (their target copy never moves)."""
from __future__ import annotations

from typing import Callable

import numpy as np
import torch as t

from oracle import fixtures as fx
from oracle import oprl_oracle as orc

EPS = float(np.float32(1e-5))       # torch's default eps as the float the device holds

# ---- the parity scenarios of tests/test_gpu_ln.py (and of the float32 feasibility check of tests/test_ln_host.py) -----------
S, A, N, G = 24, 6, 10, 3           # walker dims, REDQ's default ensemble, an actor step every third update
# (algo, B, n_min, seed of the batches).  A ReLU unit whose normalised pre-activation lies within float32 rounding of
# zero for one row is masked in one arithmetic and not in the other, and Adam's m / sqrt(v) carries that row's term into a
# moment at 10 .. 400 gates; with 10 critics x 512 units x B rows x 4 updates some seeds hold such a unit.  Rule: the
# first seed of 100, 200, 300, 400, 600 at which the float32 oracle stays within a QUARTER of the half gates of the
# float64 one (measured on the CPU: 0.07, 0.20, 0.06, 0.14, 0.12 of them; seed 100 gives 3.8, 20, 0.30, 0.36 at the last four:
# the second and third scenario miss the half gates there).
SCENARIOS = [("redq", 256, 2, 100), ("redq", 100, 2, 600), ("redq", 256, 3, 400), ("sac", 256, 2, 600), ("sac", 100, 2, 200)]


def scenario_params(algo: str):
    """(actor, critics, ln) a scenario starts from: fixture nets and non-trivial gamma / beta, float32."""
    n = N if algo == "redq" else 2
    actor = fx.make_net(31, [S, 256, 256, 2 * A])
    critics = [fx.make_net(40 + i, [S + A, 256, 256, 1]) for i in range(n)]
    gen = t.Generator().manual_seed(77)
    ln = t.zeros(n, 2, 2, 256)
    ln[:, :, 0] = 1.0 + 0.1 * t.randn(n, 2, 256, generator=gen)
    ln[:, :, 1] = 0.1 * t.randn(n, 2, 256, generator=gen)
    return actor, critics, ln


def scenario_batches(seed: int, B: int, n: int):
    out = []
    for k in range(n):
        s, a, r, d, s2 = fx.make_batch(seed + k, B, S, A)
        g = t.Generator().manual_seed(seed + 400 + k)
        out.append((s, a, r, d, s2, t.randn(B, A, generator=g), t.randn(B, A, generator=g)))
    return out


def scenario_oracle(algo: str, subset, n_min: int = 2, dtype=t.float64, tau: float = 5e-3, **kw) -> "LNOracle":
    """The oracle of a scenario: REDQ (N = 10, G = 3, the learner's defaults) or SAC with a tuned temperature."""
    actor, critics, ln = scenario_params(algo)
    if algo == "redq":
        return LNOracle("redq", S, A, actor, critics, critics, ln, ln, subset=subset, n_min=n_min, utd_ratio=G, tau=tau,
                        dtype=dtype, **kw)
    return LNOracle("sac", S, A, actor, critics, critics, ln, ln, lr_alpha=1e-3, alpha_init=0.2, tau=tau, dtype=dtype, **kw)


def digest(o: "LNOracle") -> dict:
    """The oracle's state under the key names tests/scenarios.py gates: the LN keys count as parameters / moments."""
    out = {}
    for i, (c, tg) in enumerate(zip(o.critics, o.targets)):
        for l, x in enumerate(c):
            out[f"u.critic.{i}.{l}"] = x
        for l, x in enumerate(tg):
            out[f"u.critic_target.{i}.{l}"] = x
        out[f"u.critic.{i}.ln"], out[f"u.critic_target.{i}.ln"] = o.ln[i], o.ln_target[i]
    for l, x in enumerate(o.actor):
        out[f"u.actor.{l}"] = x
    for which, opt in (("critic", o.opt_critic), ("actor", o.opt_actor)):
        for l, (m, v) in enumerate(zip(opt.m, opt.v)):
            name = "ln" if which == "critic" and l == len(opt.m) - 1 else str(l)
            out[f"u.m_{which}.{name}"], out[f"u.v_{which}.{name}"] = m, v
    out["u.log_alpha"] = o.log_alpha.reshape(1)
    if o.opt_alpha.m:
        out["u.log_alpha_m"], out["u.log_alpha_v"] = o.opt_alpha.m[0].reshape(1), o.opt_alpha.v[0].reshape(1)
    out["u.q"], out["u.y"] = o.last["q"].reshape(-1), o.last["y"].reshape(-1)
    return {k: np.asarray(v.detach().double().numpy()) for k, v in out.items()}


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


def closed_form_backward(g: t.Tensor, zh: t.Tensor, rstd: t.Tensor, gamma: t.Tensor):
    """Section 24's backward from g = dL/dn: (dz, dgamma, dbeta)."""
    gz = g * gamma
    dz = rstd * (gz - gz.mean(1, keepdim=True) - zh * (gz * zh).mean(1, keepdim=True))
    return dz, (g * zh).sum(0), g.sum(0)


class LNOracle:
    """SAC (``algo="sac"``: twin critics, the minimum of both targets and of both critics in the actor loss, an actor step
    every update) or REDQ (``algo="redq"``: ``subset(u)`` draws the target critics of update u, the mean over the
    ensemble in the actor loss, an actor step every ``utd_ratio`` updates) with LN critics.  The critic optimiser is ONE
    Adam over [the critics' parameters ..., ln]: gamma / beta step with lr_critic at the critics' step count, and their
    target copy takes the targets' Polyak step."""

    def __init__(self, algo: str, S: int, A: int, actor: list[t.Tensor], critics: list[list[t.Tensor]],
                 targets: list[list[t.Tensor]], ln: t.Tensor, ln_target: t.Tensor,
                 subset: Callable[[int], list[int]] | None = None, n_min: int = 2, utd_ratio: int = 1,
                 gamma=0.99, tau=5e-3, lr_actor=3e-4, lr_critic=3e-4, lr_alpha=3e-4, alpha_init=1.0, tune_alpha=True,
                 dtype=t.float64, eps: float = EPS, no_ln: bool = False, freeze_ln: bool = False, no_ln_polyak: bool = False):
        assert algo in ("sac", "redq")
        self.algo, self.S, self.A, self.N = algo, S, A, len(critics)
        self.M, self.G = (self.N, 1) if algo == "sac" else (n_min, utd_ratio)
        self.gamma, self.tau, self.eps = gamma, tau, eps
        cp = lambda ps: [x.detach().to(dtype).clone() for x in ps]   # noqa: E731
        self.actor = cp(actor)
        self.critics = [cp(c) for c in critics]
        self.targets = [cp(c) for c in targets]
        self.ln, self.ln_target = ln.detach().to(dtype).clone(), ln_target.detach().to(dtype).clone()
        self.subset = subset if subset is not None else (lambda u: list(range(self.N)))
        self.no_ln, self.freeze_ln, self.no_ln_polyak = no_ln, freeze_ln, no_ln_polyak
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

    def q(self, params: list[t.Tensor], ln_i: t.Tensor, s: t.Tensor, a: t.Tensor) -> t.Tensor:
        return ln_mlp(params, None if self.no_ln else ln_i, t.cat([s, a], 1), self.eps)

    def update(self, s, a, r, d, s2, e1, e2) -> None:
        u = self.update_step
        alpha = self.alpha                       # (the value before this update's temperature step)
        idx = self.subset(u)
        with t.no_grad():
            a2, logp2, _ = orc.gaussian_forward(self.actor, s2, e1, self.A)
            qn = t.cat([self.q(self.targets[i], self.ln_target[i], s2, a2) for i in idx], 1)
            y = r + (1.0 - d) * self.gamma * (qn.min(1, keepdim=True).values - alpha * logp2)
        # one Adam step over the critic arena and the LN parameters on sum_i mean_b (Q_i - y)^2
        params = [x.clone().requires_grad_(True) for x in self.flat_critics()]
        ln = self.ln.clone().requires_grad_(True)
        per = len(self.critics[0])
        qs = [self.q(params[i * per:(i + 1) * per], ln[i], s, a) for i in range(self.N)]
        loss = sum(((q - y) ** 2).mean() for q in qs)
        grads = list(t.autograd.grad(loss, params + [ln], allow_unused=True))
        g_ln = grads.pop()
        if g_ln is None:                         # (no_ln: the loss does not depend on gamma / beta)
            g_ln = t.zeros_like(self.ln)
        if self.freeze_ln or self.no_ln:
            # (the optimiser keeps the ln slot, with zero moments, so that its lists stay aligned)
            self.opt_critic.step(self.flat_critics() + [self.ln.clone()], grads + [t.zeros_like(self.ln)])
        else:
            self.opt_critic.step(self.flat_critics() + [self.ln], grads + [g_ln])
        for i in range(self.N):
            orc.polyak(self.targets[i], self.critics[i], self.tau)
        if not self.no_ln_polyak:
            orc.polyak([self.ln_target], [self.ln], self.tau)
        self.last = dict(q=qs[0].detach(), y=y, critic_loss=loss.detach(), subset=idx, g_ln=g_ln.detach())
        # the actor step on the updated critics (through LN; gamma / beta take no step here), then the temperature
        if (u + 1) % self.G == 0:
            ap = [x.clone().requires_grad_(True) for x in self.actor]
            pi, logp, _ = orc.gaussian_forward(ap, s, e2, self.A)
            qpi = t.cat([self.q(self.critics[i], self.ln[i], s, pi) for i in range(self.N)], 1)
            q_term = qpi.min(1).values.mean() if self.algo == "sac" else qpi.mean(1).mean()
            actor_loss = (alpha * logp).mean() - q_term
            g_a = list(t.autograd.grad(actor_loss, ap))
            self.opt_actor.step(self.actor, g_a)
            self.last.update(actor_loss=actor_loss.detach(), logp=logp.detach(), qpi=qpi.detach())
            if self.tune_alpha:
                g_alpha = -(self.target_entropy + logp.detach().mean().to(t.float64))
                la = [self.log_alpha.reshape(1).clone()]
                self.opt_alpha.step(la, [g_alpha.reshape(1)])
                self.log_alpha = la[0].reshape(())
        self.update_step += 1
