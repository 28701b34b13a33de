"""A D4PG update in plain torch, written from the spec (Barth-Maron et al. 2018, Bellemare et al. 2017),
for tests/test_gpu_c51_seed.py and tests/test_gpu_d4pg.py.  It computes in the dtype of its inputs (float64 in the tests)
with autograd for every gradient, takes its initial parameters from the learner, and borrows only the Adam / Polyak
arithmetic of oracle/oprl_oracle.py (as tests/redq_oracle.py does).

The categorical projection here is the usual SCATTER (floor / ceil of the fractional index, the whole mass on one atom
when they coincide); the kernel computes the same thing as a gather over triangular weights, and
tests/test_d4pg_host.py holds the two forms against each other.

``no_done`` drops the (1 - d) factor of the target and ``skip_polyak`` the Polyak steps, so that a test can show that
the comparison discriminates."""
from __future__ import annotations

import torch as t

from oracle import oprl_oracle as orc
from tests.soft_oracle import cast, mlp


def atoms(n_atoms: int, v_min: float, v_max: float, dtype=t.float64) -> t.Tensor:
    delta = (v_max - v_min) / (n_atoms - 1)
    return v_min + t.arange(n_atoms, dtype=dtype) * delta


def fractional_index(r: t.Tensor, d: t.Tensor, gamma: float, z: t.Tensor, v_min: float, v_max: float) -> t.Tensor:
    """b[B, N]: where the shifted and shrunk atom i of each row lands, in units of the atom spacing."""
    n = z.numel()
    delta = (v_max - v_min) / (n - 1)
    tz = (r.reshape(-1, 1) + ((1.0 - d.reshape(-1, 1)) * gamma) * z.reshape(1, -1)).clamp(v_min, v_max)
    return ((tz - v_min) / delta).clamp(0.0, float(n - 1))


def project_scatter(p: t.Tensor, b: t.Tensor) -> t.Tensor:
    """m[B, N] from the source probabilities p[B, N] at fractional indices b[B, N]: p_i (u - b_i) onto l = floor(b_i),
    p_i (b_i - l) onto u = ceil(b_i), and all of p_i onto l when l == u."""
    lo, up = b.floor(), b.ceil()
    same = (lo == up).to(p.dtype)
    m = t.zeros_like(p)
    m.scatter_add_(1, lo.long(), p * ((up - b) + same))
    m.scatter_add_(1, up.long(), p * (b - lo))
    return m


def critic_seed(zt: t.Tensor, z: t.Tensor, r: t.Tensor, d: t.Tensor, gamma: float, v_min: float, v_max: float):
    """What k_c51_critic_seed computes for rows of target logits zt and online logits z: (seed, m, per-row loss) with
    seed = d(mean_b loss_b) / dz by autograd."""
    n = z.shape[1]
    zs = atoms(n, v_min, v_max, z.dtype)
    m = project_scatter(t.softmax(zt, dim=1), fractional_index(r, d, gamma, zs, v_min, v_max))
    zz = z.detach().clone().requires_grad_(True)
    loss = -(m * t.log_softmax(zz, dim=1)).sum(1)
    (seed,) = t.autograd.grad(loss.mean(), [zz])
    return seed, m, loss.detach()


class D4PGOracle:
    def __init__(self, S: int, A: int, actor: list[t.Tensor], critic: list[t.Tensor], n_atoms: int, v_min: float,
                 v_max: float, gamma=0.99, tau=5e-3, lr_actor=3e-4, lr_critic=3e-4, dtype=t.float64,
                 no_done: bool = False, skip_polyak: bool = False):
        self.S, self.A = S, A
        self.actor, self.actor_target = cast(actor, dtype), cast(actor, dtype)
        self.critic, self.critic_target = cast(critic, dtype), cast(critic, dtype)
        self.v_min, self.v_max, self.gamma, self.tau = float(v_min), float(v_max), gamma, tau
        self.z = atoms(n_atoms, self.v_min, self.v_max, dtype)
        self.opt_actor, self.opt_critic = orc.Adam(lr_actor), orc.Adam(lr_critic)
        self.no_done, self.skip_polyak = no_done, skip_polyak
        self.update_step = 0
        self.last: dict = {}

    def target_distribution(self, r, d, s2) -> t.Tensor:
        with t.no_grad():
            a2 = t.tanh(mlp(self.actor_target, s2))
            pt = t.softmax(mlp(self.critic_target, t.cat([s2, a2], 1)), dim=1)
            dd = t.zeros_like(d) if self.no_done else d
            return project_scatter(pt, fractional_index(r, dd, self.gamma, self.z, self.v_min, self.v_max))

    def update(self, s, a, r, d, s2) -> None:
        m = self.target_distribution(r, d, s2)
        # the critic: one Adam step on the mean cross-entropy, then Polyak
        params = [x.clone().requires_grad_(True) for x in self.critic]
        logits = mlp(params, t.cat([s, a], 1))
        loss = -(m * t.log_softmax(logits, dim=1)).sum(1).mean()
        self.opt_critic.step(self.critic, list(t.autograd.grad(loss, params)))
        if not self.skip_polyak:
            orc.polyak(self.critic_target, self.critic, self.tau)
        self.last = dict(q=(t.softmax(logits.detach(), dim=1) * self.z).sum(1), y=(m * self.z).sum(1),
                         critic_loss=loss.detach(), m=m)
        # the actor, through the critic as just updated, then Polyak
        ap = [x.clone().requires_grad_(True) for x in self.actor]
        pi = t.tanh(mlp(ap, s))
        q = (t.softmax(mlp(self.critic, t.cat([s, pi], 1)), dim=1) * self.z).sum(1)
        actor_loss = -q.mean()
        self.opt_actor.step(self.actor, list(t.autograd.grad(actor_loss, ap)))
        if not self.skip_polyak:
            orc.polyak(self.actor_target, self.actor, self.tau)
        self.last.update(actor_loss=actor_loss.detach())
        self.update_step += 1
