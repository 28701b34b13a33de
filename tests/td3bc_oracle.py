"""A TD3+BC update in plain torch, written from the formulas of DESIGN.md §16 (Fujimoto & Gu 2021), for
tests/test_td3bc_host.py and tests/test_gpu_td3bc.py.  TD3 exactly as oracle/oprl_oracle.py's TD3Oracle (whose
forward / backward helpers, Adam and Polyak it borrows), with the actor step minimising

    L = -lambda (1/B) sum_b Q1(s_b, pi(s_b)) + (1/(B A)) sum_{b,k} (pi(s_b)_k - a_bk)^2,
    lambda = alpha / ((1/B) sum_b |Q1(s_b, pi(s_b))|)      (a constant for the gradient; no epsilon)

It computes in ``dtype`` (float64 in the GPU tests, float32 to measure what float32 arithmetic alone costs).  The
gradient is written out by hand — into the action columns, -(lambda/B) dQ1/dpi + 2 (pi - a)/(B A) — and
``actor_grads_autograd`` forms the same thing with autograd; the host test holds the two against each other.

``no_bc`` drops the cloning term and ``no_lambda`` sets lambda to 1, so that a test can show the comparison
discriminates."""
from __future__ import annotations

import torch as t

from oracle import oprl_oracle as orc
from tests.soft_oracle import cast


class TD3BCOracle(orc.TD3Oracle):
    def __init__(self, state_dim, action_dim, actor, critic1, critic2, bc_alpha=2.5, dtype=t.float64,
                 no_bc: bool = False, no_lambda: bool = False, **kw):
        super().__init__(state_dim, action_dim, cast(actor, dtype), cast(critic1, dtype), cast(critic2, dtype), **kw)
        self.bc_alpha, self.dtype = float(bc_alpha), dtype
        self.no_bc, self.no_lambda = no_bc, no_lambda

    # ---- the actor step's gradient, by hand
    def actor_grads(self, s, a):
        B, A = s.shape[0], self.A
        pi, a_acts = orc.det_policy_forward(self.actor, s)
        c_acts = orc.q_forward(self._q(self.critic, 0), s, pi)
        q = c_acts[-1]
        q_abs_mean = q.abs().mean()
        lam = t.ones_like(q_abs_mean) if self.no_lambda else self.bc_alpha / q_abs_mean
        _, dx = orc.mlp_backward(self._q(self.critic, 0), c_acts, t.full_like(q, -1.0 / B) * lam, need_dx=True, need_dw=False)
        da = dx[:, self.S:]
        if not self.no_bc:
            da = da + 2.0 * (pi - a) / (B * A)
        g_a, _ = orc.mlp_backward(self.actor, a_acts, da * (1 - pi * pi))
        info = dict(actor_loss=-q.mean(), bc_lambda=lam, q_abs_mean=q_abs_mean, bc_mse=((pi - a) ** 2).mean())
        return g_a, info

    # ---- ... and with autograd, straight from the loss
    def actor_grads_autograd(self, s, a):
        ap = [x.clone().requires_grad_(True) for x in self.actor]
        pi = t.tanh(orc.mlp_forward(ap, s)[-1])
        q = orc.q_forward(self._q(self.critic, 0), s, pi)[-1]
        lam = 1.0 if self.no_lambda else (self.bc_alpha / q.abs().mean()).detach()
        loss = -lam * q.mean()
        if not self.no_bc:
            loss = loss + ((pi - a) ** 2).mean()
        return list(t.autograd.grad(loss, ap))

    def update(self, s, a, r, d, s2, noise) -> None:
        s, a, r, d, s2, noise = (x.to(self.dtype) for x in (s, a, r, d, s2, noise))
        self.critic_step(s, a, self.td_target(r, d, s2, noise))
        if self.update_step % self.policy_freq == 0:
            g_a, info = self.actor_grads(s, a)
            self.opt_actor.step(self.actor, g_a)
            orc.polyak(self.critic_target, self.critic, self.tau)
            orc.polyak(self.actor_target, self.actor, self.tau)
            self.last.update(info, g_actor=g_a)
            self.last_actor = info
        self.update_step += 1
