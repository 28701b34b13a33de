"""An implicit-Q-learning update in plain torch, written from the formulas of DESIGN.md §17 (Kostrikov et al. 2021, the
deterministic-policy form), for tests/test_iql_host.py, tests/test_gpu_iql_seed.py and tests/test_gpu_iql.py.  It borrows
the forward / backward helpers, Adam and Polyak of oracle/oprl_oracle.py and TD3Oracle's twin critics: layout and step.

One update on rows (s, a, r, d, s'), in this order:

    vn = V(s')                                      V as it is BEFORE this update's V step
    qt = min(Q1target(s, a), Q2target(s, a));  v = V(s);  u = qt - v
    V:       loss (1/B) sum omega u^2, omega = 1 - tau where u < 0 (strict) else tau;
             gradient into V's output ((2 (v - qt)) (1/B)) omega;  one Adam step (lr_value, its own moments and count)
    critics: y = r + ((1 - d) gamma) vn;  loss mean (Q1 - y)^2 + mean (Q2 - y)^2;  one Adam step over both
    actor:   w = min(exp(beta u), c), a constant;  loss (1/B) sum_b w_b sum_k (pi(s_b)_k - a_bk)^2;
             gradient into the action columns (2/B) w (pi - a), through tanh;  one Adam step
    Polyak on the critic targets and on the actor's target (which nothing reads), every update.

It computes in ``dtype`` (float64 in the GPU tests, float32 to measure what float32 arithmetic alone costs).  The
gradients are written out by hand; ``value_grads_autograd`` / ``actor_grads_autograd`` form the same with autograd from
the losses, and the host test holds the two against each other.

Variants that a comparison must tell from the true update: ``sym`` (tau = 0.5 in the V loss), ``late`` (V(s') and u
taken AFTER the V step), ``no_clip`` (w = exp(beta u)), and another ``beta``."""
from __future__ import annotations

import torch as t

from oracle import oprl_oracle as orc
from tests.soft_oracle import cast


def seed_rows(q1, q2, v, pi, a, tau, beta, clip):
    """What k_iql_value_seed / k_iql_actor_seed compute from their rows, in the rows' dtype: u, the V seed, w, da, and the
    sums (V loss, v, u, w, rows at the clip, weighted cloning loss) over all rows."""
    B = v.shape[0]
    qt = t.min(q1, q2)
    u = qt - v
    omega = t.where(u < 0, t.full_like(u, 1.0 - tau), t.full_like(u, tau))
    seed = 2.0 * (v - qt) / B * omega
    e = t.exp(beta * u)
    w = e.clamp(max=clip)
    da = (2.0 / B) * w.reshape(B, 1) * (pi - a)
    row_sq = ((pi - a) ** 2).sum(1)
    sums = dict(v_loss=(omega * u * u).sum(), v=v.sum(), u=u.sum(), w=w.sum(), clipped=(e >= clip).to(v.dtype).sum(),
                actor=(w * row_sq).sum())
    return dict(u=u, seed=seed, w=w, da=da, omega=omega, sums=sums)


class IQLOracle(orc.TwinCritics):
    def __init__(self, state_dim, action_dim, actor, critic1, critic2, value, expectile=0.7, beta=3.0, adv_clip=100.0,
                 gamma=0.99, tau=5e-3, lr_actor=3e-4, lr_critic=3e-4, lr_value=3e-4, dtype=t.float64,
                 sym: bool = False, late: bool = False, no_clip: bool = False):
        self.S, self.A, self.dtype = state_dim, action_dim, dtype
        self.gamma, self.tau = gamma, tau
        self.expectile, self.beta, self.adv_clip = float(expectile), float(beta), float(adv_clip)
        self.sym, self.late, self.no_clip = sym, late, no_clip
        self.actor = cast(actor, dtype)
        self.actor_target = cast(actor, dtype)
        self.critic = cast(critic1, dtype) + cast(critic2, dtype)      # one optimiser over q1 then q2, as TD3Oracle
        self.critic_target = cast(self.critic, dtype)
        self.n1 = len(critic1)
        self.value = cast(value, dtype)
        self.opt_actor, self.opt_critic, self.opt_value = orc.Adam(lr_actor), orc.Adam(lr_critic), orc.Adam(lr_value)
        self.update_step = 0
        self.last: dict = {}

    # ---- u, omega and the weights from the nets as they stand
    def advantage(self, s, a):
        q1 = orc.q_forward(self._q(self.critic_target, 0), s, a)[-1]
        q2 = orc.q_forward(self._q(self.critic_target, 1), s, a)[-1]
        v_acts = orc.mlp_forward(self.value, s)
        qt = t.min(q1, q2)
        u = qt - v_acts[-1]
        return qt, u, v_acts

    def weights(self, u):
        e = t.exp(self.beta * u)
        return e if self.no_clip else e.clamp(max=self.adv_clip), e

    # ---- the V step's gradient, by hand / with autograd
    def value_grads(self, s, a):
        B = s.shape[0]
        qt, u, v_acts = self.advantage(s, a)
        tau = 0.5 if self.sym else self.expectile
        omega = t.where(u < 0, t.full_like(u, 1.0 - tau), t.full_like(u, tau))
        g, _ = orc.mlp_backward(self.value, v_acts, 2.0 * (v_acts[-1] - qt) / B * omega)
        return g, dict(v_loss=(omega * u * u).mean(), v_mean=v_acts[-1].mean(), adv_mean=u.mean(), u=u, v=v_acts[-1], qt=qt)

    def value_grads_autograd(self, s, a):
        vp = [x.clone().requires_grad_(True) for x in self.value]
        qt = self.advantage(s, a)[0].detach()
        u = qt - orc.mlp_forward(vp, s)[-1]
        tau = 0.5 if self.sym else self.expectile
        omega = t.where(u.detach() < 0, t.full_like(u, 1.0 - tau), t.full_like(u, tau)).detach()
        return list(t.autograd.grad((omega * u * u).mean(), vp))

    # ---- the actor step's gradient, by hand / with autograd
    def actor_grads(self, s, a, u):
        B = s.shape[0]
        w, e = self.weights(u)
        pi, a_acts = orc.det_policy_forward(self.actor, s)
        da = (2.0 / B) * w * (pi - a)
        g, _ = orc.mlp_backward(self.actor, a_acts, da * (1 - pi * pi))
        info = dict(actor_loss=(w * ((pi - a) ** 2).sum(1, keepdim=True)).mean(), w_mean=w.mean(),
                    clip_frac=(e >= self.adv_clip).to(u.dtype).mean(), w=w, pi=pi)
        return g, info

    def actor_grads_autograd(self, s, a, u):
        ap = [x.clone().requires_grad_(True) for x in self.actor]
        w = self.weights(u)[0].detach()
        pi = t.tanh(orc.mlp_forward(ap, s)[-1])
        return list(t.autograd.grad((w * ((pi - a) ** 2).sum(1, keepdim=True)).mean(), ap))

    def update(self, s, a, r, d, s2) -> None:
        s, a, r, d, s2 = (x.to(self.dtype) for x in (s, a, r, d, s2))
        if not self.late:
            vn = orc.mlp_forward(self.value, s2)[-1]
        g_v, vinfo = self.value_grads(s, a)
        self.opt_value.step(self.value, g_v)
        u = vinfo["u"]
        if self.late:                                   # (the variant: everything read after V has moved)
            vn = orc.mlp_forward(self.value, s2)[-1]
            u = self.advantage(s, a)[1]
        self.critic_step(s, a, r + ((1.0 - d) * self.gamma) * vn)      # (TD3's twin step, with y from V)
        g_a, ainfo = self.actor_grads(s, a, u)
        self.opt_actor.step(self.actor, g_a)
        orc.polyak(self.critic_target, self.critic, self.tau)
        orc.polyak(self.actor_target, self.actor, self.tau)
        self.last.update(q_mean=(self.last["q1"].mean() + self.last["q2"].mean()) / 2, **vinfo, **ainfo)
        self.update_step += 1
