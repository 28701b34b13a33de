"""One importance-weighted update of DDPG, TD3, SAC and REDQ in plain torch (float64 in the tests, autograd for every
gradient), written from the specification of prioritized training ("Training from it") and the
reference's order of operations — not from the device code — for tests/test_gpu_per_train.py:

    critic loss   sum_j (1/B) sum_b w_b (Q_j(s_b, a_b) - y_b)^2          (the weights enter here only)
    |TD|          td_abs_b = (1/n_critics) sum_j |Q_j(s_b, a_b) - y_b|   (before the critics' Adam step)
    actor / temperature losses: unweighted, as without the weights.

It takes its initial parameters from the learner and borrows the Adam / Polyak arithmetic of oracle/oprl_oracle.py; SAC
and REDQ are tests/soft_oracle.py's update with the weights in its loss hooks, DDPG and TD3 a body of their own.  The
knobs exist so a test can show that the comparison discriminates: ``ignore_weights`` trains with w = 1, ``weight_actor``
weights the actor loss too, ``normalise_by_sum`` divides the critic loss by sum(w) instead of B."""
from __future__ import annotations

import torch as t

from oracle import oprl_oracle as orc
from tests.redq_oracle import REDQOracle
from tests.soft_oracle import SoftOracle, cast, grad_step, mlp


class Knobs:
    def __init__(self, ignore_weights=False, weight_actor=False, normalise_by_sum=False):
        self.ignore_weights, self.weight_actor, self.normalise_by_sum = ignore_weights, weight_actor, normalise_by_sum

    def critic_loss(self, qs, y, w):
        """sum over the critics of the weighted mean squared TD error"""
        wc = t.ones_like(w) if self.ignore_weights else w
        norm = wc.sum() if self.normalise_by_sum else float(w.shape[0])
        return sum((wc * (q - y) ** 2).sum() / norm for q in qs)

    def actor_mean(self, rows, w):
        """the actor loss from its per-row terms"""
        return (w * rows).mean() if self.weight_actor else rows.mean()


def td_abs(qs, y):
    return sum((q.detach() - y).abs() for q in qs).reshape(-1) / len(qs)


class Weighted:
    """In front of a ``SoftOracle``: update(s, a, r, d, s2, w, e1, e2) with w [B, 1], and the knobs in the loss hooks."""

    def __init__(self, *args, ignore_weights=False, weight_actor=False, normalise_by_sum=False, **kw):
        super().__init__(*args, **kw)
        self.knobs = Knobs(ignore_weights, weight_actor, normalise_by_sum)

    def critic_loss(self, qs, y, w):
        return self.knobs.critic_loss(qs, y, w)

    def actor_loss(self, alpha, logp, q_row, w):
        if self.knobs.weight_actor:
            return self.knobs.actor_mean(alpha * logp - q_row.reshape(-1, 1), w)
        return super().actor_loss(alpha, logp, q_row, w)

    def update(self, s, a, r, d, s2, w, e1=None, e2=None) -> None:
        super().update(s, a, r, d, s2, e1, e2, w=w)


class WeightedREDQOracle(Weighted, REDQOracle):
    """tests/redq_oracle.py's update with the weights in the critic loss (and |TD| in ``last``)."""


class WeightedSACOracle(Weighted, SoftOracle):
    def __init__(self, algo: str, S: int, A: int, actor, critics, lr_alpha=1e-3, alpha_init=0.2, **kw):
        assert algo == "sac" and len(critics) == 2
        super().__init__(algo, S, A, actor, critics, critics, lr_alpha=lr_alpha, alpha_init=alpha_init, **kw)


class WeightedDetOracle:
    """algo: "ddpg" (one critic) or "td3" (twin critics).  update(s, a, r, d, s2, w, e1): e1 is TD3's smoothing draw."""

    def __init__(self, algo: str, S: int, A: int, actor, critics, gamma=0.99, tau=5e-3, lr_actor=3e-4, lr_critic=3e-4,
                 policy_noise=0.2, noise_clip=0.5, policy_freq=2, max_action=1.0, dtype=t.float64, **knobs):
        assert algo in ("ddpg", "td3") and len(critics) == (1 if algo == "ddpg" else 2)
        self.algo, self.S, self.A, self.gamma, self.tau = algo, S, A, gamma, tau
        self.actor, self.actor_target = cast(actor, dtype), cast(actor, dtype)
        self.critics = [cast(c, dtype) for c in critics]
        self.targets = [cast(c, dtype) for c in critics]
        self.opt_actor, self.opt_critic = orc.Adam(lr_actor), orc.Adam(lr_critic)
        self.policy_noise, self.noise_clip, self.policy_freq, self.max_action = policy_noise, noise_clip, policy_freq, max_action
        self.knobs = Knobs(**knobs)
        self.update_step = 0
        self.last: dict = {}

    def flat_critics(self):
        return [x for c in self.critics for x in c]

    def update(self, s, a, r, d, s2, w, e1=None, e2=None) -> None:
        k = self.knobs
        per = len(self.critics[0])
        sa = t.cat([s, a], 1)
        # the TD target
        with t.no_grad():
            a2 = t.tanh(mlp(self.actor_target, s2))
            if self.algo == "td3":
                n = (e1 * self.policy_noise).clamp(-self.noise_clip, self.noise_clip)
                a2 = (a2 + n).clamp(-self.max_action, self.max_action)
            qn = t.cat([mlp(c, t.cat([s2, a2], 1)) for c in self.targets], 1).min(1, keepdim=True).values
            y = r + (1.0 - d) * self.gamma * qn
            q_before = [mlp(c, sa) for c in self.critics]
        # the critics' Adam step on the weighted loss
        loss = grad_step(self.opt_critic, self.flat_critics(),
                         lambda p: k.critic_loss([mlp(p[i * per:(i + 1) * per], sa) for i in range(len(self.critics))], y, w))
        self.last = dict(q=q_before[0], y=y, td_abs=td_abs(q_before, y), critic_loss=loss)
        # the actor step on the updated critics (unweighted), the targets
        if self.algo == "ddpg" or self.update_step % self.policy_freq == 0:
            grad_step(self.opt_actor, self.actor,
                      lambda p: k.actor_mean(-mlp(self.critics[0], t.cat([s, t.tanh(mlp(p, s))], 1)), w))
            for tg, c in zip(self.targets, self.critics):
                orc.polyak(tg, c, self.tau)
            orc.polyak(self.actor_target, self.actor, self.tau)
        self.update_step += 1


def WeightedOracle(algo: str, *args, **kw):
    """The oracle of "ddpg", "td3" or "sac" (twin critics, a tuned temperature) from one constructor signature:
    (algo, S, A, actor, critics, ...)."""
    return (WeightedSACOracle if algo == "sac" else WeightedDetOracle)(algo, *args, **kw)
