"""One importance-weighted update of DDPG, TD3, SAC and REDQ in plain torch (float64 in the tests, autograd for every
gradient), written from the specification of prioritized training ("Training from it") and the
reference's order of operations — not from the device code — for tests/test_gpu_per_train.py:

    critic loss   sum_j (1/B) sum_b w_b (Q_j(s_b, a_b) - y_b)^2          (the weights enter here only)
    |TD|          td_abs_b = (1/n_critics) sum_j |Q_j(s_b, a_b) - y_b|   (before the critics' Adam step)
    actor / temperature losses: unweighted, as without the weights.

It takes its initial parameters from the learner and borrows the tanh-Gaussian head and the Adam / Polyak arithmetic of
oracle/oprl_oracle.py; REDQ extends tests/redq_oracle.py.  The knobs exist so a test can show that the comparison
discriminates: ``ignore_weights`` trains with w = 1, ``weight_actor`` weights the actor loss too, ``normalise_by_sum``
divides the critic loss by sum(w) instead of B."""
from __future__ import annotations

import math

import torch as t

from oracle import oprl_oracle as orc
from tests.redq_oracle import REDQOracle, mlp


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


def _grad_step(opt, params, loss_of):
    """one Adam step on loss_of(leaf copies of params); returns the loss"""
    leaves = [x.clone().requires_grad_(True) for x in params]
    loss = loss_of(leaves)
    opt.step(params, list(t.autograd.grad(loss, leaves)))
    return loss.detach()


def _gauss(actor, s, eps, A):
    """reparameterised tanh-Gaussian sample and its log-density, differentiable in `actor`"""
    out = mlp(actor, s)
    mu, log_std = out[:, :A], out[:, A:].clamp(orc.LOG_STD_MIN, orc.LOG_STD_MAX)
    std = log_std.exp()
    u = mu + std * eps
    normal_lp = -((u - mu) ** 2) / (2 * std * std) - log_std - 0.5 * math.log(2 * math.pi)
    log_det = 2 * math.log(2.0) + t.nn.functional.logsigmoid(2 * u) + t.nn.functional.logsigmoid(-2 * u)
    return t.tanh(u), (normal_lp - log_det).sum(1, keepdim=True)


class WeightedOracle:
    """algo: "ddpg" (one critic), "td3" or "sac" (twin critics).  update(s, a, r, d, s2, w, e1, e2): e1 is TD3's
    smoothing draw / SAC's next-state draw, e2 SAC's actor-step draw; w is [B, 1]."""

    def __init__(self, algo: str, S: int, A: int, actor, critics, gamma=0.99, tau=5e-3, lr_actor=3e-4, lr_critic=3e-4,
                 lr_alpha=1e-3, policy_noise=0.2, noise_clip=0.5, policy_freq=2, max_action=1.0, alpha_init=0.2,
                 tune_alpha=True, dtype=t.float64, **knobs):
        assert algo in ("ddpg", "td3", "sac") and len(critics) == (1 if algo == "ddpg" else 2)
        self.algo, self.S, self.A, self.gamma, self.tau = algo, S, A, gamma, tau
        cp = lambda ps: [x.detach().to(dtype).clone() for x in ps]   # noqa: E731
        self.actor, self.actor_target = cp(actor), cp(actor)
        self.critics = [cp(c) for c in critics]
        self.targets = [cp(c) for c in critics]
        self.opt_actor, self.opt_critic, self.opt_alpha = orc.Adam(lr_actor), orc.Adam(lr_critic), orc.Adam(lr_alpha)
        self.policy_noise, self.noise_clip, self.policy_freq, self.max_action = policy_noise, noise_clip, policy_freq, max_action
        self.tune_alpha, self.alpha_init = tune_alpha, alpha_init
        self.log_alpha = t.tensor(math.log(alpha_init), dtype=t.float64)
        self.target_entropy = -float(A)
        self.knobs = Knobs(**knobs)
        self.update_step = 0
        self.last: dict = {}

    @property
    def alpha(self) -> float:
        return float(self.log_alpha.exp()) if self.tune_alpha else float(self.alpha_init)

    def flat_critics(self):
        return [x for c in self.critics for x in c]

    def update(self, s, a, r, d, s2, w, e1=None, e2=None) -> None:
        algo, A, k = self.algo, self.A, self.knobs
        alpha = self.alpha                            # (the value before this update's temperature step)
        per = len(self.critics[0])
        sa = t.cat([s, a], 1)
        # the TD target
        with t.no_grad():
            logp2 = None
            if algo == "sac":
                a2, logp2 = _gauss(self.actor, s2, e1, A)
            else:
                a2 = t.tanh(mlp(self.actor_target, s2))
                if algo == "td3":
                    n = (e1 * self.policy_noise).clamp(-self.noise_clip, self.noise_clip)
                    a2 = (a2 + n).clamp(-self.max_action, self.max_action)
            qn = t.cat([mlp(c, t.cat([s2, a2], 1)) for c in self.targets], 1).min(1, keepdim=True).values
            if logp2 is not None:
                qn = qn - alpha * logp2
            y = r + (1.0 - d) * self.gamma * qn
            q_before = [mlp(c, sa) for c in self.critics]
        # the critics' Adam step on the weighted loss
        flat = self.flat_critics()
        loss = _grad_step(self.opt_critic, flat,
                          lambda p: k.critic_loss([mlp(p[i * per:(i + 1) * per], sa) for i in range(len(self.critics))], y, w))
        self.last = dict(q=q_before[0], y=y, td_abs=td_abs(q_before, y), critic_loss=loss)
        # the actor step on the updated critics (unweighted), the temperature, the targets
        if algo == "sac":
            def actor_loss(p):
                pi, logp = _gauss(p, s, e2, A)
                self.last["logp"] = logp.detach()
                qpi = t.cat([mlp(c, t.cat([s, pi], 1)) for c in self.critics], 1).min(1, keepdim=True).values
                return k.actor_mean(alpha * logp - qpi, w)
            _grad_step(self.opt_actor, self.actor, actor_loss)
            if self.tune_alpha:
                g_alpha = -(self.target_entropy + self.last["logp"].mean().to(t.float64))
                la = [self.log_alpha.reshape(1).clone()]
                self.opt_alpha.step(la, [g_alpha.reshape(1)])
                self.log_alpha = la[0].reshape(())
            for tg, c in zip(self.targets, self.critics):
                orc.polyak(tg, c, self.tau)
        elif algo == "ddpg" or self.update_step % self.policy_freq == 0:
            _grad_step(self.opt_actor, self.actor,
                       lambda p: k.actor_mean(-mlp(self.critics[0], t.cat([s, t.tanh(mlp(p, s))], 1)), w))
            for tg, c in zip(self.targets, self.critics):
                orc.polyak(tg, c, self.tau)
            orc.polyak(self.actor_target, self.actor, self.tau)
        self.update_step += 1


class WeightedREDQOracle(REDQOracle):
    """tests/redq_oracle.py's update with the weights in the critic loss (and |TD| in ``last``)."""

    def __init__(self, *args, ignore_weights=False, weight_actor=False, normalise_by_sum=False, **kw):
        super().__init__(*args, **kw)
        self.knobs = Knobs(ignore_weights, weight_actor, normalise_by_sum)

    def update(self, s, a, r, d, s2, w, e1, e2) -> None:
        u, k = self.update_step, self.knobs
        alpha = self.alpha
        idx = self.subset(u + self.subset_shift)
        sa = t.cat([s, a], 1)
        with t.no_grad():
            a2, logp2 = _gauss(self.actor, s2, e1, self.A)
            qn = t.cat([mlp(self.targets[i], t.cat([s2, a2], 1)) for i in idx], 1).min(1, keepdim=True).values
            y = r + (1.0 - d) * self.gamma * (qn - alpha * logp2)
            q_before = [mlp(c, sa) for c in self.critics]
        per = len(self.critics[0])
        flat = self.flat_critics()
        loss = _grad_step(self.opt_critic, flat,
                          lambda p: k.critic_loss([mlp(p[i * per:(i + 1) * per], sa) for i in range(self.N)], y, w))
        for i in range(self.N):
            orc.polyak(self.targets[i], self.critics[i], self.tau)
        self.last = dict(q=q_before[0], y=y, td_abs=td_abs(q_before, y), critic_loss=loss, subset=idx)
        if (u + 1) % self.G == 0:
            def actor_loss(p):
                pi, logp = _gauss(p, s, e2, self.A)
                self.last["logp"] = logp.detach()
                qpi = t.cat([mlp(c, t.cat([s, pi], 1)) for c in self.critics], 1).mean(1, keepdim=True)
                return k.actor_mean(alpha * logp - qpi, w)
            _grad_step(self.opt_actor, self.actor, actor_loss)
            if self.tune_alpha:
                g_alpha = -(self.target_entropy + self.last["logp"].mean().to(t.float64))
                la = [self.log_alpha.reshape(1).clone()]
                self.opt_alpha.step(la, [g_alpha.reshape(1)])
                self.log_alpha = la[0].reshape(())
        self.update_step += 1
