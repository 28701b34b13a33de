"""A conservative-Q-learning update in plain torch, written from the formulas of DESIGN.md §19 and the paper (Kumar et al.
2020, CQL(H) with a fixed penalty weight), for tests/test_cql_host.py, tests/test_gpu_cql_seed.py and
tests/test_gpu_cql.py.  It stands on oracle/oprl_oracle.py: SACOracle's layout of the twin critics, the tanh-Gaussian
forward and its backward seed, the MLP passes, Adam and Polyak.

One update on rows (s, a, r, d, s'), B of them, with N sampled actions per kind:

    a' ~ pi(.|s') (eps_next);  y = r + ((1 - d) gamma) (min_j Qtarget_j(s', a') - alpha log pi(a'|s'))          SAC's target
    per row b and k < N, constants for every gradient:
        u_bk = uni[b, k]                        log-density -A log 2
        p_bk ~ pi(.|s_b)   (eps[b, k])          log pi(p_bk|s_b)
        n_bk ~ pi(.|s'_b)  (eps[b, N + k])      log pi(n_bk|s'_b)
    per critic j, with c_jbe = Q_j(s_b, x_be) - logdensity(x_be) over the 3 N entries e = kind N + k, ALL evaluated at s_b:
        L_j = (1/B) sum_b (Q_j(s_b, a_b) - y_b)^2 + cql_alpha (1/B) sum_b [logsumexp_e c_jbe - Q_j(s_b, a_b)]
        seeds into the critic's output:  data row  2 (q - y) / B - cql_alpha / B;   sampled row  (cql_alpha / B) softmax(c_jb.)_e
    one Adam step over both critics' summed gradients; then SAC's actor step, temperature step and Polyak.

The critic runs on the wide rows: row b < B is (s_b, a_b), row B + b 3N + e is (s_b, x_be).  It computes in ``dtype``
(float64 in the GPU tests, float32 to measure what float32 arithmetic alone costs).  The gradients are written out by hand;
``critic_grads_autograd`` forms the same with autograd from the loss, and the host test holds the two against each other.

Variants that a comparison must tell from the true update: ``cql_alpha = 0`` (plain SAC), ``no_logd`` (no log-density
correction), ``at_next`` (the third kind evaluated at s' instead of s), ``scale_bw`` (the seeds scaled by 1/Bw, not 1/B)."""
from __future__ import annotations

import math

import torch as t

from oracle import oprl_oracle as orc


def gauss_from_raw(raw, eps, A):
    """The tanh-Gaussian sample and its log-probability from raw head rows [.., 2A] (means | log-stds) and draws [.., A]:
    gaussian_forward's formula (oracle/oprl_oracle.py), which is the reference's nn_models.py."""
    mu, ls_raw = raw[..., :A], raw[..., A:]
    ls = ls_raw.clamp(orc.LOG_STD_MIN, orc.LOG_STD_MAX)
    std = t.exp(ls)
    u = mu + std * eps
    normal_lp = -((u - mu) ** 2) / (2 * std * std) - ls - math.log(math.sqrt(2 * math.pi))
    log_det = 2 * math.log(2) + orc.logsigmoid(2 * u) + orc.logsigmoid(-2 * u)
    return t.tanh(u), (normal_lp - log_det).sum(-1)


def sampled_actions(raw_s, raw_s2, eps, uni, A, N):
    """x [B, 3N, A] and logd [B, 3N] in the entry order e = kind N + k; eps [B, 2N, A], uni [B, N, A]."""
    B = raw_s.shape[0]
    u = uni.clamp(-1.0, 1.0)
    p, lp = gauss_from_raw(raw_s.reshape(B, 1, 2 * A), eps[:, :N], A)
    n, ln = gauss_from_raw(raw_s2.reshape(B, 1, 2 * A), eps[:, N:], A)
    logd_u = t.full((B, N), -A * math.log(2.0), dtype=raw_s.dtype)
    return t.cat([u, p, n], 1), t.cat([logd_u, lp, ln], 1)


def wide_rows(s, a, x, s_third=None):
    """The critic step's rows: (s, a) first, then row B + b 3N + e = (s_b, x_be).  ``s_third``: the state of the third
    kind's rows (the ``at_next`` variant), else s_b."""
    B, E, A = x.shape
    N = E // 3
    ss = s.reshape(B, 1, -1).expand(B, E, s.shape[1]).clone()
    if s_third is not None:
        ss[:, 2 * N:] = s_third.reshape(B, 1, -1)
    return t.cat([s, ss.reshape(B * E, -1)], 0), t.cat([a, x.reshape(B * E, A)], 0)


def seed_rows(q_wide, y, logd, cql_alpha, N, scale_rows=None, no_logd=False):
    """What k_cql_seed computes for ONE critic from its outputs on the wide rows q_wide [Bw], y [B] and logd [B, 3N], in
    their dtype: the seed [Bw], the softmax [B, 3N], logsumexp [B] and the sums over all rows."""
    B, E = logd.shape
    q, qs = q_wide[:B], q_wide[B:].reshape(B, E)
    c = qs if no_logd else qs - logd
    lse = t.logsumexp(c, 1)
    p = t.softmax(c, 1)
    n = float(B if scale_rows is None else scale_rows)
    seed = t.cat([2.0 * (q - y) / n - cql_alpha / n, ((cql_alpha / n) * p).reshape(-1)], 0)
    sums = dict(sq=((q - y) ** 2).sum(), q=q.sum(), y=y.sum(), gap=(lse - q).sum(), q_rand=qs[:, :N].sum(), q_pi=qs[:, N:2 * N].sum())
    return dict(seed=seed, p=p, lse=lse, sums=sums)


class CQLOracle(orc.SACOracle):
    def __init__(self, state_dim, action_dim, actor, critic1, critic2, cql_alpha=5.0, n_actions=10, dtype=t.float64,
                 no_logd: bool = False, at_next: bool = False, scale_bw: bool = False, **kw):
        super().__init__(state_dim, action_dim, actor, critic1, critic2, **kw)
        self.dtype = dtype
        self.actor = [x.to(dtype) for x in self.actor]
        self.critic = [x.to(dtype) for x in self.critic]
        self.critic_target = [x.to(dtype) for x in self.critic_target]
        self.cql_alpha, self.N = float(cql_alpha), int(n_actions)
        self.no_logd, self.at_next, self.scale_bw = no_logd, at_next, scale_bw

    # ---- y, the wide rows and the log-densities from the nets as they stand
    def operands(self, s, a, r, d, s2, eps_next, eps, uni):
        y = self.td_target(r, d, s2, eps_next)
        raw_s, raw_s2 = orc.mlp_forward(self.actor, s)[-1], orc.mlp_forward(self.actor, s2)[-1]
        x, logd = sampled_actions(raw_s, raw_s2, eps, uni, self.A, self.N)
        ws, wa = wide_rows(s, a, x, s2 if self.at_next else None)
        return y, ws, wa, logd

    def critic_grads(self, y, ws, wa, logd):
        """The summed gradient of both critics by hand, and what the update reports."""
        B = logd.shape[0]
        Bw = ws.shape[0]
        g, info = None, {}
        for j in range(2):
            acts = orc.q_forward(self._q(self.critic, j), ws, wa)
            rows = seed_rows(acts[-1].reshape(-1), y.reshape(-1), logd, self.cql_alpha, self.N,
                             scale_rows=Bw if self.scale_bw else None, no_logd=self.no_logd)
            gj, _ = orc.mlp_backward(self._q(self.critic, j), acts, rows["seed"].reshape(-1, 1))
            g = gj if g is None else g + gj
            sm = rows["sums"]
            info[f"q{j + 1}"] = acts[-1][:B]
            info[f"td{j + 1}"] = sm["sq"] / B
            info[f"gap{j + 1}"] = sm["gap"] / B
            info[f"q_rand{j + 1}"] = sm["q_rand"] / (B * self.N)
            info[f"q_pi{j + 1}"] = sm["q_pi"] / (B * self.N)
        return g, info

    def critic_loss(self, params, y, ws, wa, logd):
        B = logd.shape[0]
        loss = 0.0
        for j in range(2):
            qw = orc.q_forward(self._q(params, j), ws, wa)[-1].reshape(-1)
            q, qs = qw[:B], qw[B:].reshape(B, -1)
            c = qs if self.no_logd else qs - logd
            loss = loss + ((q - y.reshape(-1)) ** 2).mean() + self.cql_alpha * (t.logsumexp(c, 1) - q).mean()
        return loss

    def critic_grads_autograd(self, y, ws, wa, logd):
        cp = [x.clone().requires_grad_(True) for x in self.critic]
        return list(t.autograd.grad(self.critic_loss(cp, y, ws, wa, logd), cp))

    def critic_step(self, s, a, y) -> None:
        """SAC's critic step replaced: the penalised loss on the wide rows of ``update``'s draws."""
        g_c, info = self.critic_grads(y, *self._wide)
        self.opt_critic.step(self.critic, g_c)
        self.last = dict(y=y, critic_loss=info["td1"] + info["td2"], penalty=self.cql_alpha * (info["gap1"] + info["gap2"]), **info)

    def update(self, s, a, r, d, s2, eps_next, eps_cur, eps, uni) -> None:
        s, a, r, d, s2, eps_next, eps_cur, eps, uni = (x.to(self.dtype) for x in (s, a, r, d, s2, eps_next, eps_cur, eps, uni))
        self._wide = self.operands(s, a, r, d, s2, eps_next, eps, uni)[1:]
        super().update(s, a, r, d, s2, eps_next, eps_cur)


# ---- the parity runs' fixture, shared by tests/test_cql_host.py (CPU) and tests/test_gpu_cql.py ------------------------------
ENV = "walker"
SHAPES = ((100, 2), (16, 16))      # (B, N): ragged B with Bw = 700; one data slice with the widest entry count, Bw = 784
N_UPDATES = 4
NET_SEED, CQL_ALPHA = 600, 5.0     # fixed with this oracle alone on the CPU (tests/test_gpu_cql.py's docstring has the figures)


def fixture_nets(net_seed=NET_SEED):
    from oracle import fixtures as fx
    S, A = fx.ENVS[ENV]
    return (fx.make_net(net_seed + 1, fx.actor_dims(S, A, gaussian=True)), fx.make_net(net_seed + 2, fx.critic_dims(S, A)),
            fx.make_net(net_seed + 3, fx.critic_dims(S, A)))


def parity_data(B, N, n=N_UPDATES, seed=500):
    """n updates' rows and draws: ((s, a, r, d, s2), eps_next [B, A], eps_cur [B, A], eps [B, 2N, A], uni [B, N, A])."""
    import numpy as np
    from oracle import fixtures as fx
    S, A = fx.ENVS[ENV]
    out = []
    for k in range(n):
        uni = t.from_numpy(np.random.RandomState(seed + 90 + k).uniform(-1, 1, (B, N, A)).astype(np.float32))
        out.append((fx.make_batch(seed + 10 + k, B, S, A), fx.make_noise(seed + 50 + k, (B, A)), fx.make_noise(seed + 70 + k, (B, A)),
                    fx.make_noise(seed + 30 + k, (B, 2 * N, A)), uni))
    return out


def oracle_state(o):
    """Parameters, targets, moments (and the temperature's) of an oracle under the keys tests/scenarios.py's gates go by."""
    out = {}
    for name, ps in (("critic", o.critic), ("critic_target", o.critic_target), ("actor", o.actor),
                     ("m_critic", o.opt_critic.m), ("v_critic", o.opt_critic.v), ("m_actor", o.opt_actor.m), ("v_actor", o.opt_actor.v)):
        for l, x in enumerate(ps):
            out[f"u.{name}.{l}"] = x.detach().double().numpy()
    if o.tune_alpha:
        out["u.critic.log_alpha"] = o.log_alpha.detach().double().reshape(1).numpy()      # (a parameter: the parameter gate)
    return out
