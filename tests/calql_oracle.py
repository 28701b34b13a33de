"""Cal-QL's two pieces restated for the tests, for tests/test_calql_host.py, tests/test_gpu_returns.py,
tests/test_gpu_calql_seed.py and tests/test_gpu_calql.py.

1. The return-to-go of a slot (e, t) of an episodic storage, in float64 numpy:

       len_e = the stored steps of episode e (0 for a slot past the live episodes)
       T     = the first k >= t with dones[e, k] != 0, or len_e - 1 if there is none
       G     = sum_{k = t .. T} gamma^(k - t) rewards[e, k]          (t >= len_e: the single term rewards[e, t])

   and 0 for a slot outside [0, E) x [0, L).  ``returns_f32`` restates the kernel's own float32 order (csrc/replay_returns.hip:
   chunks of 64 steps, lane l's term pw[l] r with pw[l] = float32(gamma^l), the xor butterfly with masks 1, 2 .. 32,
   G <- G + f S with f <- f pw[64]) so that the kernel can be held to it bit for bit.  ``drawn_slots`` gives the slots the
   uniform sampler draws (tests/her_oracle.py's draw, tests/nstep_oracle.py's index map), ``mixed_returns`` splits a batch
   over a prior-data replay by tests/prior_oracle.py's n_prior.

2. ``CalQLOracle(CQLOracle)``: tests/cql_oracle.py's update with the penalty's policy entries e >= N bounded below by the
   row's return-to-go, c_e = max(q_e, g_b) - logd_e, and no gradient through the bound: the seed of a bounded entry
   (q_e < g_b) is 0; q_e == g_b keeps its gradient.  The uniform entries are not bounded."""
from __future__ import annotations

import numpy as np
import torch as t

from oracle import oprl_oracle as orc
from tests import cql_oracle as co
from tests import prior_oracle as po
from tests.her_oracle import draw
from tests.nstep_oracle import index_map

F = np.float32
CHUNK = 64


def _storage(rewards, dones):
    rewards = np.asarray(rewards)
    E, L = rewards.shape[:2]
    return rewards.reshape(E, L), np.asarray(dones).reshape(E, L), E, L


def _tail(dones, lens, e, t):
    """The steps [t, T] of the sum for an in-range slot."""
    len_e = int(lens[e]) if e < len(lens) else 0
    if t >= len_e:
        return t, t
    hit = np.flatnonzero(dones[e, t:len_e] != 0)
    return t, (t + int(hit[0])) if len(hit) else len_e - 1


def returns_to_go(rewards, dones, ep_lens, ep, step, gamma, absolute=False):
    """float64 G per slot; ``absolute``: sum gamma^(k - t) |r_k| instead, what the float32 tolerance scales with."""
    rewards, dones, E, L = _storage(rewards, dones)
    out = np.zeros(len(ep), dtype=np.float64)
    for i, (e, s) in enumerate(zip(np.asarray(ep).tolist(), np.asarray(step).tolist())):
        if not (0 <= e < E and 0 <= s < L):
            continue
        t0, T = _tail(dones, ep_lens, e, s)
        r = rewards[e, t0:T + 1].astype(np.float64)
        out[i] = float(np.sum(float(gamma) ** np.arange(T + 1 - t0, dtype=np.float64) * (np.abs(r) if absolute else r)))
    return out


def returns_f32(rewards, dones, ep_lens, ep, step, gamma):
    """The kernel's summation order in numpy float32."""
    rewards, dones, E, L = _storage(rewards, dones)
    rewards = rewards.astype(F)
    pw = np.array([F(float(gamma) ** l) for l in range(CHUNK + 1)], dtype=F)      # (float)pow((double)gamma, l)
    lanes = np.arange(CHUNK)
    out = np.zeros(len(ep), dtype=F)
    for i, (e, s) in enumerate(zip(np.asarray(ep).tolist(), np.asarray(step).tolist())):
        if not (0 <= e < E and 0 <= s < L):
            continue
        t0, T = _tail(dones, ep_lens, e, s)
        g, f = F(0), F(1)
        for c0 in range(t0, T + 1, CHUNK):
            n = min(CHUNK, T + 1 - c0)
            v = np.zeros(CHUNK, dtype=F)
            v[:n] = pw[:n] * rewards[e, c0:c0 + n]
            for m in (1, 2, 4, 8, 16, 32):
                v = (v + v[lanes ^ m]).astype(F)
            g = F(g + F(f * v[0]))
            f = F(f * pw[CHUNK])
        out[i] = g
    return out


def roundings(L: int) -> int:
    """The most float32 roundings any term of the kernel's sum passes through, counted from csrc/replay_returns.hip for a
    storage of L steps per episode: the power table's entry (1), pw[l] r (1), the butterfly's six additions (6), the chunk
    factor f_c — pw[64]'s own rounding and c - 1 products (c) — f_c S_c (1), and the additions into G from chunk c on
    (n_chunks - c): 9 + n_chunks with n_chunks = ceil(L / 64) at most."""
    return 9 + (int(L) + CHUNK - 1) // CHUNK


def tolerance(rewards, dones, ep_lens, ep, step, gamma):
    """Per row: c 2^-24 sum gamma^(k - t) |r_k| with c = twice ``roundings(L)``."""
    L = np.asarray(rewards).shape[1]
    return 2.0 * roundings(L) * 2.0 ** -24 * returns_to_go(rewards, dones, ep_lens, ep, step, gamma, absolute=True)


def drawn_slots(ep_lens, seed, counter, B):
    """(ep, step) of the uniform sampler's batch (seed, counter, B) over one source with these stored steps per episode."""
    n = int(np.sum(ep_lens))
    flat = np.array([(draw(seed, counter, i)[0] * n) >> 32 for i in range(B)], dtype=np.int64)
    ep, step, _lens = index_map(ep_lens, flat)
    return ep.astype(np.int32), step.astype(np.int32)


def mixed_returns(prior_storage, prior_lens, own_storage, own_lens, share, ep, step, gamma, fn=returns_to_go):
    """G of a batch over a prior-data replay: rows [0, B_p) are slots of the prior, the rest of the online replay."""
    B = len(ep)
    Bp = po.n_prior(B, share)
    ep, step = np.asarray(ep), np.asarray(step)
    a = fn(prior_storage[2], prior_storage[3], prior_lens, ep[:Bp], step[:Bp], gamma)
    b = fn(own_storage[2], own_storage[3], own_lens, ep[Bp:], step[Bp:], gamma)
    return np.concatenate([a, b])


# ---- the calibrated seed and update --------------------------------------------------------------------------------------
def seed_rows(q_wide, y, logd, g, cql_alpha, N):
    """cql_oracle.seed_rows with the bound: what the calibrated k_cql_seed computes for ONE critic from q_wide [Bw], y [B],
    logd [B, 3N] and the returns-to-go g [B].  ``bound``: the count of policy entries with q < g."""
    B, E = logd.shape
    q, qs = q_wide[:B], q_wide[B:].reshape(B, E)
    gb = g.reshape(B, 1).to(qs.dtype)
    pol = t.arange(E) >= N
    qt = t.where(pol.reshape(1, E), t.maximum(qs, gb), qs)
    c = qt - logd
    lse = t.logsumexp(c, 1)
    p = t.softmax(c, 1)
    keep = ~(pol.reshape(1, E) & ~(qs >= gb))                 # the bound passes no gradient; q == g keeps its own
    seed = t.cat([2.0 * (q - y) / B - cql_alpha / B, ((cql_alpha / B) * p * keep.to(p.dtype)).reshape(-1)], 0)
    sums = dict(sq=((q - y) ** 2).sum(), q=q.sum(), y=y.sum(), gap=(lse - q).sum(), q_rand=qs[:, :N].sum(), q_pi=qs[:, N:2 * N].sum())
    return dict(seed=seed, p=p, lse=lse, sums=sums, bound=int((pol.reshape(1, E) & (qs < gb)).sum()))


class CalQLOracle(co.CQLOracle):
    """``update(..., g)``: the rows' returns-to-go as the last argument."""

    def critic_grads(self, y, ws, wa, logd):
        B = logd.shape[0]
        g, info, bound = None, {}, 0
        for j in range(2):
            acts = orc.q_forward(self._q(self.critic, j), ws, wa)
            rows = seed_rows(acts[-1].reshape(-1), y.reshape(-1), logd, self._g, self.cql_alpha, self.N)
            gj, _ = orc.mlp_backward(self._q(self.critic, j), acts, rows["seed"].reshape(-1, 1))
            g = gj if g is None else g + gj
            sm = rows["sums"]
            bound += rows["bound"]
            info[f"q{j + 1}"] = acts[-1][:B]
            info[f"td{j + 1}"] = sm["sq"] / B
            info[f"gap{j + 1}"] = sm["gap"] / B
            info[f"q_rand{j + 1}"] = sm["q_rand"] / (B * self.N)
            info[f"q_pi{j + 1}"] = sm["q_pi"] / (B * self.N)
        info["bound_rate"] = bound / (2.0 * B * 2 * self.N)
        return g, info

    def critic_loss(self, params, y, ws, wa, logd):
        B, E = logd.shape
        pol = (t.arange(E) >= self.N).reshape(1, E)
        loss = 0.0
        for j in range(2):
            qw = orc.q_forward(self._q(params, j), ws, wa)[-1].reshape(-1)
            q, qs = qw[:B], qw[B:].reshape(B, -1)
            c = t.where(pol, t.maximum(qs, self._g.reshape(B, 1).to(qs.dtype)), qs) - logd
            loss = loss + ((q - y.reshape(-1)) ** 2).mean() + self.cql_alpha * (t.logsumexp(c, 1) - q).mean()
        return loss

    def update(self, s, a, r, d, s2, eps_next, eps_cur, eps, uni, g) -> None:
        self._g = t.as_tensor(g).reshape(-1).to(self.dtype)
        super().update(s, a, r, d, s2, eps_next, eps_cur, eps, uni)
