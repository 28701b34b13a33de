"""Numpy restatement of the n-step gather (csrc/replay_nstep.hip), float32 operations in the kernel's
order: the specification the GPU tests hold the kernel to, bit for bit.

Per flat index: (e, t) by the cumulative-ends rule of the uniform sampler (first episode whose end exceeds the index;
none: episode 0, t = the index); m_max = max(1, min(n, len_e - t)); R = r_0, then R = fl(R + fl(pw[k] r_k)) for
k = 1 .. while the previous step's done is 0 and k < m_max; m = the steps taken, d_last = d_{m-1};
d' = d_last when m = 1, else fl(1 - fl(pw[m-1] fl(1 - d_last))); s' = states[e, t + m];
pw[k] = float32(float64(gamma) ** k)."""
from __future__ import annotations

import numpy as np

F = np.float32
MAX_N = 16


def powers(gamma: float) -> np.ndarray:
    """pw[k] = (float)pow((double)gamma, k), k = 0 .. 16."""
    return np.array([np.float64(gamma) ** k for k in range(MAX_N + 1)], dtype=np.float64).astype(F)


def index_map(ep_lens, inds):
    """flat indices -> (episode, step, stored steps of that episode), ep_lens = the live prefix of the table."""
    lens = np.asarray(ep_lens, dtype=np.int64)
    ends = np.cumsum(lens)
    inds = np.asarray(inds, dtype=np.int64)
    ep = np.searchsorted(ends, inds, side="right")
    ep = np.where(ep >= len(lens), 0, ep)            # every end <= ind: the all-True argmin
    start = np.where(ep > 0, ends[np.maximum(ep - 1, 0)], 0)
    return ep, inds - start, lens[ep]


def scan(r_row, d_row, m_max: int, pw):
    """One sample's row: (R, m, d') from r_row[0 .. m_max), d_row[0 .. m_max) as float32."""
    R, m = F(r_row[0]), 1
    while m < m_max and F(d_row[m - 1]) == F(0):
        R = F(R + F(pw[m] * F(r_row[m])))
        m += 1
    dl = F(d_row[m - 1])
    d_out = dl if m == 1 else F(F(1) - F(pw[m - 1] * F(F(1) - dl)))
    return R, m, d_out


def nstep_gather(states, actions, rewards, dones, ep_lens, inds, n: int, gamma: float):
    """states[E, L+1, S], actions[E, L, A], rewards / dones [E, L] or [E, L, 1] (float32 numpy), ep_lens = the live
    episodes' stored steps, inds = flat indices.  Returns dict(s, a, r, d, s2, m, ep, step); r, d shaped [B, 1]."""
    assert 1 <= n <= MAX_N
    states, actions = np.asarray(states, F), np.asarray(actions, F)
    E, L = actions.shape[:2]
    rewards, dones = np.asarray(rewards, F).reshape(E, L), np.asarray(dones, F).reshape(E, L)
    pw = powers(gamma)
    ep, step, lens = index_map(ep_lens, inds)
    B = len(ep)
    out_r, out_d, out_m = np.empty((B, 1), F), np.empty((B, 1), F), np.empty(B, np.int32)
    for i in range(B):
        e, t = int(ep[i]), int(step[i])
        m_max = max(1, min(n, int(lens[i]) - t))
        out_r[i, 0], out_m[i], out_d[i, 0] = scan(rewards[e, t:t + m_max], dones[e, t:t + m_max], m_max, pw)
    return dict(s=states[ep, step], a=actions[ep, step], r=out_r, d=out_d, s2=states[ep, step + out_m], m=out_m,
                ep=ep.astype(np.int32), step=step.astype(np.int32))
