"""Numpy restatement of the hindsight gather (csrc/replay_her.hip), float32 operations in the kernel's
order: the specification the GPU tests hold the kernel to, bit for bit.

Per sample i: r = philox4x32_10((counter lo, counter hi, i, 0x5a17), seed lo, seed hi), the uniform sampler's call.
The flat index is the injected one, else (r.x * n_transitions) >> 32; (e, t, len_e) by the cumulative-ends rule
(tests/nstep_oracle.py index_map).  c = len_e - 1 - t; relabelled iff c >= 1 and U < float32(ratio),
U = float32(r.y >> 8) * 2^-24 — r evaluated also when the index is injected.  t' = t + ((r.z * c) >> 32) (future) or
len_e - 2 (final); g' = states[e, t' + 1][ag]; s = states[e, t], s' = states[e, t + 1] with [g] <- g'; a, d verbatim;
dist2 = sum over k in order of fl(fl(ag(s')_k - g'_k)^2); r = 0 if dist2 <= float32(eps * eps) else -1 (sparse),
-sqrt(dist2) (dense).  Every other row is the stored transition."""
from __future__ import annotations

import numpy as np

from tests.nstep_oracle import index_map
from tests.test_redq_host import M32, philox4x32_10

F = np.float32
SAMPLE_WORD = 0x5A17
FUTURE, FINAL = 0, 1
SPARSE, DENSE = 0, 1


def draw(seed: int, counter: int, i: int):
    """The four words of sample i's draw."""
    return philox4x32_10((counter & M32, (counter >> 32) & M32, i, SAMPLE_WORD), seed & M32, (seed >> 32) & M32)


def drawn_indices(seed: int, counter: int, B: int, n_transitions: int) -> np.ndarray:
    return np.array([(draw(seed, counter, i)[0] * n_transitions) >> 32 for i in range(B)], dtype=np.int64)


def uniform(word: int) -> np.float32:
    return F(F(word >> 8) * F(1.0 / 16777216.0))


def choose_from(y: int, z: int, t: int, len_e: int, ratio: float, strategy: int) -> int:
    """t' from the draw's words y and z at step t of an episode with len_e stored steps, or -1 when the row is not
    relabelled."""
    c = len_e - 1 - t
    if not (c >= 1 and uniform(y) < F(ratio)):
        return -1
    return t + ((z * c) >> 32) if strategy == FUTURE else len_e - 2


def choose(seed: int, counter: int, i: int, t: int, len_e: int, ratio: float, strategy: int) -> int:
    """choose_from for sample i of the batch drawn with (seed, counter)."""
    _x, y, z, _w = draw(seed, counter, i)
    return choose_from(y, z, t, len_e, ratio, strategy)


def dist2(achieved, goal) -> np.float32:
    acc = F(0)
    for a, g in zip(np.asarray(achieved, F), np.asarray(goal, F)):
        d = F(a - g)
        acc = F(acc + F(d * d))
    return acc


def reward(achieved, goal, kind: int, threshold: float) -> np.float32:
    d2 = dist2(achieved, goal)
    if kind == SPARSE:
        return F(0) if d2 <= F(float(threshold) * float(threshold)) else F(-1)
    return F(-np.sqrt(d2))


def her_gather(states, actions, rewards, dones, ep_lens, seed: int, counter: int, B: int, ag_off: int, g_off: int,
               G: int, ratio: float, strategy: int, kind: int, threshold: float, inds=None):
    """states[E, L+1, S], actions[E, L, A], rewards / dones [E, L] or [E, L, 1] (float32 numpy), ep_lens = the live
    episodes' stored steps, inds = injected flat indices or None.  Returns dict(s, a, r, d, s2, ep, step, future);
    r, d shaped [B, 1]."""
    states, actions = np.asarray(states, F), np.asarray(actions, F)
    E, L = actions.shape[:2]
    rewards, dones = np.asarray(rewards, F).reshape(E, L), np.asarray(dones, F).reshape(E, L)
    if inds is None:
        inds = drawn_indices(seed, counter, B, int(np.sum(ep_lens)))
    ep, step, lens = index_map(ep_lens, inds)
    assert len(ep) == B
    s, s2 = states[ep, step].copy(), states[ep, step + 1].copy()
    r, d = rewards[ep, step].reshape(B, 1).copy(), dones[ep, step].reshape(B, 1).copy()
    future = np.full(B, -1, np.int32)
    for i in range(B):
        e, t = int(ep[i]), int(step[i])
        tp = choose(seed, counter, i, t, int(lens[i]), ratio, strategy)
        if tp < 0:
            continue
        future[i] = tp
        goal = states[e, tp + 1, ag_off:ag_off + G]
        r[i, 0] = reward(states[e, t + 1, ag_off:ag_off + G], goal, kind, threshold)
        s[i, g_off:g_off + G] = goal
        s2[i, g_off:g_off + G] = goal
    return dict(s=s, a=actions[ep, step], r=r, d=d, s2=s2, ep=ep.astype(np.int32), step=step.astype(np.int32),
                future=future)
