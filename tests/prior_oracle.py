"""Numpy restatement of the mixed gather (csrc/replay_mix.hip): the specification the GPU tests hold the
kernel to, bit for bit.

B_p = min(B, max(0, floor(share * B + 0.5))) in double arithmetic.  Row i < B_p is drawn over the prior's episode table
and storage, row i >= B_p over the online replay's: flat index = the injected one, else (r.x * n_transitions) >> 32 with
r = philox4x32_10((counter lo, counter hi, i, 0x5a17), seed lo, seed hi) (tests/her_oracle.py draw) and n_transitions
that of the row's source; (e, t) by the cumulative-ends rule (tests/nstep_oracle.py index_map).  The row is the stored
transition of its source: states[e, t], actions[e, t], rewards[e, t], dones[e, t], states[e, t + 1]."""
from __future__ import annotations

import math

import numpy as np

from tests.her_oracle import draw
from tests.nstep_oracle import index_map

F = np.float32


def n_prior(B: int, share: float) -> int:
    return min(B, max(0, int(math.floor(float(share) * B + 0.5))))


def _rows(storage, ep_lens, seed, counter, rows, inds):
    """The plain gather of batch rows `rows` (their positions in the batch) out of one source."""
    states, actions, rewards, dones = storage
    states, actions = np.asarray(states, F), np.asarray(actions, F)
    E, L = actions.shape[:2]
    rewards, dones = np.asarray(rewards, F).reshape(E, L), np.asarray(dones, F).reshape(E, L)
    n = int(np.sum(ep_lens))
    if inds is None:
        flat = np.array([(draw(seed, counter, int(i))[0] * n) >> 32 for i in rows], dtype=np.int64)
    else:
        flat = np.asarray(inds, dtype=np.int64)[rows]
    ep, step, _lens = index_map(ep_lens, flat)
    k = len(rows)
    return dict(s=states[ep, step], a=actions[ep, step], r=rewards[ep, step].reshape(k, 1), d=dones[ep, step].reshape(k, 1),
                s2=states[ep, step + 1], ep=ep.astype(np.int32), step=step.astype(np.int32))


def mix_gather(prior_storage, prior_lens, own_storage, own_lens, share: float, seed: int, counter: int, B: int, inds=None):
    """*_storage = (states[E, L+1, S], actions[E, L, A], rewards, dones) of a source, *_lens the stored steps of its live
    episodes, inds = injected flat indices (each into its row's own source) or None.  Returns dict(s, a, r, d, s2, ep,
    step, src); r, d shaped [B, 1]; src 1 for a prior row, 0 for an own row."""
    Bp = n_prior(B, share)
    parts = []
    if Bp > 0:
        parts.append(_rows(prior_storage, prior_lens, seed, counter, np.arange(Bp), inds))
    if Bp < B:
        parts.append(_rows(own_storage, own_lens, seed, counter, np.arange(Bp, B), inds))
    out = {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}
    out["src"] = (np.arange(B) < Bp).astype(np.int32)
    return out
