"""Numpy model of a replay with several open episodes, written from the rule and not from the buffer:
the specification tests/test_lanes_host.py and tests/test_gpu_lanes.py hold ``EpisodicReplayBuffer.open_lanes`` /
``add_step_rows`` to, bit for bit (everything here is a copy).

Storage: states[E, L+1, S], actions[E, L, A], rewards / dones [E, L, 1], zeros at the start.  N lanes; lane i starts in
slot i, the ring pointer at N - 1, the episode counter at N.  One step: for every lane, row i goes to (slot, t = the
slot's length) — s to states[slot, t], s' to states[slot, t + 1] — and the length grows by one.  Then every lane whose
episode is over, in lane order: the pointer walks on (cyclically) to the first slot that is not the current slot of any
lane, the closing lane's own included; that slot loses its transitions (length 0) and becomes the lane's; the counter
grows by one up to E."""
from __future__ import annotations

import numpy as np

F = np.float32


class LanesOracle:
    def __init__(self, E: int, L: int, S: int, A: int, N: int) -> None:
        assert 1 <= N <= E - 1
        self.E, self.L, self.S, self.A, self.N = E, L, S, A, N
        self.states = np.zeros((E, L + 1, S), F)
        self.actions = np.zeros((E, L, A), F)
        self.rewards = np.zeros((E, L, 1), F)
        self.dones = np.zeros((E, L, 1), F)
        self.ep_lens = np.zeros(E, np.int64)
        self.lanes = list(range(N))
        self.pointer = N - 1
        self.counter = N
        self.count = 0
        self.last_s2 = np.zeros((N, S), F)      # the s' each lane passed last
        self.evicted: list[int] = []            # every slot an eviction took, in order

    def step(self, s, a, r, d, s2, over) -> list[tuple[int, int]]:
        """Returns the (slot, t) every lane wrote."""
        s, a, s2 = np.asarray(s, F), np.asarray(a, F), np.asarray(s2, F)
        r, d = np.asarray(r, F).reshape(-1), np.asarray(d, F).reshape(-1)
        wrote = []
        for i in range(self.N):
            e = self.lanes[i]
            t = int(self.ep_lens[e])
            assert t < self.L
            self.states[e, t], self.states[e, t + 1] = s[i], s2[i]
            self.actions[e, t], self.rewards[e, t, 0], self.dones[e, t, 0] = a[i], r[i], d[i]
            self.ep_lens[e] = t + 1
            self.count += 1
            wrote.append((e, t))
        self.last_s2 = s2.copy()
        for i in range(self.N):
            if not bool(np.asarray(over).reshape(-1)[i]):
                continue
            p = self.pointer
            for _ in range(self.E):
                p = (p + 1) % self.E
                if p not in self.lanes:
                    break
            else:
                raise AssertionError("no free slot")
            self.pointer = p
            self.count -= int(self.ep_lens[p])
            self.ep_lens[p] = 0
            self.evicted.append(p)
            self.lanes[i] = p
            self.counter = min(self.counter + 1, self.E)
        return wrote

    # ---- what the sampler sees ------------------------------------------------------------------------------------------
    def live_lens(self) -> np.ndarray:
        return self.ep_lens[:self.counter].copy()

    def live_slots(self) -> list[tuple[int, int]]:
        """(e, t) of every live transition in flat-index order."""
        return [(e, t) for e in range(self.counter) for t in range(int(self.ep_lens[e]))]

    def gather(self, inds) -> dict[str, np.ndarray]:
        """The uniform sampler's rows for flat indices (the cumulative-ends rule)."""
        ends = np.cumsum(self.ep_lens[:self.counter])
        inds = np.asarray(inds, np.int64)
        ep = np.searchsorted(ends, inds, side="right")
        t = inds - np.where(ep > 0, ends[np.maximum(ep - 1, 0)], 0)
        return dict(s=self.states[ep, t], a=self.actions[ep, t], r=self.rewards[ep, t], d=self.dones[ep, t],
                    s2=self.states[ep, t + 1], ep=ep, step=t)

    def storage(self) -> list[np.ndarray]:
        return [self.states, self.actions, self.rewards, self.dones]


def random_step(rs: np.random.RandomState, N: int, S: int, A: int):
    """(s, a, r, d, s2) of one step, every value distinct with overwhelming probability."""
    return (rs.standard_normal((N, S)).astype(F), rs.uniform(-1, 1, (N, A)).astype(F), rs.standard_normal(N).astype(F),
            (rs.rand(N) < 0.2).astype(F), rs.standard_normal((N, S)).astype(F))
