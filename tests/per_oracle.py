"""The prioritized replay's sum tree (csrc/replay_prio.hip) restated in numpy, for the tests: the layout,
the node function, the leaves' maintenance at a flush, the priority update, the stratified descent and the importance
weights.  float32 arithmetic where the device computes in float32, so that the tree and the drawn slots compare bit
for bit; the weights in float64 from the formula of the spec."""
from __future__ import annotations

import numpy as np

from oprl_amd.buffers.prioritized_buffer import FANOUT, tree_layout
from tests.test_redq_host import M32, philox4x32_10

F = FANOUT
SAMPLE_WORD = 0x7E55
f32 = np.float32


def node_sums(children: np.ndarray) -> np.ndarray:
    """Nodes from their children, children.shape = [n, F]: a lane's four as (c0 + c1) + (c2 + c3), then the 64 lanes
    folded by halves, v[l] = v[l] + v[l + h] for h = 32, 16, ..., 1."""
    x = children.astype(f32).reshape(-1, 64, 4)
    v = (x[:, :, 0] + x[:, :, 1]) + (x[:, :, 2] + x[:, :, 3])
    h = 32
    while h:
        v = v[:, :h] + v[:, h:2 * h]
        h //= 2
    return v[:, 0]


def build(leaves: np.ndarray) -> np.ndarray:
    """The whole tree (every level, leaves first, zero padding) of the given leaves."""
    counts, offs = tree_layout(len(leaves))
    tree = np.zeros(offs[-1], f32)
    tree[:len(leaves)] = leaves
    for k in range(1, len(counts)):
        child = tree[offs[k - 1]:offs[k]].reshape(-1, F)
        tree[offs[k]:offs[k] + counts[k]] = node_sums(child)
    return tree


def priority(td: float, alpha: float, eps: float) -> np.float32:
    return f32(np.power(max(float(f32(td)), 0.0) + eps, alpha))


class TreeModel:
    """The leaves and p_max as the spec keeps them.  ``flush(rows, lens, n)``: the rows (e, t) a flush wrote and the
    episode table it uploaded; ``update(slots, td)``: a priority update."""

    def __init__(self, E: int, L: int, alpha: float, eps: float):
        self.E, self.L, self.alpha, self.eps = E, L, alpha, eps
        self.leaves = np.zeros(E * L, f32)
        self.lens = np.zeros(E, np.int64)       # the table the leaves stand for (0 = dead episode)
        self.p_max = f32(1.0)

    def enable(self, lens, n):
        self.leaves[:] = 0
        self.lens[:] = 0
        for e in range(n):
            self.lens[e] = lens[e]
            self.leaves[e * self.L:e * self.L + lens[e]] = self.p_max

    def flush(self, rows, lens, n):
        new = np.array([lens[e] if e < n else 0 for e in range(self.E)], np.int64)
        for e, t in rows:
            self.leaves[e * self.L + t] = self.p_max if t < new[e] else f32(0)
        for e in range(self.E):
            old = int(self.lens[e])
            for t in range(min(old, new[e]), max(old, new[e])):
                self.leaves[e * self.L + t] = self.p_max if t < new[e] else f32(0)
        self.lens = new

    def update(self, slots, td):
        slots = [int(s) for s in slots]
        for j, s in enumerate(slots):
            e, t = divmod(s, self.L)
            if s < 0 or t >= self.lens[e]:
                continue
            p = priority(td[j], self.alpha, self.eps)
            self.p_max = max(self.p_max, p)
            if s not in slots[j + 1:]:
                self.leaves[s] = p


def descend(tree: np.ndarray, n_leaves: int, B: int, seed: int, counter: int) -> list[int]:
    """The slots k_prio_sample draws, -1 for a tree without mass."""
    counts, offs = tree_layout(n_leaves)
    top = len(counts) - 1
    total = tree[offs[top]]
    seg = f32(np.float64(total) / B)
    out = []
    for j in range(B):
        r = philox4x32_10((counter & M32, (counter >> 32) & M32, j, SAMPLE_WORD), seed & M32, (seed >> 32) & M32)
        U = f32(r[0] >> 8) * f32(1.0 / 16777216.0)
        u = (f32(j) + U) * seg
        node = 0
        for k in range(top, 0, -1):
            c = tree[offs[k - 1] + node * F: offs[k - 1] + node * F + F].reshape(64, 4)
            q = np.empty((64, 4), f32)
            q[:, 0] = c[:, 0]
            for i in range(1, 4):
                q[:, i] = q[:, i - 1] + c[:, i]
            x = q[:, 3].copy()
            d = 1
            while d < 64:
                x[d:] = x[:-d] + x[d:]
                d *= 2
            ex = np.concatenate([[f32(0)], x[:-1]]).astype(f32)
            P = (ex[:, None] + q).reshape(-1)
            Pex = np.concatenate([ex[:, None], ex[:, None] + q[:, :3]], axis=1).reshape(-1)
            cf = c.reshape(-1)
            ok = np.nonzero((cf > 0) & (P > u))[0]
            if len(ok):
                i = int(ok[0])
            else:
                nz = np.nonzero(cf > 0)[0]
                if not len(nz):
                    node = -1
                    break
                i = int(nz[-1])
            u = max(f32(u - Pex[i]), f32(0))
            node = node * F + i
        out.append(node)
    return out


def weights(leaves: np.ndarray, slots, beta: float) -> np.ndarray:
    """(N · p_j / total)^-beta over the batch's largest, in float64 (N: the live slots, total: the leaves' sum)."""
    lv = leaves.astype(np.float64)
    N, total = np.count_nonzero(lv), lv.sum()
    w = (N * lv[np.asarray(slots)] / total) ** (-beta)
    return w / w.max()
