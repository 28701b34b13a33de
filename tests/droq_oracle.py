"""LayerNorm critics with dropout in front of the normalisation (DroQ), written from the definitions of DESIGN.md section
26 on top of tests/ln_oracle.py, for tests/test_droq_host.py, tests/test_gpu_droq_slice.py and tests/test_gpu_droq.py (not a
test).

Per hidden layer l, batch row b and column c
    z = W x + b;  zd = keep(b, l, c) ? z scale : 0;  (zh, n, x_l) = section 24's LayerNorm of zd
with scale the float32 value 1 / (1 - rate) the device holds, and autograd supplies dL/dz = keep ? dL/dzd scale : 0.  The
mask is an integer comparison on Philox words, reproduced here exactly (numpy uint64 arithmetic over the constants and the
noise key of tests/test_redq_host.py):
    keep = philox4x32_10((lo32 T, hi32 T, b, l 64 + c // 4), key K)[c % 4] >= thresh,   thresh = (uint32)((double)rate 2^32)
    K = noise_key(seed, rank, 6),   T = (u 4 + k) 16 + j
u the update count before the update, k the pass (0 target critics, 1 critic step, 2 actor phase), j the critic's index.

Knobs that exist only to show that a comparison discriminates: ``no_dropout`` (plain LN critics), ``no_scale`` (scale 1),
``one_mask_per_update`` (k ignored: every pass of an update draws pass 0's mask), ``plain_targets`` (pass 0 without
dropout), ``local_rows`` (b taken modulo 16, a row's index in its slice)."""
from __future__ import annotations

import numpy as np
import torch as t

from tests import ln_oracle as lno
from tests.test_redq_host import M32, noise_key, philox4x32_10

DROP_STREAM = 6                     # the noise stream of the masks (1 - 3: the update's and REDQ's, 4 - 5: CQL's)
KNOBS = ("no_dropout", "no_scale", "one_mask_per_update", "plain_targets", "local_rows")
S, A, N, G = lno.S, lno.A, lno.N, lno.G

# ---- the parity scenarios of tests/test_gpu_droq.py (and of the float32 feasibility check of tests/test_droq_host.py) --------
# (name, B, rate, seed of the batches): "droq" is REDQ with N = 2, M = 2, G = 3; "redq" N = 10, M = 2 (two 5-net launches,
# j up to 9); "sac" a tuned temperature and the split actor phase.  The seeds by section 24's rule (tests/ln_oracle.py
# SCENARIOS): the first of 100, 200, 300, 400, 600 at which the float32 oracle stays within a QUARTER of the half gates of
# the float64 one.  Measured on the CPU, as shares of the half gates over seeds 100 / 200 / 300 / 400 / 600:
#   droq B=256 rate 0.1    0.06  0.18  0.26  0.14  0.37      -> 100
#   droq B=100 rate 0.1    0.23  0.57  0.06  0.41  0.86      -> 100
#   droq B=256 rate 0.01   0.49  1.40  0.29  78    3.3       -> 300 (see below)
#   redq B=100 rate 0.1    0.48  0.20  0.12  5.7   0.42      -> 200
#   sac  B=100 rate 0.1    0.10  0.06  0.07  4.2   1.2       -> 100
# At the default rate NO seed of the five reaches a quarter (the worst key is the actor's output layer, or a ReLU unit that
# float32 masks the other way, as section 24 describes): the seed with the most room, 300, is taken, and the test asserts what
# it asserts everywhere, the HALF gates; no gate moves.
SCENARIOS = [("droq", 256, 0.1, 100), ("droq", 100, 0.1, 100), ("droq", 256, 0.01, 300), ("redq", 100, 0.1, 200),
             ("sac", 100, 0.1, 100)]


def drop_scale(rate: float) -> float:
    """1 / (1 - rate) as the float32 the device holds."""
    return float(np.float32(1) / (np.float32(1) - np.float32(rate)))


def drop_thresh(rate: float) -> int:
    """(uint32)((double)rate 2^32) of the float32 rate the C entry points take."""
    return int(float(np.float32(rate)) * 2.0 ** 32)


def drop_stream(u: int, k: int, j: int) -> int:
    return (u * 4 + k) * 16 + j


def drop_mask(key: int, T: int, B: int, rate: float, local_rows: bool = False) -> np.ndarray:
    """keep [2 hidden layers, B, 256] (bool) of the key K and the stream T."""
    b = np.arange(B, dtype=np.uint64)
    if local_rows:
        b = b % np.uint64(16)
    shape = (2, B, 64)
    x = np.full(shape, T & M32, dtype=np.uint64)
    y = np.full(shape, (T >> 32) & M32, dtype=np.uint64)
    z = np.broadcast_to(b[None, :, None], shape).copy()
    w = np.broadcast_to((np.arange(2, dtype=np.uint64) * np.uint64(64))[:, None, None]
                        + np.arange(64, dtype=np.uint64)[None, None, :], shape).copy()
    x, y, z, w = philox4x32_10((x, y, z, w), key & M32, (key >> 32) & M32)      # (it is plain integer arithmetic: arrays pass through)
    words = np.stack([x, y, z, w], axis=-1).reshape(2, B, 256)      # column c = 4 (c // 4) + c % 4
    return words >= np.uint64(drop_thresh(rate))


def drop_mlp(p: list[t.Tensor], ln: t.Tensor, x: t.Tensor, keep: np.ndarray | None, scale: float, eps: float = lno.EPS,
             rows: dict | None = None) -> t.Tensor:
    """tests/ln_oracle.py's ``ln_mlp`` with zd = keep ? z scale : 0 in front of each normalisation (``keep`` None: none).
    ``rows``: receives per hidden layer the lists z, zd, zh, rstd, n, x (the tensors of the graph)."""
    for l in range(2):
        z = x @ p[2 * l].t() + p[2 * l + 1]
        zd = z
        if keep is not None:
            zd = t.where(t.from_numpy(keep[l]), z * scale, t.zeros((), dtype=z.dtype))
        n, zh, rstd = lno.layer_norm(zd, ln[l, 0], ln[l, 1], eps)
        x = t.relu(n)
        if rows is not None:
            for k, v in (("z", z), ("zd", zd), ("zh", zh), ("rstd", rstd), ("n", n), ("x", x)):
                rows.setdefault(k, []).append(v)
    return x @ p[4].t() + p[5]


class DroQOracle(lno.LNOracle):
    """``LNOracle`` whose every ``q`` evaluation knows (u, k, j).  ``SoftOracle.update`` evaluates the critics in a fixed
    order — the M target critics of the subset, the N critics of the critic step, then (on an actor step) the N critics on
    (s, pi) — from which pass and critic index follow."""

    def __init__(self, *args, rate: float, seed: int = 7, rank: int = 0, no_dropout: bool = False, no_scale: bool = False,
                 one_mask_per_update: bool = False, plain_targets: bool = False, local_rows: bool = False, **kw):
        super().__init__(*args, **kw)
        self.rate = rate
        self.key = noise_key(seed, rank, DROP_STREAM)
        self.on = drop_thresh(rate) > 0 and not no_dropout
        self.scale = 1.0 if no_scale else drop_scale(rate)
        self.one_mask_per_update, self.plain_targets, self.local_rows = one_mask_per_update, plain_targets, local_rows
        self._n, self._idx = 0, []
        self.masks: list[tuple[int, int, int]] = []      # (u, k, j) of every evaluation of the last update

    def update(self, *batch) -> None:
        self._n, self._idx, self.masks = 0, list(self.subset(self.update_step)), []
        super().update(*batch)

    def q(self, params, ln_i, s, a):
        n, u = self._n, self.update_step
        self._n += 1
        if n < self.M:
            k, j = 0, self._idx[n]
        elif n < self.M + self.N:
            k, j = 1, n - self.M
        else:
            k, j = 2, n - self.M - self.N
        assert t.is_grad_enabled() == (k != 0) and 0 <= j < self.N
        self.masks.append((u, k, j))
        if not self.on:
            return super().q(params, ln_i, s, a)
        keep = None
        if not (k == 0 and self.plain_targets):
            T = drop_stream(u, 0 if self.one_mask_per_update else k, j)
            keep = drop_mask(self.key, T, s.shape[0], self.rate, self.local_rows)
        return drop_mlp(params, ln_i, t.cat([s, a], 1), keep, self.scale, self.eps)


def scenario_oracle(name: str, subset, rate: float, dtype=t.float64, tau: float = 5e-3, **kw) -> DroQOracle:
    """The oracle of a scenario on tests/ln_oracle.py's fixture nets: "droq" (REDQ, N = 2, M = 2, G = 3), "redq" (N = 10,
    M = 2, G = 3) or "sac" (a tuned temperature).  ``subset``: the draw of the target critics (oprl_redq_subset)."""
    actor, critics, ln = lno.scenario_params("redq" if name == "redq" else "sac")
    if name == "sac":
        return DroQOracle("sac", S, A, actor, critics, critics, ln, ln, lr_alpha=1e-3, alpha_init=0.2, tau=tau, dtype=dtype,
                          rate=rate, **kw)
    return DroQOracle("redq", S, A, actor, critics, critics, ln, ln, subset=subset, n_min=2, utd_ratio=G, tau=tau, dtype=dtype,
                      rate=rate, **kw)
