"""k_cql_rows and k_cql_seed alone (csrc/cql_seed.hip, through oprl_cql_rows / oprl_cql_seed) against tests/cql_oracle.py
in float64, on rows crafted to reach the kernels' corners; and what the kernels must leave alone.

The gate is the suite's output gate, 2e-5 relative to each key's largest reference entry.  What float32 costs here, worked
out for these rows: the log-probability's Gaussian term is (u - mu)^2 / (2 sd^2) with u = mu + sd eps rounded to float32,
so u - mu is off by up to ulp(|u|) / 2 — 5e-7 at the largest pre-tanh value used, 12 — and the term by eps 5e-7 / sd, 2e-6
at most with sd >= exp(-1) on the random rows, against log-densities whose largest is above 10.  (The row at the lower
clamp end, sd = exp(-20), has means 0: there u = sd eps is exact in both arithmetics, and the test is about the clamp.)
In the seed kernel an entry c = q - logd of magnitude 30 carries ulp(30) / 2 = 1e-6, which expf passes on as a relative
error of the softmax weight: under a tenth of the gate."""
from __future__ import annotations

import functools
import math

import numpy as np
import pytest
import torch as t

from oprl_amd import _capi
from tests import cql_oracle as co
from tests import scenarios as sc

pytestmark = pytest.mark.gpu

TOL = 2e-5                 # the suite's output gate (tests/test_gpu_c51_seed.py)
CANARY = 12345.678
BS, NS, AS = (1, 16, 17, 100), (1, 4, 16), (1, 6)
S = 5
GAMMA, ALPHA, CA = 0.99, 0.2, 5.0
NC = 2
ROW_KINDS = ("saturated", "clamp_ends", "clamp_exact")               # rows 0 .. 2 of rows_in
SEED_KINDS = ("apart60", "equal", "dominant", "q_is_y")              # rows 0 .. 3 of seed_in


def dev(x):
    return None if x is None else t.from_numpy(np.ascontiguousarray(x)).cuda()


# ---- k_cql_rows ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def rows_in(A, N):
    """100 rows (s, a, raw_s, raw_s2, eps, uni) in float32; rows 0 .. 2 are crafted, the rest random."""
    rs = np.random.RandomState(700 + 10 * A + N)
    B = 100
    s = rs.standard_normal((B, S)).astype(np.float32)
    a = rs.uniform(-1, 1, (B, A)).astype(np.float32)
    raw = [np.concatenate([rs.standard_normal((B, A)), 0.5 * rs.standard_normal((B, A))], 1).astype(np.float32) for _ in range(2)]
    eps = rs.standard_normal((B, 2 * N, A)).astype(np.float32)
    uni = rs.uniform(-1, 1, (B, N, A)).astype(np.float32)
    # saturated: |pre-tanh| near 12, the action rounds to +1 (at s) and -1 (at s'); the log-probability's tanh correction
    raw[0][0, :A], raw[0][0, A:] = 12.0, -3.0
    raw[1][0, :A], raw[1][0, A:] = -12.0, -3.0
    # both clamp ends, from outside: log-std -25 -> -20 (means 0: see the docstring), 3 -> 2
    raw[0][1, :A], raw[0][1, A:] = 0.0, -25.0
    raw[1][1, A:] = 3.0
    # ... and exactly on them
    raw[0][2, :A], raw[0][2, A:] = 0.0, -20.0
    raw[1][2, A:] = 2.0
    uni[3, 0, 0], uni[3, N - 1, A - 1] = 1.0, -1.0           # the uniform kind's own ends
    return s, a, raw[0], raw[1], eps, uni


def run_rows(A, N, sel, philox=None, extra=2):
    """k_cql_rows on the rows `sel`; inputs carry `extra` NaN rows behind them, outputs as many canary rows.  philox =
    (seed, counter): no supplied draws.  Returns (ws, wa, logd) float32 CPU tensors with the canary rows."""
    s, a, raw_s, raw_s2, eps, uni = (x[list(sel)] for x in rows_in(A, N))
    B = len(sel)
    Bw = B * (1 + 3 * N)
    pad = lambda x: dev(np.concatenate([x, np.full((extra, *x.shape[1:]), np.nan, np.float32)], 0))      # noqa: E731
    ds, da, dr, dr2, de, du = (pad(x) for x in (s, a, raw_s, raw_s2, eps, uni))
    ws = t.full((Bw + extra, S), CANARY, dtype=t.float32, device="cuda")
    wa = t.full((Bw + extra, A), CANARY, dtype=t.float32, device="cuda")
    logd = t.full((B * 3 * N + extra,), CANARY, dtype=t.float32, device="cuda")
    seed, ctr = philox if philox is not None else (0, 0)
    _capi.check(_capi.load().oprl_cql_rows(_capi.ptr(ds), _capi.ptr(da), _capi.ptr(dr), _capi.ptr(dr2),
                                           None if philox is not None else _capi.ptr(de), None if philox is not None else _capi.ptr(du),
                                           seed, ctr, B, S, A, N, _capi.ptr(ws), _capi.ptr(wa), _capi.ptr(logd),
                                           _capi.current_stream()), "oprl_cql_rows")
    t.cuda.synchronize()
    return ws.cpu(), wa.cpu(), logd.cpu()


def rows_oracle(A, N, sel):
    s, a, raw_s, raw_s2, eps, uni = (t.from_numpy(x[list(sel)]).double() for x in rows_in(A, N))
    x, logd = co.sampled_actions(raw_s, raw_s2, eps, uni, A, N)
    ws, wa = co.wide_rows(s, a, x)
    return ws, wa, logd


def check_rows(A, N, sel, got):
    B = len(sel)
    Bw, E = B * (1 + 3 * N), 3 * N
    ws, wa, logd = got
    want_ws, want_wa, want_logd = rows_oracle(A, N, sel)
    assert t.equal(ws[:Bw].double(), want_ws), "the wide states are copies"
    assert t.equal(wa[:B].double(), want_wa[:B]), "the data rows' actions are copies"
    x, want_x = wa[B:Bw].reshape(B, E, A), want_wa[B:].reshape(B, E, A)
    assert t.equal(x[:, :N].double(), want_x[:, :N]), "the supplied uniform actions, clamped, are copies"
    devs = dict(actions=sc.rel_dev(x.numpy(), want_x.numpy()), logd=sc.rel_dev(logd[:B * E].reshape(B, E).numpy(), want_logd.numpy()))
    print(f"rows A={A} N={N} B={B}: rel dev actions {devs['actions']:.2e} logd {devs['logd']:.2e} (largest |logd| {float(want_logd.abs().max()):.1f})")
    for k, v in devs.items():
        assert v < TOL, (k, v)
    assert t.all(ws[Bw:] == CANARY) and t.all(wa[Bw:] == CANARY) and t.all(logd[B * E:] == CANARY), "rows past an extent were written"
    assert t.all(t.isfinite(wa[:Bw])) and t.all(t.isfinite(logd[:B * E])) and float(wa[:Bw].abs().max()) <= 1.0


def test_the_crafted_action_rows_are_what_they_claim():
    for A in AS:
        for N in NS:
            _, _, raw_s, raw_s2, eps, uni = rows_in(A, N)
            _, wa, logd = rows_oracle(A, N, range(3))
            x = wa[3:].reshape(3, 3 * N, A)
            assert t.all(x[0, N:2 * N].float() == 1.0) and t.all(x[0, 2 * N:].float() == -1.0)      # rounds to +-1 in float32 ...
            assert t.all(x[0, N:].abs() < 1.0) and t.all(t.isfinite(logd))                            # ... and not in float64
            assert raw_s[1, A] < -20 and raw_s2[1, A] > 2 and raw_s[2, A] == -20 and raw_s2[2, A] == 2


@pytest.mark.parametrize("A", AS)
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("B", BS)
def test_rows_match_the_oracle(B, N, A):
    """B = 1: one launch per crafted row; B >= 16: rows 0 .. B - 1, the crafted ones among them."""
    for sel in ([[r] for r in range(4)] if B == 1 else [list(range(B))]):
        check_rows(A, N, sel, run_rows(A, N, sel))


def test_rows_are_bitwise_stable_and_independent_of_the_batch():
    """Two runs are bit-identical; a row's actions and log-densities keep their bits alone, inside B = 17 and B = 100, and
    at another position."""
    A, N = 6, 4
    E = 3 * N
    w100, a100, l100 = run_rows(A, N, range(100))
    again = run_rows(A, N, range(100))
    assert t.equal(w100, again[0]) and t.equal(a100, again[1]) and t.equal(l100, again[2])
    _, a17, l17 = run_rows(A, N, range(17))
    for row in (0, 1, 2, 3, 16):
        _, a1, l1 = run_rows(A, N, [row])
        for B, aB, lB in ((17, a17, l17), (100, a100, l100)):
            assert t.equal(a1[1:1 + E], aB[B + row * E:B + (row + 1) * E]) and t.equal(l1[:E], lB[row * E:(row + 1) * E]), (row, B)
        others, pos = list(range(40, 56)), 9
        _, am, lm = run_rows(A, N, others[:pos] + [row] + others[pos:])
        assert t.equal(am[17 + pos * E:17 + (pos + 1) * E], a1[1:1 + E]) and t.equal(lm[pos * E:(pos + 1) * E], l1[:E]), row


def test_philox_rows():
    """Without supplied draws: the uniform actions lie in [-1, 1], everything is finite, two runs at one counter are
    bit-identical, another counter and another seed give other draws; the uniform kind's log-density is -A log 2."""
    A, N, B = 6, 4, 100
    E = 3 * N
    _, a0, l0 = run_rows(A, N, range(B), philox=(7, 0))
    _, a0b, l0b = run_rows(A, N, range(B), philox=(7, 0))
    _, a1, _ = run_rows(A, N, range(B), philox=(7, 1))
    _, a2, _ = run_rows(A, N, range(B), philox=(8, 0))
    assert t.equal(a0, a0b) and t.equal(l0, l0b)
    Bw = B * (1 + E)
    x0, x1, x2 = (v[B:Bw].reshape(B, E, A) for v in (a0, a1, a2))
    u = x0[:, :N]
    assert float(u.min()) >= -1.0 and float(u.max()) <= 1.0 and abs(float(u.mean())) < 0.05 and float(u.std()) == pytest.approx(1 / math.sqrt(3), rel=0.05)
    assert t.all(t.isfinite(a0[:Bw])) and t.all(t.isfinite(l0[:B * E]))
    for other in (x1, x2):
        assert float((other[:, :N] != u).float().mean()) > 0.99 and float((other[:, N:] != x0[:, N:]).float().mean()) > 0.9
    assert t.all(l0[:B * E].reshape(B, E)[:, :N] == np.float32(-(np.float32(A) * np.float32(0.6931471805599453))))
    assert t.all(a0[Bw:] == CANARY) and t.all(l0[B * E:] == CANARY)


# ---- k_cql_seed ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def seed_in(N):
    """100 rows: q [NC, 100, 1 + 3N] (the data row's value first), qn1, qn2, logp2, r, d [100], logd [100, 3N], float32."""
    rs = np.random.RandomState(800 + N)
    B, E = 100, 3 * N
    q = (2.0 * rs.standard_normal((NC, B, 1 + E))).astype(np.float32)
    qn1, qn2 = (2.0 * rs.standard_normal((2, B))).astype(np.float32)
    logp2 = rs.uniform(-8, 2, B).astype(np.float32)
    r = rs.uniform(0, 1, B).astype(np.float32)
    d = (rs.uniform(0, 1, B) < 0.2).astype(np.float32)
    logd = rs.uniform(-9, 3, (B, E)).astype(np.float32)
    logd[:, :N] = np.float32(-6 * math.log(2.0))
    # entries 60 apart (logd 0): the max-subtraction
    q[:, 0, 1:], logd[0] = rs.uniform(-30, 30, (NC, E)), 0.0
    q[:, 0, 1], q[:, 0, E] = -30.0, 30.0
    # all entries equal: c = 1.25 exactly (quarters are float32 numbers)
    logd[1] = 0.25 * rs.randint(-20, 8, E)
    q[:, 1, 1:] = 1.25 + logd[1]
    # one entry dominant by 200
    q[:, 2, 1:], logd[2] = rs.uniform(-1, 1, (NC, E)), 0.0
    q[:, 2, 1 + E // 2] = 201.0
    # q == y bitwise: d = 1 makes y = r in float32 as in float64
    d[3] = 1.0
    q[:, 3, 0] = r[3]
    return q, qn1, qn2, logp2, r, d, logd


def wide_q(q, sel):
    """[NC, Bw] in the kernel's layout from q[:, sel]: the data rows' values, then every row's entries."""
    x = q[:, list(sel)]
    return np.concatenate([x[:, :, 0], x[:, :, 1:].reshape(NC, -1)], 1)


def run_seed(N, sel, extra=2, ca=CA):
    q, qn1, qn2, logp2, r, d, logd = seed_in(N)
    sel = list(sel)
    B, E = len(sel), 3 * N
    Bw, n = B * (1 + E), (B + 15) // 16
    # (q is [NC][Bw] with no gap between the critics: the canary rows sit behind the last one)
    dq = dev(np.concatenate([wide_q(q, sel).reshape(-1), np.full(extra, np.nan, np.float32)]))
    pad = lambda x: dev(np.concatenate([x[sel].reshape(-1), np.full(extra, np.nan, np.float32)]))      # noqa: E731
    d1, d2, dl, dr, dd, dld = (pad(x) for x in (qn1, qn2, logp2, r, d, logd))
    seed = t.full((NC * Bw + extra,), CANARY, dtype=t.float32, device="cuda")
    y = t.full((B + extra,), CANARY, dtype=t.float32, device="cuda")
    part = t.full((NC * n + 1, 4), CANARY, dtype=t.float32, device="cuda")
    part_cql = t.full((NC * n + 1, 4), CANARY, dtype=t.float32, device="cuda")
    _capi.check(_capi.load().oprl_cql_seed(_capi.ptr(dq), _capi.ptr(d1), _capi.ptr(d2), _capi.ptr(dl), _capi.ptr(dr), _capi.ptr(dd),
                                           _capi.ptr(dld), ALPHA, GAMMA, ca, NC, B, N, _capi.ptr(seed), _capi.ptr(y), _capi.ptr(part),
                                           _capi.ptr(part_cql), _capi.current_stream()), "oprl_cql_seed")
    t.cuda.synchronize()
    return seed.cpu(), y.cpu(), part.cpu(), part_cql.cpu()


@functools.lru_cache(maxsize=None)
def seed_oracle(N, sel, ca=CA):
    q, qn1, qn2, logp2, r, d, logd = seed_in(N)
    sel = list(sel)
    B = len(sel)
    f = lambda x: t.from_numpy(x[sel]).double()      # noqa: E731
    y = f(r) + ((1.0 - f(d)) * GAMMA) * (t.min(f(qn1), f(qn2)) - ALPHA * f(logp2))
    qw = t.from_numpy(wide_q(q, sel)).double()
    rows = [co.seed_rows(qw[j], y, f(logd), ca, N) for j in range(NC)]
    n = (B + 15) // 16
    part, part_cql = t.zeros(NC, n, 3, dtype=t.float64), t.zeros(NC, n, 3, dtype=t.float64)
    for j in range(NC):
        qd, qs = qw[j, :B], qw[j, B:].reshape(B, 3 * N)
        cols = t.stack([(qd - y) ** 2, qd, y, rows[j]["lse"] - qd, qs[:, :N].sum(1), qs[:, N:2 * N].sum(1)], 1)
        for i in range(n):
            sums = cols[16 * i:16 * (i + 1)].sum(0)
            part[j, i], part_cql[j, i] = sums[:3], sums[3:]
    return t.stack([x["seed"] for x in rows]), t.stack([x["p"] for x in rows]), y, part, part_cql


def check_seed(N, sel, got):
    B, E = len(sel), 3 * N
    Bw, n = B * (1 + E), (B + 15) // 16
    seed, y, part, part_cql = got
    want_seed, want_p, want_y, want_part, want_cql = seed_oracle(N, tuple(sel))
    seed2 = seed[:NC * Bw].reshape(NC, Bw)
    devs = dict(seed=sc.rel_dev(seed2.numpy(), want_seed.numpy()), y=sc.rel_dev(y[:B].numpy(), want_y.numpy()))
    for k, name in enumerate(("sum_sq", "sum_q", "sum_y")):
        devs[name] = sc.rel_dev(part[:NC * n, k].reshape(NC, n).numpy(), want_part[:, :, k].numpy())
    for k, name in enumerate(("sum_gap", "sum_q_rand", "sum_q_pi")):
        devs[name] = sc.rel_dev(part_cql[:NC * n, k].reshape(NC, n).numpy(), want_cql[:, :, k].numpy())
    # each sampled row's softmax on its own, relative to 1
    p = seed2[:, B:].reshape(NC, B, E).double() * B / CA
    devs["softmax"] = float((p - want_p).abs().max())
    print(f"seed N={N} B={B}: " + " ".join(f"{k} {v:.2e}" for k, v in devs.items()))
    for k, v in devs.items():
        assert v < TOL, (k, v)
    assert float((p.sum(2) - 1).abs().max()) <= 1e-5
    assert t.all(seed[NC * Bw:] == CANARY) and t.all(y[B:] == CANARY), "rows past an extent were written"
    assert t.all(part[NC * n:] == CANARY) and t.all(part_cql[NC * n:] == CANARY) and t.all(part[:, 3] == CANARY) and t.all(part_cql[:, 3] == CANARY)
    assert t.all(t.isfinite(seed[:NC * Bw])) and t.all(t.isfinite(part[:NC * n, :3])) and t.all(t.isfinite(part_cql[:NC * n, :3]))


def test_the_crafted_seed_rows_are_what_they_claim():
    for N in NS:
        q, qn1, qn2, logp2, r, d, logd = seed_in(N)
        E = 3 * N
        c = q[:, :, 1:].astype(np.float64) - logd.astype(np.float64)
        assert np.all(c[:, 0].max(1) - c[:, 0].min(1) == 60) and np.all(c[:, 1] == 1.25)
        srt = np.sort(c[:, 2], 1)
        assert np.all(srt[:, -1] - srt[:, -2] >= 200) if E > 1 else True
        assert d[3] == 1 and np.all(q[:, 3, 0] == r[3])


@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("B", BS)
def test_seeds_and_sums_match_the_oracle(B, N):
    """B = 1: one launch per crafted row (rows 0 .. 3); B >= 16: rows 0 .. B - 1.  Then the crafted rows' exact claims."""
    for sel in ([[r] for r in range(4)] if B == 1 else [list(range(B))]):
        check_seed(N, sel, run_seed(N, sel))
    E = 3 * N
    seed = run_seed(N, [3] if B == 1 else range(B))[0]
    seeds_of = lambda row: [seed[j * B * (1 + E) + B + row * E:j * B * (1 + E) + B + (row + 1) * E] for j in range(NC)]     # noqa: E731
    inv_B = np.float32(1.0) / np.float32(B)
    data_row = 0 if B == 1 else 3
    for j in range(NC):           # q == y bitwise: the data row's seed is exactly -cql_alpha (1/B)
        assert float(seed[j * B * (1 + E) + data_row]) == float(np.float32(-CA) * inv_B)
    if B > 1:
        for s in seeds_of(1):     # all entries equal: the softmax is exactly uniform
            assert t.all(s == s[0]) and float(s[0]) == pytest.approx(CA / (E * B), rel=1e-6)
        for s in seeds_of(2):     # one entry dominant by 200: its seed is cql_alpha (1/B), the others' exactly 0
            assert float(s[E // 2]) == float(np.float32(CA) * inv_B) and int((s != 0).sum()) == 1


@pytest.mark.parametrize("N", NS)
def test_a_seed_row_does_not_depend_on_its_batch(N):
    """Two runs are bit-identical.  The seeds end in one multiplication by the float32 1 / B: alone (B = 1) a row's seeds
    are the values before it, and those times the float32 1 / 17 and 1 / 100 are bitwise the seeds inside those batches;
    y keeps its bits.  Moved to another position among other rows at B = 17, every output keeps its bits."""
    E = 3 * N
    s100, y100, p100, c100 = run_seed(N, range(100))
    again = run_seed(N, range(100))
    assert all(t.equal(x, z) for x, z in zip((s100, y100, p100, c100), again))
    s17, y17, _, _ = run_seed(N, range(17))
    inv = lambda B: t.tensor(np.float32(1.0) / np.float32(B))     # noqa: E731  (the launch's 1/B)

    def row_of(seed, B, row):
        Bw = B * (1 + E)
        return t.cat([t.cat([seed[j * Bw + row:j * Bw + row + 1], seed[j * Bw + B + row * E:j * Bw + B + (row + 1) * E]]) for j in range(NC)])

    for row in (0, 1, 2, 3, 16):
        s1, y1, _, _ = run_seed(N, [row])
        alone = row_of(s1, 1, 0)
        assert t.equal(alone * inv(17), row_of(s17, 17, row)) and t.equal(alone * inv(100), row_of(s100, 100, row)), row
        assert t.equal(y1[0], y17[row]) and t.equal(y1[0], y100[row]), row
        others, pos = list(range(40, 56)), 9
        sm, ym, _, _ = run_seed(N, others[:pos] + [row] + others[pos:])
        assert t.equal(row_of(sm, 17, pos), row_of(s17, 17, row)) and t.equal(ym[pos], y17[row]), row


def test_without_a_penalty_weight_the_seed_is_the_td_seed():
    """cql_alpha = 0: the sampled rows' seeds are exactly 0, the data rows' are 2 (q - y) / B."""
    N, B = 4, 17
    seed, y, _, _ = run_seed(N, range(B), ca=0.0)
    want = seed_oracle(N, tuple(range(B)), 0.0)[0]
    Bw = B * (1 + 3 * N)
    for j in range(NC):
        assert t.all(seed[j * Bw + B:(j + 1) * Bw] == 0)
        assert sc.rel_dev(seed[j * Bw:j * Bw + B].numpy(), want[j, :B].numpy()) < TOL


def test_the_entry_points_refuse_bad_arguments():
    lib = _capi.load()
    x = t.zeros(4096, device="cuda")
    p = _capi.ptr(x)
    for B, S_, A, N in ((0, 3, 2, 2), (4, 0, 2, 2), (4, 3, 0, 2), (4, 3, 2, 0), (4, 3, 2, 17), (2 ** 26, 16, 2, 1)):
        rc = lib.oprl_cql_rows(p, p, p, p, None, None, 0, 0, B, S_, A, N, p, p, p, None)
        assert rc == -1 and len(lib.oprl_last_error()) > 0, (B, S_, A, N)
    assert lib.oprl_cql_rows(None, p, p, p, None, None, 0, 0, 4, 3, 2, 2, p, p, p, None) == -1
    assert lib.oprl_cql_rows(p, p, p, p, None, None, 0, 0, 4, 3, 2, 2, p, p, None, None) == -1
    for nc, B, N, ca in ((0, 4, 2, 5.0), (99, 4, 2, 5.0), (2, 0, 2, 5.0), (2, 4, 0, 5.0), (2, 4, 17, 5.0), (2, 4, 2, -1.0),
                         (2, 4, 2, float("nan")), (2, 4, 2, float("inf")), (2, 2 ** 29, 1, 5.0)):
        rc = lib.oprl_cql_seed(p, p, p, p, p, p, p, ALPHA, GAMMA, ca, nc, B, N, p, p, p, p, None)
        assert rc == -1 and len(lib.oprl_last_error()) > 0, (nc, B, N, ca)
    assert lib.oprl_cql_seed(None, p, p, p, p, p, p, ALPHA, GAMMA, CA, 2, 4, 2, p, p, p, p, None) == -1
    assert lib.oprl_cql_seed(p, p, p, p, p, p, p, ALPHA, GAMMA, CA, 2, 4, 2, p, p, p, None, None) == -1
    t.cuda.synchronize()
    assert t.all(x == 0)
