"""The calibrated k_cql_seed alone (csrc/cql_seed.hip, through oprl_cql_seed_cal) against
tests/calql_oracle.py in float64, on tests/test_gpu_cql_seed.py's rows (crafted ones among them) and at its gate for the
same outputs — 2e-5 relative to each key's largest reference entry — with returns-to-go on the scale of the critics'
values, so that some policy entries are bounded and some are not; the count of bounded entries exactly; and the bound's
ends: g = -inf is the plain kernel bit for bit, g = 1e30 zeroes every policy entry's seed, q == g keeps its gradient."""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch as t

from oprl_amd import _capi
from tests import calql_oracle as cal
from tests import scenarios as sc
from tests.test_gpu_cql_seed import ALPHA, CA, CANARY, GAMMA, TOL, dev, seed_in

pytestmark = pytest.mark.gpu

BS, NS, NCS = (1, 16, 17, 100), (1, 2, 16), (1, 2)
EQ_ROW = 5            # the row whose g is, bitwise, critic 0's value at its first policy entry


@functools.lru_cache(maxsize=None)
def returns_in(N):
    """g [100] float32 on the scale of q (2 N(0, 1)): about half of the policy entries lie under it."""
    g = (2.0 * np.random.RandomState(900 + N).standard_normal(100)).astype(np.float32)
    g[EQ_ROW] = seed_in(N)[0][0, EQ_ROW, 1 + N]
    return g


def wide_q(q, sel, nc):
    x = q[:nc, list(sel)]
    return np.concatenate([x[:, :, 0], x[:, :, 1:].reshape(nc, -1)], 1)


def run(N, sel, nc, g=None, extra=2, plain=False):
    """oprl_cql_seed_cal (plain: oprl_cql_seed) on the rows `sel`: NaN behind every input, canaries behind every output."""
    q, qn1, qn2, logp2, r, d, logd = seed_in(N)
    sel = list(sel)
    B, E = len(sel), 3 * N
    Bw, n = B * (1 + E), (B + 15) // 16
    dq = dev(np.concatenate([wide_q(q, sel, nc).reshape(-1), np.full(extra, np.nan, np.float32)]))
    pad = lambda x: dev(np.concatenate([x[sel].reshape(-1), np.full(extra, np.nan, np.float32)]))      # noqa: E731
    d1, d2, dl, dr, dd, dld = (pad(x) for x in (qn1, qn2, logp2, r, d, logd))
    seed = t.full((nc * Bw + extra,), CANARY, dtype=t.float32, device="cuda")
    y = t.full((B + extra,), CANARY, dtype=t.float32, device="cuda")
    part = t.full((nc * n + 1, 4), CANARY, dtype=t.float32, device="cuda")
    part_cql = t.full((nc * n + 1, 4), CANARY, dtype=t.float32, device="cuda")
    head = (_capi.ptr(dq), _capi.ptr(d1), _capi.ptr(d2), _capi.ptr(dl), _capi.ptr(dr), _capi.ptr(dd), _capi.ptr(dld), ALPHA, GAMMA, CA,
            nc, B, N, _capi.ptr(seed), _capi.ptr(y), _capi.ptr(part), _capi.ptr(part_cql))
    lib = _capi.load()
    if plain:
        _capi.check(lib.oprl_cql_seed(*head, _capi.current_stream()), "oprl_cql_seed")
    else:
        dg = dev(np.concatenate([np.asarray(g, np.float32)[sel] if np.ndim(g) else np.full(B, g, np.float32), np.full(extra, np.nan, np.float32)]))
        _capi.check(lib.oprl_cql_seed_cal(*head, _capi.ptr(dg), _capi.current_stream()), "oprl_cql_seed_cal")
    t.cuda.synchronize()
    return seed.cpu(), y.cpu(), part.cpu(), part_cql.cpu()


def oracle(N, sel, nc, g):
    q, qn1, qn2, logp2, r, d, logd = seed_in(N)
    sel = list(sel)
    B = len(sel)
    f = lambda x: t.from_numpy(x[sel]).double()      # noqa: E731
    y = f(r) + ((1.0 - f(d)) * GAMMA) * (t.min(f(qn1), f(qn2)) - ALPHA * f(logp2))
    qw = t.from_numpy(wide_q(q, sel, nc)).double()
    gd = t.from_numpy(np.asarray(g, np.float32)[sel]).double()
    rows = [cal.seed_rows(qw[j], y, f(logd), gd, CA, N) for j in range(nc)]
    n = (B + 15) // 16
    part, part_cql = t.zeros(nc, n, 3, dtype=t.float64), t.zeros(nc, n, 4, dtype=t.float64)
    for j in range(nc):
        qd, qs = qw[j, :B], qw[j, B:].reshape(B, 3 * N)
        cnt = (qs[:, N:] < gd.reshape(B, 1)).sum(1).double()
        cols = t.stack([(qd - y) ** 2, qd, y, rows[j]["lse"] - qd, qs[:, :N].sum(1), qs[:, N:2 * N].sum(1), cnt], 1)
        for i in range(n):
            sums = cols[16 * i:16 * (i + 1)].sum(0)
            part[j, i], part_cql[j, i] = sums[:3], sums[3:]
    return t.stack([x["seed"] for x in rows]), y, part, part_cql, sum(x["bound"] for x in rows)


def check(N, sel, nc, got):
    B, E = len(sel), 3 * N
    Bw, n = B * (1 + E), (B + 15) // 16
    seed, y, part, part_cql = got
    g = returns_in(N)
    want_seed, want_y, want_part, want_cql, bound = oracle(N, sel, nc, g)
    seed2 = seed[:nc * Bw].reshape(nc, Bw)
    devs = dict(seed=sc.rel_dev(seed2.numpy(), want_seed.numpy()), y=sc.rel_dev(y[:B].numpy(), want_y.numpy()))
    for k, name in enumerate(("sum_sq", "sum_q", "sum_y")):
        devs[name] = sc.rel_dev(part[:nc * n, k].reshape(nc, n).numpy(), want_part[:, :, k].numpy())
    for k, name in enumerate(("sum_gap", "sum_q_rand", "sum_q_pi")):
        devs[name] = sc.rel_dev(part_cql[:nc * n, k].reshape(nc, n).numpy(), want_cql[:, :, k].numpy())
    print(f"calibrated seed N={N} B={B} nc={nc}: " + " ".join(f"{k} {v:.2e}" for k, v in devs.items()) + f"; bounded {bound} of {nc * B * 2 * N}")
    for k, v in devs.items():
        assert v < TOL, (k, v)
    # the count of bounded entries per slice, exactly (the comparison is one of float32 inputs); their seeds are exactly 0
    assert t.equal(part_cql[:nc * n, 3].reshape(nc, n).double(), want_cql[:, :, 3])
    qs = t.from_numpy(wide_q(seed_in(N)[0], sel, nc))[:, B:].reshape(nc, B, E)
    bounded = qs < t.from_numpy(g[list(sel)]).reshape(1, B, 1)
    bounded[:, :, :N] = False
    assert int(bounded.sum()) == bound and t.all(seed2[:, B:].reshape(nc, B, E)[bounded] == 0)
    assert t.all(seed[nc * Bw:] == CANARY) and t.all(y[B:] == CANARY), "rows past an extent were written"
    assert t.all(part[nc * n:] == CANARY) and t.all(part_cql[nc * n:] == CANARY) and t.all(part[:, 3] == CANARY)
    assert t.all(t.isfinite(seed[:nc * Bw])) and t.all(t.isfinite(part[:nc * n, :3])) and t.all(t.isfinite(part_cql[:nc * n]))
    return bound


@pytest.mark.parametrize("nc", NCS)
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("B", BS)
def test_calibrated_seeds_and_sums_match_the_oracle(B, N, nc):
    """B = 1: one launch per crafted row and the equality row; B >= 16: rows 0 .. B - 1, those rows among them."""
    total = 0
    for sel in ([[r] for r in (0, 1, 2, 3, EQ_ROW)] if B == 1 else [list(range(B))]):
        total += check(N, sel, nc, run(N, sel, nc, returns_in(N)))
    if B >= 16:
        assert 0 < total < nc * B * 2 * N          # some entries at the bound and some not


@pytest.mark.parametrize("nc", NCS)
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("B", BS)
def test_the_ends_of_the_bound(B, N, nc):
    """g = -inf: every output of oprl_cql_seed bit for bit, slot 3 aside (it counts 0).  g = 1e30: every policy entry's
    seed is exactly 0, the uniform entries' and the data rows' are finite, the count is B 2N."""
    sel = [EQ_ROW] if B == 1 else list(range(B))
    E = 3 * N
    Bw, n = B * (1 + E), (B + 15) // 16
    plain, low = run(N, sel, nc, plain=True), run(N, sel, nc, -np.inf)
    for k, (a, b) in enumerate(zip(plain[:3], low[:3])):
        assert t.equal(a.view(t.int32), b.view(t.int32)), k
    assert t.equal(plain[3][:, :3].view(t.int32), low[3][:, :3].view(t.int32))
    assert t.all(plain[3][:, 3] == CANARY), "the plain kernel leaves slot 3 alone"
    assert t.all(low[3][:nc * n, 3] == 0) and low[3][nc * n, 3] == CANARY
    seed, y, part, part_cql = run(N, sel, nc, 1e30)
    s2 = seed[:nc * Bw].reshape(nc, Bw)
    ent = s2[:, B:].reshape(nc, B, E)
    assert t.all(ent[:, :, N:] == 0) and t.all(t.isfinite(s2))
    assert t.equal(s2[:, :B].view(t.int32), plain[0][:nc * Bw].reshape(nc, Bw)[:, :B].view(t.int32))       # the data rows' seeds do not see g
    assert t.equal(y.view(t.int32), plain[1].view(t.int32))
    assert float(part_cql[:nc * n, 3].sum()) == nc * B * 2 * N
    assert t.all(t.isfinite(part_cql[:nc * n])) and t.all(seed[nc * Bw:] == CANARY)


@pytest.mark.parametrize("N", NS)
def test_an_entry_at_the_bound_keeps_its_gradient(N):
    """q_e == g_b bitwise (critic 0, the row's first policy entry): the seed is the plain kernel's, not 0, and the entry is
    not counted; an entry one ulp below is bounded."""
    q = seed_in(N)[0]
    g = returns_in(N)
    assert g[EQ_ROW] == q[0, EQ_ROW, 1 + N]
    for B, sel in ((1, [EQ_ROW]), (17, list(range(17)))):
        row, E = sel.index(EQ_ROW), 3 * N
        seed, _, _, part_cql = run(N, sel, 2, g)
        at = B + row * E + N                                        # critic 0's seed of that entry
        assert float(seed[at]) > 0
        below = (q[0, sel, 1 + N:].reshape(len(sel), -1) < g[sel].reshape(-1, 1)).sum()
        assert float(part_cql[:(B + 15) // 16, 3].sum()) == float(below)
        up = g.copy()
        up[EQ_ROW] = np.nextafter(g[EQ_ROW], np.float32(np.inf))
        seed_up, _, _, part_up = run(N, sel, 2, up)
        assert float(seed_up[at]) == 0 and float(part_up[:(B + 15) // 16, 3].sum()) == float(below) + 1


def test_the_entry_point_refuses_bad_arguments():
    lib = _capi.load()
    x = t.zeros(4096, device="cuda")
    p = _capi.ptr(x)
    for nc, B, N, ca in ((0, 4, 2, 5.0), (99, 4, 2, 5.0), (2, 0, 2, 5.0), (2, 4, 0, 5.0), (2, 4, 17, 5.0), (2, 4, 2, -1.0),
                         (2, 4, 2, float("nan")), (2, 2 ** 29, 1, 5.0)):
        rc = lib.oprl_cql_seed_cal(p, p, p, p, p, p, p, ALPHA, GAMMA, ca, nc, B, N, p, p, p, p, p, None)
        assert rc == -1 and b"oprl_cql_seed_cal" in lib.oprl_last_error(), (nc, B, N, ca)
    assert lib.oprl_cql_seed_cal(p, p, p, p, p, p, p, ALPHA, GAMMA, CA, 2, 4, 2, p, p, p, p, None, None) == -1
    assert b"returns" in lib.oprl_last_error()
    assert lib.oprl_cql_seed_cal(None, p, p, p, p, p, p, ALPHA, GAMMA, CA, 2, 4, 2, p, p, p, p, p, None) == -1
    t.cuda.synchronize()
    assert t.all(x == 0)
