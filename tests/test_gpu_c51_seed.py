"""k_c51_critic_seed alone (csrc/c51_seed.hip, through oprl_c51_seed) against tests/d4pg_oracle.py in float64: the
projected target distribution m, the seed (softmax(z) - m) / B and the per-row cross-entropy, on rows crafted to reach
the projection's corners; and what the kernel must leave alone.

Every atom grid here has the spacing 0.5 (v_min = -4), which float32 and float64 both hold exactly, so that "r on an
atom" is an integer fractional index in the kernel and in the oracle alike."""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch as t

from oprl_amd import _capi
from tests import d4pg_oracle as do
from tests import scenarios as sc

pytestmark = pytest.mark.gpu

TOL = 2e-5                 # the suite's output gate (tests/test_gpu_algos.py)
GAMMA = 0.99
V_MIN, DELTA = -4.0, 0.5
KINDS = ("on_atom", "between", "above", "below", "squeezed", "spread")
CANARY = 12345.678
BS, NS = (1, 16, 17, 100), (2, 5, 41, 48)


def v_max(N):
    return V_MIN + (N - 1) * DELTA


def ld_of(N):
    return (N + 3) // 4 * 4          # the learner's row stride (ldq)


@functools.lru_cache(maxsize=None)
def rows(N):
    """100 rows (zt, z, r, d) in float32; row b is of kind KINDS[b % 6] for b < 12, the rest are random."""
    rs = np.random.RandomState(900 + N)
    B = 100
    zt = (2.0 * rs.standard_normal((B, N))).astype(np.float32)
    z = (2.0 * rs.standard_normal((B, N))).astype(np.float32)
    r = rs.uniform(V_MIN - 1.0, v_max(N) + 1.0, B).astype(np.float32)
    d = (rs.uniform(0, 1, B) < 0.2).astype(np.float32)
    span = v_max(N) - V_MIN
    for b in range(12):
        kind = KINDS[b % 6]
        k = (b // 6 + N // 2) % N                                  # an atom in the middle
        if kind == "on_atom":
            r[b], d[b] = V_MIN + k * DELTA, 1.0
        elif kind == "between":
            r[b], d[b] = V_MIN + min(k, N - 2) * DELTA + 0.3 * DELTA, 1.0
        elif kind == "above":
            r[b], d[b] = v_max(N) + 100.0, 0.0
        elif kind == "below":
            r[b], d[b] = V_MIN - 100.0, 0.0
        elif kind == "squeezed":                                   # gamma (1 - d) = 0.0495: the atoms land within 5 % of the grid
            d[b] = 0.95
            g = (1.0 - 0.95) * GAMMA
            r[b] = V_MIN + 0.4 * span - g * V_MIN
        else:                                                      # logits from -30 to 30
            zt[b] = rs.uniform(-30, 30, N)
            z[b] = rs.uniform(-30, 30, N)
            zt[b, 0], zt[b, N - 1], z[b, N - 1], z[b, 0] = -30.0, 30.0, -30.0, 30.0
            # (p' peaks on the last atom and, with this r, stays at that end; p peaks on the first: a seed of order one.
            # With both peaks on one atom the true seed is 1e-11 all over, below what float32 can tell from p = 1, and a
            # one-row comparison relative to its own largest entry would ask for exactly that.)
            r[b], d[b] = 0.25 * DELTA, 0.0
    return zt, z, r, d


def test_the_crafted_rows_are_what_they_claim():
    """In float64, from the rows' float32 values: integer b, fractional b, all mass on the last / the first atom,
    several source atoms between one pair of target atoms, logits 60 apart."""
    for N in NS:
        zt, z, r, d = (t.from_numpy(x).double() for x in rows(N))
        zs = do.atoms(N, V_MIN, v_max(N))
        assert t.equal(zs.float().double(), zs), "the atoms are float32 numbers"
        b = do.fractional_index(r, d, GAMMA, zs, V_MIN, v_max(N))
        m = do.project_scatter(t.softmax(zt, 1), b)
        for row in range(12):
            kind = KINDS[row % 6]
            if kind == "on_atom":
                assert d[row] == 1 and t.all(b[row] == b[row, 0]) and b[row, 0] == b[row, 0].round()
                assert float(m[row].max()) == pytest.approx(1.0, abs=1e-12)
            elif kind == "between":
                assert d[row] == 1 and 0.2 < float(b[row, 0] - b[row, 0].floor()) < 0.4
                assert int((m[row] > 0).sum()) == 2
            elif kind == "above":
                assert t.all(b[row] == N - 1) and float(m[row, N - 1]) == pytest.approx(1.0, abs=1e-12)
            elif kind == "below":
                assert t.all(b[row] == 0) and float(m[row, 0]) == pytest.approx(1.0, abs=1e-12)
            elif kind == "squeezed":
                fl = b[row].floor()
                assert 0 < float(b[row].max() - b[row].min()) < 0.05 * N
                assert max(int((fl == v).sum()) for v in fl.unique()) >= 2
            else:
                assert float(z[row].max() - z[row].min()) == 60 and float(zt[row].max() - zt[row].min()) == 60
                assert int(m[row].argmax()) >= N - 2 and int(z[row].argmax()) == 0


def run_kernel(N, sel, extra=2):
    """The kernel on the rows `sel` of rows(N), in buffers with `extra` canary rows behind them and NaN in the input
    pad columns.  Returns (seed, m, loss) as float32 CPU tensors of all B + extra rows."""
    zt, z, r, d = rows(N)
    B, ld = len(sel), ld_of(N)

    def padded(x):
        out = np.full((B + extra, ld), np.nan, np.float32)
        out[:B, :N] = x[sel]
        return t.from_numpy(out).cuda()

    dzt, dz = padded(zt), padded(z)
    dr, dd = t.from_numpy(r[sel]).cuda(), t.from_numpy(d[sel]).cuda()
    seed = t.full((B + extra, ld), CANARY, dtype=t.float32, device="cuda")
    m = t.full((B + extra, ld), CANARY, dtype=t.float32, device="cuda")
    loss = t.full((B + extra,), CANARY, dtype=t.float32, device="cuda")
    _capi.check(_capi.load().oprl_c51_seed(_capi.ptr(dzt), _capi.ptr(dz), _capi.ptr(dr), _capi.ptr(dd), GAMMA, V_MIN,
                                            v_max(N), N, B, ld, _capi.ptr(seed), _capi.ptr(m), _capi.ptr(loss),
                                            _capi.current_stream()), "oprl_c51_seed")
    t.cuda.synchronize()
    return seed.cpu(), m.cpu(), loss.cpu()


@functools.lru_cache(maxsize=None)
def oracle(N, sel):
    zt, z, r, d = (t.from_numpy(x[list(sel)]).double() for x in rows(N))
    return do.critic_seed(zt, z, r, d, GAMMA, V_MIN, v_max(N))


def check_against_oracle(N, sel, got):
    B = len(sel)
    seed, m, loss = got
    want_seed, want_m, want_loss = oracle(N, tuple(sel))
    devs = dict(seed=sc.rel_dev(seed[:B, :N].numpy(), want_seed.numpy()), m=sc.rel_dev(m[:B, :N].numpy(), want_m.numpy()),
                loss=sc.rel_dev(loss[:B].numpy(), want_loss.numpy()))
    sums = float((m[:B, :N].double().sum(1) - 1).abs().max())
    print(f"N={N} B={B}: rel dev seed {devs['seed']:.2e} m {devs['m']:.2e} loss {devs['loss']:.2e}; max |sum m - 1| {sums:.2e}")
    for k, v in devs.items():
        assert v < TOL, (k, v)
    assert sums <= 1e-5
    assert t.all(seed[:B, N:] == 0) and t.all(m[:B, N:] == 0), "pad columns"
    assert t.all(seed[B:] == CANARY) and t.all(m[B:] == CANARY) and t.all(loss[B:] == CANARY), "rows past B were written"
    assert t.all(t.isfinite(seed[:B])) and t.all(t.isfinite(loss[:B]))


@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("B", BS)
def test_seed_m_and_loss_match_the_oracle(B, N):
    """B = 1: one launch per crafted kind (rows 0 .. 5); B >= 16: rows 0 .. B - 1, which hold every kind twice."""
    if B == 1:
        for row in range(6):
            check_against_oracle(N, [row], run_kernel(N, [row]))
        return
    check_against_oracle(N, list(range(B)), run_kernel(N, list(range(B))))


@pytest.mark.parametrize("N", NS)
def test_a_row_does_not_depend_on_its_batch(N):
    """Rows 0 .. 5 (the crafted kinds) and row 16 (the first of a second slice): m and the loss are bitwise the same alone,
    inside B = 17 and inside B = 100.  The seed is (p - m) times the float32 1 / B, one last multiplication: alone
    (B = 1) it is p - m itself, and that times the float32 1 / 17 and 1 / 100 is bitwise the seed inside those batches.
    Moved to another position among other rows at B = 17, every output keeps its bits."""
    s100, m100, l100 = run_kernel(N, list(range(100)))
    s17, m17, l17 = run_kernel(N, list(range(17)))
    assert t.equal(m100[:17], m17[:17]) and t.equal(l100[:17], l17[:17])
    inv = lambda B: t.tensor(np.float32(1.0) / np.float32(B))     # noqa: E731  (the launch's inv_B)
    for row in (0, 1, 2, 3, 4, 5, 16):
        s1, m1, l1 = run_kernel(N, [row])
        assert t.equal(m1[0], m17[row]) and t.equal(m1[0], m100[row]), row
        assert t.equal(l1[0], l17[row]) and t.equal(l1[0], l100[row]), row
        assert t.equal(s1[0] * inv(17), s17[row]) and t.equal(s1[0] * inv(100), s100[row]), row
        others, pos = list(range(40, 56)), 9
        sm, mm, lm = run_kernel(N, others[:pos] + [row] + others[pos:])
        assert t.equal(sm[pos], s17[row]) and t.equal(mm[pos], m17[row]) and t.equal(lm[pos], l17[row]), row


def test_the_entry_point_refuses_bad_arguments():
    lib = _capi.load()
    x = t.zeros(64, device="cuda")
    p = _capi.ptr(x)
    for args in ((1, 4, 4), (49, 4, 52), (5, 4, 4), (5, 0, 8), (5, 4, 68)):       # (N, B, ld)
        N, B, ld = args
        rc = lib.oprl_c51_seed(p, p, p, p, GAMMA, -1.0, 1.0, N, B, ld, p, p, p, None)
        assert rc == -1 and len(lib.oprl_last_error()) > 0, args
    assert lib.oprl_c51_seed(p, p, p, p, GAMMA, 1.0, 1.0, 5, 4, 8, p, p, p, None) == -1
    assert lib.oprl_c51_seed(None, p, p, p, GAMMA, -1.0, 1.0, 5, 4, 8, p, p, p, None) == -1
