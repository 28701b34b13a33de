"""k_iql_value_seed / k_iql_actor_seed (csrc/iql_seed.hip) alone, through oprl_iql_seed, against float64.

The first rows of every case are crafted for what the kernels can get wrong (B = 1 keeps the first only): an ordinary
row; qt == v bitwise (u and the seed exactly 0, and u = 0 is NOT "below": omega = tau); u = +-1e-6, +-1e-3, +-0.25 (the
sign picks omega); beta u = +-200 (exp overflows to +inf: w must be the clip; exp underflows: w must be exactly 0);
beta u 2e-3 under and 2e-3 over log c — no row lies within 1e-3 of it, asserted, so the count of rows at the clip is
exact.  The remaining rows are random with |u| < 1.2.  Which of the two target rows holds the minimum alternates.

Gates: the project's output gate, 2e-5 relative to the key's largest reference entry, for u, the seed rows, w, the action
gradients and every per-slice sum; the count of rows at the clip is exact.  Because that gate says little about a small
entry next to a large one, each row is also held on its own: u is the float32 difference bitwise, the seed's ratio to
2 (v - qt) / B is omega to 1e-5, and w is within 2e-5 of its own reference (float32 expf is good to a few ulp, 2.4e-7,
and the rounding of beta u moves exp by at most 6e-8 |beta u| <= 3e-7 relative below the clip: a hundredth of that)."""
from __future__ import annotations

import math

import numpy as np
import pytest
import torch as t

from oprl_amd import _capi

pytestmark = pytest.mark.gpu

TOL = 2e-5
BETA, CLIP = 3.0, 100.0
SENTINEL = 777.0
PAD = 40                      # floats behind every output's extent that must stay untouched
CASES = [(B, A, tau) for B in (1, 16, 17, 100) for A in (1, 6) for tau in (0.5, 0.7, 0.9)]
OUT = ("u", "seed", "w", "da", "part_v", "part_w", "part_a")


def crafted_u(beta: float = BETA, clip: float = CLIP) -> list[float]:
    lc = math.log(clip)
    return [0.37, 0.0, 1e-6, -1e-6, 1e-3, -1e-3, 0.25, -0.25, 200.0 / beta, -200.0 / beta, (lc - 2e-3) / beta, (lc + 2e-3) / beta]


def inputs(B: int, A: int):
    rs = np.random.RandomState(1000 * A + B)
    u = np.concatenate([crafted_u(), rs.uniform(-1.2, 1.2, max(B - 12, 0))])[:B]
    v = rs.standard_normal(B).astype(np.float32)
    qt = (v.astype(np.float64) + u).astype(np.float32)
    qt[u == 0.0] = v[u == 0.0]
    other = (qt + rs.uniform(0.01, 1.0, B).astype(np.float32)).astype(np.float32)
    first = np.arange(B) % 2 == 0
    q1, q2 = np.where(first, qt, other).astype(np.float32), np.where(first, other, qt).astype(np.float32)
    pi = np.tanh(rs.standard_normal((B, A))).astype(np.float32)
    a = rs.uniform(-1, 1, (B, A)).astype(np.float32)
    return q1, q2, v, pi, a


def padded(x: np.ndarray | None, n: int) -> t.Tensor:
    """n + PAD floats on the device: x first (or sentinels), sentinels behind."""
    buf = t.full((n + PAD,), SENTINEL, dtype=t.float32, device="cuda")
    if x is not None:
        buf[:n] = t.from_numpy(np.ascontiguousarray(x).reshape(-1)).cuda()
    return buf


def extents(B: int, A: int) -> dict:
    n_sl = (B + 15) // 16
    return dict(q1=B, q2=B, v=B, pi=B * A, a=B * A, u=B, seed=B, w=B, da=B * A, part_v=4 * n_sl, part_w=4 * n_sl, part_a=4 * n_sl)


def run(rows, B: int, A: int, tau: float, beta: float = BETA, clip: float = CLIP):
    ext = extents(B, A)
    dev = {k: padded(x, ext[k]) for k, x in zip(("q1", "q2", "v", "pi", "a"), rows)}
    dev.update({k: padded(None, ext[k]) for k in OUT})
    rc = _capi.load().oprl_iql_seed(*(_capi.ptr(dev[k]) for k in ("q1", "q2", "v", "pi", "a")), tau, beta, clip, B, A,
                                    *(_capi.ptr(dev[k]) for k in OUT), _capi.current_stream())
    _capi.check(rc, "oprl_iql_seed")
    t.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in dev.items()}


def reference(rows, B: int, A: int, tau: float, beta: float = BETA, clip: float = CLIP) -> dict:
    q1, q2, v, pi, a = (x.astype(np.float64) for x in rows)
    n_sl = (B + 15) // 16
    qt = np.minimum(q1, q2)
    u = qt - v
    omega = np.where(u < 0, 1.0 - tau, tau)
    e = np.exp(beta * u)
    w = np.minimum(e, clip)
    at_clip = (e >= clip).astype(np.float64)
    sl = lambda x: np.concatenate([x, np.zeros(16 * n_sl - B)]).reshape(n_sl, 16).sum(1)      # noqa: E731
    return dict(u=u, omega=omega, seed=2.0 * (v - qt) / B * omega, w=w, at_clip=at_clip, e=e,
                da=(2.0 / B) * w[:, None] * (pi - a),
                part_v=np.stack([sl(omega * u * u), sl(v), sl(u)], 1), part_w=np.stack([sl(w), sl(at_clip)], 1),
                part_a=sl(w * ((pi - a) ** 2).sum(1)))


def rel(got, want) -> float:
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-300))


@pytest.mark.parametrize("B,A,tau", CASES, ids=[f"B{b}-A{a}-tau{x}" for b, a, x in CASES])
def test_iql_seed_against_float64(B, A, tau):
    rows = inputs(B, A)
    out, ref = run(rows, B, A, tau), reference(rows, B, A, tau)
    q1, q2, v, pi, a = rows
    n_sl = (B + 15) // 16
    # the rows are what the docstring says
    assert np.abs(BETA * ref["u"] - math.log(CLIP)).min() > 1e-3
    if B >= 12:
        assert ref["u"][1] == 0.0 and (ref["u"] > 0).any() and (ref["u"] < 0).any()
        assert 1e-7 < ref["u"][2] < 2e-6 and -2e-6 < ref["u"][3] < -1e-7
        assert ref["at_clip"].sum() >= 2 and ref["e"][9] < 1e-60 and np.isfinite(ref["e"]).all() and ref["e"][8] > 1e80
        assert ref["at_clip"][10] == 0.0 and ref["at_clip"][11] == 1.0
    part_v, part_w, part_a = (out[k][:4 * n_sl].reshape(n_sl, 4) for k in ("part_v", "part_w", "part_a"))
    devs = {
        "u": rel(out["u"][:B], ref["u"]),
        "seed": rel(out["seed"][:B], ref["seed"]),
        "w": rel(out["w"][:B], ref["w"]),
        "da": rel(out["da"][:B * A], ref["da"].reshape(-1)),
        "sum omega u^2 per slice": rel(part_v[:, 0], ref["part_v"][:, 0]),
        "sum v per slice": rel(part_v[:, 1], ref["part_v"][:, 1]),
        "sum u per slice": rel(part_v[:, 2], ref["part_v"][:, 2]),
        "sum w per slice": rel(part_w[:, 1], ref["part_w"][:, 0]),
        "sum w (pi - a)^2 per slice": rel(part_a[:, 1], ref["part_a"]),
    }
    print(f"B={B} A={A} tau={tau}: " + ", ".join(f"{k} {x:.2e}" for k, x in devs.items()))
    for k, x in devs.items():
        assert x <= TOL, f"{k}: rel dev {x:.3e} > {TOL:.0e}"
    # the count of rows at the clip is exact
    assert np.array_equal(part_w[:, 2].astype(np.float64), ref["part_w"][:, 1])
    # row by row: u is the float32 difference, 0 where qt == v; the seed carries the row's omega; w on its own scale
    qt32 = np.minimum(q1, q2)
    assert np.array_equal(out["u"][:B], qt32 - v)
    zero = qt32 == v
    assert np.all(out["seed"][:B][zero] == 0.0) and np.all(out["u"][:B][zero] == 0.0)
    nz = ~zero
    ratio = out["seed"][:B][nz].astype(np.float64) / (2.0 * (v[nz].astype(np.float64) - qt32[nz]) / B)
    assert np.abs(ratio / ref["omega"][nz] - 1.0).max() <= 1e-5 if nz.any() else True
    under = ref["e"] < 1e-60
    assert np.all(out["w"][:B][under] == 0.0)                                   # exp underflows: exactly 0
    assert np.all(out["w"][:B][ref["at_clip"] == 1.0] == np.float32(CLIP))       # at the clip (+inf included): exactly c
    mid = ~under
    assert np.abs(out["w"][:B][mid] / ref["w"][mid] - 1.0).max() <= TOL
    assert np.isfinite(out["w"][:B]).all() and np.isfinite(out["da"][:B * A]).all()
    # the first column of the second and third tables and the third of the third are zeros, column 3 is nobody's
    assert np.all(part_w[:, 0] == 0) and np.all(part_a[:, 0] == 0) and np.all(part_a[:, 2] == 0)
    for p in (part_v, part_w, part_a):
        assert np.all(p[:, 3] == SENTINEL)
    # nothing is written past the extents and the inputs are only read
    for k, n in extents(B, A).items():
        assert np.all(out[k][n:] == SENTINEL), f"{k}: written past {n}"
    for k, x in zip(("q1", "q2", "v", "pi", "a"), rows):
        assert np.array_equal(out[k][:x.size], x.reshape(-1)), k


def test_beta_zero_gives_unit_weights():
    """beta = 0: every w is exactly 1.0f, whatever u is (the +-66 rows included), and no row is at the clip."""
    B, A = 100, 6
    rows = inputs(B, A)
    out = run(rows, B, A, 0.7, beta=0.0)
    assert np.all(out["w"][:B] == np.float32(1.0))
    n_sl = (B + 15) // 16
    part_w = out["part_w"][:4 * n_sl].reshape(n_sl, 4)
    assert np.all(part_w[:, 2] == 0.0) and part_w[:, 1].sum() == float(B)
    ref = reference(rows, B, A, 0.7, beta=0.0)
    assert rel(out["da"][:B * A], ref["da"].reshape(-1)) <= TOL


@pytest.mark.parametrize("B,A", [(17, 6), (100, 1)], ids=["B17-A6", "B100-A1"])
def test_two_runs_are_bit_identical(B, A):
    rows = inputs(B, A)
    x, y = run(rows, B, A, 0.7), run(rows, B, A, 0.7)
    for k in x:
        assert np.array_equal(x[k], y[k]), k


def test_a_rows_results_do_not_depend_on_b_or_position():
    """The rows of a B = 17 case inside a B = 100 case, at other positions and across a workgroup's slices: u and w are the
    same bits (the seed and da carry 1/B); the same B with the rows permuted permutes u, the seed, w and da bitwise."""
    A = 6
    small = inputs(17, A)
    big = inputs(100, A)
    at = np.array([3 + 5 * i for i in range(17)])          # positions 3, 8, ..., 83
    mixed = [x.copy() for x in big]
    for x, s in zip(mixed, small):
        x[at] = s
    a, b = run(small, 17, A, 0.7), run(mixed, 100, A, 0.7)
    for k in ("u", "w"):
        assert np.array_equal(a[k][:17], b[k][:100][at]), k
    perm = np.random.RandomState(3).permutation(100)
    c = run([x[perm] for x in mixed], 100, A, 0.7)
    for k in ("u", "seed", "w"):
        assert np.array_equal(c[k][:100], b[k][:100][perm]), k
    assert np.array_equal(c["da"][:100 * A].reshape(100, A), b["da"][:100 * A].reshape(100, A)[perm])


def test_bad_arguments_are_refused_before_any_launch():
    lib = _capi.load()
    z = t.zeros(64, device="cuda")
    p = _capi.ptr(z)
    nan, inf = float("nan"), float("inf")
    for tau, beta, clip, B, A, word in ((0.0, 3.0, 100.0, 4, 2, b"expectile"), (1.0, 3.0, 100.0, 4, 2, b"expectile"),
                                        (nan, 3.0, 100.0, 4, 2, b"expectile"), (0.7, -1.0, 100.0, 4, 2, b"beta"),
                                        (0.7, inf, 100.0, 4, 2, b"beta"), (0.7, nan, 100.0, 4, 2, b"beta"),
                                        (0.7, 3.0, 0.0, 4, 2, b"adv_clip"), (0.7, 3.0, -1.0, 4, 2, b"adv_clip"),
                                        (0.7, 3.0, inf, 4, 2, b"adv_clip"), (0.7, 3.0, 1e300, 4, 2, b"adv_clip"),
                                        (0.7, 3.0, 100.0, 0, 2, b"B >= 1"), (0.7, 3.0, 100.0, 4, 0, b"A >= 1")):
        assert lib.oprl_iql_seed(p, p, p, p, p, tau, beta, clip, B, A, p, p, p, p, p, p, p, _capi.current_stream()) == -1
        msg = lib.oprl_last_error()
        assert b"oprl_iql_seed" in msg and word in msg, msg
    t.cuda.synchronize()
    assert float(z.abs().max()) == 0.0
