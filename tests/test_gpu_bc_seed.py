"""k_bc_seed / k_bc_mix (csrc/bc_seed.hip) alone, through oprl_bc_seed, against float64.

The rows are crafted for what the kernels can get wrong: q comes in pairs (m, -m (1 + 1e-4)) in shuffled order with m
log-uniform over 1e-3 .. 1e3, so that sum q is about 1e-4 of sum |q| — a kernel that normalised by |mean q| instead of
mean |q| would be off by four orders of magnitude — and B = 1025 forces a second, ragged pass of the strided sum.

Gates: the project's output gate, 2e-5 relative to the key's largest reference entry, for lambda, mean |q|, the seed
rows, the mixed action gradients and the sums of squares.  The per-slice sums of q cancel by construction, and a float32
sum of 16 terms cannot be nearer to the exact one than a few eps of the sum of their MAGNITUDES, so that key is gated
at 2e-5 of the largest per-slice sum of |q|."""
from __future__ import annotations

import numpy as np
import pytest
import torch as t

from oprl_amd import _capi

pytestmark = pytest.mark.gpu

TOL = 2e-5
ALPHA = 2.5
SENTINEL = 777.0
PAD = 40                      # floats behind every output's extent that must stay untouched
SHAPES = [(B, A) for B in (1, 16, 17, 100, 1025) for A in (1, 6, 21)]


def crafted_q(B: int) -> np.ndarray:
    rs = np.random.RandomState(B)
    if B == 1:
        return np.array([-0.37], np.float32)
    m = 10.0 ** rs.uniform(-3, 3, B // 2)
    m[0], m[-1] = 1e-3, 1e3                              # the whole span, whatever was drawn
    q = np.concatenate([m, -m * (1 + 1e-4), [1e-3] * (B % 2)])
    return q[rs.permutation(B)].astype(np.float32)


def inputs(B: int, A: int):
    rs = np.random.RandomState(1000 * A + B)
    pi = np.tanh(rs.standard_normal((B, A))).astype(np.float32)
    a = rs.uniform(-1, 1, (B, A)).astype(np.float32)
    da = (rs.standard_normal((B, A)) * 10.0 ** rs.uniform(-4, 0, (B, 1))).astype(np.float32)
    return crafted_q(B), pi, a, da


def padded(x: np.ndarray | None, n: int) -> t.Tensor:
    """n + PAD floats on the device: x first (or sentinels), sentinels behind."""
    buf = t.full((n + PAD,), SENTINEL, dtype=t.float32, device="cuda")
    if x is not None:
        buf[:n] = t.from_numpy(x.reshape(-1)).cuda()
    return buf


def run(B: int, A: int, alpha: float = ALPHA):
    q, pi, a, da = inputs(B, A)
    n_sl, n_mix = (B + 15) // 16, (B * A + 15) // 16
    dev = dict(q=padded(q, B), pi=padded(pi, B * A), a=padded(a, B * A), da=padded(da, B * A), seed=padded(None, B),
               scal=padded(None, 4), part_q=padded(None, 4 * n_sl), part_sq=padded(None, n_mix))
    rc = _capi.load().oprl_bc_seed(*(_capi.ptr(dev[k]) for k in ("q", "pi", "a", "da")), alpha, B, A,
                                   *(_capi.ptr(dev[k]) for k in ("seed", "scal", "part_q", "part_sq")), _capi.current_stream())
    _capi.check(rc, "oprl_bc_seed")
    t.cuda.synchronize()
    return (q, pi, a, da), {k: v.cpu().numpy() for k, v in dev.items()}


def rel(got, want, scale=None) -> float:
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.abs(got - want).max() / max(np.abs(want).max() if scale is None else scale, 1e-300))


@pytest.mark.parametrize("B,A", SHAPES, ids=[f"B{b}-A{a}" for b, a in SHAPES])
def test_bc_seed_against_float64(B, A):
    (q, pi, a, da), out = run(B, A)
    n_sl, n_mix = (B + 15) // 16, (B * A + 15) // 16
    q64, pi64, a64, da64 = (x.astype(np.float64) for x in (q, pi, a, da))
    if B > 1:
        assert abs(q64.sum()) < 1e-3 * np.abs(q64).sum()            # the rows are what the docstring says
        assert np.abs(q64).min() <= 1.001e-3 and np.abs(q64).max() >= 0.999e3
    mean_abs = np.abs(q64).mean()
    lam = ALPHA / mean_abs
    pad = lambda x, n: np.concatenate([x, np.zeros(n - len(x))])      # noqa: E731
    q_sl = pad(q64, 16 * n_sl).reshape(n_sl, 16)
    part_q = out["part_q"][:4 * n_sl].reshape(n_sl, 4)
    devs = {
        "lambda": rel(out["scal"][0], lam),
        "mean |q|": rel(out["scal"][1], mean_abs),
        "seed": rel(out["seed"][:B], np.full(B, -lam / B)),
        "sum q per slice": rel(part_q[:, 1], q_sl.sum(1), scale=np.abs(q_sl).sum(1).max()),
        "da": rel(out["da"][:B * A], (da64 + (2.0 / (B * A)) * (pi64 - a64)).reshape(-1)),
        "sum (pi - a)^2 per slice": rel(out["part_sq"][:n_mix], pad(((pi64 - a64) ** 2).reshape(-1), 16 * n_mix).reshape(n_mix, 16).sum(1)),
    }
    print(f"B={B} A={A}: " + ", ".join(f"{k} {v:.2e}" for k, v in devs.items()))
    for k, v in devs.items():
        assert v <= TOL, f"{k}: rel dev {v:.3e} > {TOL:.0e}"
    # columns 0 and 2 of a slice's partial sums are written as zeros, column 3 is nobody's
    assert np.all(part_q[:, 0] == 0) and np.all(part_q[:, 2] == 0) and np.all(part_q[:, 3] == SENTINEL)
    # nothing is written past the extents, the spare scalars are left alone and the inputs are only read
    for k, n in (("seed", B), ("scal", 2), ("part_q", 4 * n_sl), ("part_sq", n_mix), ("da", B * A), ("q", B),
                 ("pi", B * A), ("a", B * A)):
        assert np.all(out[k][n:] == SENTINEL), f"{k}: written past {n}"
    assert np.array_equal(out["q"][:B], q) and np.array_equal(out["pi"][:B * A], pi.reshape(-1))
    assert np.array_equal(out["a"][:B * A], a.reshape(-1))


@pytest.mark.parametrize("B,A", [(17, 6), (1025, 21)], ids=["B17-A6", "B1025-A21"])
def test_two_runs_are_bit_identical(B, A):
    _, x = run(B, A)
    _, y = run(B, A)
    for k in x:
        assert np.array_equal(x[k], y[k]), k


def test_lambda_scales_with_alpha():
    """alpha = 0.5 gives a fifth of alpha = 2.5's lambda to rounding; mean |q|, the sums of q and k_bc_mix's outputs do
    not depend on alpha."""
    _, x = run(100, 6, alpha=2.5)
    _, y = run(100, 6, alpha=0.5)
    assert y["scal"][0] == pytest.approx(x["scal"][0] / 5, rel=1e-6) and y["scal"][1] == x["scal"][1]
    assert np.array_equal(x["part_q"], y["part_q"]) and np.array_equal(x["da"], y["da"])


def test_bad_arguments_are_refused_before_any_launch():
    lib = _capi.load()
    z = t.zeros(64, device="cuda")
    p = _capi.ptr(z)
    for alpha, B, A in ((0.0, 4, 2), (-1.0, 4, 2), (float("nan"), 4, 2), (float("inf"), 4, 2), (2.5, 0, 2), (2.5, 4, 0)):
        assert lib.oprl_bc_seed(p, p, p, p, alpha, B, A, p, p, p, p, _capi.current_stream()) == -1
        assert b"oprl_bc_seed" in lib.oprl_last_error()
    t.cuda.synchronize()
    assert float(z.abs().max()) == 0.0
