"""k_mlp_slice_ln with dropout in front of both normalisations (csrc/ln_slice.hip) alone, through
oprl_mlp_ln_drop, against the float64 oracle of tests/droq_oracle.py, whose mask is the kernel's Philox comparison restated
in numpy: max-norm relative deviation <= 2e-5 on every output — the net's output, per hidden layer x, dz (now dL/dz, masked
and scaled) and zh, rstd, the gradient over the action columns, and the reduced dgamma | dbeta.

Shapes: inputs 17 + 6; B = 1, 16 (one full slice), 17 (the smallest batch at which a row index local to the slice gives a
wrong mask), 100 (ragged: 7 slices); rates 0.1 and 0.5.  A stream above 2^32, the mask of the neighbouring stream as a wrong
oracle, the forward-only + backward-only pair against the whole launch, run-to-run bits, untouched rows >= B, rate 0 against
oprl_mlp_ln, and the refusals."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest
import torch as t

from oprl_amd import _capi
from tests import droq_oracle as do
from tests import scenarios as sc
from tests.test_gpu_ln_slice import EPS, SENT, TOL, W, Net, check, make_case
from tests.test_redq_host import noise_key

pytestmark = pytest.mark.gpu

KEY = noise_key(7, 0, do.DROP_STREAM)
STREAM = do.drop_stream(3, 1, 1)
ROW_KEYS = ("x", "dz", "zh", "rstd")


def oracle(p, ln, s, a, dout, rate, stream=STREAM, key=KEY, scale=None, **mask_kw):
    """Every output of oprl_mlp_ln_drop in float64, by autograd through the masked, scaled z."""
    p64 = [x.double() for x in p]
    ln64 = ln.double().requires_grad_(True)
    a64 = a.double().requires_grad_(True)
    keep = do.drop_mask(key, stream, s.shape[0], rate, **mask_kw) if do.drop_thresh(rate) > 0 else None
    rows: dict = {}
    out = do.drop_mlp(p64, ln64, t.cat([s.double(), a64], 1), keep, do.drop_scale(rate) if scale is None else scale,
                      float(np.float32(EPS)), rows)
    for z in rows["z"]:
        z.retain_grad()
    (out * dout.double()).sum().backward()
    return dict(out=out.detach(), x=t.stack([x.detach() for x in rows["x"]]), zh=t.stack([x.detach() for x in rows["zh"]]),
                dz=t.stack([z.grad for z in rows["z"]]), rstd=t.stack([r.detach().reshape(-1) for r in rows["rstd"]]),
                dx1=a64.grad, dln=ln64.grad)


def run(net, ln, s, a, dout, rate, stream=STREAM, key=KEY, rows=None, split=0):
    """oprl_mlp_ln_drop on ``net`` (tests/test_gpu_ln_slice.py Net): every output array, rows >= B included."""
    B, rows = s.shape[0], rows or s.shape[0]
    full = lambda *shape: t.full(shape, SENT, dtype=t.float32, device="cuda")       # noqa: E731
    o = dict(out=full(B, 1), x=full(2, rows, W), dz=full(2, rows, W), zh=full(2, rows, W), rstd=full(2, rows),
             dx1=full(B, a.shape[1]), dln=full(2, 2, W))
    lnd, sd, ad, dd = (x.cuda().contiguous() for x in (ln, s, a, dout))
    _, desc = net.mlp._packed_desc()
    with _capi.on_device(sd.device):
        rc = _capi.load().oprl_mlp_ln_drop(C.byref(desc), _capi.ptr(lnd), EPS, _capi.ptr(sd), s.shape[1], _capi.ptr(ad), a.shape[1],
                                           B, rows, split, _capi.ptr(dd), _capi.ptr(o["out"]), _capi.ptr(o["x"]), _capi.ptr(o["dz"]),
                                           _capi.ptr(o["zh"]), _capi.ptr(o["rstd"]), _capi.ptr(o["dx1"]), _capi.ptr(o["dln"]),
                                           _capi.current_stream(), rate, key, stream)
    _capi.check(rc, "oprl_mlp_ln_drop")
    t.cuda.synchronize()
    return {k: v.cpu() for k, v in o.items()}


def gates_away(got, want, B):
    """(max over the outputs of deviation / TOL, that output)."""
    worst = (0.0, "")
    for k, w in want.items():
        g = got[k][:, :B] if k in ROW_KEYS else got[k]
        worst = max(worst, (sc.rel_dev(g.double().numpy(), w.numpy()) / TOL, k))
    return worst


@pytest.mark.parametrize("rate", [0.1, 0.5])
@pytest.mark.parametrize("B", [1, 16, 17, 100])
def test_every_output_against_float64(B, rate):
    p, ln, s, a, dout = make_case(17, 6, B)
    got = run(Net(p), ln, s, a, dout, rate)
    check(got, oracle(p, ln, s, a, dout, rate), B)
    # the dropped columns are exactly zero where the definition says so: dL/dz, and with it the share of the mask
    keep = do.drop_mask(KEY, STREAM, B, rate)
    assert bool((got["dz"][:, :B][t.from_numpy(~keep)] == 0).all())


def test_the_high_word_of_the_stream_counts():
    """stream = 2^33 + 5: a launch that dropped the high word would draw the mask of stream 5."""
    B, rate, stream = 17, 0.1, 2 ** 33 + 5
    p, ln, s, a, dout = make_case(17, 6, B, seed=4)
    got = run(Net(p), ln, s, a, dout, rate, stream=stream)
    check(got, oracle(p, ln, s, a, dout, rate, stream=stream), B)
    r, k = gates_away(got, oracle(p, ln, s, a, dout, rate, stream=5), B)
    print(f"low word only: {r:.1f} gates at {k}")
    assert r >= 10.0


def test_the_neighbouring_stream_and_local_rows_are_wrong_oracles():
    """The oracle with the mask of stream + 1 is at least ten gates away (the project's rule for a wrong oracle,
    tests/test_gpu_ln.py), and so is the one whose rows are numbered inside their slice, from B = 17 on, and the one
    without the scale — which only rstd and dz show: the normalisation cancels a common factor of its input up to eps, so
    through a learner that knob is invisible (tests/test_gpu_droq.py) and is held here."""
    B, rate = 17, 0.1
    p, ln, s, a, dout = make_case(17, 6, B, seed=5)
    got = run(Net(p), ln, s, a, dout, rate)
    check(got, oracle(p, ln, s, a, dout, rate), B)
    for what, kw in (("stream + 1", dict(stream=STREAM + 1)), ("local rows", dict(local_rows=True)), ("key + 1", dict(key=KEY + 1)),
                     ("no scale", dict(scale=1.0))):
        r, k = gates_away(got, oracle(p, ln, s, a, dout, rate, **kw), B)
        print(f"{what}: {r:.1f} gates at {k}")
        assert r >= 10.0, f"{what}: only {r:.1f} gates away"


@pytest.mark.parametrize("B", [17, 100])
def test_split_launches_equal_the_whole_launch_bitwise(B):
    """The backward-only launch regenerates the mask of the forward-only launch whose rows it reloads."""
    p, ln, s, a, dout = make_case(17, 6, B, seed=13)
    net = Net(p)
    whole, split = run(net, ln, s, a, dout, 0.1, rows=B + 5), run(net, ln, s, a, dout, 0.1, rows=B + 5, split=1)
    for k in whole:
        assert t.equal(whole[k], split[k]), k


def test_two_runs_give_the_same_bits():
    p, ln, s, a, dout = make_case(17, 6, 100, seed=11)
    net = Net(p)
    first, second = run(net, ln, s, a, dout, 0.5), run(net, ln, s, a, dout, 0.5)
    for k in first:
        assert t.equal(first[k], second[k]), k


def test_a_ragged_batch_touches_no_row_behind_it():
    B, rows = 100, 112
    p, ln, s, a, dout = make_case(17, 6, B, seed=9)
    got = run(Net(p), ln, s, a, dout, 0.1, rows=rows)
    check(got, oracle(p, ln, s, a, dout, 0.1), B)
    for k in ROW_KEYS:
        assert bool((got[k][:, B:] == SENT).all()), f"{k}: rows >= B were written"


def test_rate_zero_is_oprl_mlp_ln_bitwise():
    p, ln, s, a, dout = make_case(17, 6, 100, seed=15)
    net = Net(p)
    plain = net.run(ln, s, a, dout, rows=105)
    for rate in (0.0, 1e-12):        # (a rate below 2^-32: threshold 0, the mode off)
        got = run(net, ln, s, a, dout, rate, rows=105)
        for k in plain:
            assert t.equal(plain[k], got[k]), (rate, k)


def test_refusals():
    p, ln, s, a, dout = make_case(17, 6, 4)
    net = Net(p)
    lib = _capi.load()
    _, desc = net.mlp._packed_desc()
    src, buf = t.zeros(2 * 2 * W, device="cuda"), t.zeros(2 * 8 * W, device="cuda")      # inputs | outputs (all aliased: unread)
    inp, ptr = _capi.ptr(src), _capi.ptr(buf)
    st = _capi.current_stream()
    call = lambda rate=0.1, eps=EPS, k1=6, B=4, rows=4: lib.oprl_mlp_ln_drop(   # noqa: E731
        C.byref(desc), inp, eps, inp, 17, inp, k1, B, rows, 0, inp, ptr, ptr, ptr, ptr, ptr, ptr, ptr, st, rate, KEY, STREAM)
    for kw, word in ((dict(rate=1.0), b"rate"), (dict(rate=-0.1), b"rate"), (dict(rate=float("nan")), b"rate"), (dict(rate=1.5), b"rate"),
                     (dict(eps=0.0), b"eps"), (dict(k1=5), b"input dim"), (dict(B=0), b"B"), (dict(rows=3), b"rows")):
        assert call(**kw) == -1 and word in lib.oprl_last_error(), (kw, lib.oprl_last_error())
        assert b"oprl_mlp_ln_drop" in lib.oprl_last_error()
    assert lib.oprl_mlp_ln_drop(None, inp, EPS, inp, 17, inp, 6, 4, 4, 0, inp, ptr, ptr, ptr, ptr, ptr, ptr, ptr, st, 0.1, KEY, STREAM) == -1
    assert call() == 0
    t.cuda.synchronize()
