"""k_mlp_slice_ln and k_ln_adam (csrc/ln_slice.hip) alone, through oprl_mlp_ln, against the float64 oracle of
tests/ln_oracle.py: max-norm relative deviation <= 2e-5 on every output — the net's output, per hidden
layer x, dz and zh, rstd, the gradient over the action columns, and the reduced dgamma | dbeta.

Shapes: inputs 17 + 6 and 24 + 6; B = 1 (a single row), 16 (one full slice), 100 (ragged: 7 slices, 4 live rows in the
last).  Offset rows (|mean| ~ 30 std: a one-pass variance lands at 4e-5 .. 1.4e-4 there, two passes at <= 4.4e-6), constant
rows (var = 0), untouched rows >= B, run-to-run bits, and the forward-only + backward-only pair against the whole launch."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest
import torch as t
from torch import nn

from oprl_amd import _capi
from oprl_amd.algos.nn_models import MLP
from oracle import fixtures as fx
from tests import ln_oracle as lno
from tests import scenarios as sc
from tests.hip_adapters import load_params

pytestmark = pytest.mark.gpu

TOL = 2e-5
W = 256
SENT = -7.5e8          # what the output arrays hold before the call
EPS = 1e-5


def make_case(S, A, B, seed=3, offset=0.0, constant=False):
    """(net parameters, ln [2, 2, 256], s, a, dout): float32 host tensors."""
    p = fx.make_net(60 + seed, [S + A, W, W, 1])
    gen = t.Generator().manual_seed(seed)
    if offset:
        p[1] = p[1] + offset
        p[3] = p[3] + offset
    if constant:                      # zero hidden weights and constant biases: every row of z is one number
        p[0], p[2] = t.zeros_like(p[0]), t.zeros_like(p[2])
        p[1], p[3] = t.full_like(p[1], 0.5), t.full_like(p[3], -0.25)
    ln = t.zeros(2, 2, W)
    ln[:, 0] = 1.0 + 0.3 * t.randn(2, W, generator=gen)
    ln[:, 1] = 0.3 * t.randn(2, W, generator=gen)
    s = t.randn(B, S, generator=gen)
    a = t.rand(B, A, generator=gen) * 2 - 1
    dout = t.randn(B, 1, generator=gen)
    return p, ln, s, a, dout


def oracle(p, ln, s, a, dout):
    """Every output of oprl_mlp_ln in float64, by autograd."""
    p64 = [x.double() for x in p]
    ln64 = ln.double().requires_grad_(True)
    a64 = a.double().requires_grad_(True)
    keep: dict = {}
    out = lno.ln_mlp(p64, ln64, t.cat([s.double(), a64], 1), float(np.float32(EPS)), keep)
    for z in keep["z"]:
        z.retain_grad()
    (out * dout.double()).sum().backward()
    rstd = [1.0 / t.sqrt(z.detach().var(1, unbiased=False) + float(np.float32(EPS))) for z in keep["z"]]
    return dict(out=out.detach(), x=t.stack([x.detach() for x in keep["x"]]), zh=t.stack([x.detach() for x in keep["zh"]]),
                dz=t.stack([z.grad for z in keep["z"]]), rstd=t.stack(rstd), dx1=a64.grad, dln=ln64.grad)


class Net:
    """One packed critic on the device; ``run`` calls oprl_mlp_ln and returns every output array (rows >= B included)."""

    def __init__(self, p):
        self.mlp = MLP(p[0].shape[1], 1, (W, W), nn.ReLU(inplace=True)).cuda()
        load_params(self.mlp, [x.cuda() for x in p])

    def run(self, ln, s, a, dout, rows=None, split=0):
        B, rows = s.shape[0], rows or s.shape[0]
        full = lambda *shape: t.full(shape, SENT, dtype=t.float32, device="cuda")       # noqa: E731
        o = dict(out=full(B, 1), x=full(2, rows, W), dz=full(2, rows, W), zh=full(2, rows, W), rstd=full(2, rows),
                 dx1=full(B, a.shape[1]), dln=full(2, 2, W))
        self.dev = [x.cuda().contiguous() for x in (ln, s, a, dout)]
        lnd, sd, ad, dd = self.dev
        _, desc = self.mlp._packed_desc()
        with _capi.on_device(sd.device):
            rc = _capi.load().oprl_mlp_ln(C.byref(desc), _capi.ptr(lnd), EPS, _capi.ptr(sd), s.shape[1], _capi.ptr(ad), a.shape[1],
                                          B, rows, split, _capi.ptr(dd), _capi.ptr(o["out"]), _capi.ptr(o["x"]), _capi.ptr(o["dz"]),
                                          _capi.ptr(o["zh"]), _capi.ptr(o["rstd"]), _capi.ptr(o["dx1"]), _capi.ptr(o["dln"]),
                                          _capi.current_stream())
        _capi.check(rc, "oprl_mlp_ln")
        t.cuda.synchronize()
        return {k: v.cpu() for k, v in o.items()}


def check(got, want, B):
    for k, w in want.items():
        g = got[k][:, :B] if k in ("x", "dz", "zh", "rstd") else got[k]
        assert bool(t.isfinite(g).all()), k
        dev = sc.rel_dev(g.double().numpy(), w.numpy())
        print(f"{k}: {dev:.2e}")
        assert dev <= TOL, f"{k}: rel dev {dev:.3e} > {TOL:.1e}"


@pytest.mark.parametrize("S,A", [(17, 6), (24, 6)], ids=["17+6", "24+6"])
@pytest.mark.parametrize("B", [1, 16, 100])
def test_every_output_against_float64(S, A, B):
    p, ln, s, a, dout = make_case(S, A, B)
    check(Net(p).run(ln, s, a, dout), oracle(p, ln, s, a, dout), B)


def test_offset_rows_need_the_two_pass_variance():
    """Hidden biases shifted by +30: |mean| is about 30 std.  E[z^2] - mu^2 loses the variance's low bits there and
    misses the gate; mean of (z - mu)^2 over the registers does not."""
    p, ln, s, a, dout = make_case(24, 6, 100, seed=5, offset=30.0)
    want = oracle(p, ln, s, a, dout)
    z0 = t.cat([s, a], 1).double() @ p[0].double().t() + p[1].double()
    assert float((z0.mean(1).abs() / z0.std(1)).min()) > 20.0
    check(Net(p).run(ln, s, a, dout), want, 100)


def test_constant_rows_give_zero_zh_and_finite_results():
    p, ln, s, a, dout = make_case(17, 6, 16, seed=7, constant=True)
    got = Net(p).run(ln, s, a, dout)
    assert float(got["zh"].abs().max()) == 0.0
    for k, v in got.items():
        assert bool(t.isfinite(v).all()), k
    want = oracle(p, ln, s, a, dout)
    assert float(want["zh"].abs().max()) == 0.0
    for k in ("out", "x", "rstd", "dln"):
        assert sc.rel_dev(got[k].double().numpy(), want[k].numpy()) <= TOL, k
    # dz of layer 1 (layer 0's is zero behind the zero weights), where rstd = 1 / sqrt(eps) multiplies a difference that is
    # zero in exact arithmetic only when gamma g is constant: gate it against the oracle's scale, and dx1 = 0 exactly
    assert sc.rel_dev(got["dz"][1].double().numpy(), want["dz"][1].numpy()) <= TOL
    assert float(got["dz"][0].abs().max()) == 0.0 and float(got["dx1"].abs().max()) == 0.0


def test_a_ragged_batch_sums_its_live_rows_and_touches_no_other():
    B, rows = 100, 112
    p, ln, s, a, dout = make_case(24, 6, B, seed=9)
    got = Net(p).run(ln, s, a, dout, rows=rows)
    want = oracle(p, ln, s, a, dout)              # (sums over the 100 live rows)
    check(got, want, B)
    for k in ("x", "dz", "zh", "rstd"):
        assert bool((got[k][:, B:] == SENT).all()), f"{k}: rows >= B were written"


def test_two_runs_give_the_same_bits():
    p, ln, s, a, dout = make_case(24, 6, 100, seed=11)
    net = Net(p)
    first, second = net.run(ln, s, a, dout), net.run(ln, s, a, dout)
    for k in first:
        assert t.equal(first[k], second[k]), k


@pytest.mark.parametrize("B", [16, 100])
def test_split_launches_equal_the_whole_launch_bitwise(B):
    """A forward-only launch that keeps x, zh and rstd, then a backward-only launch that reloads them."""
    p, ln, s, a, dout = make_case(24, 6, B, seed=13)
    net = Net(p)
    whole, split = net.run(ln, s, a, dout, rows=B + 5), net.run(ln, s, a, dout, rows=B + 5, split=1)
    for k in whole:
        assert t.equal(whole[k], split[k]), k


def test_refusals():
    p, ln, s, a, dout = make_case(17, 6, 4)
    net = Net(p)
    lib = _capi.load()
    _, desc = net.mlp._packed_desc()
    src, buf = t.zeros(2 * 2 * W, device="cuda"), t.zeros(2 * 8 * W, device="cuda")      # inputs | outputs (all aliased: unread)
    inp, ptr = _capi.ptr(src), _capi.ptr(buf)
    st = _capi.current_stream()
    call = lambda eps=EPS, k1=6, B=4, rows=4: lib.oprl_mlp_ln(C.byref(desc), inp, eps, inp, 17, inp, k1, B, rows, 0, inp, ptr,   # noqa: E731
                                                              ptr, ptr, ptr, ptr, ptr, ptr, st)
    for kw, word in ((dict(eps=0.0), b"eps"), (dict(eps=float("nan")), b"eps"), (dict(k1=5), b"input dim"), (dict(B=0), b"B"),
                     (dict(rows=3), b"rows")):
        assert call(**kw) == -1 and word in lib.oprl_last_error(), (kw, lib.oprl_last_error())
    wide = MLP(23, 1, (512, 512), nn.ReLU(inplace=True)).cuda()
    _, d512 = wide._packed_desc()
    assert lib.oprl_mlp_ln(C.byref(d512), ptr, EPS, ptr, 17, ptr, 6, 4, 4, 0, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, st) == -1
    assert b"256" in lib.oprl_last_error()
    assert call() == 0
    t.cuda.synchronize()
