"""Host side of DroQ's dropout in the LayerNorm critics (no GPU): the two C-ABI additions are declared,
exported and bound and refuse what they can without a device, the classes and the scripts refuse before anything is built, the
state_dict key rule, the oracle (tests/droq_oracle.py) against tests/ln_oracle.py at rate 0 and against the closed-form
backward, the dropped share of the mask, and the feasibility of the parity gates: the oracle in float32 stays within half of
them of its float64 run."""
from __future__ import annotations

import ctypes as C
from dataclasses import fields
from pathlib import Path

import numpy as np
import pytest
import torch as t

from oprl_amd import _capi
from oprl_amd.algos import base_algorithm as base
from oprl_amd.algos.droq import DroQ
from oprl_amd.algos.redq import REDQ
from oprl_amd.algos.sac import SAC
from oprl_amd.logging import NullLogger
from tests import droq_oracle as do
from tests import ln_oracle as lno
from tests import scenarios as sc
from tests.config_scripts import load_config
from tests.support import assert_abi_bound
from tests.test_ln_host import _FakeLearner, _subset
from tests.test_redq_host import M32, noise_key, philox4x32_10

ROOT = Path(__file__).resolve().parents[1]
ENTRIES = {"oprl_learner_set_dropout": 2, "oprl_mlp_ln_drop": 22}
TOL = 2e-5
INVALID = -1


def test_the_abi_additions_are_bound():
    lib, header = assert_abi_bound(ENTRIES)
    assert _capi.SIGNATURES["oprl_mlp_ln_drop"][1][:19] == _capi.SIGNATURES["oprl_mlp_ln"][1]
    assert _capi.SIGNATURES["oprl_mlp_ln_drop"][1][19:] == [C.c_float, C.c_uint64, C.c_uint64]
    for text in ("T = (u 4 + k) 16 + j", "stream 6", "leaves the mode off", "(uint32)((double)rate 2^32)"):
        assert text in header, text
    # what is refused without a GPU: null handles, and the rate ahead of everything that needs the device
    assert lib.oprl_learner_set_dropout(None, 0.1) == INVALID and b"null learner" in lib.oprl_last_error()
    assert lib.oprl_mlp_ln_drop(None, None, 1e-5, None, 4, None, 2, 4, 4, 0, *([None] * 9), 0.1, 1, 2) == INVALID
    assert b"oprl_mlp_ln_drop: null" in lib.oprl_last_error()
    assert lib.oprl_mlp_ln(None, None, 1e-5, None, 4, None, 2, 4, 4, 0, *([None] * 9)) == INVALID
    assert b"oprl_mlp_ln: null" in lib.oprl_last_error()


def test_the_view_stays_inside_the_kernel_argument_limit():
    text = (ROOT / "oprl_amd" / "csrc" / "ln_slice.h").read_text()
    assert "static_assert(sizeof(LnView) == 80" in text and "static_assert(sizeof(MlpMultiLnArgs) <= 4096" in text


# ---- the classes --------------------------------------------------------------------------------------------------------------
def test_the_field_is_off_by_default_and_droq_is_redq_with_its_recipe():
    for cls in (SAC, REDQ):
        algo = cls(logger=NullLogger(), state_dim=4, action_dim=2)
        assert algo.dropout == 0.0 and algo.layer_norm is False
    d = DroQ(logger=NullLogger(), state_dim=4, action_dim=2)
    assert isinstance(d, REDQ)
    assert (d.n_critics, d.n_min, d.utd_ratio, d.layer_norm, d.dropout) == (2, 2, 20, True, 0.01)
    assert [f.name for f in fields(DroQ)] == [f.name for f in fields(REDQ)]
    import oprl.algos.droq as alias
    assert alias.DroQ is DroQ


@pytest.mark.parametrize("cls", [SAC, REDQ, DroQ], ids=["sac", "redq", "droq"])
@pytest.mark.parametrize("kw,msg", [
    (dict(dropout=0.1, layer_norm=False), "needs layer_norm=True"),
    (dict(dropout=1.0, layer_norm=True), r"\[0, 1\)"),
    (dict(dropout=-0.01, layer_norm=True), r"\[0, 1\)"),
    (dict(dropout=float("nan"), layer_norm=True), r"\[0, 1\)"),
    (dict(dropout=0.1, layer_norm=True, prioritized=True), "priorit"),
    (dict(dropout=0.1, layer_norm=True, precision="bf16"), "f32"),
], ids=["no-ln", "one", "negative", "nan", "prioritized", "bf16"])
def test_the_classes_refuse_before_any_gpu_call(cls, kw, msg, monkeypatch):
    import oprl_amd.algos.redq as redq_mod
    import oprl_amd.algos.sac as sac_mod
    for mod in (sac_mod, redq_mod):
        monkeypatch.setattr(mod, "require_gpu", lambda device: pytest.fail("the GPU was asked for"))
    algo = cls(logger=NullLogger(), state_dim=4, action_dim=2, **kw)
    with pytest.raises(ValueError, match=msg):
        algo.create()
    with pytest.raises(ValueError, match=msg):
        base.check_layer_norm_config(algo)


def test_the_critic_modules_forward_says_it_is_the_inference_form():
    from oprl_amd.algos import nn_models
    assert "never does" in nn_models._forward_sa_ln.__doc__ and "dropout" in nn_models._forward_sa_ln.__doc__


def test_state_dict_key_rule(monkeypatch):
    """``critic_dropout`` (the rate) rides only while the mode is on; a checkpoint with it does not load into a learner
    without, nor the reverse, nor one of another rate."""
    monkeypatch.setattr(t.cuda, "synchronize", lambda *a, **k: None)
    assert base.DROPOUT_STATE_KEY == "critic_dropout"
    on, off, other = _FakeLearner(True), _FakeLearner(True), _FakeLearner(True)
    on._dropout, other._dropout = 0.1, 0.2
    sd_on, sd_off = on.state_dict(), off.state_dict()
    assert sd_on["critic_dropout"] == 0.1 and "critic_dropout" not in sd_off
    with pytest.raises(ValueError, match="critic_dropout"):
        off.load_state_dict(sd_on)
    with pytest.raises(ValueError, match="critic_dropout"):
        on.load_state_dict(sd_off)
    with pytest.raises(ValueError, match="critic_dropout"):
        other.load_state_dict(sd_on)
    again = _FakeLearner(True)
    again._dropout = 0.1
    again.load_state_dict(sd_on)
    off.load_state_dict(sd_off)


# ---- the oracle ---------------------------------------------------------------------------------------------------------------
def test_the_mask_is_the_documented_philox_comparison():
    """The vectorised mask against tests/test_redq_host.py's scalar Philox, word by word, at a stream above 2^32."""
    key, T, B, rate = noise_key(7, 0, do.DROP_STREAM), 2 ** 33 + 5, 19, 0.1
    assert do.DROP_STREAM == 6 and do.drop_thresh(rate) == int(float(np.float32(0.1)) * 2 ** 32) and do.drop_thresh(0.0) == 0
    assert do.drop_thresh(1e-12) == 0 and do.drop_stream(3, 2, 9) == (3 * 4 + 2) * 16 + 9
    keep = do.drop_mask(key, T, B, rate)
    assert keep.shape == (2, B, 256) and keep.dtype == np.bool_
    for l, b, c in [(0, 0, 0), (0, 0, 3), (1, 0, 4), (1, 18, 255), (0, 17, 130), (1, 3, 77)]:
        words = philox4x32_10((T & M32, T >> 32, b, l * 64 + c // 4), key & M32, key >> 32)
        assert bool(keep[l, b, c]) == (words[c % 4] >= do.drop_thresh(rate)), (l, b, c)
    local = do.drop_mask(key, T, B, rate, local_rows=True)
    assert np.array_equal(local[:, :16], keep[:, :16]) and np.array_equal(local[:, 16:], keep[:, :3])
    assert not np.array_equal(keep, do.drop_mask(key, T + 1, B, rate)) and not np.array_equal(keep, do.drop_mask(key, 5, B, rate))
    assert do.drop_scale(0.1) == float(np.float32(1) / (np.float32(1) - np.float32(0.1))) != 1 / 0.9


def test_the_dropped_share():
    """100 rows x 2 layers x 256 columns at rate 0.1: within five binomial standard deviations of 0.1
    (5 sqrt(0.1 0.9 / 51200) = 0.0066).  Deterministic: key and stream are fixed."""
    keep = do.drop_mask(noise_key(7, 0, do.DROP_STREAM), do.drop_stream(0, 1, 0), 100, 0.1)
    n = keep.size
    assert n == 51200
    share, band = 1.0 - keep.mean(), 5.0 * np.sqrt(0.1 * 0.9 / n)
    print(f"dropped share {share:.5f}, band +-{band:.5f}")
    assert abs(band - 0.0066) < 5e-5 and abs(share - 0.1) <= band


def _oracle(name, rate, dtype=t.float64, **kw):
    return do.scenario_oracle(name, _subset(lno.N if name == "redq" else 2, 2), rate, dtype, **kw)


@pytest.mark.parametrize("name", ["droq", "sac"])
def test_rate_zero_is_the_ln_oracle_bit_for_bit(name):
    B = 100
    a = _oracle(name, 0.0)
    if name == "sac":
        b = lno.scenario_oracle("sac", None)
    else:
        actor, critics, ln = lno.scenario_params("sac")
        b = lno.LNOracle("redq", lno.S, lno.A, actor, critics, critics, ln, ln, subset=_subset(2, 2), n_min=2, utd_ratio=lno.G)
    for batch in lno.scenario_batches(100, B, 3):
        for o in (a, b):
            o.update(*(x.double() for x in batch))
    da, db = lno.digest(a), lno.digest(b)
    assert da.keys() == db.keys()
    for k in da:
        assert np.array_equal(da[k], db[k]), k
    # every evaluation knew its (u, k, j): the last update was an actor step
    want = [(2, 0, j) for j in a._idx] + [(2, 1, 0), (2, 1, 1), (2, 2, 0), (2, 2, 1)]
    assert a.masks == want


def test_the_oracles_backward_is_the_closed_form():
    """dL/dz = keep ? dz scale : 0 with dz section 24's closed form taken over the zh of zd; dgamma / dbeta over that zh.
    One row has every column dropped: section 24's constant row, zh = 0 and everything finite."""
    gen = t.Generator().manual_seed(5)
    B, Wd, rate = 37, 256, 0.5
    scale = do.drop_scale(rate)
    keep = t.from_numpy(do.drop_mask(noise_key(7, 0, 6), 9, B, rate)[0]).clone()
    keep[3] = False
    z = (t.randn(B, Wd, dtype=t.float64, generator=gen) * 3 + 2).requires_grad_(True)
    gamma = t.randn(Wd, dtype=t.float64, generator=gen).requires_grad_(True)
    beta = t.randn(Wd, dtype=t.float64, generator=gen).requires_grad_(True)
    zd = t.where(keep, z * scale, t.zeros((), dtype=t.float64))
    n, zh, rstd = lno.layer_norm(zd, gamma, beta)
    g = t.randn(B, Wd, dtype=t.float64, generator=gen) * (n.detach() > 0)        # ReLU-masked, as the kernels see it
    dz_a, dg_a, db_a = t.autograd.grad(n, [z, gamma, beta], g)
    dzd, dg, db = lno.closed_form_backward(g, zh.detach(), rstd.detach(), gamma.detach())
    dz = t.where(keep, dzd * scale, t.zeros((), dtype=t.float64))
    for got, ref in ((dz, dz_a), (dg, dg_a), (db, db_a)):
        assert float((got - ref).abs().max()) <= 1e-12 * float(ref.abs().max())
    assert float(zh[3].detach().abs().max()) == 0.0 and float(dz[3].abs().max()) == 0.0 and bool(t.isfinite(rstd).all())
    assert t.equal(n[3].detach(), beta.detach())


def test_the_knobs_change_the_oracle():
    B = 100
    o = {k: _oracle("droq", 0.1, **({k: True} if k else {})) for k in ("", *do.KNOBS)}
    for batch in lno.scenario_batches(100, B, 3):
        for x in o.values():
            x.update(*(v.double() for v in batch))
    right = lno.digest(o[""])
    for k in do.KNOBS:
        assert not np.array_equal(lno.digest(o[k])["u.critic.0.0"], right["u.critic.0.0"]), k


# ---- feasibility of the gates -------------------------------------------------------------------------------------------------
IDS = [f"{n}-B{b}-p{r}" for n, b, r, _ in do.SCENARIOS]


@pytest.mark.parametrize("name,B,rate,seed", do.SCENARIOS, ids=IDS)
def test_float32_stays_within_half_the_gates(name, B, rate, seed):
    """The parity scenarios of tests/test_gpu_droq.py, four updates, the oracle in float32 against itself in float64: within
    HALF the suite's gates (TOL = 2e-5 on outputs, PARAM_TOL = 1e-4 on parameters and moments), so a correct fp32 kernel
    has room.  Both runs draw the same masks: an integer comparison has no rounding.  tests/droq_oracle.py SCENARIOS has
    the rule the seeds were chosen by and the figures."""
    o64, o32 = _oracle(name, rate), _oracle(name, rate, dtype=t.float32)
    for batch in lno.scenario_batches(seed, B, 4):
        o64.update(*(x.double() for x in batch))
        o32.update(*(x.float() for x in batch))
    worst = sc.compare(lno.digest(o32), lno.digest(o64), TOL / 2, param_tol=sc.PARAM_TOL / 2)
    print(f"{name} B={B} rate={rate}: worst {worst[0]} {worst[1]:.2e}")


# ---- configs/droq.py, --dropout -------------------------------------------------------------------------------------------------
ENV = ["--env", "synthetic:walker-walk"]


def test_the_config_scripts_take_the_flag(monkeypatch):
    for name, cls in (("sac", SAC), ("redq", REDQ)):
        mod = load_config(monkeypatch, name, [*ENV, "--layer-norm", "--dropout", "0.05"])
        assert mod.script.algo_cls is cls and mod.script.algo_kwargs(mod.script.args) == dict(layer_norm=True, dropout=0.05)
    mod = load_config(monkeypatch, "droq", ENV)
    assert mod.script.algo_cls is DroQ and mod.script.args.layer_norm is True and mod.script.algo_kwargs(mod.script.args) == {}
    mod = load_config(monkeypatch, "droq", [*ENV, "--dropout", "0.1"])
    assert mod.script.algo_kwargs(mod.script.args) == dict(dropout=0.1)
    assert "configs/droq.py --env walker-walk" in (ROOT / "configs" / "droq.py").read_text()


@pytest.mark.parametrize("name,argv,msg", [
    ("sac", ["--dropout", "0.1"], "--dropout without --layer-norm"),
    ("redq", ["--dropout", "0.1"], "--dropout without --layer-norm"),
    ("redq", ["--layer-norm", "--dropout", "1.0"], r"\[0, 1\)"),
    ("droq", ["--dropout", "-0.5"], r"\[0, 1\)"),
    ("droq", ["--per"], "--layer-norm.*--per"),
    ("droq", ["--seeds", "2"], "--layer-norm.*--seeds"),
])
def test_the_config_scripts_refuse(monkeypatch, name, argv, msg):
    """... before an environment is built."""
    import oprl_amd.environment as env
    monkeypatch.setattr(env, "make_env", lambda *a, **k: pytest.fail("an environment was built"))
    with pytest.raises(ValueError, match=msg):
        load_config(monkeypatch, name, [*ENV, *argv])


def test_the_bench_tool_lists_the_cases():
    text = (ROOT / "tools" / "bench_algos.py").read_text()
    assert '("DroQ walker' in text and '("REDQ-LN-drop walker N=10' in text and "dropout=0.01" in text
