"""Host side of the LayerNorm critics (no GPU): the two C-ABI additions are declared, exported and bound and
refuse null arguments, the build lists the new source, the classes and the scripts refuse what the learner would before
anything is built, the state_dict key rules, the oracle's LN against torch's and its gradients against the closed form,
and the feasibility of the parity gates: the oracle in float32 stays within half of them of its float64 run."""
from __future__ import annotations

import ctypes as C
from pathlib import Path

import numpy as np
import pytest
import torch as t

from oprl_amd import _capi
from oprl_amd.algos import base_algorithm as base
from oprl_amd.algos.calql import CalQL
from oprl_amd.algos.cql import CQL
from oprl_amd.algos.nn_models import CriticLayerNorm, DoubleCritic, attach_layer_norm
from oprl_amd.algos.redq import REDQ, EnsembleCritic
from oprl_amd.algos.sac import SAC
from oprl_amd.logging import NullLogger
from oracle import fixtures as fx
from tests import ln_oracle as lno
from tests import scenarios as sc
from tests.config_scripts import load_config
from tests.support import assert_abi_bound, assert_source_built

ROOT = Path(__file__).resolve().parents[1]
ENTRIES = {"oprl_learner_set_layernorm": 2, "oprl_mlp_ln": 19}
TOL = 2e-5


def test_the_abi_additions_are_bound():
    lib, header = assert_abi_bound(ENTRIES)
    assert "typedef struct oprl_layernorm {" in header
    assert [f for f, _ in _capi.OprlLayerNorm._fields_] == ["theta", "theta_target", "adam_m", "adam_v", "eps"]
    # null handles and structs are refused without a GPU
    d = _capi.OprlLayerNorm()
    assert lib.oprl_learner_set_layernorm(None, C.byref(d)) == -1 and b"null learner" in lib.oprl_last_error()
    assert lib.oprl_mlp_ln(None, None, 1e-5, None, 4, None, 2, 4, 4, 0, *([None] * 9)) == -1 and b"null" in lib.oprl_last_error()


def test_the_build_lists_the_new_source():
    assert_source_built("ln_slice")


def test_layer_norm_is_the_last_public_field_and_off_by_default():
    from dataclasses import fields
    for cls in (SAC, REDQ):
        names = [f.name for f in fields(cls) if f.init and not f.name.startswith("_")]
        assert names[-1] == "layer_norm"
        assert cls(logger=NullLogger(), state_dim=4, action_dim=2).layer_norm is False


@pytest.mark.parametrize("cls", [SAC, REDQ], ids=["sac", "redq"])
@pytest.mark.parametrize("kw,msg", [
    (dict(prioritized=True), "priorit"),
    (dict(export_grads=True), "export"),
    (dict(precision="bf16"), "f32"),
    (dict(precision="x2"), "f32"),
], ids=["prioritized", "export_grads", "bf16", "x2"])
def test_the_classes_refuse_before_any_gpu_call(cls, kw, msg, monkeypatch):
    import oprl_amd.algos.redq as redq_mod
    import oprl_amd.algos.sac as sac_mod
    for mod in (sac_mod, redq_mod):
        monkeypatch.setattr(mod, "require_gpu", lambda device: pytest.fail("the GPU was asked for"))
    algo = cls(logger=NullLogger(), state_dim=4, action_dim=2, layer_norm=True, **kw)
    with pytest.raises(ValueError, match=msg):
        algo.create()
    with pytest.raises(ValueError, match="layer_norm"):
        base.check_layer_norm_config(algo)


@pytest.mark.parametrize("cls", [CQL, CalQL], ids=["cql", "calql"])
def test_the_cql_classes_refuse_layer_norm(cls):
    with pytest.raises(ValueError, match="layer_norm"):
        cls(logger=NullLogger(), state_dim=4, action_dim=2, layer_norm=True)


# ---- the holder and the modules ---------------------------------------------------------------------------------------------
def test_the_holder_is_no_submodule_and_the_modules_apply_it():
    S, A = 5, 3
    h = CriticLayerNorm(2).make_state()
    th, tg, m, v = h.tensors()
    assert th.shape == (2, 2, 2, 256) and th.dtype == t.float32
    assert bool((th[:, :, 0] == 1).all()) and bool((th[:, :, 1] == 0).all()) and t.equal(tg, th) and tg is not th
    assert float(m.abs().max()) == 0.0 and float(v.abs().max()) == 0.0 and h.eps == 1e-5
    c = DoubleCritic(S, A, (256, 256), t.nn.ReLU(inplace=True))
    n_params = len(list(c.parameters()))
    s, a = fx.make_batch(1, 7, S, A)[:2]
    plain = c(s, a)
    attach_layer_norm(c, h, False)
    assert len(list(c.parameters())) == n_params and "_ln" not in dict(c.named_modules())
    with t.no_grad():
        th[0, 0, 0].mul_(1.5)
        th[1, 1, 1].add_(0.25)
    q1, q2 = c(s, a)
    for j, q in enumerate((q1, q2)):
        want = lno.ln_mlp([p.detach() for p in (c.q1, c.q2)[j].parameters()], th[j], t.cat([s, a], 1), eps=h.eps)
        assert sc.rel_dev(q.detach().numpy(), want.numpy()) <= 1e-6
        assert sc.rel_dev(q.detach().numpy(), plain[j].detach().numpy()) > 1e-2
    assert t.equal(c.Q1(s, a), q1)
    e = EnsembleCritic(S, A, 3)
    h3 = CriticLayerNorm(3).make_state()
    attach_layer_norm(e, h3, True)
    out = e(s, a)
    assert out.shape == (7, 3)
    want = lno.ln_mlp([p.detach() for p in e.nets[2].parameters()], h3.target[2], t.cat([s, a], 1), eps=h3.eps)
    assert sc.rel_dev(out[:, 2:3].detach().numpy(), want.numpy()) <= 1e-6


class _FakeLearner:
    """HipLearner's state_dict / load_state_dict over host tensors: the key rules without a handle."""

    state_dict = base.HipLearner.state_dict
    load_state_dict = base.HipLearner.load_state_dict

    def __init__(self, ln: bool):
        z = lambda: t.zeros(4)       # noqa: E731
        self.algo_name, self.device = "sac", t.device("cpu")
        self.actor_arena, self.actor_m, self.actor_v, self.critic_arena, self.critic_m, self.critic_v = (z() for _ in range(6))
        self._tg = [z()]
        self.log_alpha, self._iql_on = None, False
        self._ln = CriticLayerNorm(2).make_state() if ln else None
        self.handle = None

        class Lib:
            @staticmethod
            def oprl_learner_get_counters(h, cnt):
                return 0

            @staticmethod
            def oprl_learner_set_counters(h, cnt):
                return 0
        self.lib = Lib()

    def target_arenas(self):
        return self._tg

    def sync_params(self):
        pass


def test_state_dict_key_rules(monkeypatch):
    monkeypatch.setattr(t.cuda, "synchronize", lambda *a, **k: None)
    with_ln, without = _FakeLearner(True), _FakeLearner(False)
    sd_ln, sd = with_ln.state_dict(), without.state_dict()
    assert set(base.LN_STATE_KEYS) == {"critic_ln", "critic_ln_target", "critic_ln_m", "critic_ln_v"}
    assert set(base.LN_STATE_KEYS) <= set(sd_ln) and not set(base.LN_STATE_KEYS) & set(sd)
    with pytest.raises(ValueError, match="critic_ln"):
        without.load_state_dict(sd_ln)
    with pytest.raises(ValueError, match="critic_ln"):
        with_ln.load_state_dict(sd)
    sd_ln["critic_ln"][1, 0, 1, 7] = 3.0
    sd_ln["critic_ln_v"][0, 1, 0, 2] = 0.5
    other = _FakeLearner(True)
    other.load_state_dict(sd_ln)
    assert float(other._ln.theta[1, 0, 1, 7]) == 3.0 and float(other._ln.v[0, 1, 0, 2]) == 0.5
    without.load_state_dict(sd)


# ---- the oracle -----------------------------------------------------------------------------------------------------------
def test_the_oracles_layer_norm_is_torchs_and_its_gradients_the_closed_form():
    gen = t.Generator().manual_seed(5)
    B, W = 37, 256
    z = (t.randn(B, W, dtype=t.float64, generator=gen) * 3 + 2).requires_grad_(True)
    gamma = t.randn(W, dtype=t.float64, generator=gen).requires_grad_(True)
    beta = t.randn(W, dtype=t.float64, generator=gen).requires_grad_(True)
    n, zh, rstd = lno.layer_norm(z, gamma, beta)
    want = t.nn.functional.layer_norm(z, (W,), gamma, beta, lno.EPS)
    assert float((n - want).detach().abs().max()) <= 1e-13 * float(want.detach().abs().max())
    g = t.randn(B, W, dtype=t.float64, generator=gen) * (n.detach() > 0)        # ReLU-masked, as the kernels see it
    dz_a, dg_a, db_a = t.autograd.grad(n, [z, gamma, beta], g)
    dz, dg, db = lno.closed_form_backward(g, zh.detach(), rstd.detach(), gamma.detach())
    for got, ref in ((dz, dz_a), (dg, dg_a), (db, db_a)):
        assert float((got - ref).abs().max()) <= 1e-12 * float(ref.abs().max())
    # a constant row: var = 0 gives zh = 0 and finite results
    n0, zh0, rstd0 = lno.layer_norm(t.full((2, W), 4.0, dtype=t.float64), gamma.detach(), beta.detach())
    assert float(zh0.abs().max()) == 0.0 and bool(t.isfinite(rstd0).all()) and t.equal(n0[0], beta.detach())


def test_the_knobs_change_the_oracle():
    o = {k: _oracle("redq", 256, **({k: True} if k else {})) for k in ("", "no_ln", "freeze_ln", "no_ln_polyak")}
    ln0 = o[""].ln.clone()
    for s, a, r, d, s2, e1, e2 in lno.scenario_batches(100, 256, 2):
        for x in o.values():
            x.update(*(v.double() for v in (s, a, r, d, s2, e1, e2)))
    assert not t.equal(o[""].ln, o["freeze_ln"].ln) and t.equal(o["freeze_ln"].ln, ln0)
    assert not t.equal(o[""].ln_target, ln0) and t.equal(o["no_ln_polyak"].ln_target, ln0)
    assert not t.equal(o[""].critics[0][0], o["no_ln"].critics[0][0])


# ---- feasibility of the gates -------------------------------------------------------------------------------------------------
def _subset(n, m):
    lib = _capi.load()

    def draw(u):
        out = (C.c_int32 * m)()
        _capi.check(lib.oprl_redq_subset(7, 0, u, n, m, out), "oprl_redq_subset")
        return list(out)
    return draw


def _oracle(algo, B, n_min=2, dtype=t.float64, **kw):
    return lno.scenario_oracle(algo, _subset(lno.N, n_min), n_min, dtype, **kw)


@pytest.mark.parametrize("algo,B,n_min,seed", lno.SCENARIOS, ids=[f"{a}-B{b}-M{m}" for a, b, m, _ in lno.SCENARIOS])
def test_float32_stays_within_half_the_gates(algo, B, n_min, seed):
    """The parity scenarios of tests/test_gpu_ln.py, four updates, the oracle in float32 against itself in float64:
    within HALF the suite's gates (TOL = 2e-5 on outputs, PARAM_TOL = 1e-4 on parameters and moments), so a correct fp32
    kernel has room.  The batches' seeds were chosen for this (tests/ln_oracle.py SCENARIOS has the rule and the figures):
    seed 100 misses at two of the five scenarios by a ReLU unit that float32 masks the other way."""
    o64, o32 = _oracle(algo, B, n_min), _oracle(algo, B, n_min, dtype=t.float32)
    for batch in lno.scenario_batches(seed, B, 4):
        o64.update(*(x.double() for x in batch))
        o32.update(*(x.float() for x in batch))
    worst = sc.compare(lno.digest(o32), lno.digest(o64), TOL / 2, param_tol=sc.PARAM_TOL / 2)
    print(f"{algo} B={B} M={n_min}: worst {worst[0]} {worst[1]:.2e}")


# ---- configs/sac.py, configs/redq.py ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,cls", [("sac", SAC), ("redq", REDQ)])
def test_the_config_scripts_take_the_flag(monkeypatch, name, cls):
    mod = load_config(monkeypatch, name, ["--env", "synthetic:walker-walk", "--layer-norm"])
    assert mod.script.args.layer_norm is True and mod.script.algo_cls is cls
    assert mod.script.algo_kwargs(mod.script.args) == dict(layer_norm=True)
    mod = load_config(monkeypatch, name, ["--env", "synthetic:walker-walk"])
    assert mod.script.algo_kwargs(mod.script.args) == dict(layer_norm=False)


def test_the_rlpd_command_line_is_documented_and_parses(monkeypatch):
    line = "configs/redq.py --layer-norm --prior-data D.npz --prior-share 0.5"
    assert line in (ROOT / "configs" / "redq.py").read_text() and line in (ROOT / "README.md").read_text()
    mod = load_config(monkeypatch, "redq", ["--env", "synthetic:walker-walk", *line.split()[1:]])
    a = mod.script.args
    assert (a.layer_norm, a.prior_data, a.prior_share) == (True, "D.npz", 0.5)


@pytest.mark.parametrize("name", ["sac", "redq"])
@pytest.mark.parametrize("argv,msg", [(["--per"], "--per"), (["--seeds", "2"], "--seeds")], ids=["per", "seeds"])
def test_the_config_scripts_refuse(monkeypatch, name, argv, msg):
    """... before an environment is built."""
    import oprl_amd.environment as env
    monkeypatch.setattr(env, "make_env", lambda *a, **k: pytest.fail("an environment was built"))
    with pytest.raises(ValueError, match="--layer-norm.*" + msg):
        load_config(monkeypatch, name, ["--env", "synthetic:walker-walk", "--layer-norm", *argv])
