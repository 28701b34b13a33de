"""Host side of IQL (no GPU): the five C-ABI additions are declared, exported and bound, the build lists the new source,
the alias import works, configs/iql.py parses its flags and refuses what it must, what the Python class refuses it
refuses before the GPU is touched, the oracle's hand-written gradients are autograd's, and each of its variants moves
the actor or V."""
from __future__ import annotations

import sys
from pathlib import Path

import pytest
import torch as t

from oprl_amd.algos.iql import IQL
from oprl_amd.logging import NullLogger
from oracle import fixtures as fx
from tests.iql_oracle import IQLOracle
from tests.config_scripts import load_config
from tests.support import assert_abi_bound, assert_class_refuses, assert_source_built, small_nets

ROOT = Path(__file__).resolve().parents[1]
ENTRIES = {"oprl_learner_set_iql": 6, "oprl_learner_read_iql": 3, "oprl_learner_get_iql_step": 2,
           "oprl_learner_set_iql_step": 2, "oprl_iql_seed": 18}


def test_the_abi_additions_are_bound():
    lib, _header = assert_abi_bound(ENTRIES, mode_name="iql")            # a mode, not an algorithm: IQL is no field of the hparams
    # null arguments are refused without a GPU
    assert lib.oprl_learner_set_iql(None, None, 0.7, 3.0, 100.0, 3e-4) == -1 and b"null" in lib.oprl_last_error()
    assert lib.oprl_learner_read_iql(None, None, None) == -1 and b"null" in lib.oprl_last_error()
    assert lib.oprl_learner_get_iql_step(None, None) == -1 and b"null" in lib.oprl_last_error()
    assert lib.oprl_learner_set_iql_step(None, 3) == -1 and b"null" in lib.oprl_last_error()
    assert lib.oprl_iql_seed(*([None] * 5), 0.7, 3.0, 100.0, 4, 2, *([None] * 8)) == -1
    assert b"null" in lib.oprl_last_error()


def test_the_build_lists_the_new_source():
    assert_source_built("iql_seed")


def test_exports():
    import oprl.algos.iql
    import oprl_amd.algos
    from oprl_amd.algos.td3 import TD3
    assert oprl.algos.iql.IQL is IQL and oprl_amd.algos.IQL is IQL
    assert issubclass(IQL, TD3)
    algo = IQL(logger=NullLogger(), state_dim=4, action_dim=2)
    assert (algo.expectile, algo.beta, algo.adv_clip, algo.lr_value, algo.policy_freq) == (0.7, 3.0, 100.0, 3e-4, 1)


def test_the_config_script_parses_its_flags(monkeypatch):
    mod = load_config(monkeypatch, "iql", ["--env", "synthetic:walker-walk", "--dataset", "d.npz", "--expectile", "0.9", "--beta", "10",
                                           "--adv-clip", "50", "--updates", "300", "--batch", "64", "--updates-per-call", "20",
                                           "--no-normalize", "--n-step", "3"])
    a = mod.script.args
    assert (a.dataset, a.expectile, a.beta, a.adv_clip, a.updates, a.batch, a.updates_per_call, a.no_normalize, a.n_step) == \
        ("d.npz", 0.9, 10.0, 50.0, 300, 64, 20, True, 3)
    assert mod.hparams_of(a) == dict(expectile=0.9, beta=10.0, adv_clip=50.0, batch_size=64)
    assert mod.config.state_dim == 24 and mod.config.action_dim == 6
    assert mod.script.algo_cls is IQL and not mod.script.takes_per
    mod = load_config(monkeypatch, "iql", ["--env", "synthetic:cheetah-run"])
    a = mod.script.args
    assert (a.dataset, a.expectile, a.beta, a.adv_clip, a.batch, a.no_normalize, a.n_step) == (None, 0.7, 3.0, 100.0, 256, False, 1)
    with pytest.raises(ValueError, match="--dataset"):
        mod.run()
    # the other scripts still parse as before
    from oprl_amd.parse_args import parse_args
    monkeypatch.setattr(sys, "argv", ["ddpg.py"])
    assert not hasattr(parse_args(), "expectile")


@pytest.mark.parametrize("argv,msg", [
    (["--per"], "--per"),
    (["--num-envs", "4"], "--num-envs"),
    (["--num-envs", "4", "--open-episodes"], "--open-episodes"),
    (["--open-episodes"], "--open-episodes"),
    (["--seeds", "2"], "--seeds"),
], ids=["per", "num-envs", "num-envs-open", "open-episodes", "seeds"])
def test_the_config_script_refuses(monkeypatch, argv, msg):
    """... before an environment is built or a file is opened."""
    import oprl_amd.buffers.offline_dataset as ds
    import oprl_amd.environment as env
    monkeypatch.setattr(env, "make_env", lambda *a, **k: pytest.fail("an environment was built"))
    monkeypatch.setattr(ds, "load_dataset", lambda *a, **k: pytest.fail("a dataset was opened"))
    with pytest.raises(ValueError, match=msg):
        load_config(monkeypatch, "iql", ["--env", "synthetic:walker-walk", *argv])


@pytest.mark.parametrize("kw,msg", [
    (dict(precision="x2"), "f32"),
    (dict(precision="bf16"), "f32"),
    (dict(export_grads=True), "export_grads"),
    (dict(prioritized=True), "priorit"),
    (dict(policy_freq=2), "policy_freq"),
    (dict(expectile=0.0), "expectile"),
    (dict(expectile=1.0), "expectile"),
    (dict(expectile=float("nan")), "expectile"),
    (dict(beta=-1.0), "beta"),
    (dict(beta=float("inf")), "beta"),
    (dict(adv_clip=0.0), "adv_clip"),
    (dict(adv_clip=float("nan")), "adv_clip"),
    (dict(lr_value=0.0), "lr_value"),
    (dict(lr_value=float("inf")), "lr_value"),
], ids=["x2", "bf16", "export_grads", "prioritized", "policy_freq", "tau-0", "tau-1", "tau-nan", "beta-negative", "beta-inf",
        "clip-0", "clip-nan", "lr-0", "lr-inf"])
def test_the_class_refuses_before_any_gpu_call(kw, msg, monkeypatch):
    """ValueError at construction; and again from create() for fields set afterwards — before require_gpu, which a
    machine without a GPU would fail with RuntimeError instead."""
    import oprl_amd.algos.td3 as mod
    assert_class_refuses(IQL, mod, kw, msg, monkeypatch)


def test_a_prioritized_buffer_is_refused():
    from oprl_amd.algos.base_algorithm import refuse_prioritized

    class Buf:
        prioritized = True
    with pytest.raises(ValueError, match="importance weights"):
        refuse_prioritized(IQL(logger=NullLogger(), state_dim=4, action_dim=2), Buf())


# ---- the oracle ----------------------------------------------------------------------------------------------------------
def small_oracle(**kw):
    S, A = 5, 3
    nets = small_nets(S, A, value=True)
    kw.setdefault("adv_clip", 1.2)       # (binds on some rows of these batches: asserted below)
    return IQLOracle(S, A, *nets, **kw), S, A


@pytest.mark.parametrize("kw", [{}, dict(sym=True), dict(no_clip=True), dict(beta=0.5, adv_clip=1.02), dict(expectile=0.9)],
                         ids=["iql", "sym", "no_clip", "beta-0.5", "tau-0.9"])
def test_the_manual_gradients_are_autograds(kw):
    """In float64, after one update (so that the nets have moved apart from their targets)."""
    o, S, A = small_oracle(**kw)
    B = 37
    o.update(*fx.make_batch(1, B, S, A))
    s, a = (x.double() for x in fx.make_batch(3, B, S, A)[:2])
    g_v, info = o.value_grads(s, a)
    u = info["u"]
    assert float((u < 0).sum()) > 0 and float((u > 0).sum()) > 0          # both branches of omega
    g_a, ainfo = o.actor_grads(s, a, u)
    if not kw.get("no_clip"):
        assert 0.0 < float(ainfo["clip_frac"]) < 1.0                          # the clip binds on some rows only
    for manual, auto in ((g_v, o.value_grads_autograd(s, a)), (g_a, o.actor_grads_autograd(s, a, u))):
        for g, h in zip(manual, auto):
            assert float((g - h).abs().max()) <= 1e-12 * max(float(h.abs().max()), 1e-30) + 1e-18


def test_every_variant_moves_the_actor_or_v():
    """tau = 0.5, V(s') and u read after the V step, no clip and another beta each end somewhere else after three
    updates; and the critic step of update 0 reads V(s') from before the V step (the late variant's critic differs)."""
    lr = dict(lr_value=1e-2)          # (V moves far enough in one step for "before or after its step" to show in three updates)
    o, S, A = small_oracle(**lr)
    variants = {"sym": small_oracle(sym=True, **lr)[0], "late": small_oracle(late=True, **lr)[0],
                "no_clip": small_oracle(no_clip=True, **lr)[0], "beta": small_oracle(beta=1.0, **lr)[0]}
    B = 20
    for k in range(3):
        batch = fx.make_batch(5 + k, B, S, A)
        for x in (o, *variants.values()):
            x.update(*batch)
        if k == 0:
            assert all(t.equal(x, y) for x, y in zip(o.critic, variants["no_clip"].critic))     # (the clip is the actor's alone)
            assert not all(t.equal(x, y) for x, y in zip(o.critic, variants["late"].critic))
    for name, other in variants.items():
        moved = max(float((x - y).abs().max()) for x, y in zip(o.actor + o.value, other.actor + other.value))
        assert moved > 1e-5, (name, moved)
