"""Host side of TD3+BC (no GPU): the three C-ABI additions are declared, exported and bound, the build lists the new
source, the alias import works, configs/td3_bc.py parses its flags and refuses what it must, what the Python class
refuses it refuses before the GPU is touched, and the oracle's hand-written gradient is autograd's."""
from __future__ import annotations

import sys
from pathlib import Path

import pytest
import torch as t

from oprl_amd.algos.td3_bc import TD3BC
from oprl_amd.logging import NullLogger
from oracle import fixtures as fx
from tests.td3bc_oracle import TD3BCOracle
from tests.config_scripts import load_config
from tests.support import assert_abi_bound, assert_class_refuses, assert_source_built, small_nets

ROOT = Path(__file__).resolve().parents[1]
ENTRIES = {"oprl_learner_set_bc": 2, "oprl_learner_read_bc": 3, "oprl_bc_seed": 12}


def test_the_abi_additions_are_bound():
    lib, _header = assert_abi_bound(ENTRIES, mode_name="td3bc")          # a mode, not an algorithm: BC is no field of the hparams
    # null arguments are refused without a GPU
    assert lib.oprl_learner_set_bc(None, 2.5) == -1 and b"null" in lib.oprl_last_error()
    assert lib.oprl_learner_read_bc(None, None, None) == -1 and b"null" in lib.oprl_last_error()
    assert lib.oprl_bc_seed(None, None, None, None, 2.5, 4, 2, None, None, None, None, None) == -1
    assert b"null" in lib.oprl_last_error()


def test_the_build_lists_the_new_source():
    assert_source_built("bc_seed")


def test_exports():
    import oprl.algos.td3_bc
    import oprl.buffers.offline_dataset
    import oprl.trainers.offline_trainer
    import oprl_amd.algos
    from oprl_amd.algos.td3 import TD3
    assert oprl.algos.td3_bc.TD3BC is TD3BC and oprl_amd.algos.TD3BC is TD3BC
    assert issubclass(TD3BC, TD3)
    assert oprl.buffers.offline_dataset.fill_replay.__module__ == "oprl_amd.buffers.offline_dataset"
    assert oprl.trainers.offline_trainer.OfflineTrainer.__module__ == "oprl_amd.trainers.offline_trainer"
    algo = TD3BC(logger=NullLogger(), state_dim=4, action_dim=2)
    assert algo.bc_alpha == 2.5 and algo.policy_freq == 2


def test_the_config_script_parses_its_flags(monkeypatch):
    mod = load_config(monkeypatch, "td3_bc", ["--env", "synthetic:walker-walk", "--dataset", "d.npz", "--bc-alpha", "1.5",
                                              "--updates", "300", "--batch", "64", "--no-normalize", "--n-step", "3"])
    a = mod.script.args
    assert (a.dataset, a.bc_alpha, a.updates, a.batch, a.no_normalize, a.n_step) == ("d.npz", 1.5, 300, 64, True, 3)
    assert mod.alpha_of(a) == dict(bc_alpha=1.5, batch_size=64)
    assert mod.config.state_dim == 24 and mod.config.action_dim == 6
    assert mod.script.algo_cls is TD3BC and not mod.script.takes_per
    mod = load_config(monkeypatch, "td3_bc", ["--env", "synthetic:cheetah-run"])
    a = mod.script.args
    assert (a.dataset, a.bc_alpha, a.batch, a.no_normalize, a.n_step) == (None, 2.5, 256, False, 1)
    with pytest.raises(ValueError, match="--dataset"):
        mod.run()
    # the other scripts still parse as before
    from oprl_amd.parse_args import parse_args
    monkeypatch.setattr(sys, "argv", ["ddpg.py"])
    assert not hasattr(parse_args(), "bc_alpha")


@pytest.mark.parametrize("argv,msg", [
    (["--per"], "--per"),
    (["--num-envs", "4"], "--num-envs"),
    (["--num-envs", "4", "--open-episodes"], "--open-episodes"),
    (["--open-episodes"], "--open-episodes"),
], ids=["per", "num-envs", "num-envs-open", "open-episodes"])
def test_the_config_script_refuses(monkeypatch, argv, msg):
    """... before an environment is built or a file is opened."""
    import oprl_amd.buffers.offline_dataset as ds
    import oprl_amd.environment as env
    monkeypatch.setattr(env, "make_env", lambda *a, **k: pytest.fail("an environment was built"))
    monkeypatch.setattr(ds, "load_dataset", lambda *a, **k: pytest.fail("a dataset was opened"))
    with pytest.raises(ValueError, match=msg):
        load_config(monkeypatch, "td3_bc", ["--env", "synthetic:walker-walk", *argv])


@pytest.mark.parametrize("kw,msg", [
    (dict(precision="x2"), "f32"),
    (dict(precision="bf16"), "f32"),
    (dict(export_grads=True), "export_grads"),
    (dict(prioritized=True), "priorit"),
    (dict(bc_alpha=0.0), "bc_alpha"),
    (dict(bc_alpha=-1.0), "bc_alpha"),
    (dict(bc_alpha=float("nan")), "bc_alpha"),
    (dict(bc_alpha=float("inf")), "bc_alpha"),
], ids=["x2", "bf16", "export_grads", "prioritized", "alpha-0", "alpha-negative", "alpha-nan", "alpha-inf"])
def test_the_class_refuses_before_any_gpu_call(kw, msg, monkeypatch):
    """ValueError at construction; and again from create() for fields set afterwards — before require_gpu, which a
    machine without a GPU would fail with RuntimeError instead."""
    import oprl_amd.algos.td3 as mod
    assert_class_refuses(TD3BC, mod, kw, msg, monkeypatch)


def test_a_prioritized_buffer_is_refused():
    from oprl_amd.algos.base_algorithm import refuse_prioritized

    class Buf:
        prioritized = True
    with pytest.raises(ValueError, match="importance weights"):
        refuse_prioritized(TD3BC(logger=NullLogger(), state_dim=4, action_dim=2), Buf())


# ---- the oracle ----------------------------------------------------------------------------------------------------------
def small_oracle(**kw):
    S, A = 5, 3
    return TD3BCOracle(S, A, *small_nets(S, A), **kw), S, A


@pytest.mark.parametrize("kw", [{}, dict(no_bc=True), dict(no_lambda=True), dict(bc_alpha=0.3)],
                         ids=["td3bc", "no_bc", "no_lambda", "alpha-0.3"])
def test_the_manual_gradient_is_autograds(kw):
    """In float64, after one update (so that critic and actor have moved apart from their targets)."""
    o, S, A = small_oracle(**kw)
    B = 37
    o.update(*fx.make_batch(1, B, S, A), fx.make_noise(2, (B, A)))
    s, a = (x.double() for x in fx.make_batch(3, B, S, A)[:2])
    manual, info = o.actor_grads(s, a)
    auto = o.actor_grads_autograd(s, a)
    for g, h in zip(manual, auto):
        assert float((g - h).abs().max()) <= 1e-12 * max(float(h.abs().max()), 1e-30) + 1e-18
    if not kw.get("no_lambda"):
        assert float(info["bc_lambda"]) == pytest.approx(o.bc_alpha / float(info["q_abs_mean"]), rel=1e-14)
    else:
        assert float(info["bc_lambda"]) == 1.0


def test_the_variants_differ_and_the_critic_step_is_td3s():
    """no_bc and no_lambda give other actors; the critic after update 0 is TD3Oracle's, bit for bit (it steps before
    the actor), and so is a whole run with the cloning term dropped and lambda = 1: plain TD3."""
    from oracle import oprl_oracle as orc
    o, S, A = small_oracle()
    nb, _, _ = small_oracle(no_bc=True)
    nl, _, _ = small_oracle(no_lambda=True)
    plain, _, _ = small_oracle(no_bc=True, no_lambda=True)
    td3 = orc.TD3Oracle(S, A, *[[x.double() for x in n] for n in (o.actor, o._q(o.critic, 0), o._q(o.critic, 1))])
    B = 20
    for k in range(3):
        batch = [x.double() for x in (*fx.make_batch(5 + k, B, S, A), fx.make_noise(9 + k, (B, A)))]
        for x in (o, nb, nl, plain, td3):
            x.update(*batch)
        if k == 0:
            assert all(t.equal(x, y) for x, y in zip(o.critic, td3.critic))
    assert all(t.equal(x, y) for x, y in zip(plain.actor + plain.critic + plain.critic_target, td3.actor + td3.critic + td3.critic_target))
    for other in (nb, nl, td3):
        assert max(float((x - y).abs().max()) for x, y in zip(o.actor, other.actor)) > 1e-5
