"""Host side of CQL (no GPU): the five C-ABI additions are declared, exported and bound, the build lists the new source,
the alias import works, configs/cql.py parses its flags and refuses what it must, what the Python class refuses it
refuses before the GPU is touched, the oracle's hand-written seeds are autograd's, and each of its variants moves the
critics at the GPU comparison's own shapes."""
from __future__ import annotations

import sys
from pathlib import Path

import pytest
import torch as t

from oprl_amd.algos.cql import CQL, wide_rows
from oprl_amd.logging import NullLogger
from oracle import fixtures as fx
from tests import cql_oracle as co
from tests import scenarios as sc
from tests.config_scripts import load_config
from tests.support import assert_abi_bound, assert_class_refuses, assert_source_built, small_nets

ROOT = Path(__file__).resolve().parents[1]
ENTRIES = {"oprl_learner_set_cql": 3, "oprl_learner_read_cql": 3, "oprl_learner_set_cql_noise": 3, "oprl_cql_rows": 16,
           "oprl_cql_seed": 18}


def test_the_abi_additions_are_bound():
    lib, _header = assert_abi_bound(ENTRIES, mode_name="cql")            # a mode, not an algorithm: CQL is no field of the hparams
    # null arguments are refused without a GPU
    assert lib.oprl_learner_set_cql(None, 5.0, 10) == -1 and b"null" in lib.oprl_last_error()
    assert lib.oprl_learner_read_cql(None, None, None) == -1 and b"null" in lib.oprl_last_error()
    assert lib.oprl_learner_set_cql_noise(None, None, None) == -1 and b"null" in lib.oprl_last_error()
    assert lib.oprl_cql_rows(*([None] * 6), 0, 0, 4, 3, 2, 2, *([None] * 4)) == -1 and b"null" in lib.oprl_last_error()
    assert lib.oprl_cql_seed(*([None] * 7), 0.2, 0.99, 5.0, 2, 4, 2, *([None] * 5)) == -1 and b"null" in lib.oprl_last_error()


def test_the_build_lists_the_new_source():
    assert_source_built("cql_seed")


def test_exports_and_the_workspace_the_class_asks_for():
    import oprl.algos.cql
    import oprl_amd.algos
    from oprl_amd.algos.sac import SAC
    assert oprl.algos.cql.CQL is CQL and oprl_amd.algos.CQL is CQL
    assert issubclass(CQL, SAC)
    algo = CQL(logger=NullLogger(), state_dim=4, action_dim=2)
    assert (algo.cql_alpha, algo.cql_n_actions, algo.batch_size, algo.tune_alpha) == (5.0, 10, 256, False)
    # oprl_learner_create sets no ceiling on max_batch: the default N stays the paper's 10, and create() sizes the
    # workspace for batch_size (1 + 3 N) rows
    assert wide_rows(256, 10) == 7936 and wide_rows(100, 2) == 700 and wide_rows(16, 16) == 784


def test_the_config_script_parses_its_flags(monkeypatch):
    mod = load_config(monkeypatch, "cql", ["--env", "synthetic:walker-walk", "--dataset", "d.npz", "--cql-alpha", "1.5", "--cql-actions", "4",
                                           "--tune-alpha", "--updates", "300", "--batch", "64", "--updates-per-call", "20",
                                           "--no-normalize", "--n-step", "3"])
    a = mod.script.args
    assert (a.dataset, a.cql_alpha, a.cql_actions, a.tune_alpha, a.updates, a.batch, a.updates_per_call, a.no_normalize, a.n_step) == \
        ("d.npz", 1.5, 4, True, 300, 64, 20, True, 3)
    assert mod.hparams_of(a) == dict(cql_alpha=1.5, cql_n_actions=4, tune_alpha=True, batch_size=64)
    assert mod.config.state_dim == 24 and mod.config.action_dim == 6
    assert mod.script.algo_cls is CQL and not mod.script.takes_per
    mod = load_config(monkeypatch, "cql", ["--env", "synthetic:cheetah-run"])
    a = mod.script.args
    assert (a.dataset, a.cql_alpha, a.cql_actions, a.tune_alpha, a.batch, a.no_normalize, a.n_step) == (None, 5.0, 10, False, 256, False, 1)
    with pytest.raises(ValueError, match="--dataset"):
        mod.run()
    # the other scripts still parse as before
    from oprl_amd.parse_args import parse_args
    monkeypatch.setattr(sys, "argv", ["ddpg.py"])
    assert not hasattr(parse_args(), "cql_alpha")


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
        load_config(monkeypatch, "cql", ["--env", "synthetic:walker-walk", *argv])


@pytest.mark.parametrize("kw,msg", [
    (dict(precision="x2"), "f32"),
    (dict(precision="bf16"), "f32"),
    (dict(export_grads=True), "export_grads"),
    (dict(prioritized=True), "priorit"),
    (dict(cql_alpha=-1.0), "cql_alpha"),
    (dict(cql_alpha=float("nan")), "cql_alpha"),
    (dict(cql_alpha=float("inf")), "cql_alpha"),
    (dict(cql_n_actions=0), "cql_n_actions"),
    (dict(cql_n_actions=17), "cql_n_actions"),
    (dict(cql_n_actions=2.5), "cql_n_actions"),
], ids=["x2", "bf16", "export_grads", "prioritized", "alpha-negative", "alpha-nan", "alpha-inf", "N-0", "N-17", "N-fraction"])
def test_the_class_refuses_before_any_gpu_call(kw, msg, monkeypatch):
    """ValueError at construction; and again from create() for fields set afterwards — before require_gpu, which a
    machine without a GPU would fail with RuntimeError instead."""
    import oprl_amd.algos.sac as mod
    assert_class_refuses(CQL, mod, kw, msg, monkeypatch)


def test_a_prioritized_buffer_is_refused():
    from oprl_amd.algos.base_algorithm import refuse_prioritized

    class Buf:
        prioritized = True
    with pytest.raises(ValueError, match="importance weights"):
        refuse_prioritized(CQL(logger=NullLogger(), state_dim=4, action_dim=2), Buf())


# ---- the oracle ----------------------------------------------------------------------------------------------------------
def small_oracle(**kw):
    S, A = 5, 3
    kw.setdefault("n_actions", 4)
    return co.CQLOracle(S, A, *small_nets(S, A, gaussian=True), **kw), S, A


def draws(seed, B, A, N):
    import numpy as np
    uni = t.from_numpy(np.random.RandomState(seed + 3).uniform(-1, 1, (B, N, A)).astype(np.float32))
    return fx.make_noise(seed, (B, A)), fx.make_noise(seed + 1, (B, A)), fx.make_noise(seed + 2, (B, 2 * N, A)), uni


@pytest.mark.parametrize("kw", [{}, dict(cql_alpha=0.0), dict(no_logd=True), dict(at_next=True), dict(n_actions=1), dict(tune_alpha=True)],
                         ids=["cql", "alpha-0", "no_logd", "at_next", "N-1", "tune_alpha"])
def test_the_manual_seeds_are_autograds(kw):
    """In float64, after one update (so that the critics have moved apart from their targets): the hand-written seeds,
    sent down the critics by the oracle's backward pass, give the gradient autograd takes from the loss."""
    o, S, A = small_oracle(**kw)
    B = 37
    o.update(*fx.make_batch(1, B, S, A), *draws(20, B, A, o.N))
    batch = [x.double() for x in fx.make_batch(3, B, S, A)]
    en, _, eps, uni = (x.double() for x in draws(30, B, A, o.N))
    y, ws, wa, logd = o.operands(*batch, en, eps, uni)
    assert ws.shape == (B * (1 + 3 * o.N), S) and logd.shape == (B, 3 * o.N)
    manual, info = o.critic_grads(y, ws, wa, logd)
    auto = o.critic_grads_autograd(y, ws, wa, logd)
    assert len(manual) == len(auto) == 12
    for g, h in zip(manual, auto):
        assert float((g - h).abs().max()) <= 1e-12 * max(float(h.abs().max()), 1e-30) + 1e-18
    if o.cql_alpha > 0:
        assert float(info["gap1"]) > 0             # logsumexp over 3 N >= 3 entries with densities below 1 lies above Q on most rows


def test_the_seed_rows_sum_as_the_loss_says():
    """Per critic the sampled rows' seeds of a minibatch row sum to cql_alpha / B (a softmax), so with the data row's
    -cql_alpha / B the penalty's seeds of a row sum to zero; scale_bw divides by Bw instead."""
    q = t.randn(5 * 7, dtype=t.float64, generator=t.Generator().manual_seed(1))
    y = t.randn(5, dtype=t.float64, generator=t.Generator().manual_seed(2))
    logd = t.randn(5, 6, dtype=t.float64, generator=t.Generator().manual_seed(3))
    rows = co.seed_rows(q, y, logd, 3.0, 2)
    pen = rows["seed"][:5] - 2.0 * (q[:5] - y) / 5 + rows["seed"][5:].reshape(5, 6).sum(1)
    assert float(pen.abs().max()) < 1e-15
    assert t.allclose(co.seed_rows(q, y, logd, 3.0, 2, scale_rows=35)["seed"] * 7, rows["seed"], rtol=0, atol=1e-15)


@pytest.mark.parametrize("B,N", co.SHAPES, ids=[f"B{b}-N{n}" for b, n in co.SHAPES])
def test_every_variant_moves_a_critic_parameter(B, N):
    """At the GPU comparison's own nets, rows and draws (tests/test_gpu_cql.py), within three updates: cql_alpha = 0, no
    log-density correction, the third kind evaluated at s' and seeds scaled by 1/Bw each leave some critic parameter
    more than ten parameter gates from the true update's, so that comparison can tell them apart."""
    S, A = fx.ENVS[co.ENV]
    mk = lambda ca=co.CQL_ALPHA, **kw: co.CQLOracle(S, A, *co.fixture_nets(), cql_alpha=ca, n_actions=N, **kw)    # noqa: E731
    o = mk()
    variants = {"cql_alpha = 0": mk(0.0), "no_logd": mk(no_logd=True), "at_next": mk(at_next=True), "scale_bw": mk(scale_bw=True)}
    for batch, en, ec, eps, uni in co.parity_data(B, N, 3):
        for x in (o, *variants.values()):
            x.update(*batch, en, ec, eps, uni)
    for name, other in variants.items():
        gates = max(sc.rel_dev(x.numpy(), y.numpy()) for x, y in zip(other.critic, o.critic)) / sc.PARAM_TOL
        assert gates > 10.0, (name, gates)
