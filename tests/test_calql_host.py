"""Host side of Cal-QL (no GPU): the four C-ABI additions are declared, exported and bound and refuse null
handles, the build lists the new source, the alias import works, the class refuses what CQL refuses and ``update()``
without returns, the returns oracle gives the hand-computed values and its float32 restatement stays inside its own
tolerance, the calibrated oracle's seeds are autograd's, and configs/calql.py refuses its flags before an environment is
built or a file is looked at."""
from __future__ import annotations

from pathlib import Path

import numpy as np
import pytest
import torch as t

from oprl_amd import _capi
from oprl_amd.algos.calql import CalQL
from oprl_amd.algos.cql import CQL
from oprl_amd.logging import NullLogger
from oracle import fixtures as fx
from tests import calql_oracle as cal
from tests.config_scripts import load_config
from tests.support import assert_abi_bound, assert_class_refuses, assert_source_built, small_nets

ROOT = Path(__file__).resolve().parents[1]
ENTRIES = {"oprl_replay_returns": 7, "oprl_cql_seed_cal": 19, "oprl_learner_set_calql": 2, "oprl_learner_update_calql": 11}


def test_the_abi_additions_are_bound():
    lib, _header = assert_abi_bound(ENTRIES, mode_name="calql")          # a form of a mode
    # oprl_cql_seed's signature and g
    assert len(_capi.SIGNATURES["oprl_cql_seed_cal"][1]) == len(_capi.SIGNATURES["oprl_cql_seed"][1]) + 1
    # null handles and pointers are refused without a GPU
    assert lib.oprl_replay_returns(None, 4, None, None, 0.99, None, None) == -1 and b"null" in lib.oprl_last_error()
    assert lib.oprl_learner_set_calql(None, 1) == -1 and b"null" in lib.oprl_last_error()
    assert lib.oprl_learner_update_calql(*([None] * 7), 4, None, None, None) == -1 and b"null" in lib.oprl_last_error()
    assert lib.oprl_cql_seed_cal(*([None] * 7), 0.2, 0.99, 5.0, 2, 4, 2, *([None] * 6)) == -1 and b"null" in lib.oprl_last_error()


def test_the_build_lists_the_new_source():
    assert_source_built("replay_returns", header=False)


def test_exports():
    import oprl.algos.calql
    import oprl_amd.algos
    assert oprl.algos.calql.CalQL is CalQL and oprl_amd.algos.CalQL is CalQL
    assert issubclass(CalQL, CQL)
    algo = CalQL(logger=NullLogger(), state_dim=4, action_dim=2)
    assert (algo.cql_alpha, algo.cql_n_actions, algo.batch_size, algo.tune_alpha) == (5.0, 10, 256, False)


@pytest.mark.parametrize("kw,msg", [
    (dict(precision="x2"), "f32"),
    (dict(precision="bf16"), "f32"),
    (dict(export_grads=True), "export_grads"),
    (dict(prioritized=True), "priorit"),
    (dict(cql_alpha=-1.0), "cql_alpha"),
    (dict(cql_n_actions=17), "cql_n_actions"),
], ids=["x2", "bf16", "export_grads", "prioritized", "alpha-negative", "N-17"])
def test_the_class_refuses_before_any_gpu_call(kw, msg, monkeypatch):
    import oprl_amd.algos.sac as mod
    assert_class_refuses(CalQL, mod, kw, msg, monkeypatch)


def test_update_needs_returns():
    """Said before the learner is looked at: an instance that was never created raises the same ValueError."""
    algo = CalQL(logger=NullLogger(), state_dim=4, action_dim=2, batch_size=3)
    rows = fx.make_batch(1, 3, 4, 2)
    with pytest.raises(ValueError, match="returns"):
        algo.update(*rows)
    with pytest.raises(ValueError, match="priorit"):
        algo.update(*rows, returns=t.zeros(3), weights=t.ones(3))


def test_a_cpu_buffer_has_no_returns():
    from oprl_amd.buffers.episodic_buffer import EpisodicReplayBuffer
    buf = EpisodicReplayBuffer(buffer_size_transitions=20, state_dim=3, action_dim=1, max_episode_lenth=5).create()
    with pytest.raises(RuntimeError, match="cuda"):
        buf.returns_to_go([0], [0])


# ---- the returns oracle ----------------------------------------------------------------------------------------------------
def hand_storage():
    r = np.zeros((3, 4), np.float32)
    d = np.zeros((3, 4), np.float32)
    r[0, :3] = [1, 2, 3]
    r[1, :3] = [1, 2, 3]
    d[1, 1] = 1
    r[2] = [5, 6, 7, 8]
    return r, d, [3, 3]            # two live episodes of three steps; slot 2 is past them


def test_the_oracle_on_hand_written_storage():
    r, d, lens = hand_storage()
    G = lambda e, s, gamma=0.5: float(cal.returns_to_go(r, d, lens, [e], [s], gamma)[0])      # noqa: E731
    assert G(0, 0) == 2.75                     # 1 + 0.5 2 + 0.25 3
    assert G(1, 0) == 2.0                      # a done at step 1 ends the sum there
    assert G(1, 1) == 2.0 and G(1, 2) == 3.0   # ... at the done itself; behind it the tail goes on
    assert G(0, 1) == 3.5 and G(0, 2) == 3.0
    assert G(0, 0, 1.0) == 6.0
    assert G(0, 3) == 0.0 and G(2, 1) == 6.0   # t >= len_e: the single stored term
    assert G(3, 0) == 0.0 and G(-1, 0) == 0.0 and G(0, 4) == 0.0 and G(0, -1) == 0.0      # outside the storage
    assert float(cal.returns_to_go(-r, d, lens, [0], [0], 0.5, absolute=True)[0]) == 2.75
    got = cal.returns_f32(r, d, lens, [0, 1, 0, 2, 3], [0, 0, 3, 1, 0], 0.5)
    assert got.dtype == np.float32 and got.tolist() == [2.75, 2.0, 0.0, 6.0, 0.0]


def test_the_float32_restatement_stays_inside_the_tolerance():
    """Tails over one, two and three chunks of 64, random rewards of both signs: the restated order is within
    c 2^-24 sum gamma^k |r_k| of float64 with c = 2 (9 + ceil(L / 64)), the bound DESIGN.md §21 counts."""
    L = 150
    rng = np.random.RandomState(3)
    r = rng.randn(4, L).astype(np.float32) * 3
    d = np.zeros((4, L), np.float32)
    d[1, 100] = 1
    lens = [150, 129, 64, 1]
    ep = np.repeat(np.arange(4), L)
    step = np.tile(np.arange(L), 4)
    assert cal.roundings(L) == 12 and cal.roundings(12) == 10 and cal.roundings(1000) == 25
    for gamma in (1.0, 0.99, 0.5):
        want = cal.returns_to_go(r, d, lens, ep, step, gamma)
        got = cal.returns_f32(r, d, lens, ep, step, gamma).astype(np.float64)
        tol = cal.tolerance(r, d, lens, ep, step, gamma)
        assert np.all(np.abs(got - want) <= tol), float(np.max(np.abs(got - want) / np.maximum(tol, 1e-300)))


def test_mixed_returns_split_by_row_index():
    r, d, lens = hand_storage()
    prior, own = (None, None, r, d), (None, None, 2 * r, d)
    got = cal.mixed_returns(prior, lens, own, lens, 0.5, [0, 0, 0, 0, 0], [0, 0, 0, 0, 0], 0.5)
    assert got.tolist() == [2.75, 2.75, 2.75, 5.5, 5.5]          # n_prior(5, 0.5) = 3


# ---- the calibrated oracle -------------------------------------------------------------------------------------------------
def small_oracle(**kw):
    S, A = 5, 3
    kw.setdefault("n_actions", 4)
    return cal.CalQLOracle(S, A, *small_nets(S, A, gaussian=True), **kw), S, A


def draws(seed, B, A, N):
    uni = t.from_numpy(np.random.RandomState(seed + 3).uniform(-1, 1, (B, N, A)).astype(np.float32))
    return fx.make_noise(seed, (B, A)), fx.make_noise(seed + 1, (B, A)), fx.make_noise(seed + 2, (B, 2 * N, A)), uni


def test_the_calibrated_seeds_are_autograds():
    """In float64: the hand-written seeds with the gradient mask give the gradient autograd takes from the loss with
    max(q, g) inside the logsumexp; some entries are bounded and some are not, so both branches are in it."""
    o, S, A = small_oracle()
    B = 37
    g0 = t.linspace(-1.0, 1.0, B, dtype=t.float64)
    o.update(*fx.make_batch(1, B, S, A), *draws(20, B, A, o.N), g0)
    batch = [x.double() for x in fx.make_batch(3, B, S, A)]
    en, _, eps, uni = (x.double() for x in draws(30, B, A, o.N))
    y, ws, wa, logd = o.operands(*batch, en, eps, uni)
    q = orc_q(o, ws, wa)[B:]
    o._g = t.quantile(q, 0.5) + 0.0 * g0                     # the median of the entries' values: about half are bounded
    manual, info = o.critic_grads(y, ws, wa, logd)
    assert 0.2 < info["bound_rate"] < 0.8
    auto = o.critic_grads_autograd(y, ws, wa, logd)
    for g, h in zip(manual, auto):
        assert float((g - h).abs().max()) <= 1e-12 * max(float(h.abs().max()), 1e-30) + 1e-18


def orc_q(o, ws, wa):
    from oracle import oprl_oracle as orc
    return orc.q_forward(o._q(o.critic, 0), ws, wa)[-1].reshape(-1)


def test_the_bound_at_its_ends_and_at_equality():
    from tests import cql_oracle as co
    gen = t.Generator().manual_seed(1)
    B, N = 5, 2
    q = t.randn(B * (1 + 3 * N), dtype=t.float64, generator=gen)
    y = t.randn(B, dtype=t.float64, generator=gen)
    logd = t.randn(B, 3 * N, dtype=t.float64, generator=gen)
    plain = co.seed_rows(q, y, logd, 3.0, N)
    low = cal.seed_rows(q, y, logd, t.full((B,), -float("inf"), dtype=t.float64), 3.0, N)
    assert t.equal(low["seed"], plain["seed"]) and t.equal(low["lse"], plain["lse"]) and low["bound"] == 0
    high = cal.seed_rows(q, y, logd, t.full((B,), 1e30, dtype=t.float64), 3.0, N)
    assert high["bound"] == B * 2 * N
    assert float(high["seed"][B:].reshape(B, 3 * N)[:, N:].abs().max()) == 0.0
    assert t.equal(high["seed"][:B], plain["seed"][:B])
    # q_e == g_b exactly: the entry keeps its gradient and is not counted
    g = q[B:].reshape(B, 3 * N)[:, N].clone()
    eq = cal.seed_rows(q, y, logd, g, 3.0, N)
    assert bool((eq["seed"][B:].reshape(B, 3 * N)[:, N] > 0).all())
    assert eq["bound"] == int((q[B:].reshape(B, 3 * N)[:, N:] < g.reshape(B, 1)).sum())


# ---- configs/calql.py -------------------------------------------------------------------------------------------------------
def test_the_config_script_parses_its_flags(monkeypatch):
    mod = load_config(monkeypatch, "calql", ["--env", "synthetic:walker-walk", "--dataset", "d.npz", "--cql-alpha", "1.5", "--cql-actions", "4",
                                             "--tune-alpha", "--updates", "300", "--batch", "64", "--updates-per-call", "20",
                                             "--no-normalize", "--finetune-steps", "40", "--prior-share", "0.25"])
    a = mod.script.args
    assert (a.dataset, a.cql_alpha, a.cql_actions, a.tune_alpha, a.updates, a.batch, a.updates_per_call, a.no_normalize) == \
        ("d.npz", 1.5, 4, True, 300, 64, 20, True)
    assert (mod.finetune_steps, a.prior_share) == (40, 0.25)
    assert mod.hparams_of(a) == dict(cql_alpha=1.5, cql_n_actions=4, tune_alpha=True, batch_size=64)
    assert mod.script.algo_cls is CalQL and not mod.script.takes_per
    mod = load_config(monkeypatch, "calql", ["--env", "synthetic:cheetah-run", "--n-step", "3"])
    assert mod.finetune_steps == 0 and mod.script.args.n_step == 3
    with pytest.raises(ValueError, match="--dataset"):
        mod.run()


@pytest.mark.parametrize("argv,msg", [
    (["--her"], "--her"),
    (["--per"], "--per"),
    (["--num-envs", "4"], "--num-envs"),
    (["--open-episodes"], "--open-episodes"),
    (["--seeds", "2"], "--seeds"),
    (["--finetune-steps", "10", "--n-step", "3"], "--n-step"),
    (["--finetune-steps", "-1"], "--finetune-steps"),
    (["--prior-data", "p.npz"], "--prior-data"),
], ids=["her", "per", "num-envs", "open-episodes", "seeds", "finetune-nstep", "finetune-negative", "prior-data"])
def test_the_config_script_refuses(monkeypatch, argv, msg):
    """... before an environment is built or a file is opened."""
    import oprl_amd.buffers.offline_dataset as ds
    import oprl_amd.environment as env
    monkeypatch.setattr(env, "make_env", lambda *a, **k: pytest.fail("an environment was built"))
    monkeypatch.setattr(ds, "load_dataset", lambda *a, **k: pytest.fail("a dataset was opened"))
    with pytest.raises(ValueError, match=msg):
        load_config(monkeypatch, "calql", ["--env", "synthetic:walker-walk", "--dataset", "none.npz", *argv])
