"""CPU tests of hindsight replay's host side: the C-ABI surface and its null-handle checks, the build
list, the alias, the Python buffer's validation, the command-line flags and what configs/_common.py refuses, the
goal-conditioned synthetic environment, and the statistics of tests/her_oracle.py's draws (no GPU needed)."""
from __future__ import annotations

import math
import sys
from pathlib import Path

import numpy as np
import pytest

from oprl_amd import _capi
from tests import her_oracle as ho
from tests import support
from tests.config_scripts import load_config

ROOT = Path(__file__).resolve().parents[1]
HER_FUNCS = {"oprl_replay_set_her": 8, "oprl_replay_sample_her": 14}


def cpu_buffer(**kw):
    from oprl_amd.buffers.hindsight_buffer import HindsightEpisodicReplayBuffer
    args = dict(state_dim=12, action_dim=3, goal_dim=3, achieved_offset=6, desired_offset=9, threshold=0.1)
    return support.cpu_buffer(HindsightEpisodicReplayBuffer, **{**args, **kw})


# ---- ABI and bindings ---------------------------------------------------------------------------------------------------
def test_her_functions_are_declared_bound_and_exported():
    support.assert_abi_bound(HER_FUNCS)
    assert len(_capi.ALGO) == 6


def test_her_functions_refuse_null_handles_without_a_gpu():
    lib = _capi.load()
    assert lib.oprl_replay_set_her(None, 6, 9, 3, 0.8, 0, 0, 0.05) == -1
    assert b"null replay handle" in lib.oprl_last_error()
    assert lib.oprl_replay_set_her(None, 0, 0, 0, 0.0, 0, 0, 0.0) == -1
    assert lib.oprl_replay_sample_her(None, 4, None, 0, 0, *([None] * 8), None) == -1
    assert len(lib.oprl_last_error()) > 0


def test_source_is_built_and_alias_resolves():
    support.assert_source_built("replay_her", header=False)
    from oprl.buffers.hindsight_buffer import HindsightEpisodicReplayBuffer as Aliased
    from oprl.environment.synthetic_goal import SyntheticGoalEnv as AliasedEnv
    from oprl_amd.buffers.episodic_buffer import EpisodicReplayBuffer
    from oprl_amd.buffers.hindsight_buffer import HindsightEpisodicReplayBuffer
    from oprl_amd.environment.synthetic_goal import SyntheticGoalEnv
    assert Aliased is HindsightEpisodicReplayBuffer and issubclass(Aliased, EpisodicReplayBuffer)
    assert AliasedEnv is SyntheticGoalEnv


# ---- the buffer class -----------------------------------------------------------------------------------------------------
def test_defaults_fields_and_state_dict():
    b = cpu_buffer().create()
    assert (b.her_ratio, b.strategy, b.reward) == (0.8, "future", "sparse") and len(b) == 0
    assert not getattr(b, "prioritized", False) and getattr(b, "n_step", 1) == 1
    sd = b.state_dict()
    assert sd["her"] == dict(goal_dim=3, achieved_offset=6, desired_offset=9, her_ratio=0.8, strategy="future",
                             reward="sparse", threshold=0.1)
    c = cpu_buffer(her_ratio=0.5, strategy="final", reward="dense", threshold=0.3, achieved_offset=0).create()
    c.load_state_dict(sd)
    assert (c.her_ratio, c.strategy, c.reward, c.threshold, c.achieved_offset) == (0.8, "future", "sparse", 0.1, 6)
    b.add_transition(np.ones(12), np.zeros(3), -1.0, False)
    assert len(b) == 1 and float(b.rewards[0, 0, 0]) == -1.0
    with pytest.raises(RuntimeError, match="MI355X"):
        b.sample(4)


@pytest.mark.parametrize("kw", [
    dict(goal_dim=0), dict(goal_dim=17, state_dim=40, achieved_offset=0, desired_offset=20), dict(goal_dim=2.5),
    dict(achieved_offset=-1), dict(desired_offset=10), dict(achieved_offset=10),              # a range outside [0, S)
    dict(achieved_offset=7), dict(achieved_offset=9), dict(achieved_offset=8, desired_offset=6),   # overlapping ranges
], ids=lambda kw: "-".join(f"{k}={v}" for k, v in kw.items()))
def test_bad_layouts_are_refused(kw):
    with pytest.raises(ValueError):
        cpu_buffer(**kw).create()


@pytest.mark.parametrize("kw", [dict(her_ratio=-0.1), dict(her_ratio=1.5), dict(her_ratio=float("nan")),
                                dict(her_ratio=float("inf"))])
def test_bad_ratios_are_refused(kw):
    with pytest.raises(ValueError, match="her_ratio"):
        cpu_buffer(**kw).create()


@pytest.mark.parametrize("kw", [dict(threshold=-1e-3), dict(threshold=float("nan")), dict(threshold=float("inf"))])
def test_bad_thresholds_are_refused(kw):
    with pytest.raises(ValueError, match="threshold"):
        cpu_buffer(**kw).create()


@pytest.mark.parametrize("kw", [dict(strategy="episode"), dict(strategy=0), dict(reward="shaped")])
def test_bad_strategies_and_reward_kinds_are_refused(kw):
    with pytest.raises(ValueError):
        cpu_buffer(**kw).create()


@pytest.mark.parametrize("kw", [dict(her_ratio=0.0), dict(her_ratio=1.0), dict(threshold=0.0), dict(strategy="final"),
                                dict(reward="dense"), dict(achieved_offset=0, desired_offset=3),
                                dict(goal_dim=16, state_dim=40, achieved_offset=2, desired_offset=21),
                                dict(goal_dim=1, achieved_offset=11, desired_offset=0)])
def test_edge_fields_are_accepted(kw):
    cpu_buffer(**kw).create()


# ---- flags and config -----------------------------------------------------------------------------------------------------
def test_her_flags(monkeypatch):
    from oprl_amd.parse_args import check_her, parse_args, parse_args_distrib
    monkeypatch.setattr(sys, "argv", ["x"])
    a = parse_args()
    assert (a.her, a.her_ratio, a.her_strategy) == (False, 0.8, "future") and not check_her(a)
    assert (a.n_step, a.per, a.num_envs, a.open_episodes, a.precision, a.env) == (1, False, 1, False, "f32", "cartpole-balance")
    assert not hasattr(parse_args_distrib(), "her")
    monkeypatch.setattr(sys, "argv", ["x", "--her", "--her-ratio", "0.5", "--her-strategy", "final"])
    a = parse_args()
    assert (a.her, a.her_ratio, a.her_strategy) == (True, 0.5, "final") and check_her(a)
    monkeypatch.setattr(sys, "argv", ["x", "--her", "--her-strategy", "episode"])
    with pytest.raises(SystemExit):
        parse_args()


GOAL_ENV = ["--env", "synthetic:goal-reach-2d"]


def test_config_refuses_her_with_per(monkeypatch):
    with pytest.raises(ValueError, match="--per"):
        load_config(monkeypatch, "ddpg", [*GOAL_ENV, "--her", "--per"])


def test_config_refuses_her_with_n_step(monkeypatch):
    with pytest.raises(ValueError, match="--n-step 3"):
        load_config(monkeypatch, "td3", [*GOAL_ENV, "--her", "--n-step", "3"])


def test_config_refuses_her_without_a_goal_layout(monkeypatch):
    with pytest.raises(ValueError, match="goal layout"):
        load_config(monkeypatch, "sac", ["--env", "synthetic:walker-walk", "--her"])


def test_config_refuses_her_in_the_offline_scripts(monkeypatch):
    with pytest.raises(ValueError, match="--her"):
        load_config(monkeypatch, "iql", [*GOAL_ENV, "--her"])


def test_config_builds_the_hindsight_buffer_from_the_environments_layout(monkeypatch):
    from oprl_amd.buffers.hindsight_buffer import HindsightEpisodicReplayBuffer
    mod = load_config(monkeypatch, "ddpg", [*GOAL_ENV, "--her", "--her-ratio", "0.5", "--device", "cpu"])
    assert mod.script.her and (mod.config.state_dim, mod.config.action_dim) == (8, 2)
    buf = mod.make_replay_buffer()
    assert type(buf) is HindsightEpisodicReplayBuffer
    assert (buf.goal_dim, buf.achieved_offset, buf.desired_offset, buf.her_ratio, buf.strategy, buf.max_episode_lenth) == (
        2, 4, 6, 0.5, "future", 50)
    assert buf.threshold == mod.make_env(seed=0).goal_layout["threshold"]
    # without the flag the same script builds what it built before
    from oprl_amd.buffers.episodic_buffer import EpisodicReplayBuffer
    plain = load_config(monkeypatch, "ddpg", [*GOAL_ENV, "--device", "cpu"])
    assert not plain.script.her and type(plain.make_replay_buffer()) is EpisodicReplayBuffer


# ---- the goal environment -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("task,S,A,G", [("goal-reach-2d", 8, 2, 2), ("goal-reach-3d", 12, 3, 3)])
def test_goal_env_shapes_layout_and_determinism(task, S, A, G):
    from oprl_amd.environment.make_env import make_env
    from oprl_amd.environment.synthetic import DM_CONTROL_DIMS
    assert task not in DM_CONTROL_DIMS and len(DM_CONTROL_DIMS) == 16

    def rollout(seed):
        env = make_env("synthetic:" + task, seed=seed)
        assert env.observation_space.shape == (S,) and env.action_space.shape == (A,) and env.env_family == "synthetic"
        lay = env.goal_layout
        assert (lay["achieved_offset"], lay["desired_offset"], lay["goal_dim"]) == (2 * G, 3 * G, G) and lay["threshold"] > 0
        rows, goals = [], []
        for _ep in range(2):
            obs, _ = env.reset()
            assert obs.dtype == np.float32 and obs.shape == (S,)
            goals.append(obs[3 * G:].copy())
            for k in range(env.episode_length):
                nxt, r, term, trunc, _ = env.step(env.sample_action())
                # the achieved goal is the position, the desired goal stays for the episode, the reward is the oracle's
                assert np.array_equal(nxt[2 * G:3 * G], nxt[:G]) and np.array_equal(nxt[3 * G:], goals[-1])
                assert r == float(ho.reward(nxt[2 * G:3 * G], nxt[3 * G:], ho.SPARSE, lay["threshold"])) and r in (0.0, -1.0)
                assert not term and trunc == (k == env.episode_length - 1)
                rows.append(np.concatenate([nxt, [r]]))
        assert env.episode_length == 50 and not np.array_equal(goals[0], goals[1])
        return np.array(rows)
    a, b, c = rollout(3), rollout(3), rollout(4)
    assert np.array_equal(a, b) and not np.array_equal(a, c)


def test_goal_env_reward_is_the_oracles_function_at_the_threshold():
    from oprl_amd.environment.synthetic_goal import sparse_reward
    rs = np.random.RandomState(0)
    hits = 0
    for _ in range(2000):
        a, g = rs.uniform(-1, 1, 3).astype(np.float32), rs.uniform(-1, 1, 3).astype(np.float32)
        thr = float(np.sqrt(np.float64(ho.dist2(a, g)))) * rs.choice([0.999999, 1.0, 1.000001])
        want = float(ho.reward(a, g, ho.SPARSE, thr))
        assert sparse_reward(a, g, thr) == want
        hits += want == 0.0
    assert 200 < hits < 1800          # both answers occur
    assert sparse_reward([0.5, 0.5], [0.5, 0.5], 0.0) == 0.0


def test_make_env_keeps_its_names_and_its_refusals():
    from oprl_amd.environment.make_env import make_env
    from oprl_amd.environment.synthetic import SyntheticEnv
    assert type(make_env("synthetic:walker-walk")) is SyntheticEnv and type(make_env("walker-walk")) is SyntheticEnv
    for name in ("goal-reach-2d", "synthetic:goal-reach-4d", "Ant-v4"):
        with pytest.raises(ValueError):
            make_env(name)


# ---- the oracle's draws -------------------------------------------------------------------------------------------------
N_ROWS, SEED = 100_000, 20260117


@pytest.fixture(scope="module")
def words():
    """The (y, z) words of N_ROWS draws: 100 batches (counters 0 .. 99) of 1000 rows under one seed."""
    return [ho.draw(SEED, counter, i)[1:3] for counter in range(100) for i in range(1000)]


def _choose(word, t, len_e, ratio, strategy):
    return ho.choose_from(*word, t, len_e, ratio, strategy)


def test_choose_draws_the_words_it_decides_from():
    for counter, i, t, len_e in ((0, 0, 0, 12), (3, 17, 4, 12), (99, 999, 10, 12), (5, 5, 11, 12), (7, 1, 0, 1), (7, 2, 0, 2)):
        for ratio in (0.0, 0.5, 0.8, 1.0):
            for strategy in (ho.FUTURE, ho.FINAL):
                assert ho.choose(SEED, counter, i, t, len_e, ratio, strategy) == _choose(
                    ho.draw(SEED, counter, i)[1:3], t, len_e, ratio, strategy)


@pytest.mark.parametrize("ratio", [0.5, 0.8])
def test_relabelled_share_of_eligible_rows(words, ratio):
    """Rows cycle through t = 0 .. 11 of a 12-step episode: t = 11 (c = 0) is never relabelled, the others with
    probability ratio, within 4 sigma (binomial)."""
    n = hit = 0
    for j, w in enumerate(words):
        t = j % 12
        tp = _choose(w, t, 12, ratio, ho.FUTURE)
        if t == 11:
            assert tp == -1
            continue
        n += 1
        hit += tp >= 0
        assert tp == -1 or t <= tp <= 10
    sigma = math.sqrt(ratio * (1 - ratio) / n)
    print(f"ratio {ratio}: {hit}/{n} = {hit / n:.5f}, {(hit / n - ratio) / sigma:+.2f} sigma")
    assert abs(hit / n - ratio) < 4 * sigma


def test_future_bins_are_uniform(words):
    """t = 3 of a 12-step episode, c = 8: every t' in 3 .. 10 within 5 sigma of 1/8."""
    bins = np.zeros(8, np.int64)
    for w in words:
        tp = _choose(w, 3, 12, 1.0, ho.FUTURE)
        assert 3 <= tp <= 10
        bins[tp - 3] += 1
    n = int(bins.sum())
    sigma = math.sqrt(n * (1 / 8) * (7 / 8))
    print("t' bins", bins.tolist(), "worst", f"{np.abs(bins - n / 8).max() / sigma:.2f} sigma")
    assert n == N_ROWS and np.all(np.abs(bins - n / 8) < 5 * sigma)


def test_ratio_zero_one_and_final(words):
    for j, w in enumerate(words):
        len_e = 1 + j % 12
        t = (j // 12) % len_e
        c = len_e - 1 - t
        assert _choose(w, t, len_e, 0.0, ho.FUTURE) == -1 and _choose(w, t, len_e, 0.0, ho.FINAL) == -1
        assert (_choose(w, t, len_e, 1.0, ho.FUTURE) >= 0) == (c >= 1)
        assert _choose(w, t, len_e, 1.0, ho.FINAL) == (len_e - 2 if c >= 1 else -1)


def test_oracle_gather_on_a_hand_written_episode():
    """E = 2, L = 4, S = 4 = [x | y | achieved | desired], G = 1: relabelled rows carry the later achieved goal in
    both states and a reward from the distance; rows past the candidates and every a, d are the stored ones."""
    E, L, S = 2, 4, 4
    states = np.zeros((E, L + 1, S), np.float32)
    states[:, :, 2] = np.arange(E * (L + 1), dtype=np.float32).reshape(E, L + 1)      # achieved: 0 .. 4 | 5 .. 9
    states[:, :, 3] = 100
    states[0, 4, 2] = 1e9                                                              # the never-written last row
    actions = np.arange(E * L, dtype=np.float32).reshape(E, L, 1)
    rewards, dones = np.full((E, L), -1, np.float32), np.zeros((E, L), np.float32)
    dones[0, 3] = 1
    g = ho.her_gather(states, actions, rewards, dones, [4, 3], SEED, 0, 7, 2, 3, 1, 1.0, ho.FINAL, ho.DENSE, 0.0,
                      inds=np.arange(7))
    assert list(g["ep"]) == [0] * 4 + [1] * 3 and list(g["step"]) == [0, 1, 2, 3, 0, 1, 2]
    assert list(g["future"]) == [2, 2, 2, -1, 1, 1, -1]
    # episode 0: g' = achieved(states[0, 3]) = 3; achieved(s') = 1, 2, 3 -> r = -2, -1, -0
    assert list(g["r"][:, 0]) == [-2, -1, 0, -1, -1, 0, -1]
    # (row 3's s' IS the never-written row, as in the plain gather; no goal and no reward is taken from it)
    assert g["s2"][3, 2] == 1e9 and np.all(np.abs(g["s2"][:, 3]) < 1e3) and np.all(np.abs(g["r"]) < 1e3)
    assert list(g["s"][:, 3]) == [3, 3, 3, 100, 7, 7, 100] and list(g["s2"][:, 3]) == [3, 3, 3, 100, 7, 7, 100]
    assert list(g["s"][:, 2]) == [0, 1, 2, 3, 5, 6, 7] and list(g["d"][:, 0]) == [0, 0, 0, 1, 0, 0, 0]
    assert np.array_equal(g["a"][:, 0], [0, 1, 2, 3, 4, 5, 6])
    # sparse, threshold 1: |delta| = 2 misses, 1 and 0 hit
    g = ho.her_gather(states, actions, rewards, dones, [4, 3], SEED, 0, 7, 2, 3, 1, 1.0, ho.FINAL, ho.SPARSE, 1.0,
                      inds=np.arange(7))
    assert list(g["r"][:, 0]) == [-1, 0, 0, -1, 0, 0, -1]
