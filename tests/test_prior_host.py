"""CPU tests of prior data's host side: the C-ABI surface and its null-handle checks, the build list,
the alias, the Python buffer's validation and its split of a batch, NormalizedObsEnv against ObsNorm applied by hand,
the numpy oracle on hand-written storage, and every flag refusal of the online and the offline scripts (no GPU
needed)."""
from __future__ import annotations

import math
import sys
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest

from oprl_amd import _capi
from tests import prior_oracle as po
from tests import support
from tests.config_scripts import load_config

ROOT = Path(__file__).resolve().parents[1]
PRIOR_FUNCS = {"oprl_replay_set_prior": 3, "oprl_replay_sample_mix": 14}


def plain_buffer(**kw):
    from oprl_amd.buffers.episodic_buffer import EpisodicReplayBuffer
    args = dict(buffer_size_transitions=120, state_dim=5, action_dim=2, max_episode_lenth=12)
    args.update(kw)
    return EpisodicReplayBuffer(**args).create()


def cpu_buffer(prior="default", **kw):
    from oprl_amd.buffers.prior_buffer import PriorDataReplayBuffer
    args = dict(state_dim=5, action_dim=2, prior=plain_buffer() if isinstance(prior, str) else prior)
    return support.cpu_buffer(PriorDataReplayBuffer, **{**args, **kw})


# ---- ABI and bindings ---------------------------------------------------------------------------------------------------
def test_prior_functions_are_declared_bound_and_exported():
    support.assert_abi_bound(PRIOR_FUNCS)
    # the arity and shape of oprl_replay_sample_her
    assert _capi.SIGNATURES["oprl_replay_sample_mix"] == _capi.SIGNATURES["oprl_replay_sample_her"]


def test_prior_functions_refuse_null_handles_without_a_gpu():
    lib = _capi.load()
    assert lib.oprl_replay_set_prior(None, None, 0.5) == -1
    assert b"null replay handle" in lib.oprl_last_error()
    assert lib.oprl_replay_sample_mix(None, 4, None, 0, 0, *([None] * 8), None) == -1
    assert len(lib.oprl_last_error()) > 0


def test_source_is_built_and_alias_resolves():
    support.assert_source_built("replay_mix", header=False)
    from oprl.buffers.prior_buffer import PriorDataReplayBuffer as Aliased
    from oprl.environment.normalized import NormalizedObsEnv as AliasedEnv
    from oprl.trainers.finetune import finetune as aliased_finetune
    from oprl_amd.buffers.episodic_buffer import EpisodicReplayBuffer
    from oprl_amd.buffers.prior_buffer import PriorDataReplayBuffer
    from oprl_amd.environment.normalized import NormalizedObsEnv
    from oprl_amd.trainers.finetune import finetune
    assert Aliased is PriorDataReplayBuffer and issubclass(Aliased, EpisodicReplayBuffer)
    assert AliasedEnv is NormalizedObsEnv and aliased_finetune is finetune


# ---- the buffer class -----------------------------------------------------------------------------------------------------
def test_defaults_host_container_and_state_dict():
    prior = plain_buffer()
    b = cpu_buffer(prior).create()
    assert b.prior is prior and b.prior_share == 0.5 and len(b) == 0 and b.n_prior(256) == 128
    for k in range(3):
        prior.add_transition(np.ones(5), np.zeros(2), 1.0, False)
    assert len(prior) == 3 and len(b) == 0            # len() is the online count: the trainers gate on it
    b.add_transition(np.ones(5), np.zeros(2), -1.0, False)
    assert len(b) == 1 and float(b.rewards[0, 0, 0]) == -1.0
    with pytest.raises(RuntimeError, match="MI355X"):
        b.sample(4)
    sd = b.state_dict()
    assert sd["prior_share"] == 0.5 and "prior" not in sd      # the dataset is not stored
    c = cpu_buffer(prior, prior_share=0.25).create()
    c.load_state_dict(sd)
    assert c.prior_share == 0.5 and c.prior is prior and len(c) == 1
    c.prior = None
    assert c.n_prior(64) == 0
    c.prior, c.prior_share = prior, 1.0
    assert c.n_prior(64) == 64
    with pytest.raises(ValueError, match="prior_share"):
        c.load_state_dict({**sd, "prior_share": 1.5})


@pytest.mark.parametrize("share", [-0.1, 1.5, float("nan"), float("inf"), "0.5", None, True])
def test_bad_shares_are_refused(share):
    with pytest.raises(ValueError, match="prior_share"):
        cpu_buffer(prior_share=share).create()


def test_bad_priors_are_refused():
    from oprl_amd.buffers.episodic_buffer import EpisodicReplayBuffer
    from oprl_amd.buffers.hindsight_buffer import HindsightEpisodicReplayBuffer
    from oprl_amd.buffers.nstep_buffer import NStepEpisodicReplayBuffer
    from oprl_amd.buffers.prioritized_buffer import PrioritizedEpisodicReplayBuffer
    kw = dict(buffer_size_transitions=120, state_dim=5, action_dim=2, max_episode_lenth=12)
    with pytest.raises(ValueError, match="dims"):
        cpu_buffer(plain_buffer(state_dim=6)).create()
    with pytest.raises(ValueError, match="dims"):
        cpu_buffer(plain_buffer(action_dim=3)).create()
    with pytest.raises(ValueError, match="n-step"):
        cpu_buffer(NStepEpisodicReplayBuffer(n_step=3, **kw).create()).create()
    with pytest.raises(ValueError, match="hindsight"):
        cpu_buffer(HindsightEpisodicReplayBuffer(goal_dim=1, achieved_offset=0, desired_offset=1, **kw).create()).create()
    with pytest.raises(ValueError, match="prioritized"):
        cpu_buffer(PrioritizedEpisodicReplayBuffer(**kw).create()).create()
    with pytest.raises(ValueError, match="prior of its own"):
        cpu_buffer(cpu_buffer().create()).create()
    with pytest.raises(ValueError, match="EpisodicReplayBuffer expected"):
        cpu_buffer(prior=object()).create()
    with pytest.raises(RuntimeError, match="create"):
        cpu_buffer(EpisodicReplayBuffer(**kw)).create()           # a prior that was never created
    b = cpu_buffer().create()
    b.prior = b
    with pytest.raises(ValueError, match="itself"):
        b._validate()
    # a prior of other episode slots and steps per episode is what the mode is for; no prior at all is the mode off
    cpu_buffer(plain_buffer(buffer_size_transitions=40, max_episode_lenth=4)).create()
    assert cpu_buffer(None).create().n_prior(32) == 0


SHARES = [0, 0.1, 1 / 3, 0.5, 0.7, 1]


def test_n_prior_is_the_rounded_share_of_the_batch():
    from oprl_amd.buffers.prior_buffer import n_prior_rows
    assert n_prior_rows(1, 0.5) == 1 and n_prior_rows(17, 0.5) == 9
    for share in SHARES:
        b = cpu_buffer(prior_share=share).create()
        exact = Fraction(share)            # the double's exact value
        for B in range(1, 301):
            n = b.n_prior(B)
            assert n == n_prior_rows(B, share) == po.n_prior(B, share) and 0 <= n <= B
            assert n == min(B, max(0, int(math.floor(share * B + 0.5))))
            # round-half-up of share * B, to within the one rounding of the double product
            assert abs(Fraction(n) - exact * B) <= Fraction(1, 2) + Fraction(1, 10 ** 9), (share, B, n)
            if share in (0, 1):
                assert n == share * B
        assert [b.n_prior(B) for B in (1, 2, 3)] == {0: [0, 0, 0], 0.1: [0, 0, 0], 1 / 3: [0, 1, 1], 0.5: [1, 1, 2],
                                                     0.7: [1, 1, 2], 1: [1, 2, 3]}[share]


# ---- the environment wrapper ------------------------------------------------------------------------------------------
def test_normalized_env_against_obs_norm_by_hand():
    from oprl_amd.buffers.offline_dataset import NORM_EPS, ObsNorm
    from oprl_amd.environment.normalized import NormalizedObsEnv
    from oprl_amd.environment.synthetic import SyntheticEnv
    rs = np.random.RandomState(0)
    norm = ObsNorm(mean=rs.standard_normal(6), std=rs.uniform(0.0, 2.0, 6))
    norm.std[2] = 0.0                      # a constant column: the epsilon keeps the quotient finite
    raw, env = SyntheticEnv("reacher-easy", seed=4, episode_length=7), NormalizedObsEnv(SyntheticEnv("reacher-easy", seed=4, episode_length=7), norm)
    assert env.env_family == "synthetic" and env.episode_length == 7 and env.S == 6
    assert env.observation_space.shape == (6,) and env.action_space.shape == (2,)
    a, b = raw.reset()[0], env.reset()[0]

    def by_hand(x):
        return ((x.astype(np.float64) - norm.mean) / (norm.std + NORM_EPS)).astype(np.float32)
    assert b.dtype == np.float32 and np.array_equal(b, by_hand(a)) and np.array_equal(b, norm(a))
    for k in range(7):
        act = raw.sample_action()
        assert np.array_equal(act, env.sample_action())          # the wrapped environment's own generator
        x, r, term, trunc, _ = raw.step(act)
        y, r2, term2, trunc2, info = env.step(act)
        assert np.array_equal(y, by_hand(x)) and (r, term, trunc) == (r2, term2, trunc2) and info == {}
        assert trunc == (k == 6) and np.all(np.isfinite(y))
    with pytest.raises(ValueError, match="ObsNorm"):
        NormalizedObsEnv(raw, None)
    with pytest.raises(AttributeError):
        env.no_such_attribute


# ---- the oracle -------------------------------------------------------------------------------------------------------------
def test_oracle_on_hand_written_storage():
    """Prior: E = 2, L = 3; online: E = 2, L = 2; S = A = 1.  Injected indices are flat indices into the row's own
    source; drawn ones stay below that source's count."""
    def storage(E, L, off):
        s = off + np.arange(E * (L + 1), dtype=np.float32).reshape(E, L + 1, 1)
        a = off + 100 + np.arange(E * L, dtype=np.float32).reshape(E, L, 1)
        return s, a, a + 100, np.zeros((E, L, 1), np.float32)
    P, O = storage(2, 3, 0), storage(2, 2, 1000)
    g = po.mix_gather(P, [3, 2], O, [2, 1], 0.5, 7, 0, 6, inds=np.array([0, 3, 4, 0, 1, 2]))
    assert list(g["src"]) == [1, 1, 1, 0, 0, 0]
    assert list(g["ep"]) == [0, 1, 1, 0, 0, 1] and list(g["step"]) == [0, 0, 1, 0, 1, 0]
    assert list(g["s"][:, 0]) == [0, 4, 5, 1000, 1001, 1003] and list(g["s2"][:, 0]) == [1, 5, 6, 1001, 1002, 1004]
    assert list(g["a"][:, 0]) == [100, 103, 104, 1100, 1101, 1102] and list(g["r"][:, 0]) == [200, 203, 204, 1200, 1201, 1202]
    for share, src in ((0.0, [0] * 5), (1.0, [1] * 5), (0.3, [1, 1, 0, 0, 0])):
        g = po.mix_gather(P, [3, 2], O, [2, 1], share, 7, 3, 5)
        assert list(g["src"]) == src and g["s"].shape == (5, 1) and g["r"].shape == (5, 1)
        assert np.all(g["s"][np.array(src) == 1] < 1000) and np.all(g["s"][np.array(src) == 0] >= 1000)


# ---- flags and config -----------------------------------------------------------------------------------------------------
def test_prior_flags(monkeypatch):
    from oprl_amd.parse_args import check_finetune, check_prior, parse_args, parse_args_distrib
    monkeypatch.setattr(sys, "argv", ["x"])
    a = parse_args()
    assert (a.prior_data, a.prior_share) == (None, 0.5) and not check_prior(a) and check_finetune(a) == 0
    assert (a.n_step, a.per, a.num_envs, a.open_episodes, a.her, a.precision) == (1, False, 1, False, False, "f32")
    assert not hasattr(parse_args_distrib(), "prior_data")
    monkeypatch.setattr(sys, "argv", ["x", "--prior-data", "d.npz", "--prior-share", "0.25"])
    a = parse_args()
    assert (a.prior_data, a.prior_share) == ("d.npz", 0.25) and check_prior(a)


@pytest.mark.parametrize("extra,word", [(["--per"], "--per"), (["--n-step", "3"], "--n-step 3"), (["--her"], "--her"),
                                        (["--num-envs", "4"], "--num-envs 4"),
                                        (["--num-envs", "4", "--open-episodes"], "--num-envs 4"),
                                        (["--open-episodes"], "--open-episodes"), (["--prior-share", "1.5"], "--prior-share"),
                                        (["--prior-share", "-0.1"], "--prior-share"), (["--prior-share", "nan"], "--prior-share")])
def test_check_prior_refuses(monkeypatch, extra, word):
    from oprl_amd.parse_args import check_prior, parse_args
    monkeypatch.setattr(sys, "argv", ["x", "--prior-data", "d.npz", *extra])
    with pytest.raises(ValueError, match=word):
        check_prior(parse_args())


NO_FILE = ["--prior-data", "/nonexistent/never_read.npz"]       # refused before the file is looked at
NO_ENV = ["--env", "no-such-environment"]                       # ... and before an environment is built


@pytest.mark.parametrize("script,extra,word", [("ddpg", ["--per"], "--per"), ("td3", ["--n-step", "3"], "--n-step 3"),
                                               ("sac", ["--her"], "--her"), ("redq", ["--num-envs", "2"], "--num-envs 2"),
                                               ("tqc", ["--open-episodes"], "--open-episodes"),
                                               ("d4pg", ["--prior-share", "2"], "--prior-share")])
def test_online_scripts_refuse_before_anything_is_built(monkeypatch, script, extra, word):
    with pytest.raises(ValueError, match=word):
        load_config(monkeypatch, script, [*NO_ENV, *NO_FILE, *extra])
    with pytest.raises(ValueError, match="no-such-environment"):      # (what is refused next, once the flags agree)
        load_config(monkeypatch, script, [*NO_ENV, *NO_FILE])


@pytest.mark.parametrize("script", ["td3_bc", "iql", "cql"])
def test_offline_scripts_refuse(monkeypatch, script):
    env = ["--env", "synthetic:reacher-easy", "--device", "cpu"]
    with pytest.raises(ValueError, match="--finetune-steps with --n-step 3"):
        load_config(monkeypatch, script, [*env, "--finetune-steps", "100", "--n-step", "3"])
    with pytest.raises(ValueError, match="--finetune-steps -1"):
        load_config(monkeypatch, script, [*env, "--finetune-steps", "-1"])
    with pytest.raises(ValueError, match="--prior-share"):
        load_config(monkeypatch, script, [*env, "--finetune-steps", "100", "--prior-share", "1.01"])
    with pytest.raises(ValueError, match="--prior-data"):
        load_config(monkeypatch, script, [*env, "--prior-data", "d.npz"])
    # the default is today's behaviour: no fine-tuning, and --n-step alone is still accepted
    mod = load_config(monkeypatch, script, [*env, "--n-step", "3"])
    assert mod.finetune_steps == 0
    mod = load_config(monkeypatch, script, [*env, "--finetune-steps", "100", "--prior-share", "0.25"])
    assert mod.finetune_steps == 100 and mod.script.args.prior_share == 0.25


def test_online_script_builds_the_prior_buffer_from_the_dataset(monkeypatch, tmp_path):
    """configs/sac.py --prior-data on a CPU device: the dataset goes, not normalised, into a replay sized by its pieces,
    and the training buffer is a PriorDataReplayBuffer over it."""
    from oprl_amd.buffers.episodic_buffer import EpisodicReplayBuffer
    from oprl_amd.buffers.prior_buffer import PriorDataReplayBuffer
    rs = np.random.RandomState(1)
    N, S, A = 30, 6, 2
    obs = (5.0 + rs.standard_normal((N, S))).astype(np.float32)
    term = np.zeros(N, bool)
    term[[9, 29]] = True
    tout = np.zeros(N, bool)
    tout[19] = True
    path = tmp_path / "d.npz"
    np.savez(path, observations=obs, actions=rs.uniform(-1, 1, (N, A)).astype(np.float32), rewards=rs.rand(N).astype(np.float32),
             terminals=term, timeouts=tout, next_observations=obs + 1)
    env = ["--env", "synthetic:reacher-easy", "--device", "cpu"]
    mod = load_config(monkeypatch, "sac", [*env, "--prior-data", str(path), "--prior-share", "0.25"])
    assert mod.script.prior
    buf = mod.make_replay_buffer()
    assert type(buf) is PriorDataReplayBuffer and type(buf.prior) is EpisodicReplayBuffer and buf.prior_share == 0.25
    assert len(buf) == 0 and len(buf.prior) == N and buf.prior.ep_lens[:3] == [10, 10, 10] and buf.n_prior(256) == 64
    assert buf.prior._max_episodes == 4 and (buf.prior.state_dim, buf.prior.action_dim) == (S, A)
    assert np.array_equal(buf.prior.states[0, :10].numpy(), obs[:10])           # stored as they are
    assert np.array_equal(buf.prior.states[1, 10].numpy(), obs[19] + 1)         # the timeout row's next state
    # a dataset of other dims is refused by the loader's own check
    np.savez(tmp_path / "bad.npz", observations=obs[:, :5], actions=rs.rand(N, A).astype(np.float32), rewards=rs.rand(N).astype(np.float32),
             terminals=term)
    with pytest.raises(ValueError, match="dims"):
        load_config(monkeypatch, "sac", [*env, "--prior-data", str(tmp_path / "bad.npz")]).make_replay_buffer()
    # without the flag the same script builds what it built before
    plain = load_config(monkeypatch, "sac", env)
    assert not plain.script.prior and type(plain.make_replay_buffer()) is EpisodicReplayBuffer
