"""Host logic of acting for many environments: the episode assembler and interval rule of VecTrainer,
explore_rows / exploit_rows of policies whose net is on the CPU, and the command line.  No GPU."""
import sys

import numpy as np
import pytest
import torch as t
from torch import nn

from oprl_amd.trainers.vec_trainer import EpisodeAssembler, VecTrainer, crossed


def test_assembler_keeps_records_in_order_and_closes_episodes_per_environment():
    S, A = 3, 2
    asm = EpisodeAssembler(2)
    rs = np.random.RandomState(0)
    sent = {0: [], 1: []}
    closed = []
    # environment 0: episodes of 3 and 2 steps; environment 1: one episode of 4 steps, one left open
    plan = [(0, False), (1, False), (0, False), (1, False), (0, True), (1, False), (0, False), (1, True), (0, True), (1, False)]
    for env, over in plan:
        s, a, r = rs.standard_normal(S), rs.uniform(-1, 1, A), float(rs.uniform())
        sent[env].append(np.concatenate([s, a, [r, float(over)]]).astype(np.float32))
        rows = asm.add(env, s, a, r, over, over)
        if not over:
            assert rows is None                      # nothing is handed out before the episode ends
        else:
            closed.append((env, rows))
    assert [(e, len(r)) for e, r in closed] == [(0, 3), (1, 4), (0, 2)]
    assert asm.pending(0) == 0 and asm.pending(1) == 1
    got = {0: np.concatenate([r for e, r in closed if e == 0]), 1: np.concatenate([r for e, r in closed if e == 1])}
    assert got[0].dtype == np.float32 and got[0].shape == (5, S + A + 2)
    assert np.array_equal(got[0], np.stack(sent[0]))
    assert np.array_equal(got[1], np.stack(sent[1][:4]))


class _RecordingBuffer:
    def __init__(self):
        self.calls = []

    def add_transitions(self, rows, episode_done=False):
        self.calls.append((np.array(rows), episode_done))


class _CountingEnv:
    """Observation = [id, t]; the episode of environment `ident` lasts `length` steps."""

    def __init__(self, ident, length):
        self.ident, self.length, self.t = ident, length, 0

    def reset(self):
        self.t = 0
        return np.array([self.ident, 0.0], np.float32), {}

    def sample_action(self):
        return np.array([0.5], np.float32)

    def step(self, action):
        self.t += 1
        return np.array([self.ident, self.t], np.float32), 1.0, False, self.t >= self.length, {}


def test_collect_writes_whole_episodes_only():
    buf = _RecordingBuffer()
    envs = [_CountingEnv(0, 2), _CountingEnv(1, 3)]
    tr = VecTrainer(logger=None, make_env_test=None, replay_buffer=buf, algo=None, envs=envs, start_steps=10 ** 6)
    assert tr.env is envs[0]
    asm = EpisodeAssembler(2)
    obs = np.stack([e.reset()[0] for e in envs])
    obs = tr._collect_rows(0, obs, asm)
    assert buf.calls == [] and obs.tolist() == [[0, 1], [1, 1]]
    obs = tr._collect_rows(2, obs, asm)
    assert len(buf.calls) == 1 and buf.calls[0][1] is True
    assert buf.calls[0][0][:, :2].tolist() == [[0, 0], [0, 1]]           # environment 0's two states, in order
    assert obs.tolist() == [[0, 0], [1, 2]]                              # ... and it was reset
    obs = tr._collect_rows(4, obs, asm)
    assert len(buf.calls) == 2 and buf.calls[1][0][:, :2].tolist() == [[1, 0], [1, 1], [1, 2]]
    assert buf.calls[1][0][:, 2:].tolist() == [[0.5, 1.0, 0.0]] * 3      # action, reward, done (truncation is no terminal)


def test_periodic_work_fires_when_its_interval_is_crossed():
    assert crossed(0, 4, 4) == 4 and crossed(4, 8, 4) == 8
    assert crossed(4, 7, 4) is None and crossed(5, 8, 4) == 8
    assert crossed(6, 10, 4) == 8                    # a multiple strictly inside (prev, cur]
    assert crossed(8, 12, 4) == 12 and crossed(8, 11, 4) is None
    assert crossed(0, 256, 100) == 200               # several crossed at once: the last one, once
    assert crossed(3, 9, 0) is None and crossed(3, 9, -1) is None
    # every multiple is seen exactly once by a loop that moves in steps of 3
    fired = [crossed(s, s + 3, 10) for s in range(0, 60, 3)]
    assert [f for f in fired if f is not None] == [10, 20, 30, 40, 50, 60]


def _per_row(fn, x):
    return np.stack([fn(r) for r in x])


def test_cpu_policies_rows_equal_per_row_calls(monkeypatch):
    from oprl_amd.algos.nn_models import DeterministicPolicy, GaussianActor
    S, A, N = 7, 3, 5
    t.manual_seed(0)
    x = np.random.RandomState(1).standard_normal((N, S)).astype(np.float32)
    det = DeterministicPolicy(S, A, hidden_units=(32, 32), expl_noise=0.3)
    assert np.allclose(det.exploit_rows(x), _per_row(det.exploit, x), rtol=0, atol=1e-6)
    noise = t.from_numpy(np.random.RandomState(2).standard_normal((N, A)).astype(np.float32))
    real = t.randn
    monkeypatch.setattr(t, "randn", lambda *a, **k: noise)
    rows = det.explore_rows(x)
    single = []
    for i in range(N):
        monkeypatch.setattr(t, "randn", lambda *a, _i=i, **k: noise[_i])
        single.append(det.explore(x[i]))
    monkeypatch.setattr(t, "randn", real)
    assert rows.shape == (N, A) and np.allclose(rows, np.stack(single), rtol=0, atol=1e-6)
    assert np.abs(rows).max() <= 1.0                                          # clipped
    with t.no_grad():
        raw = det.mlp.nn(t.from_numpy(x)).numpy() + 0.3 * noise.numpy()
    assert np.allclose(rows, np.clip(raw, -1, 1), atol=1e-6)                  # noise and clip, NO tanh
    assert not np.allclose(rows, np.tanh(raw), atol=1e-3)

    ga = GaussianActor(S, A, hidden_units=(32, 32), hidden_activation=nn.ReLU(), device="cpu")
    assert np.allclose(ga.exploit_rows(x), _per_row(ga.exploit, x), rtol=0, atol=1e-6)
    ga.train()
    monkeypatch.setattr(t, "randn", lambda *a, **k: noise)
    rows = ga.explore_rows(x)
    monkeypatch.setattr(t, "randn", real)
    single = []
    for i in range(N):       # the CPU single-row path draws through randn_like inside forward(): inject eps there
        with t.no_grad():
            single.append(ga.forward(t.from_numpy(x[i:i + 1]), eps=noise[i:i + 1])[0].numpy()[0])
    assert np.allclose(rows, np.stack(single), rtol=0, atol=1e-6)
    ga.eval()
    assert np.allclose(ga.explore_rows(x), ga.exploit_rows(x))                # eval mode: tanh(mean)
    assert np.allclose(ga.explore_rows(x), _per_row(ga.explore, x), atol=1e-6)


def test_num_envs_flag_parses_with_default_one(monkeypatch):
    from oprl_amd.parse_args import parse_args
    monkeypatch.setattr(sys, "argv", ["prog"])
    assert parse_args().num_envs == 1
    monkeypatch.setattr(sys, "argv", ["prog", "--num-envs", "16", "--env", "walker-walk"])
    assert parse_args().num_envs == 16


def test_runner_refuses_a_num_envs_outside_one_launch():
    from oprl_amd.runners.train import env_seeds, run_training
    assert env_seeds(3, 4)[0] == 3 and len(set(env_seeds(3, 4))) == 4
    with pytest.raises(ValueError, match="num_envs"):
        run_training(None, None, None, None, None, num_envs=0)
    with pytest.raises(ValueError, match="num_envs"):
        run_training(None, None, None, None, None, num_envs=257)
