"""Host logic of several open replay episodes: the C-ABI surface, ``open_lanes`` / ``add_step_rows`` on a
CPU container against tests/lanes_oracle.py, the refusals, the checkpoint in mid-episode, ``VecTrainer._collect_open``
and the command line.  No GPU; every comparison is of copies, so bit for bit."""
import re
import sys
from pathlib import Path

import numpy as np
import pytest
import torch as t

from tests.lanes_oracle import LanesOracle, random_step

ROOT = Path(__file__).resolve().parents[1]
E, L, N, S, A = 7, 4, 3, 3, 2


def make(E=E, L=L, S=S, A=A, cls=None, **kw):
    from oprl_amd.buffers.episodic_buffer import EpisodicReplayBuffer
    return (cls or EpisodicReplayBuffer)(buffer_size_transitions=E * L, state_dim=S, action_dim=A, max_episode_lenth=L,
                                         device="cpu", **kw).create()


def assert_equal(buf, ora):
    for name, want in zip(("states", "actions", "rewards", "dones"), ora.storage()):
        assert np.array_equal(getattr(buf, name).numpy(), want), name
    assert buf.ep_lens == ora.ep_lens.tolist()
    assert (buf.episodes_counter, buf._ep_pointer, len(buf), buf._lanes) == (ora.counter, ora.pointer, ora.count, ora.lanes)


def overs(rs, lens, lanes, p=0.3):
    """Seeded random closes; a lane whose episode is full after this step must close."""
    over = rs.rand(len(lanes)) < p
    for i, e in enumerate(lanes):
        if lens[e] + 1 >= L:
            over[i] = True
    return over


def run(rs, calls, *targets):
    """`calls` seeded steps into every target (buffers and oracles alike); the closes follow the first one's table."""
    for _ in range(calls):
        step = random_step(rs, N, S, A)
        first = targets[0]
        over = overs(rs, first.ep_lens, first._lanes if hasattr(first, "_lanes") else first.lanes)
        for x in targets:
            (x.step if isinstance(x, LanesOracle) else x.add_step_rows)(*step, over)


def test_symbol_is_declared_bound_and_exported():
    from oprl_amd import _capi
    header = (ROOT / "include" / "oprl_amd.h").read_text()
    assert re.search(r"\bint oprl_replay_write_rows\s*\(", header) and "#define OPRL_ABI_VERSION 4" in header
    lib = _capi.load()
    assert "oprl_replay_write_rows" in _capi.SIGNATURES and len(_capi.SIGNATURES["oprl_replay_write_rows"][1]) == 12
    assert hasattr(lib, "oprl_replay_write_rows")
    assert _capi.OPRL_ABI_VERSION == 4 and lib.oprl_abi_version() == 4
    assert lib.oprl_replay_write_rows(None, 1, None, None, None, None, None, None, None, None, 0, None) == -1
    assert b"null" in lib.oprl_last_error()


def test_two_hundred_steps_equal_the_oracle():
    buf, ora = make(), LanesOracle(E, L, S, A, N)
    buf.open_lanes(N)
    assert_equal(buf, ora)
    rs = np.random.RandomState(0)
    seen_full, seen_double = False, False
    for _ in range(200):
        step = random_step(rs, N, S, A)
        over = overs(rs, ora.ep_lens, ora.lanes)
        held = list(ora.lanes)
        n_evicted = len(ora.evicted)
        wrote = ora.step(*step, over)
        buf.add_step_rows(*step, over)
        assert_equal(buf, ora)
        took = ora.evicted[n_evicted:]
        seen_full |= any(k == L - 1 for _, k in wrote)
        seen_double |= len(took) >= 2
        # an open lane's slot is never evicted: every eviction of a call spares the slots held just before it
        assert len(took) == int(over.sum())
        for i, slot in zip(np.flatnonzero(over), took):
            assert slot not in held
            held[i] = slot
        assert held == buf._lanes
        for i, (e, k) in enumerate(wrote):
            if buf.ep_lens[e] > k:          # the step is live: behind it lies the next state that was passed in
                assert np.array_equal(buf.states[e, k + 1].numpy(), step[4][i])
        assert len(buf) == sum(buf.ep_lens) and len(set(buf._lanes)) == N
    assert seen_full and seen_double and len(ora.evicted) > 2 * E        # full episodes, double closes, several ring wraps


def test_a_full_lane_raises_and_changes_nothing():
    buf = make()
    buf.open_lanes(N)
    rs = np.random.RandomState(1)
    never = np.zeros(N, bool)
    for _ in range(L):
        buf.add_step_rows(*random_step(rs, N, S, A), never)
    snap = ([getattr(buf, k).clone() for k in ("states", "actions", "rewards", "dones")], list(buf.ep_lens),
            buf.episodes_counter, buf._ep_pointer, len(buf), list(buf._lanes))
    with pytest.raises(IndexError, match="full"):
        buf.add_step_rows(*random_step(rs, N, S, A), np.ones(N, bool))
    with pytest.raises(ValueError, match="expected"):
        buf.add_step_rows(*random_step(rs, N + 1, S, A), np.ones(N + 1, bool))
    now = ([getattr(buf, k) for k in ("states", "actions", "rewards", "dones")], list(buf.ep_lens),
           buf.episodes_counter, buf._ep_pointer, len(buf), list(buf._lanes))
    assert all(t.equal(x, y) for x, y in zip(snap[0], now[0])) and snap[1:] == now[1:]


def test_open_lanes_refusals_and_the_single_episode_methods():
    buf = make()
    for n in (0, -1, 257, E, True, 2.5):
        with pytest.raises(ValueError, match="open_lanes"):
            buf.open_lanes(n)
    with pytest.raises(RuntimeError, match="no lanes"):
        buf.add_step_rows(*random_step(np.random.RandomState(0), N, S, A), np.zeros(N, bool))
    buf.open_lanes(E - 1)                       # the most this buffer takes
    buf = make()
    buf.open_lanes(N)
    buf.open_lanes(N)                           # the same n again: nothing happens
    assert buf._lanes == [0, 1, 2] and buf._ep_pointer == N - 1 and buf.episodes_counter == N
    with pytest.raises(RuntimeError, match="lanes are open"):
        buf.open_lanes(N + 1)
    s, a = np.zeros(S, np.float32), np.zeros(A, np.float32)
    with pytest.raises(RuntimeError, match="open lanes"):
        buf.add_transition(s, a, 0.0, False)
    with pytest.raises(RuntimeError, match="open lanes"):
        buf.add_transitions(np.zeros((2, S + A + 2), np.float32))
    with pytest.raises(RuntimeError, match="open lanes"):
        buf.add_episode([(s, a, 0.0, False, s)])
    used = make()
    used.add_transition(s, a, 0.0, False)
    with pytest.raises(RuntimeError, match="holds transitions"):
        used.open_lanes(N)
    # a buffer without lanes is today's buffer
    assert used._lanes == [] and used.state_dict()["lanes"] == [] and len(used) == 1


@pytest.mark.parametrize("kind", ["plain", "nstep"])
def test_checkpoint_in_mid_episode_resumes_the_lanes(kind):
    from oprl_amd.buffers.nstep_buffer import NStepEpisodicReplayBuffer
    cls, kw = (NStepEpisodicReplayBuffer, dict(n_step=3)) if kind == "nstep" else (None, {})
    straight, ora = make(cls=cls, **kw), LanesOracle(E, L, S, A, N)
    straight.open_lanes(N)
    rs = np.random.RandomState(3)
    run(rs, 37, ora, straight)
    assert any(0 < ora.ep_lens[e] < L for e in ora.lanes) and len(ora.evicted) > E       # running episodes, after a wrap
    sd = straight.state_dict()
    assert sd["lanes"] == ora.lanes
    resumed = make(cls=cls, **kw)
    resumed.load_state_dict(sd)
    again = np.random.RandomState(0)
    again.set_state(rs.get_state())
    run(rs, 20, ora, straight)              # the uninterrupted run ...
    run(again, 20, resumed)                 # ... and the resumed one, from the same 20 steps
    assert_equal(straight, ora)
    assert_equal(resumed, ora)
    # a checkpoint from before lanes existed has no entry: it loads with none
    old = make().state_dict()
    del old["lanes"]
    fresh = make()
    fresh.open_lanes(N)
    fresh.load_state_dict(old)
    assert fresh._lanes == []
    fresh.add_transition(np.zeros(S, np.float32), np.zeros(A, np.float32), 0.0, False)


class _RecordingBuffer:
    def __init__(self):
        self.calls, self.lanes = [], None

    def open_lanes(self, n):
        self.lanes = n

    def add_step_rows(self, *args):
        self.calls.append([np.array(x) for x in args])


class _CountingEnv:
    """Observation = [id, t]; the episode of environment `ident` lasts `length` steps and ends by termination when
    `terminal` (else by truncation)."""

    def __init__(self, ident, length, terminal=False):
        self.ident, self.length, self.terminal, self.t = ident, length, terminal, 0

    def reset(self):
        self.t = 0
        return np.array([self.ident, 0.0], np.float32), {}

    def sample_action(self):
        return np.array([0.5], np.float32)

    def step(self, action):
        self.t += 1
        end = self.t >= self.length
        return np.array([self.ident, self.t], np.float32), 1.0 + self.ident, end and self.terminal, end and not self.terminal, {}


def test_collect_open_makes_one_call_per_iteration_with_the_terminal_observation():
    from oprl_amd.trainers.vec_trainer import VecTrainer
    buf = _RecordingBuffer()
    envs = [_CountingEnv(0, 2), _CountingEnv(1, 3, terminal=True)]
    tr = VecTrainer(logger=None, make_env_test=None, replay_buffer=buf, algo=None, envs=envs, start_steps=10 ** 6,
                    open_episodes=True)
    obs = np.stack([e.reset()[0] for e in envs])
    obs = tr._collect_open(0, obs)
    assert len(buf.calls) == 1 and obs.tolist() == [[0, 1], [1, 1]]
    s, a, r, d, s2, over = buf.calls[0]
    assert s.tolist() == [[0, 0], [1, 0]] and s2.tolist() == [[0, 1], [1, 1]] and a.tolist() == [[0.5], [0.5]]
    assert a.dtype == np.float32 and r.tolist() == [1.0, 2.0] and d.tolist() == [0, 0] and over.tolist() == [False, False]
    obs = tr._collect_open(2, obs)
    assert len(buf.calls) == 2
    s, a, r, d, s2, over = buf.calls[1]
    assert s.tolist() == [[0, 1], [1, 1]] and over.tolist() == [True, False]
    assert s2.tolist() == [[0, 2], [1, 2]]                    # environment 0's truncation observation, not the reset one
    assert d.tolist() == [0, 0]                               # truncation is no terminal
    assert obs.tolist() == [[0, 0], [1, 2]]                   # ... and what comes back for it is the reset observation
    obs = tr._collect_open(4, obs)
    s, a, r, d, s2, over = buf.calls[2]
    assert len(buf.calls) == 3 and over.tolist() == [False, True] and d.tolist() == [0, 1]
    assert s2.tolist() == [[0, 1], [1, 3]] and obs.tolist() == [[0, 1], [1, 0]]
    # the flag is off by default and the assembler path is what it was
    assert VecTrainer(logger=None, make_env_test=None, replay_buffer=buf, algo=None, envs=envs).open_episodes is False


def test_open_episodes_flag_parses_and_needs_several_environments(monkeypatch):
    from oprl_amd.parse_args import parse_args
    from oprl_amd.runners.train import run_training
    monkeypatch.setattr(sys, "argv", ["prog"])
    assert parse_args().open_episodes is False
    monkeypatch.setattr(sys, "argv", ["prog", "--num-envs", "16", "--open-episodes"])
    args = parse_args()
    assert args.open_episodes is True and args.num_envs == 16
    with pytest.raises(ValueError, match="open_episodes"):
        run_training(None, None, None, None, None, num_envs=1, open_episodes=True)
