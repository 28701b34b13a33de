"""The offline dataset loader on a CPU replay buffer (no GPU): buffers/offline_dataset.py — reading and validating the
.npz, cutting the rows into episodes and pieces, the hand-written final next state of every piece, dropped rows,
observation statistics, overflow — and the OfflineTrainer's call arithmetic with a fake algorithm."""
from __future__ import annotations

import numpy as np
import pytest

from oprl_amd.buffers.episodic_buffer import EpisodicReplayBuffer
from oprl_amd.buffers.offline_dataset import (NORM_EPS, ObsNorm, OfflineData, cut_pieces, fill_replay, load_dataset,
                                               obs_statistics)
from oprl_amd.logging import NullLogger

S, A = 3, 2


def dataset(lengths, ends, next_obs=False, timeouts_key=True, seed=0) -> OfflineData:
    """Episodes of the given lengths, each ending in "terminal", "timeout" or "none" (no flag: only sensible last)."""
    rs = np.random.RandomState(seed)
    N = sum(lengths)
    obs = rs.standard_normal((N, S)).astype(np.float32) * np.array([1.0, 5.0, 0.1], np.float32) + np.array([0.0, 2.0, -1.0], np.float32)
    term, tout = np.zeros(N, bool), np.zeros(N, bool)
    last = np.cumsum(lengths) - 1
    for i, kind in zip(last, ends):
        term[i], tout[i] = kind == "terminal", kind == "timeout"
    return OfflineData(obs, rs.uniform(-1, 1, (N, A)).astype(np.float32), rs.standard_normal(N).astype(np.float32), term,
                       tout if timeouts_key else None, rs.standard_normal((N, S)).astype(np.float32) if next_obs else None)


def buffer(L, slots):
    return EpisodicReplayBuffer(buffer_size_transitions=slots * L, state_dim=S, action_dim=A, max_episode_lenth=L).create()


def stored(buf, e):
    n = buf.ep_lens[e]
    return (buf.states[e, :n].numpy(), buf.actions[e, :n].numpy(), buf.rewards[e, :n, 0].numpy(), buf.dones[e, :n, 0].numpy(),
            buf.states[e, n].numpy())


def test_load_dataset_reads_and_validates(tmp_path):
    d = dataset([4, 3], ["terminal", "timeout"], next_obs=True)
    p = tmp_path / "d.npz"
    np.savez(p, observations=d.observations, actions=d.actions, rewards=d.rewards.reshape(-1, 1), terminals=d.terminals,
             timeouts=d.timeouts, next_observations=d.next_observations, infos=np.zeros(3))
    got = load_dataset(p)
    for k in ("observations", "actions", "rewards", "terminals", "timeouts", "next_observations"):
        assert np.array_equal(getattr(got, k), getattr(d, k)), k
    assert got.rewards.shape == (7,) and got.terminals.dtype == bool and len(got) == 7
    np.savez(p, observations=d.observations, actions=d.actions, rewards=d.rewards, terminals=d.terminals)
    got = load_dataset(p)
    assert got.timeouts is None and got.next_observations is None
    np.savez(p, observations=d.observations, actions=d.actions, rewards=d.rewards)
    with pytest.raises(ValueError, match="terminals"):
        load_dataset(p)
    bad = d.observations.copy()
    bad[2, 1] = np.nan
    for kw, msg in ((dict(observations=bad), "finite"), (dict(actions=d.actions[:5]), "actions"),
                    (dict(rewards=d.rewards[:5]), "rewards"), (dict(observations=d.observations.reshape(-1)), r"\[N, S\]"),
                    (dict(next_observations=d.observations[:, :2]), "next_observations")):
        np.savez(p, **{**dict(observations=d.observations, actions=d.actions, rewards=d.rewards, terminals=d.terminals), **kw})
        with pytest.raises(ValueError, match=msg):
            load_dataset(p)


def test_terminal_episodes():
    d = dataset([4, 3, 5], ["terminal"] * 3, timeouts_key=False)
    buf = buffer(10, 4)
    assert fill_replay(buf, d, normalize=False) is None
    assert buf.ep_lens == [4, 3, 5, 0] and len(buf) == 12 and buf.episodes_counter == 4 and buf._ep_pointer == 3
    lo = 0
    for e, n in enumerate([4, 3, 5]):
        s, a, r, dn, final = stored(buf, e)
        assert np.array_equal(s, d.observations[lo:lo + n]) and np.array_equal(a, d.actions[lo:lo + n])
        assert np.array_equal(r, d.rewards[lo:lo + n]) and list(dn) == [0.0] * (n - 1) + [1.0]
        assert np.array_equal(final, d.observations[lo + n - 1])        # a terminal row: its own observation (times 1 - d = 0)
        lo += n


def test_timeout_episodes_with_next_observations():
    d = dataset([4, 3], ["timeout", "timeout"], next_obs=True)
    buf = buffer(10, 3)
    fill_replay(buf, d, normalize=False)
    assert buf.ep_lens == [4, 3, 0] and cut_pieces(d, 10)[1] == 0
    for e, (lo, n) in enumerate([(0, 4), (4, 3)]):
        s, _a, _r, dn, final = stored(buf, e)
        assert np.array_equal(s, d.observations[lo:lo + n]) and not dn.any()
        assert np.array_equal(final, d.next_observations[lo + n - 1])


def test_timeout_episodes_without_next_observations_drop_their_last_row():
    """... and so does a last episode that simply stops; an episode of one such row leaves nothing."""
    d = dataset([4, 1, 3, 2], ["timeout", "timeout", "terminal", "none"])
    pieces, dropped = cut_pieces(d, 10)
    assert dropped == 3 and [(p.start, p.stop, p.next_row) for p in pieces] == [(0, 3, 3), (5, 8, 7), (8, 9, 9)]
    buf = buffer(10, 4)
    fill_replay(buf, d, normalize=False)
    assert buf.ep_lens == [3, 3, 1, 0] and len(buf) == len(d) - dropped
    s, _a, _r, dn, final = stored(buf, 0)
    assert np.array_equal(s, d.observations[0:3]) and not dn.any()
    assert np.array_equal(final, d.observations[3])          # the dropped row's observation is the kept rows' last next state
    s, _a, _r, dn, final = stored(buf, 2)
    assert np.array_equal(s, d.observations[8:9]) and np.array_equal(final, d.observations[9]) and not dn.any()


@pytest.mark.parametrize("end", ["terminal", "timeout"])
def test_a_long_episode_is_cut_into_three_pieces(end):
    L = 4
    n = 2 * L + 3
    d = dataset([n, 2], [end, "terminal"], next_obs=False)
    buf = buffer(L, 5)
    fill_replay(buf, d, normalize=False)
    drop = 0 if end == "terminal" else 1
    assert buf.ep_lens == [L, L, 3 - drop, 2, 0] and len(buf) == len(d) - drop
    for e, (lo, m, nxt) in enumerate([(0, L, L), (L, L, 2 * L), (2 * L, 3 - drop, n - 1)]):
        s, a, _r, dn, final = stored(buf, e)
        assert np.array_equal(s, d.observations[lo:lo + m]) and np.array_equal(a, d.actions[lo:lo + m])
        assert np.array_equal(final, d.observations[nxt])      # cut mid-episode: the following row's observation
        assert list(dn) == [0.0] * (m - 1) + [1.0 if (e == 2 and end == "terminal") else 0.0]
    # with next_observations nothing is dropped and every piece ends on its own row's next observation
    d2 = dataset([n], ["timeout"], next_obs=True)
    buf = buffer(L, 4)
    fill_replay(buf, d2, normalize=False)
    assert buf.ep_lens == [L, L, 3, 0]
    for e, last in enumerate([L - 1, 2 * L - 1, n - 1]):
        assert np.array_equal(stored(buf, e)[4], d2.next_observations[last])


def test_normalisation_statistics():
    d = dataset([6, 5], ["terminal", "timeout"], next_obs=True)
    buf = buffer(8, 3)
    norm = fill_replay(buf, d)
    x = d.observations.astype(np.float64)
    assert isinstance(norm, ObsNorm) and norm.mean.dtype == np.float64
    assert np.array_equal(norm.mean, x.mean(0)) and np.array_equal(norm.std, x.std(0, ddof=0))
    assert np.array_equal(obs_statistics(d).std, norm.std) and NORM_EPS == 1e-3
    want = ((x - x.mean(0)) / (x.std(0) + 1e-3)).astype(np.float32)
    assert np.array_equal(stored(buf, 0)[0], want[:6]) and np.array_equal(stored(buf, 1)[0], want[6:])
    nxt = ((d.next_observations.astype(np.float64) - x.mean(0)) / (x.std(0) + 1e-3)).astype(np.float32)
    assert np.array_equal(stored(buf, 0)[4], nxt[5]) and np.array_equal(stored(buf, 1)[4], nxt[10])
    assert np.array_equal(norm(d.observations[3]), want[3]) and norm(d.observations).dtype == np.float32
    assert np.array_equal(stored(buf, 0)[1], d.actions[:6])          # actions and rewards are stored as they are
    assert abs(float(want.mean())) < 1e-6 and set(norm.state_dict()) == {"mean", "std"}


def test_overflow_raises_and_nothing_wraps():
    d = dataset([4, 3, 5], ["terminal"] * 3)
    buf = buffer(10, 3)                     # three pieces need four slots: the pointer moves onto one more
    with pytest.raises(ValueError, match="do not fit"):
        fill_replay(buf, d)
    assert len(buf) == 0 and buf.ep_lens == [0, 0, 0] and buf._ep_pointer == 0
    buf = buffer(10, 5)
    fill_replay(buf, dataset([4], ["terminal"]))
    with pytest.raises(ValueError, match="do not fit"):          # slots 1 .. 4 are free, slot 0 would be evicted
        fill_replay(buf, dataset([2, 2, 2, 2], ["terminal"] * 4))
    assert buf.ep_lens == [4, 0, 0, 0, 0]
    fill_replay(buf, dataset([2, 2, 2], ["terminal"] * 3))       # (a second dataset behind the first fits)
    assert buf.ep_lens == [4, 2, 2, 2, 0] and len(buf) == 10
    with pytest.raises(ValueError, match="dims"):
        fill_replay(EpisodicReplayBuffer(buffer_size_transitions=40, state_dim=S + 1, action_dim=A, max_episode_lenth=10).create(), d)
    lanes = buffer(10, 6)
    lanes.open_lanes(2)
    with pytest.raises(ValueError, match="lanes"):
        fill_replay(lanes, d)


# ---- the trainer's call arithmetic ----------------------------------------------------------------------------------------
class FakeAlgo:
    gamma = 0.99
    update_step = 0

    def __init__(self):
        self.calls = []

    def check_created(self):
        pass

    def update_from_buffer(self, buf, batch_size, n_updates=1):
        self.calls.append((batch_size, n_updates))


def test_offline_trainer_runs_whole_calls_and_does_its_periodic_work_between_them(monkeypatch):
    from oprl_amd.trainers.offline_trainer import OfflineTrainer
    buf = buffer(10, 3)
    fill_replay(buf, dataset([4, 3], ["terminal"] * 2))
    algo = FakeAlgo()
    tr = OfflineTrainer(logger=NullLogger(), make_env_test=None, replay_buffer=buf, algo=algo, num_updates=70,
                        updates_per_call=16, batch_size=32, eval_interval=32, save_policy_every=0, stdout_log_every=0)
    evals = []
    monkeypatch.setattr(tr, "evaluate", lambda: evals.append(sum(k for _, k in algo.calls)) or {"return": 0.0})
    tr.train()
    assert algo.calls == [(32, 16)] * 4 + [(32, 6)]
    assert evals == [32, 64]                 # on the call boundaries that pass a multiple of eval_interval
    with pytest.raises(ValueError, match="empty"):
        OfflineTrainer(logger=NullLogger(), make_env_test=None, replay_buffer=buffer(10, 3), algo=algo).train()

    class NBuf:
        n_step, gamma = 3, 0.95
        def check_created(self): pass
        def __len__(self): return 5
    with pytest.raises(ValueError, match="gamma"):
        OfflineTrainer(logger=NullLogger(), make_env_test=None, replay_buffer=NBuf(), algo=algo).train()
