"""Offline training end to end on the GPU: a dataset rolled from SyntheticEnv, fill_replay into an HBM
replay, OfflineTrainer over a TD3BC learner — against 64 sample() + update() pairs from the same start, bit for bit —
and the next states the loader writes by hand as the sampler returns them."""
from __future__ import annotations

import numpy as np
import pytest
import torch as t

from oprl_amd.algos.td3_bc import TD3BC
from oprl_amd.buffers.episodic_buffer import EpisodicReplayBuffer
from oprl_amd.buffers.offline_dataset import OfflineData, fill_replay
from oprl_amd.environment.synthetic import SyntheticEnv
from oprl_amd.logging import NullLogger
from oprl_amd.trainers.offline_trainer import OfflineTrainer

pytestmark = pytest.mark.gpu

ENV, EPISODES, STEPS, B = "cheetah-run", 6, 50, 64


def make_env(seed):
    return SyntheticEnv(ENV, seed=seed, episode_length=STEPS)


@pytest.fixture(scope="module")
def data() -> OfflineData:
    """6 episodes x 50 steps under uniform actions; the synthetic environment never terminates: every episode ends in
    a timeout, and next_observations is kept so that no row is dropped."""
    env = make_env(3)
    cols = [[] for _ in range(6)]
    for _ in range(EPISODES):
        obs, _ = env.reset()
        over = False
        while not over:
            a = env.sample_action()
            nxt, r, term, trunc, _ = env.step(a)
            for c, v in zip(cols, (obs, a, r, term, trunc, nxt)):
                c.append(v)
            obs, over = nxt, term or trunc
    o, a, r, term, tout, nxt = cols
    return OfflineData(np.asarray(o, np.float32), np.asarray(a, np.float32), np.asarray(r, np.float32), np.asarray(term, bool),
                       np.asarray(tout, bool), np.asarray(nxt, np.float32))


def filled(data, seed=11):
    S, A = data.observations.shape[1], data.actions.shape[1]
    buf = EpisodicReplayBuffer(buffer_size_transitions=(EPISODES + 1) * STEPS, state_dim=S, action_dim=A,
                               max_episode_lenth=STEPS, device="cuda", seed=seed).create()
    return buf, fill_replay(buf, data)


def learner(data):
    t.manual_seed(0)
    return TD3BC(logger=NullLogger(), state_dim=data.observations.shape[1], action_dim=data.actions.shape[1], max_batch=256,
                 log_every=10 ** 9).create()


def test_the_trainer_equals_sample_and_update_pairs_bitwise(data):
    assert len(data) == EPISODES * STEPS and data.timeouts.sum() == EPISODES and not data.terminals.any()
    buf, norm = filled(data)
    assert len(buf) == EPISODES * STEPS and buf.ep_lens[:EPISODES] == [STEPS] * EPISODES
    algo, loop = learner(data), learner(data)
    loop.load_state_dict(algo.state_dict())
    tr = OfflineTrainer(logger=NullLogger(), make_env_test=make_env, replay_buffer=buf, algo=algo, obs_norm=norm,
                        num_updates=64, updates_per_call=16, batch_size=B, eval_interval=0, save_policy_every=0,
                        stdout_log_every=0, num_eval_episodes=2, seed=5)
    tr.train()
    assert algo.update_step == 64
    ret = tr.evaluate()["return"]
    assert np.isfinite(ret) and 0.0 < ret <= STEPS            # rewards lie in (0, 1]
    for _ in range(64):
        buf._sample_counter = loop.update_step
        loop.update(*buf.sample(B))
    t.cuda.synchronize()
    algo.learner.check()
    x, y = algo.state_dict(), loop.state_dict()
    assert x["counters"] == y["counters"] and x["counters"][:3] == [64, 64, 32]
    for k in ("actor", "actor_m", "actor_v", "critic", "critic_m", "critic_v"):
        assert t.equal(x[k], y[k]), k
    for p, q in zip(x["targets"], y["targets"]):
        assert t.equal(p, q)
    assert algo.learner.read_bc() == loop.learner.read_bc() and algo.learner.read_bc()["bc_mse"] > 0
    assert not t.equal(x["actor"], learner(data).state_dict()["actor"])


def test_the_last_rows_next_states_are_the_datasets(data, tmp_path):
    """Every episode's last row, sampled by its flat index: its next state is the dataset's next_observations of that
    row (the slot the loader writes by hand), normalised like every other observation; and the policy is saved with the
    statistics next to it."""
    buf, norm = filled(data)
    last = np.arange(EPISODES) * STEPS + STEPS - 1
    inds = np.concatenate([last, last - 1])
    s, a, r, d, s2 = (x.cpu().numpy() for x in buf.sample(len(inds), inds=inds))
    rows = np.concatenate([last, last - 1])
    assert np.array_equal(s, norm(data.observations[rows])) and np.array_equal(a, data.actions[rows])
    assert np.array_equal(r[:, 0], data.rewards[rows]) and not d.any()
    assert np.array_equal(s2[:EPISODES], norm(data.next_observations[last]))
    assert np.array_equal(s2[EPISODES:], norm(data.observations[last]))         # inside an episode: the following row
    algo = learner(data)
    tr = OfflineTrainer(logger=NullLogger(tmp_path), make_env_test=make_env, replay_buffer=buf, algo=algo, obs_norm=norm)
    tr.save_policy(tmp_path / "weights" / "64.w")
    with np.load(tmp_path / "weights" / "64.w.norm.npz") as z:
        assert np.array_equal(z["mean"], norm.mean) and np.array_equal(z["std"], norm.std)
    assert (tmp_path / "weights" / "64.w").stat().st_size > 0
