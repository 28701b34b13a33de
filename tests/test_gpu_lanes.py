"""GPU tests of several open replay episodes (csrc/replay_rows.hip): what oprl_replay_write_rows puts into
HBM against tests/lanes_oracle.py, through both host paths; the uniform, n-step and prioritized samplers and a learner's
step_n over such a replay; what the C entry point refuses; its order against the classic write path; VecTrainer with
open episodes.  Everything compared is a copy: every comparison is bit for bit."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest
import torch as t

from oprl_amd import _capi
from tests import nstep_oracle as no
from tests.lanes_oracle import LanesOracle, random_step
from tests.support import INVALID, assert_same_state, loop_updates, refused

pytestmark = pytest.mark.gpu
NAMES = ("states", "actions", "rewards", "dones")


def make(E, L, S, A, cls=None, **kw):
    from oprl_amd.buffers.episodic_buffer import EpisodicReplayBuffer
    return (cls or EpisodicReplayBuffer)(buffer_size_transitions=E * L, state_dim=S, action_dim=A, max_episode_lenth=L,
                                         device="cuda", seed=7, **kw).create()


def scripted_over(call: int, lens, lanes, L: int, stride: int = 1) -> np.ndarray:
    """Lane i closes every (2 i + 3) stride-th call (lanes close in different calls, and in the same one when their
    periods meet), every lane closes in every 13 stride-th call, and a lane whose episode is full after this step has to."""
    over = np.array([(call + 1) % ((2 * i + 3) * stride) == 0 for i in range(len(lanes))]) | ((call + 1) % (13 * stride) == 0)
    if call < 2 * L:
        over[0] = False                         # lane 0's first episodes run to the full length: a step at t = L - 1
    for i, e in enumerate(lanes):
        if lens[e] + 1 >= L:
            over[i] = True
    return over


def drive(buf, ora, calls: int, stride: int = 1):
    """`calls` scripted steps into the buffer and the oracle; returns [(wrote, over)] per call."""
    rs = np.random.RandomState(0)
    log = []
    for call in range(calls):
        step = random_step(rs, ora.N, ora.S, ora.A)
        over = scripted_over(call, ora.ep_lens, ora.lanes, ora.L, stride)
        log.append((ora.step(*step, over), over))
        buf.add_step_rows(*step, over)
    return log


def assert_equal(buf, ora):
    for name, want in zip(NAMES, ora.storage()):
        got = getattr(buf, name).cpu().numpy()
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), name
    assert buf.ep_lens == ora.ep_lens.tolist()
    assert (buf.episodes_counter, buf._ep_pointer, len(buf), buf._lanes) == (ora.counter, ora.pointer, ora.count, ora.lanes)


def wrapped(E, L, S, A, N, calls, cls=None, stride=1, **kw):
    buf, ora = make(E, L, S, A, cls=cls, **kw), LanesOracle(E, L, S, A, N)
    buf.open_lanes(N)
    log = drive(buf, ora, calls, stride)
    assert len(ora.evicted) >= 2 * E, "the script must wrap the ring at least twice"
    return buf, ora, log


# ---- 1, 2: storage ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 4, 5])
@pytest.mark.parametrize("S,A", [(3, 2), (17, 6)])
def test_storage_equals_the_oracle_after_the_ring_wrapped_twice(S, A, N):
    E, L = 6, 5
    buf, ora, log = wrapped(E, L, S, A, N, 40 if N > 1 else 70)
    assert_equal(buf, ora)
    assert any(k == L - 1 for wrote, _ in log for _, k in wrote)         # a step at t = L - 1 wrote states[e, L]
    if N > 1:
        closes = [int(over.sum()) for _, over in log]
        assert 1 in closes and max(closes) >= 2                          # closes alone and together


@pytest.mark.parametrize("N", [16, 17, 256])
def test_both_host_paths_equal_the_oracle(N):
    """N = 16: the kernel reads the pinned records itself; 17: they are copied to device staging first; 256: the most."""
    E, L, S, A = 300, 3, 5, 2
    buf, ora = make(E, L, S, A), LanesOracle(E, L, S, A, N)
    buf.open_lanes(N)
    drive(buf, ora, 12)
    assert len(ora.evicted) > 0
    assert_equal(buf, ora)


# ---- 3, 4: the samplers -------------------------------------------------------------------------------------------------
def test_uniform_sample_of_every_live_index_and_the_open_tails():
    buf, ora, _ = wrapped(6, 5, 17, 6, 4, 43)
    n = len(buf)
    assert n == ora.count == len(ora.live_slots())
    got, (ep, st) = buf.sample(n, inds=np.arange(n), return_indices=True)
    want = ora.gather(np.arange(n))
    assert np.array_equal(ep.cpu().numpy(), want["ep"]) and np.array_equal(st.cpu().numpy(), want["step"])
    for k, x in zip(("s", "a", "r", "d", "s2"), got):
        assert np.array_equal(x.cpu().numpy().view(np.uint32), want[k].view(np.uint32)), k
    # the last stored step of every running episode: its s2 is the next state that lane passed last, not a never-written row
    slots, tails = ora.live_slots(), 0
    for lane, e in enumerate(ora.lanes):
        k = int(ora.ep_lens[e])
        if k == 0:
            continue                # (the lane closed in the last call: its new episode holds nothing yet)
        row = got[4][slots.index((e, k - 1))].cpu().numpy()
        assert np.array_equal(row, ora.last_s2[lane]) and np.any(row != 0)
        tails += 1
    assert tails >= 2


def test_nstep_sample_over_lanes_equals_the_nstep_oracle():
    from oprl_amd.buffers.nstep_buffer import NStepEpisodicReplayBuffer
    buf, ora, _ = wrapped(8, 8, 17, 6, 4, 80, cls=NStepEpisodicReplayBuffer, stride=2, n_step=3, gamma=0.99)
    n = len(buf)
    got, (ep, st), m = buf.sample(n, inds=np.arange(n), return_indices=True, return_steps=True)
    want = no.nstep_gather(*ora.storage(), ora.live_lens(), np.arange(n), 3, 0.99)
    assert np.array_equal(ep.cpu().numpy(), want["ep"]) and np.array_equal(st.cpu().numpy(), want["step"])
    assert np.array_equal(m.cpu().numpy(), want["m"]) and set(want["m"].tolist()) == {1, 2, 3}
    for k, x in zip(("s", "a", "r", "d", "s2"), got):
        assert np.array_equal(x.cpu().numpy().view(np.uint32), want[k].view(np.uint32)), k


# ---- 5: the sum tree ----------------------------------------------------------------------------------------------------
def test_prioritized_replay_with_lanes():
    from oprl_amd.buffers.prioritized_buffer import PrioritizedEpisodicReplayBuffer
    E, L, N = 6, 5, 4
    buf, ora, _ = wrapped(E, L, 17, 6, N, 43, cls=PrioritizedEpisodicReplayBuffer)

    def live_mask():
        mask = np.zeros((E, L), bool)
        for e, k in ora.live_slots():
            mask[e, k] = True
        return mask

    assert np.array_equal(buf.priorities().cpu().numpy(), live_mask().astype(np.float32))
    buf.sample(64)
    slots = buf.last_slots.cpu().numpy()
    assert live_mask().reshape(-1)[slots].all() and bool((buf.last_weights > 0).all())
    # new priorities for every live slot, then one more step of every lane
    live = np.flatnonzero(live_mask().reshape(-1)).astype(np.int32)
    buf.update_priorities(live, np.linspace(0.5, 3.0, len(live), dtype=np.float32))
    before = buf.priorities().cpu().numpy().copy()
    assert len(set(before.reshape(-1)[live].tolist())) == len(live) and before.max() > 1.0
    step = random_step(np.random.RandomState(99), N, 17, 6)
    over = np.array([int(ora.ep_lens[e]) + 1 >= L for e in ora.lanes])      # only a lane that is full afterwards closes
    n_evicted = len(ora.evicted)
    wrote = ora.step(*step, over)
    buf.add_step_rows(*step, over)
    after = buf.priorities().cpu().numpy()
    touched = np.zeros((E, L), bool)
    for e, k in wrote:
        touched[e, k] = True
    for e in ora.evicted[n_evicted:]:
        touched[e, :] = True
    assert int((before[~touched] > 0).sum()) >= 5
    assert np.array_equal(after[~touched], before[~touched])           # the updated leaves of untouched slots stay
    p_max = float(before.max())
    for e, k in wrote:
        if live_mask()[e, k]:
            assert after[e, k] == np.float32(p_max)                    # a new row enters with the largest priority so far
    assert np.array_equal(after > 0, live_mask())


# ---- 6: a learner over the same table ----------------------------------------------------------------------------------
def _ddpg(S, A):
    from oprl_amd.algos.ddpg import DDPG
    from oprl_amd.logging import NullLogger
    t.manual_seed(0)
    return DDPG(logger=NullLogger("/tmp/oprl_amd_test"), state_dim=S, action_dim=A, device="cuda", precision="f32").create()


def test_step_n_over_a_lanes_replay_equals_sample_then_update():
    S, A, B = 24, 6, 32
    buf, ora, _ = wrapped(12, 10, S, A, 4, 200, stride=3)
    assert len(buf) >= B
    fused, loop = _ddpg(S, A), _ddpg(S, A)
    assert_same_state(fused, loop)
    print("launch form at B = 32:", fused.debug_form(B))
    fused.learner.step_n(buf.handle, 3, B, seed=11)
    loop_updates(loop, buf, 3, 11, B)
    assert_same_state(fused, loop)
    assert fused.update_step == 3
    assert_equal(buf, ora)


# ---- 7, 8: the C entry point --------------------------------------------------------------------------------------------
def _i32(x):
    return np.asarray(x, dtype=np.int32)


def _p(x, kind=C.c_void_p):
    return None if x is None else x.ctypes.data_as(kind)


def write_rows(buf, ep, k, s, a, r, d, s2, lens, counter, n=None):
    i32 = C.POINTER(C.c_int32)
    return buf._lib.oprl_replay_write_rows(buf._handle, len(ep) if n is None else n, _p(ep, i32), _p(k, i32), _p(s), _p(a),
                                           _p(r), _p(d), _p(s2), _p(lens, i32), counter, _capi.current_stream())


def test_c_level_refusals_change_nothing():
    E, L, S, A, N = 6, 5, 3, 2, 4
    buf, ora, _ = wrapped(E, L, S, A, N, 43)
    n = len(buf)
    t.cuda.synchronize()
    tensors = {k: v.clone() for k, v in buf._tensors.items()}
    sample = [x.clone() for x in buf.sample(n, inds=np.arange(n))]
    rs = np.random.RandomState(5)
    big = 300
    s, a, r, d, s2 = random_step(rs, big, S, A)
    lens, counter = _i32(buf.ep_lens), buf.episodes_counter
    free = [e for e in range(E) if e not in buf._lanes]
    ok_ep, ok_t = _i32([free[0], free[1]]), _i32([0, 1])
    bad_lens = lens.copy()
    bad_lens[0] = L + 1
    cases = {
        "n = 0": dict(ep=ok_ep, k=ok_t, n=0),
        "n = 257": dict(ep=_i32(np.arange(257) % E), k=_i32(np.zeros(257)), n=257),
        "a duplicate ep": dict(ep=_i32([free[0], free[1], free[0]]), k=_i32([0, 0, 1])),
        "t = L": dict(ep=ok_ep, k=_i32([0, L])),
        "ep = E": dict(ep=_i32([free[0], E]), k=ok_t),
        "ep = -1": dict(ep=_i32([-1, free[0]]), k=ok_t),
        "a null s2": dict(ep=ok_ep, k=ok_t, s2=None),
        "a table set_lens refuses": dict(ep=ok_ep, k=ok_t, lens=bad_lens),
    }
    for what, kw in cases.items():
        args = dict(s=s, a=a, r=r, d=d, s2=s2, lens=lens, counter=counter)
        args.update(kw)
        refused(write_rows(buf, **args), INVALID)
        t.cuda.synchronize()
        for k, v in buf._tensors.items():
            assert t.equal(v, tensors[k]), (what, k)
        for x, y in zip(buf.sample(n, inds=np.arange(n)), sample):
            assert t.equal(x, y), what
    # ... and the same arguments, valid, are taken: the handle is as usable as before
    assert write_rows(buf, ok_ep, ok_t, s, a, r, d, s2, lens, counter) == 0
    t.cuda.synchronize()
    assert np.array_equal(buf._tensors["states"][free[1], 1:3].cpu().numpy(), np.stack([s[1], s2[1]]))
    assert np.array_equal(buf._tensors["actions"][free[0], 0].cpu().numpy(), a[0])


def test_a_classic_row_staged_before_write_rows_lands_before_it():
    E, L, S, A = 4, 5, 3, 2
    buf = make(E, L, S, A)
    lib, h = buf._lib, buf._handle
    rs = np.random.RandomState(6)
    s_old, s_other, a_old = rs.standard_normal(S).astype(np.float32), rs.standard_normal(S).astype(np.float32), np.ones(A, np.float32)
    s, a, r, d, s2 = random_step(rs, 1, S, A)
    # two classic rows are staged and NOT flushed: one for slot (1, 0), one for slot (2, 3)
    assert lib.oprl_replay_write(h, 1, 0, _p(s_old), _p(a_old), 5.0, 1.0) == 0
    assert lib.oprl_replay_write(h, 2, 3, _p(s_other), _p(a_old), 6.0, 0.0) == 0
    # the later call writes slot (1, 0) too
    lens = _i32([0, 1, 0, 0])
    assert write_rows(buf, _i32([1]), _i32([0]), s, a, r, d, s2, lens, 2) == 0
    t.cuda.synchronize()
    st = buf._tensors                                  # (raw storage: reading it flushes nothing)
    assert np.array_equal(st["states"][2, 3].cpu().numpy(), s_other) and float(st["rewards"][2, 3, 0]) == 6.0   # it went ahead
    assert np.array_equal(st["states"][1, 0:2].cpu().numpy(), np.stack([s[0], s2[0]]))                          # the later value wins
    assert np.array_equal(st["actions"][1, 0].cpu().numpy(), a[0])
    assert float(st["rewards"][1, 0, 0]) == float(r[0]) and float(st["dones"][1, 0, 0]) == float(d[0])
    assert lib.oprl_replay_flush(h, _capi.current_stream()) == 0            # nothing is left to land later
    t.cuda.synchronize()
    assert np.array_equal(st["states"][1, 0].cpu().numpy(), s[0])


# ---- 9: the trainer -----------------------------------------------------------------------------------------------------
def test_vec_trainer_with_open_episodes_learns_from_the_fourth_iteration():
    from oprl_amd.environment.synthetic import SyntheticEnv
    from oprl_amd.logging import NullLogger
    from oprl_amd.trainers.vec_trainer import VecTrainer
    N, B, L, steps = 4, 16, 25, 240
    algo = _ddpg(24, 6)
    buf = make(40, L, 24, 6)

    def make_env(seed):
        return SyntheticEnv("walker-walk", seed, episode_length=L)

    counts = []

    class Counting(VecTrainer):
        def _collect_open(self, steps, obs):
            if steps > 0:
                counts.append(self.algo.learner.update_count)       # the count after the previous iteration
            return super()._collect_open(steps, obs)

    trainer = Counting(envs=[make_env(100 + i) for i in range(N)], open_episodes=True, logger=NullLogger("/tmp/oprl_amd_test"),
                       make_env_test=make_env, replay_buffer=buf, algo=algo, num_steps=steps, start_steps=0, batch_size=B,
                       eval_interval=10 ** 9, save_policy_every=0, stdout_log_every=10 ** 9, num_eval_episodes=1, seed=0)
    trainer.train()
    t.cuda.synchronize()
    counts.append(algo.learner.update_count)
    iterations = steps // N
    assert counts == [4 * max(0, k - 3) for k in range(1, iterations + 1)]       # the first update in iteration 4, not 25
    assert len(buf) == steps and buf._lanes == [8, 9, 10, 11] and buf.ep_lens[:12] == [L] * 8 + [10] * 4
    for m in (algo.actor, algo.critic, algo.actor_target, algo.critic_target):
        assert bool(t.isfinite(m._oprl_arena).all())
    algo.learner.check()
    # every stored step has its next state: the environments' own observations chain through the episodes
    states = buf.states.cpu().numpy()
    assert all(np.any(states[e, buf.ep_lens[e]] != 0) for e in range(12))
