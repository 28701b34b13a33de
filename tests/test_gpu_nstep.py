"""GPU tests of n-step returns out of the HBM replay (csrc/replay_nstep.hip): the gather kernel bit for
bit against tests/nstep_oracle.py and, at n = 1, against the uniform sampler; the learners' step_n over an n-step replay
against sample() + update() pairs, and its TD target against float64; what is refused; the checkpoint round trip."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest
import torch as t

from oprl_amd import _capi
from tests import nstep_oracle as no
from tests import scenarios as sc
from tests import support
from tests.support import (INVALID, STATE, assert_same_state, fill_random, live_lens, loop_updates, refused, set_table,  # noqa: F401
                           storage)

pytestmark = pytest.mark.gpu
TOL = 2e-5          # the output gate of tests/test_gpu_algos.py
KEYS = ("s", "a", "r", "d", "s2")


def make_buffer(E, L, S, A, n_step=3, gamma=0.99, seed=7, cls=None):
    from oprl_amd.buffers.nstep_buffer import NStepEpisodicReplayBuffer
    kw = dict(n_step=n_step) if cls is None else {}
    buf = (cls or NStepEpisodicReplayBuffer)(buffer_size_transitions=E * L, state_dim=S, action_dim=A,
                                             max_episode_lenth=L, gamma=gamma, device="cuda", seed=seed, **kw).create()
    return fill_random(buf, gen_seed=1000 + E + L)


def set_mode(buf, n, gamma):
    buf.n_step, buf.gamma = n, gamma
    buf._set_nstep()


def uniform_sample(buf, B, inds=None):
    """The uniform sampler's answer on the same handle and (seed, counter): the mode is switched off for the call."""
    from oprl_amd.buffers.episodic_buffer import EpisodicReplayBuffer
    n, counter = buf.n_step, buf._sample_counter
    set_mode(buf, 1, buf.gamma)
    out = EpisodicReplayBuffer.sample(buf, B, inds=inds, return_indices=True)
    set_mode(buf, n, buf.gamma)
    buf._sample_counter = counter
    return out


def flat_indices(buf, ep, step):
    starts = np.concatenate([[0], np.cumsum(live_lens(buf))[:-1]])
    return starts[ep.cpu().numpy()] + step.cpu().numpy()


def assert_matches_oracle(buf, got, ep, step, m, inds, n, gamma):
    want = no.nstep_gather(*storage(buf), live_lens(buf), inds, n, gamma)
    assert np.array_equal(ep.cpu().numpy(), want["ep"]) and np.array_equal(step.cpu().numpy(), want["step"])
    assert np.array_equal(m.cpu().numpy(), want["m"]), (m.cpu().numpy(), want["m"])
    for k, x in zip(KEYS, got):
        assert np.array_equal(x.cpu().numpy().view(np.uint32), want[k].view(np.uint32)), (n, gamma, k)
    return want


# E = 12, L = 20, S = 3, A = 2: ten closed episodes, one of them empty, and a tail in progress
LENS = [1, 2, 5, 20, 7, 0, 3, 20, 11, 4]
TAIL = 6


@pytest.fixture(scope="module")
def replay():
    """Written through the buffer's own API.  Dones: episodes 0, 3, 4, 9 end in done = 1; episode 7 (full length) is
    truncated, done = 0 throughout; episode 8 holds the non-binary 0.5 at step 3; the tail, written with add_transitions
    and not closed, has done = 1 at step 2 of its 6 stored steps."""
    S, A = 3, 2
    buf = make_buffer(12, 20, S, A)
    rs = np.random.RandomState(5)
    for e, n in enumerate([*LENS, TAIL]):
        rows = rs.standard_normal((n, S + A + 2)).astype(np.float32)
        rows[:, S + A + 1] = 0
        if e in (0, 3, 4, 9):
            rows[-1, S + A + 1] = 1
        if e == 8:
            rows[3, S + A + 1] = 0.5
        if e == 10:
            rows[2, S + A + 1] = 1
        buf.add_transitions(rows, episode_done=e < len(LENS))
    assert live_lens(buf) == [*LENS, TAIL] and len(buf) == sum(LENS) + TAIL
    return buf


@pytest.mark.parametrize("B", ["live", 61, 1])
@pytest.mark.parametrize("drawn", [False, True], ids=["injected", "drawn"])
def test_n1_equals_the_uniform_sampler_bit_for_bit(replay, B, drawn):
    buf = replay
    N = len(buf)
    B = N if B == "live" else B
    inds = None if drawn else (np.arange(N) if B == N else np.random.RandomState(B).randint(0, N, B))
    set_mode(buf, 1, 0.99)
    buf._sample_counter = 3
    want, (w_ep, w_st) = uniform_sample(buf, B, inds)
    got, (ep, st), m = buf.sample(B, inds=inds, return_indices=True, return_steps=True)      # the n-step kernel at n = 1
    for k, x, y in zip(KEYS, got, want):
        assert t.equal(x.view(t.int32), y.view(t.int32)), k
    assert t.equal(ep, w_ep) and t.equal(st, w_st) and bool((m == 1).all())
    if not drawn and B == N:
        assert sorted(zip(ep.tolist(), st.tolist())) == [(e, k) for e, n in enumerate([*LENS, TAIL]) for k in range(n)]


@pytest.mark.parametrize("gamma", [0.99, 0.9])
@pytest.mark.parametrize("n", [2, 3, 5, 16])
def test_bitexact_against_the_oracle(replay, n, gamma):
    buf = replay
    N = len(buf)
    set_mode(buf, n, gamma)
    got, (ep, st), m = buf.sample(N, inds=np.arange(N), return_indices=True, return_steps=True)
    want = assert_matches_oracle(buf, got, ep, st, m, np.arange(N), n, gamma)
    if n == 5:          # no branch of the scan goes unexercised
        assert set(want["m"].tolist()) == {1, 2, 3, 4, 5}
    # m never runs past a done or the stored end, whatever the never-written rows hold
    dones, lens = storage(buf)[3].reshape(12, 20), np.asarray(live_lens(buf))
    e, k, mm = want["ep"], want["step"], want["m"]
    assert np.all(k + mm <= lens[e]) and all(np.all(dones[a, b:b + c - 1] == 0) for a, b, c in zip(e, k, mm))
    # device-drawn rows: the uniform sampler's (episode, step) for the same (seed, counter), a ragged batch
    buf._sample_counter = 11
    _, (u_ep, u_st) = uniform_sample(buf, 61)
    got, (ep, st), m = buf.sample(61, return_indices=True, return_steps=True)
    assert t.equal(ep, u_ep) and t.equal(st, u_st)
    assert_matches_oracle(buf, got, ep, st, m, flat_indices(buf, ep, st), n, gamma)


def test_oprl_replay_sample_forwards_to_the_nstep_gather(replay):
    """EpisodicReplayBuffer.sample (oprl_replay_sample) on a handle in n-step mode returns the n-step rows."""
    from oprl_amd.buffers.episodic_buffer import EpisodicReplayBuffer
    buf = replay
    set_mode(buf, 3, 0.99)
    inds = np.arange(len(buf))
    via_plain = EpisodicReplayBuffer.sample(buf, len(buf), inds=inds)
    for x, y in zip(via_plain, buf.sample(len(buf), inds=inds)):
        assert t.equal(x, y)
    assert not t.equal(via_plain[2], uniform_sample(buf, len(buf), inds)[0][2])


def test_coarse_episode_table():
    """More episodes than the 2048 LDS entries of the table: the coarse table and its global finish, where the
    episode's end is read from global memory too."""
    E, L, n, gamma = 2500, 4, 3, 0.99
    buf = make_buffer(E, L, 3, 2, n_step=n, gamma=gamma)
    rs = np.random.RandomState(2)
    buf._tensors["dones"].copy_(t.as_tensor((rs.rand(E, L, 1) < 0.2).astype(np.float32)))
    set_table(buf, rs.randint(0, L + 1, size=E))
    got, (ep, st), m = buf.sample(512, return_indices=True, return_steps=True)
    want = assert_matches_oracle(buf, got, ep, st, m, flat_indices(buf, ep, st), n, gamma)
    assert set(want["m"].tolist()) == {1, 2, 3} and len(set(want["ep"].tolist())) > 300


def test_after_eviction_the_old_tail_is_never_read():
    """The ring wraps onto a 10-step episode's slot and refills it with 3 steps: rows 3 .. 9 of the old episode (huge
    rewards, done = 0) stay in storage and must enter no R and no s'."""
    S, A, L = 3, 2, 10
    buf = make_buffer(4, L, S, A, n_step=5, gamma=0.9)
    rs = np.random.RandomState(8)
    for n, big in ((10, True), (5, False), (5, False), (5, False), (3, False)):
        rows = rs.standard_normal((n, S + A + 2)).astype(np.float32)
        rows[:, S + A + 1] = 0
        if big:
            rows[:, S + A] += 1e6
        buf.add_transitions(rows, episode_done=True)
    assert buf.ep_lens == [3, 0, 5, 5] and buf.episodes_counter == 4 and len(buf) == 13
    assert float(buf.rewards[0, 3:].min()) > 1e5                     # the old tail is still there
    got, (ep, st), m = buf.sample(13, inds=np.arange(13), return_indices=True, return_steps=True)
    want = assert_matches_oracle(buf, got, ep, st, m, np.arange(13), 5, 0.9)
    assert float(got[2].abs().max()) < 1e3 and list(want["m"][:3]) == [3, 2, 1]


# ---- learners -----------------------------------------------------------------------------------------------------------
LS, LA, LB, LN, LGAMMA = 24, 6, 64, 3, 0.99


@pytest.fixture(scope="module")
def learner_replays():
    """An n-step replay (n = 3) at walker dims and a plain replay over the same storage contents and table."""
    from oprl_amd.buffers.episodic_buffer import EpisodicReplayBuffer
    E, L = 40, 30
    return support.twin_replays(make_buffer(E, L, LS, LA, n_step=LN, gamma=LGAMMA),
                                make_buffer(E, L, LS, LA, n_step=LN, gamma=LGAMMA, cls=EpisodicReplayBuffer), E, L)


def make_algo(name, prec):
    return support.make_algo(name, prec, LS, LA)


@pytest.mark.parametrize("name,prec", [("ddpg", "f32"), ("td3", "f32"), ("sac", "f32"), ("tqc", "f32"), ("ddpg", "x2"),
                                       ("ddpg", "bf16")])
def test_step_n_over_an_nstep_replay_equals_sample_then_update(learner_replays, name, prec):
    nbuf, pbuf = learner_replays
    fused, loop = make_algo(name, prec), make_algo(name, prec)
    assert_same_state(fused, loop)
    print(name, prec, "launch form at B = 64:", fused.debug_form(LB))
    fused.learner.step_n(nbuf.handle, 3, LB, seed=11)
    loop_updates(loop, nbuf, 3, 11, LB)
    assert_same_state(fused, loop)
    assert fused.update_step == 3
    # the n-step rows are not the one-step rows (the comparison above is not vacuous)
    nbuf._sample_counter = pbuf._sample_counter = 0
    nbuf.seed = pbuf.seed = 11
    assert not t.equal(nbuf.sample(LB)[4], pbuf.sample(LB)[4])
    # no flag is left behind: step_n over a plain replay, against the twin whose learner never saw the n-step handle
    fused.learner.step_n(pbuf.handle, 3, LB, seed=12)
    loop.learner.step_n(pbuf.handle, 3, LB, seed=12)
    assert_same_state(fused, loop)
    assert fused.update_step == 6


def mlp64(params, x):
    ps = [p.detach().cpu().double() for p in params]
    for i in range(0, len(ps), 2):
        x = x @ ps[i].T + ps[i + 1]
        if i + 2 < len(ps):
            x = t.relu(x)
    return x


def test_ddpg_td_target_is_the_nstep_target(learner_replays):
    """debug_q_y's y of the first update against float64 R + gamma^m (1 - d_last) Qbar(s_{t+m}, pibar(s_{t+m})) from the
    learner's own target parameters; the one-step target of the same slots misses the same gate."""
    nbuf, _ = learner_replays
    algo = make_algo("ddpg", "f32")
    actor_t = [p.clone() for p in algo.actor_target.parameters()]
    critic_t = [p.clone() for p in algo.critic_target.parameters()]
    algo.learner.step_n(nbuf.handle, 1, LB, seed=5)
    _q, y = algo.learner.debug_q_y(LB)
    algo.learner.check()
    nbuf.seed, nbuf._sample_counter = 5, 0
    _rows, (ep, st), m = nbuf.sample(LB, return_indices=True, return_steps=True)
    ep, st, m = ep.cpu().long(), st.cpu().long(), m.cpu().long()
    states, _a, rewards, dones = (t.as_tensor(x).double() for x in storage(nbuf))
    rewards, dones = rewards.squeeze(-1), dones.squeeze(-1)

    def target(steps, R, d_last):
        s2 = states[ep, st + steps]
        qn = mlp64(critic_t, t.cat([s2, t.tanh(mlp64(actor_t, s2))], dim=1)).reshape(-1)
        return R + LGAMMA ** steps.double() * (1 - d_last) * qn

    R = t.zeros(LB, dtype=t.float64)
    for k in range(LN):
        R += t.where(k < m, LGAMMA ** k * rewards[ep, t.minimum(st + k, st + m - 1)], t.zeros(()).double())
    y_n = target(m, R, dones[ep, st + m - 1])
    y_1 = target(t.ones_like(m), rewards[ep, st], dones[ep, st])
    dev_n, dev_1 = sc.rel_dev(y.cpu().numpy(), y_n.numpy()), sc.rel_dev(y.cpu().numpy(), y_1.numpy())
    print(f"y vs the float64 n-step target {dev_n:.2e}, vs the one-step target {dev_1:.2e}; m counts {t.bincount(m).tolist()}")
    assert int(m.max()) == LN and int(m.min()) == 1
    assert dev_n < TOL
    assert not dev_1 < TOL


# ---- refusals ---------------------------------------------------------------------------------------------------------
def test_refusals(learner_replays):
    from oprl_amd.buffers.episodic_buffer import EpisodicReplayBuffer
    from oprl_amd.buffers.prioritized_buffer import PrioritizedEpisodicReplayBuffer
    from oprl_amd.group import LearnerGroup
    lib = _capi.load()
    nbuf, _ = learner_replays
    plain = EpisodicReplayBuffer(buffer_size_transitions=40, state_dim=3, action_dim=2, max_episode_lenth=10,
                                 device="cuda").create()
    for n, gamma in ((0, 0.99), (17, 0.99), (3, 0.0), (3, 1.5)):
        refused(lib.oprl_replay_set_nstep(plain._handle, n, gamma), INVALID)
    assert lib.oprl_replay_set_nstep(plain._handle, 1, 1.0) == 0 and lib.oprl_replay_set_nstep(plain._handle, 16, 1.0) == 0
    # n-step and the sum tree exclude each other, either way round
    refused(lib.oprl_replay_prio_enable(plain._handle, 0.6, 1e-6, None), STATE)
    assert lib.oprl_replay_set_nstep(plain._handle, 1, 1.0) == 0           # n = 1 switches the mode off ...
    assert lib.oprl_replay_prio_enable(plain._handle, 0.6, 1e-6, None) == 0    # ... and the tree is allowed again
    prio = PrioritizedEpisodicReplayBuffer(buffer_size_transitions=40, state_dim=3, action_dim=2, max_episode_lenth=10,
                                           device="cuda").create()
    refused(lib.oprl_replay_set_nstep(prio._handle, 3, 0.99), STATE)
    t.cuda.synchronize()
    # the packed learners gather one-step rows inside their launches
    members = [make_algo("ddpg", "f32") for _ in range(2)]
    g = LearnerGroup(members)
    seeds = (C.c_uint64 * 2)(1, 2)
    refused(lib.oprl_group_step_n(g.handle, nbuf.handle, 1, LB, seeds, _capi.current_stream()), STATE)
    assert members[0].update_step == 0
    # the sampler's gamma^(m-1) multiplies the learner's gamma: they must be one number
    set_mode(nbuf, LN, 0.95)
    try:
        msg = refused(lib.oprl_learner_step_n(members[0].learner.handle, nbuf.handle, 1, LB, 0, _capi.current_stream()), INVALID)
        assert b"gamma" in msg and members[0].update_step == 0
        with pytest.raises(ValueError, match="gamma"):
            members[0].update_from_buffer(nbuf, LB)
    finally:
        set_mode(nbuf, LN, LGAMMA)
    assert lib.oprl_learner_step_n(members[0].learner.handle, nbuf.handle, 1, LB, 0, _capi.current_stream()) == 0
    t.cuda.synchronize()
    members[0].learner.check()


def test_checkpoint_round_trip(replay):
    buf = replay
    set_mode(buf, 5, 0.9)
    buf._sample_counter = 17
    sd = buf.state_dict()
    assert sd["n_step"] == 5 and sd["gamma"] == 0.9
    twin = make_buffer(12, 20, 3, 2, n_step=2, gamma=0.5, seed=99)
    twin.load_state_dict(sd)
    assert (twin.n_step, twin.gamma, twin.seed, twin._sample_counter) == (5, 0.9, buf.seed, 17)
    a, (a_ep, a_st), a_m = buf.sample(61, return_indices=True, return_steps=True)
    b, (b_ep, b_st), b_m = twin.sample(61, return_indices=True, return_steps=True)
    for x, y in zip(a, b):
        assert t.equal(x.view(t.int32), y.view(t.int32))
    assert t.equal(a_ep, b_ep) and t.equal(a_st, b_st) and t.equal(a_m, b_m) and int(a_m.max()) > 1
