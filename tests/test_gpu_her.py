"""GPU tests of hindsight experience replay out of the HBM replay (csrc/replay_her.hip): the gather
kernel bit for bit against tests/her_oracle.py, the sparse reward at its threshold, the dense reward against numpy, the
equivalences with the uniform sampler, memory safety, what is refused, the checkpoint round trip, the learners' step_n
over a hindsight replay against sample() + update() pairs, and the trainer loop on the goal-conditioned environment."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest
import torch as t

from oprl_amd import _capi
from tests import her_oracle as ho
from tests import support
from tests.support import INVALID, STATE, assert_same_state, fill_random, live_lens, loop_updates, refused, set_table, storage

pytestmark = pytest.mark.gpu
KEYS = ("s", "a", "r", "d", "s2")
STRATEGY = {"future": ho.FUTURE, "final": ho.FINAL}
KIND = {"sparse": ho.SPARSE, "dense": ho.DENSE}
SENT_F, SENT_I = 12345.0, -777


def make_buffer(E, L, S, A, seed=7, cls=None, **her):
    from oprl_amd.buffers.hindsight_buffer import HindsightEpisodicReplayBuffer
    buf = (cls or HindsightEpisodicReplayBuffer)(buffer_size_transitions=E * L, state_dim=S, action_dim=A,
                                                 max_episode_lenth=L, device="cuda", seed=seed, **her).create()
    return fill_random(buf, ("actions", "rewards", "dones", "states"), gen_seed=1000 + E + L)


def set_mode(buf, **kw):
    for k, v in kw.items():
        setattr(buf, k, v)
    buf._validate()
    buf._set_her()


def oracle(buf, B, counter, inds=None):
    return ho.her_gather(*storage(buf), live_lens(buf), buf.seed, counter, B, buf.achieved_offset, buf.desired_offset,
                         buf.goal_dim, buf.her_ratio, STRATEGY[buf.strategy], KIND[buf.reward], buf.threshold, inds=inds)


def sample(buf, B, counter, inds=None):
    """buf.sample at a given counter, every output as numpy: dict(s, a, r, d, s2, ep, step, future)."""
    buf._sample_counter = counter
    rows, (ep, st), fut = buf.sample(B, inds=inds, return_indices=True, return_relabel=True)
    out = {k: x.cpu().numpy() for k, x in zip(KEYS, rows)}
    out.update(ep=ep.cpu().numpy(), step=st.cpu().numpy(), future=fut.cpu().numpy())
    return out


def assert_same(got, want, what=""):
    for k in ("ep", "step", "future"):
        if k in got and k in want:
            assert np.array_equal(got[k], want[k]), (what, k, got[k], want[k])
    for k in KEYS:
        a, b = np.ascontiguousarray(got[k]).view(np.uint32), np.ascontiguousarray(want[k]).view(np.uint32)
        assert a.shape == b.shape and np.array_equal(a, b), (what, k, np.argwhere(a != b)[:4].tolist())


# E = 8, L = 12: seven episodes, lengths 1, 2 and 12 among them, slot 3 evicted (no stored steps)
LENS = [1, 2, 12, 0, 5, 7, 12]
N_LIVE = sum(LENS)
TASK = dict(goal_dim=3, achieved_offset=6, desired_offset=9, threshold=0.1)      # goal-reach-3d's layout, S = 12


@pytest.fixture(scope="module")
def replay():
    buf = make_buffer(8, 12, 12, 2, **TASK)
    set_table(buf, LENS)
    return buf


@pytest.fixture(scope="module")
def plain_twin():
    """A plain replay over the same storage contents and table."""
    from oprl_amd.buffers.episodic_buffer import EpisodicReplayBuffer
    buf = make_buffer(8, 12, 12, 2, cls=EpisodicReplayBuffer)
    set_table(buf, LENS)
    return buf


def injected(B):
    return np.arange(B) % N_LIVE if B >= 16 else np.array([20 + B])


@pytest.mark.parametrize("B", [1, 16, 17, 61])
@pytest.mark.parametrize("drawn", [False, True], ids=["injected", "drawn"])
@pytest.mark.parametrize("strategy", ["future", "final"])
def test_bitexact_against_the_oracle(replay, plain_twin, strategy, drawn, B):
    buf = replay
    set_mode(buf, her_ratio=0.8, strategy=strategy, reward="sparse", threshold=1.5, **{k: TASK[k] for k in TASK if k != "threshold"})
    inds = None if drawn else injected(B)
    counter = 5 + B
    got, want = sample(buf, B, counter, inds), oracle(buf, B, counter, inds)
    assert_same(got, want, (strategy, drawn, B))
    # the slots are the uniform sampler's for the same (seed, counter)
    plain_twin.seed, plain_twin._sample_counter = buf.seed, counter
    _rows, (ep, st) = plain_twin.sample(B, inds=inds, return_indices=True)
    assert np.array_equal(ep.cpu().numpy(), got["ep"]) and np.array_equal(st.cpu().numpy(), got["step"])
    if B == 61:          # no case goes unexercised: relabelled and stored rows, rows without a candidate, both rewards
        fut, lens = want["future"], np.asarray(LENS)[want["ep"]]
        c = lens - 1 - want["step"]
        assert np.any(fut >= 0) and np.any((fut < 0) & (c >= 1)) and np.any(c == 0) and np.all(fut[c < 1] == -1)
        assert np.all((fut < 0) | ((fut >= want["step"]) & (fut <= lens - 2)))
        assert {0.0, -1.0} <= set(want["r"][fut >= 0, 0].tolist())
        if strategy == "final":
            assert np.all(fut[fut >= 0] == (lens - 2)[fut >= 0])
        else:
            assert np.any(fut == want["step"]) and np.any(fut > want["step"])


@pytest.mark.parametrize("G,ag,g", [(1, 37, 5), (16, 1, 22)])
def test_bitexact_at_the_smallest_and_the_largest_goal(G, ag, g):
    """S = 40 with the two goal ranges apart from each other and from the row's ends."""
    buf = make_buffer(8, 12, 40, 2, goal_dim=G, achieved_offset=ag, desired_offset=g, threshold=1.0 * G ** 0.5, her_ratio=0.8)
    set_table(buf, LENS)
    for strategy, kind in (("future", "sparse"), ("final", "dense")):
        set_mode(buf, strategy=strategy, reward=kind)
        got, want = sample(buf, 17, 3), oracle(buf, 17, 3)
        assert_same(got, want, (G, strategy, kind))
        assert np.any(want["future"] >= 0) and np.any(want["future"] < 0)
    # only the desired-goal columns of a relabelled row differ from the stored one
    rel = want["future"] >= 0
    states = storage(buf)[0]
    changed = got["s"] != states[want["ep"], want["step"]]
    assert not changed[~rel].any() and not np.delete(changed, np.s_[g:g + G], axis=1).any()


def test_coarse_episode_table():
    """2500 episodes: more than the 2048 table entries the kernel holds in LDS, so the table is staged coarsely and an
    episode's end comes from global memory.  Lengths 0 .. 4: relabelled rows, eligible rows left stored and rows without
    a candidate all occur, from episodes on both sides of entry 2048 (the oracle alone gives 255 / 58 / 199 such rows,
    443 distinct episodes and 101 rows from episodes >= 2048)."""
    buf = make_buffer(2500, 4, 8, 2, goal_dim=2, achieved_offset=4, desired_offset=6, threshold=1.5, her_ratio=0.8)
    lens = np.random.RandomState(2).randint(0, 5, size=2500)
    set_table(buf, lens)
    for strategy in ("future", "final"):
        set_mode(buf, strategy=strategy, reward="sparse")
        got, want = sample(buf, 512, 3), oracle(buf, 512, 3)
        assert_same(got, want, ("coarse", strategy))
        fut, c = want["future"], lens[want["ep"]] - 1 - want["step"]
        assert np.any(fut >= 0) and np.any((fut < 0) & (c >= 1)) and np.any(c == 0)
        assert len(np.unique(want["ep"])) > 300 and np.any(want["ep"] >= 2048)


# ---- the reward ---------------------------------------------------------------------------------------------------------
def test_sparse_reward_at_its_threshold(replay):
    """One relabelled row's dist2 against thresholds whose float32 square is that dist2, one float below it and one
    float above it; then t' = t and a threshold of 0."""
    buf = replay
    B, counter = 61, 9
    set_mode(buf, her_ratio=1.0, strategy="future", reward="dense", threshold=0.0, **{k: TASK[k] for k in TASK if k != "threshold"})
    base = oracle(buf, B, counter)
    states = storage(buf)[0]
    j = int(np.flatnonzero(base["future"] > base["step"])[0])
    e, tt, tp = int(base["ep"][j]), int(base["step"][j]), int(base["future"][j])
    d2 = ho.dist2(states[e, tt + 1, 6:9], states[e, tp + 1, 6:9])
    assert d2 > 0
    F = np.float32
    for target, want_r in ((d2, 0.0), (np.nextafter(d2, F(0)), -1.0), (np.nextafter(d2, F(np.inf)), 0.0)):
        eps = float(np.sqrt(np.float64(target)))
        assert F(eps * eps) == target          # the threshold's float32 square is the value aimed at
        set_mode(buf, reward="sparse", threshold=eps)
        got = sample(buf, B, counter)
        assert_same(got, oracle(buf, B, counter), ("threshold", eps))
        print(f"dist2 {d2!r} against thr2 {target!r}: r = {got['r'][j, 0]}")
        assert got["r"][j, 0] == want_r and np.array_equal(got["future"], base["future"])
    # a threshold of 0: exactly the rows whose goal is their own next state's (t' = t) are hits
    set_mode(buf, reward="sparse", threshold=0.0)
    got = sample(buf, B, counter)
    assert_same(got, oracle(buf, B, counter), "threshold 0")
    rel, own = got["future"] >= 0, got["future"] == got["step"]
    assert own.any() and (rel & ~own).any()
    assert np.all(got["r"][own, 0] == 0.0) and np.all(got["r"][rel & ~own, 0] == -1.0)
    # ... and they are hits under every threshold and in dense mode
    set_mode(buf, reward="dense")
    assert np.all(sample(buf, B, counter)["r"][own, 0] == 0.0)


def test_dense_reward_is_within_one_ulp_of_numpy(replay):
    buf = replay
    set_mode(buf, her_ratio=1.0, strategy="future", reward="dense", threshold=0.0)
    N = N_LIVE
    got = sample(buf, N, 2, np.arange(N))
    states = storage(buf)[0]
    rel = np.flatnonzero(got["future"] >= 0)
    want = np.array([-np.sqrt(ho.dist2(states[e, k + 1, 6:9], states[e, f + 1, 6:9]))
                     for e, k, f in zip(got["ep"][rel], got["step"][rel], got["future"][rel])], np.float32)
    r = got["r"][rel, 0]
    ulps = np.abs(r.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
    print(f"dense reward: {len(rel)} rows, {int((ulps > 0).sum())} differ from numpy's float32 sqrt, worst {int(ulps.max())} ulp")
    assert len(rel) == sum(max(n - 1, 0) for n in LENS) and np.all(ulps <= 1) and np.all(r <= 0)
    stored = got["future"] < 0
    assert np.array_equal(got["r"][stored, 0], storage(buf)[2].reshape(8, 12)[got["ep"][stored], got["step"][stored]])


# ---- equivalences and memory safety ---------------------------------------------------------------------------------------
def raw_sample(buf, B, counter, pad, fn, inds=None):
    """The C entry itself into outputs `pad` rows longer than B, prefilled with sentinels."""
    S, A = buf.state_dim, buf.action_dim
    f = [t.full((B + pad, w), SENT_F, dtype=t.float32, device="cuda") for w in (S, A, 1, 1, S)]
    ints = [t.full((B + pad,), SENT_I, dtype=t.int32, device="cuda") for _ in range(3 if fn.endswith("_her") else 2)]
    idx = None if inds is None else t.as_tensor(inds).to(device="cuda", dtype=t.int64).contiguous()
    h = buf.handle
    _capi.check(getattr(_capi.load(), fn)(h, B, _capi.ptr(idx), buf.seed, counter, *[_capi.ptr(x) for x in f],
                                          *[_capi.ptr(x) for x in ints], _capi.current_stream()), fn)
    t.cuda.synchronize()
    out = {k: x.cpu().numpy() for k, x in zip(KEYS, f)}
    out.update({k: x.cpu().numpy() for k, x in zip(("ep", "step", "future"), ints)})
    return out


@pytest.mark.parametrize("drawn", [False, True], ids=["injected", "drawn"])
def test_ratio_zero_equals_the_uniform_sampler_of_a_plain_handle(replay, plain_twin, drawn):
    buf = replay
    set_mode(buf, her_ratio=0.0, strategy="future", reward="sparse", threshold=0.1)
    plain_twin.seed = buf.seed
    inds = None if drawn else np.arange(61) % N_LIVE
    got = raw_sample(buf, 61, 4, 0, "oprl_replay_sample_her", inds)
    want = raw_sample(plain_twin, 61, 4, 0, "oprl_replay_sample", inds)
    assert_same(got, want, "ratio 0")
    assert np.all(got["future"] == -1)


def test_index_past_every_end_is_the_plain_gathers_row(replay, plain_twin):
    """Flat indices >= the live transitions: episode 0 and t = the index, as the uniform sampler reads them, relabelled
    under no ratio."""
    buf = replay
    set_mode(buf, her_ratio=1.0, strategy="final", reward="dense", threshold=0.1)
    plain_twin.seed = buf.seed
    inds = np.array([N_LIVE, N_LIVE + 1, 3, N_LIVE + 5])
    got = raw_sample(buf, 4, 1, 0, "oprl_replay_sample_her", inds)
    want = raw_sample(plain_twin, 4, 1, 0, "oprl_replay_sample", inds)
    assert list(got["ep"]) == [0, 0, 2, 0] and list(got["step"]) == [N_LIVE, N_LIVE + 1, 0, N_LIVE + 5]
    assert list(got["future"]) == [-1, -1, 10, -1]
    for k in KEYS:
        assert np.array_equal(got[k][[0, 1, 3]].view(np.uint32), want[k][[0, 1, 3]].view(np.uint32)), k


def test_oprl_replay_sample_forwards_to_the_hindsight_gather(replay, plain_twin):
    buf = replay
    set_mode(buf, her_ratio=0.8, strategy="future", reward="sparse", threshold=1.5)
    via_plain = raw_sample(buf, 61, 6, 0, "oprl_replay_sample")            # EpisodicReplayBuffer.sample's entry
    direct = raw_sample(buf, 61, 6, 0, "oprl_replay_sample_her")
    assert_same(via_plain, direct, "forward")
    plain_twin.seed = buf.seed
    stored = raw_sample(plain_twin, 61, 6, 0, "oprl_replay_sample")
    assert not np.array_equal(via_plain["s"], stored["s"]) and np.array_equal(via_plain["a"], stored["a"])


@pytest.mark.parametrize("B", [1, 17])
def test_nothing_is_written_past_the_batch_and_two_runs_agree(replay, B):
    buf = replay
    set_mode(buf, her_ratio=0.8, strategy="future", reward="dense", threshold=0.1)
    a = raw_sample(buf, B, 8, 40, "oprl_replay_sample_her")
    b = raw_sample(buf, B, 8, 40, "oprl_replay_sample_her")
    for k in a:
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k
        tail = a[k][B:]
        assert np.all(tail == (SENT_I if tail.dtype == np.int32 else SENT_F)), k
    assert_same({k: v[:B] for k, v in a.items()}, oracle(buf, B, 8), "head")


def test_lanes_replay_matches_the_oracle():
    """Three open episodes written a step at a time (next states included); lane 1's first episode ends after 3 steps."""
    S, A = 12, 3
    buf = make_buffer(6, 8, S, A, her_ratio=1.0, **TASK)
    buf.open_lanes(3)
    rs = np.random.RandomState(3)
    for k in range(5):
        over = np.array([False, k == 2, False])
        buf.add_step_rows(rs.standard_normal((3, S)), rs.standard_normal((3, A)), rs.standard_normal(3), over.astype(np.float32),
                          rs.standard_normal((3, S)), over)
    assert live_lens(buf) == [5, 3, 5, 2] and len(buf) == 15
    for strategy in ("future", "final"):
        set_mode(buf, strategy=strategy, threshold=2.0)
        got, want = sample(buf, 17, 1), oracle(buf, 17, 1)
        assert_same(got, want, ("lanes", strategy))
        assert np.any(want["future"] >= 0) and np.any(want["future"] < 0)


# ---- refusals and round trips -----------------------------------------------------------------------------------------------
LONG = dict(min_len=21)             # these refusals explain themselves: more than 20 bytes of message
LS, LA, LB = 12, 3, 32


def make_algo(name, prec):
    return support.make_algo(name, prec, LS, LA)


@pytest.fixture(scope="module")
def learner_replays():
    """A hindsight replay at goal-reach-3d's dims and a plain replay over the same storage contents and table."""
    from oprl_amd.buffers.episodic_buffer import EpisodicReplayBuffer
    E, L = 20, 12
    return support.twin_replays(make_buffer(E, L, LS, LA, **TASK), make_buffer(E, L, LS, LA, cls=EpisodicReplayBuffer), E, L)


def test_refusals(learner_replays):
    from oprl_amd.buffers.episodic_buffer import EpisodicReplayBuffer
    from oprl_amd.buffers.prioritized_buffer import PrioritizedEpisodicReplayBuffer
    from oprl_amd.group import LearnerGroup
    lib = _capi.load()
    kw = dict(buffer_size_transitions=40, state_dim=12, action_dim=2, max_episode_lenth=10, device="cuda")
    plain = EpisodicReplayBuffer(**kw).create()
    h = plain._handle
    nan, inf = float("nan"), float("inf")
    for args, word in (((6, 9, -1, 0.8, 0, 0, 0.1), b"goal dimension"), ((6, 9, 17, 0.8, 0, 0, 0.1), b"goal dimension"),
                       ((-1, 9, 3, 0.8, 0, 0, 0.1), b"inside"), ((6, 10, 3, 0.8, 0, 0, 0.1), b"inside"),
                       ((12, 0, 1, 0.8, 0, 0, 0.1), b"inside"), ((7, 9, 3, 0.8, 0, 0, 0.1), b"overlap"),
                       ((4, 4, 1, 0.8, 0, 0, 0.1), b"overlap"), ((6, 9, 3, -0.1, 0, 0, 0.1), b"share"),
                       ((6, 9, 3, 1.1, 0, 0, 0.1), b"share"), ((6, 9, 3, nan, 0, 0, 0.1), b"share"),
                       ((6, 9, 3, 0.8, 0, 0, -1e-3), b"threshold"), ((6, 9, 3, 0.8, 0, 0, nan), b"threshold"),
                       ((6, 9, 3, 0.8, 0, 0, inf), b"threshold"), ((6, 9, 3, 0.8, 2, 0, 0.1), b"strategy"),
                       ((6, 9, 3, 0.8, -1, 0, 0.1), b"strategy"), ((6, 9, 3, 0.8, 0, 2, 0.1), b"reward")):
        refused(lib.oprl_replay_set_her(h, *args), INVALID, word, **LONG)
    # ... changing nothing: the mode is still off
    plain.add_transition(np.zeros(12), np.zeros(2), 0.0, False)
    out = [t.zeros((4, w), device="cuda") for w in (12, 2, 1, 1, 12)]
    ptrs = [_capi.ptr(x) for x in out]
    refused(lib.oprl_replay_sample_her(plain.handle, 4, None, 0, 0, *ptrs, None, None, None, _capi.current_stream()), STATE,
            b"goal layout", **LONG)
    # hindsight excludes n-step returns and the sum tree, either way round
    assert lib.oprl_replay_set_nstep(h, 3, 0.99) == 0
    refused(lib.oprl_replay_set_her(h, 6, 9, 3, 0.8, 0, 0, 0.1), STATE, b"n-step", **LONG)
    assert lib.oprl_replay_set_nstep(h, 1, 0.99) == 0
    assert lib.oprl_replay_set_her(h, 6, 9, 3, 0.8, 0, 0, 0.1) == 0
    assert lib.oprl_replay_set_her(h, 0, 3, 3, 0.0, 1, 1, 0.0) == 0 and lib.oprl_replay_set_her(h, 11, 0, 1, 1.0, 0, 0, 1e30) == 0
    refused(lib.oprl_replay_set_nstep(h, 3, 0.99), STATE, b"hindsight", **LONG)
    assert lib.oprl_replay_set_nstep(h, 1, 0.99) == 0                      # (n = 1 is the mode off: nothing to refuse)
    refused(lib.oprl_replay_prio_enable(h, 0.6, 1e-6, None), STATE, b"hindsight", **LONG)
    assert lib.oprl_replay_sample_her(plain.handle, 4, None, 0, 0, *ptrs, None, None, None, _capi.current_stream()) == 0
    assert lib.oprl_replay_set_her(h, 0, 0, 0, 0.0, 0, 0, 0.0) == 0        # G = 0 switches the mode off ...
    assert lib.oprl_replay_set_nstep(h, 3, 0.99) == 0 and lib.oprl_replay_set_nstep(h, 1, 0.99) == 0
    assert lib.oprl_replay_prio_enable(h, 0.6, 1e-6, None) == 0            # ... and both are allowed again
    refused(lib.oprl_replay_set_her(h, 6, 9, 3, 0.8, 0, 0, 0.1), STATE, b"prioritized", **LONG)
    prio = PrioritizedEpisodicReplayBuffer(**kw).create()
    refused(lib.oprl_replay_set_her(prio._handle, 6, 9, 3, 0.8, 0, 0, 0.1), STATE, b"prioritized", **LONG)
    t.cuda.synchronize()
    # the packed learners gather stored rows inside their launches
    hbuf, _ = learner_replays
    members = [make_algo("ddpg", "f32") for _ in range(2)]
    g = LearnerGroup(members)
    seeds = (C.c_uint64 * 2)(1, 2)
    refused(lib.oprl_group_step_n(g.handle, hbuf.handle, 1, LB, seeds, _capi.current_stream()), STATE, b"hindsight", **LONG)
    assert members[0].update_step == 0 and members[1].update_step == 0


def test_checkpoint_round_trip(replay):
    buf = replay
    set_mode(buf, her_ratio=0.5, strategy="final", reward="dense", threshold=0.25)
    buf._sample_counter = 17
    sd = buf.state_dict()
    assert sd["her"]["strategy"] == "final" and sd["her"]["her_ratio"] == 0.5
    twin = make_buffer(8, 12, 12, 2, seed=99, goal_dim=2, achieved_offset=0, desired_offset=2, threshold=1.0)
    twin.load_state_dict(sd)
    assert (twin.goal_dim, twin.achieved_offset, twin.desired_offset, twin.her_ratio, twin.strategy, twin.reward,
            twin.threshold, twin.seed, twin._sample_counter) == (3, 6, 9, 0.5, "final", "dense", 0.25, buf.seed, 17)
    a, b = sample(buf, 61, 17), sample(twin, 61, 17)
    assert_same(a, b, "round trip")
    assert np.any(a["future"] >= 0)


# ---- learners ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,prec", [("ddpg", "f32"), ("td3", "x2"), ("sac", "f32")])
def test_step_n_over_a_hindsight_replay_equals_sample_then_update(learner_replays, name, prec):
    hbuf, pbuf = learner_replays
    set_mode(hbuf, her_ratio=0.8, strategy="future", reward="sparse", threshold=1.5)
    fused, loop = make_algo(name, prec), make_algo(name, prec)
    assert_same_state(fused, loop)
    print(name, prec, "launch form at B = 32:", fused.debug_form(LB))
    fused.learner.step_n(hbuf.handle, 3, LB, seed=11)
    loop_updates(loop, hbuf, 3, 11, LB)
    assert_same_state(fused, loop)
    assert fused.update_step == 3
    # the relabelled rows are not the stored rows (the comparison above is not vacuous)
    hbuf._sample_counter = pbuf._sample_counter = 0
    hbuf.seed = pbuf.seed = 11
    a, b = hbuf.sample(LB), pbuf.sample(LB)
    assert not t.equal(a[0], b[0]) and not t.equal(a[2], b[2]) and t.equal(a[1], b[1])
    # update_from_buffer over the buffer class: one more update, alone and with the next observation's action riding
    fused.update_from_buffer(hbuf, LB)
    loop_updates(loop, hbuf, 1, 11, LB)
    assert_same_state(fused, loop)
    obs = np.linspace(-1, 1, LS).astype(np.float32)
    fused.update_from_buffer(hbuf, LB, act_next=obs)
    act = fused.actor.explore(obs)
    loop_updates(loop, hbuf, 1, 11, LB)
    assert_same_state(fused, loop)
    assert fused.update_step == 5 and np.all(np.isfinite(act)) and np.shape(act)[-1] == LA
    # no flag is left behind: step_n over a plain replay, against the twin whose learner never saw the hindsight handle
    fused.learner.step_n(pbuf.handle, 3, LB, seed=12)
    loop.learner.step_n(pbuf.handle, 3, LB, seed=12)
    assert_same_state(fused, loop)
    assert fused.update_step == 8


# ---- the trainer loop ---------------------------------------------------------------------------------------------------
def test_trainer_on_the_goal_environment_relabels_what_the_oracle_relabels():
    """BaseTrainer, DDPG, synthetic:goal-reach-2d, 120 environment steps.  Before every update the test draws the
    update's own batch — the buffer's seed, the learner's update count — with return_relabel, and holds every row's t'
    to the oracle's choice from the same words and the episode table of that moment."""
    from oprl_amd.algos.ddpg import DDPG
    from oprl_amd.buffers.hindsight_buffer import HindsightEpisodicReplayBuffer
    from oprl_amd.environment.make_env import make_env
    from oprl_amd.logging import NullLogger
    from oprl_amd.trainers.base_trainer import BaseTrainer
    B, ratio = 32, 0.8
    env = make_env("synthetic:goal-reach-2d", seed=0)
    lay = env.goal_layout
    assert (env.S, env.A, lay["goal_dim"]) == (8, 2, 2)
    t.manual_seed(0)
    algo = DDPG(logger=NullLogger("/tmp/oprl_amd_test"), state_dim=8, action_dim=2, device="cuda", max_batch=B).create()
    before = algo.actor._oprl_arena.clone()
    buf = HindsightEpisodicReplayBuffer(buffer_size_transitions=2000, state_dim=8, action_dim=2,
                                        max_episode_lenth=env.episode_length, device="cuda", seed=5, her_ratio=ratio,
                                        **lay).create()
    log = []
    update_from_buffer = algo.update_from_buffer

    def recording(replay_buffer, batch_size, **kw):
        counter = replay_buffer._sample_counter
        replay_buffer._sample_counter = algo.update_step
        _rows, (ep, st), fut = replay_buffer.sample(batch_size, return_indices=True, return_relabel=True)
        replay_buffer._sample_counter = counter
        log.append((algo.update_step, list(live_lens(replay_buffer)), ep.cpu().numpy(), st.cpu().numpy(), fut.cpu().numpy()))
        return update_from_buffer(replay_buffer, batch_size, **kw)
    algo.update_from_buffer = recording
    np.random.seed(0)
    BaseTrainer(logger=NullLogger("/tmp/oprl_amd_test"), env=env, make_env_test=lambda s: make_env("synthetic:goal-reach-2d", seed=s),
                replay_buffer=buf, algo=algo, num_steps=120, start_steps=60, batch_size=B, eval_interval=10 ** 9,
                save_policy_every=0, stdout_log_every=10 ** 9).train()
    t.cuda.synchronize()
    algo.learner.check()
    assert algo.update_step == 121 - (B - 1) == len(log) and len(buf) == 121 and live_lens(buf) == [50, 50, 21]
    assert t.isfinite(algo.actor._oprl_arena).all() and not t.equal(before, algo.actor._oprl_arena)
    assert t.isfinite(algo.state_dict()["critic"]).all()
    rows = relabelled = want_relabelled = eligible = 0
    for counter, lens, ep, st, fut in log:
        want = np.array([ho.choose(buf.seed, counter, i, int(st[i]), lens[int(ep[i])], ratio, ho.FUTURE) for i in range(B)])
        assert np.array_equal(fut, want), counter
        rows += B
        relabelled += int((fut >= 0).sum())
        want_relabelled += int((want >= 0).sum())
        eligible += int((np.asarray(lens)[ep] - 1 - st >= 1).sum())
    print(f"{len(log)} training batches: {relabelled} of {rows} rows relabelled ({eligible} eligible, share "
          f"{relabelled / eligible:.4f} at ratio {ratio})")
    # (the batches' draws are independent: the share of the eligible rows is binomial around the ratio)
    assert relabelled == want_relabelled and abs(relabelled / eligible - ratio) < 5 * (ratio * (1 - ratio) / eligible) ** 0.5
    # the stored rewards are the environment's sparse ones
    assert set(np.unique(buf.rewards.cpu().numpy()[:3, :, 0]).tolist()) <= {0.0, -1.0}
