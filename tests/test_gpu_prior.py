"""GPU tests of prior data in the batch (csrc/replay_mix.hip): the mixed gather bit for bit against
tests/prior_oracle.py and against the plain sampler on twin handles, the coarse episode table on either side, memory
safety, the forward from oprl_replay_sample, unflushed prior rows, what is refused, the checkpoint round trip, the
learners' step_n over a mixed replay against sample() + update() pairs, and the two uses end to end: IQL fine-tuned
online after OfflineTrainer, and SAC from scratch through the --prior-data path."""
from __future__ import annotations

import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch as t

from oprl_amd import _capi
from tests import prior_oracle as po
from tests import support
from tests.config_scripts import load_config
from tests.support import INVALID, STATE, fill_random, live_lens, loop_updates, refused, set_table, storage

pytestmark = pytest.mark.gpu
KEYS = ("s", "a", "r", "d", "s2")
INTS = ("ep", "step", "src")
SENT_F, SENT_I = 12345.0, -777
LONG = dict(min_len=21)             # these refusals explain themselves: more than 20 bytes of message


@pytest.fixture(scope="module", autouse=True)
def generators_as_found():
    """The global generators (python, numpy, torch on the host and on the GPU) leave this module as they entered it:
    the tests here seed them (learners built from t.manual_seed(0), the runners' set_seed), and modules that run later
    build networks from whatever state they find."""
    import random
    state = random.getstate(), np.random.get_state(), t.get_rng_state(), t.cuda.get_rng_state_all()
    yield
    random.setstate(state[0])
    np.random.set_state(state[1])
    t.set_rng_state(state[2])
    t.cuda.set_rng_state_all(state[3])


def make_buffer(E, L, S, A, seed=7, prior=None, share=0.5, fill=True):
    """A plain replay, or with `prior` a PriorDataReplayBuffer over it; every row random normal (the never-written ones
    too), the same values for the same (E, L, S, A)."""
    from oprl_amd.buffers.episodic_buffer import EpisodicReplayBuffer
    from oprl_amd.buffers.prior_buffer import PriorDataReplayBuffer
    kw = dict(buffer_size_transitions=E * L, state_dim=S, action_dim=A, max_episode_lenth=L, device="cuda", seed=seed)
    buf = (PriorDataReplayBuffer(prior=prior, prior_share=share, **kw) if prior is not None else EpisodicReplayBuffer(**kw)).create()
    return fill_random(buf, ("actions", "rewards", "dones", "states"), gen_seed=1000 + E + L) if fill else buf


def oracle(buf, B, counter, inds=None):
    p = buf.prior
    return po.mix_gather(storage(p), live_lens(p), storage(buf), live_lens(buf), buf.prior_share, buf.seed, counter, B, inds=inds)


def as_numpy(rows, pair=None, src=None):
    out = {k: x.cpu().numpy() for k, x in zip(KEYS, rows)}
    if pair is not None:
        out.update(ep=pair[0].cpu().numpy(), step=pair[1].cpu().numpy())
    if src is not None:
        out["src"] = src.cpu().numpy()
    return out


def sample(buf, B, counter, inds=None):
    """buf.sample at a given counter, every output as numpy: dict(s, a, r, d, s2, ep, step[, src])."""
    buf._sample_counter = counter
    if hasattr(buf, "prior"):
        return as_numpy(*buf.sample(B, inds=inds, return_indices=True, return_source=True))
    return as_numpy(*buf.sample(B, inds=inds, return_indices=True))


def assert_same(got, want, what="", rows=slice(None)):
    for k in INTS:
        if k in got and k in want:
            assert np.array_equal(got[k][rows], want[k][rows]), (what, k, got[k][rows], want[k][rows])
    for k in KEYS:
        a, b = np.ascontiguousarray(got[k][rows]).view(np.uint32), np.ascontiguousarray(want[k][rows]).view(np.uint32)
        assert a.shape == b.shape and np.array_equal(a, b), (what, k, np.argwhere(a != b)[:4].tolist())


# Prior: E = 8, L = 12, seven episodes, lengths 1, 2 and 12 among them, slot 3 evicted.  Online: E = 6, L = 5 — another
# steps-per-episode, so a row gathered with the other source's strides is a different row.
P_LENS, O_LENS = [1, 2, 12, 0, 5, 7, 12], [5, 1, 3, 0, 2]
N_P, N_O = sum(P_LENS), sum(O_LENS)
_cache: dict = {}


def trio(S, A):
    """(prior, online over it, plain twin of online) at these dims, built once."""
    if (S, A) not in _cache:
        prior = make_buffer(8, 12, S, A)
        set_table(prior, P_LENS)
        online, twin = make_buffer(6, 5, S, A, prior=prior), make_buffer(6, 5, S, A)
        for b in (online, twin):
            set_table(b, O_LENS)
        assert all(t.equal(online._tensors[k], twin._tensors[k]) for k in twin._tensors)
        _cache[(S, A)] = prior, online, twin
    return _cache[(S, A)]


def set_mode(buf, prior, share):
    """The buffer's two fields, validated and applied to the handle (what create() and load_state_dict() do)."""
    buf.prior, buf.prior_share = prior, share
    buf._validate()
    buf._set_prior()


def set_share(buf, share):
    set_mode(buf, buf.prior, share)


def injected(B, Bp):
    """A flat index into its own source for every row."""
    i = np.arange(B)
    return np.where(i < Bp, (3 + 5 * i) % N_P, (1 + 3 * i) % N_O)


@pytest.mark.parametrize("share", [0, 0.25, 0.5, 1])
@pytest.mark.parametrize("B", [1, 16, 17, 61, 256])
@pytest.mark.parametrize("drawn", [False, True], ids=["injected", "drawn"])
@pytest.mark.parametrize("S,A", [(12, 2), (40, 7)])
def test_bitexact_against_the_oracle_and_the_plain_sampler(S, A, drawn, B, share):
    prior, buf, twin = trio(S, A)
    set_share(buf, share)
    Bp = buf.n_prior(B)
    assert Bp == po.n_prior(B, share) and (share not in (0, 1) or Bp == share * B)
    inds = None if drawn else injected(B, Bp)
    counter = 5 + B
    got, want = sample(buf, B, counter, inds), oracle(buf, B, counter, inds)
    assert_same(got, want, (S, A, drawn, B, share))
    assert np.array_equal(got["src"], (np.arange(B) < Bp).astype(np.int32))
    # rows [0, Bp) are the plain sample of the prior, rows [Bp, B) the plain sample of the online replay's twin, at the
    # same (B, seed, counter); each twin gets only the indices that are its own
    prior.seed = twin.seed = buf.seed
    if Bp > 0:
        assert_same(got, sample(prior, B, counter, None if drawn else np.where(np.arange(B) < Bp, inds, 0)), "prior rows", slice(0, Bp))
    if Bp < B:
        assert_same(got, sample(twin, B, counter, None if drawn else np.where(np.arange(B) >= Bp, inds, 0)), "own rows", slice(Bp, B))
    if B == 256 and share == 0.5 and drawn:       # both sources' episodes all occur, the 1-step ones too
        assert set(got["ep"][:Bp]) == {0, 1, 2, 4, 5, 6} and set(got["ep"][Bp:]) == {0, 1, 2, 4}
        assert got["step"][:Bp].max() == 11 and got["step"][Bp:].max() == 4


SMALL_LENS = [5, 2, 4]


@pytest.mark.parametrize("coarse_is_prior", [True, False], ids=["coarse-prior", "coarse-online"])
def test_coarse_episode_table_on_either_side(coarse_is_prior):
    """2100 episodes of lengths 1 and 2: more than the 2048 table entries the kernel holds in LDS per source, so that
    source's table is staged coarsely and finished by global probes, while the other source (3 episodes) is staged whole —
    in the one workgroup that straddles B_p, both at once."""
    S, A, B = 3, 1, 61
    big_lens = 1 + (np.random.RandomState(2).rand(2100) < 0.5)
    shapes = ((2100, 2, big_lens), (4, 5, SMALL_LENS))
    (Ep, Lp, lens_p), (Eo, Lo, lens_o) = shapes if coarse_is_prior else shapes[::-1]
    prior = make_buffer(Ep, Lp, S, A)
    set_table(prior, lens_p)
    buf, twin = make_buffer(Eo, Lo, S, A, prior=prior), make_buffer(Eo, Lo, S, A)
    for b in (buf, twin):
        set_table(b, lens_o)
    Bp = buf.n_prior(B)
    assert Bp == 31 and Bp % 16 != 0
    got, want = sample(buf, B, 3), oracle(buf, B, 3)
    assert_same(got, want, "coarse")
    prior.seed = twin.seed = buf.seed
    assert_same(got, sample(prior, B, 3), "prior rows", slice(0, Bp))
    assert_same(got, sample(twin, B, 3), "own rows", slice(Bp, B))
    big = got["ep"][:Bp] if coarse_is_prior else got["ep"][Bp:]
    assert len(np.unique(big)) > 25 and big.max() > 1500 and (got["ep"][Bp:] if coarse_is_prior else got["ep"][:Bp]).max() <= 2
    n_big = int(np.sum(big_lens))
    inds = np.where((np.arange(B) < Bp) == coarse_is_prior, (np.arange(B) * 53 + n_big - 40) % n_big, np.arange(B) % sum(SMALL_LENS))
    assert_same(sample(buf, B, 4, inds), oracle(buf, B, 4, inds), "coarse, injected")


# ---- memory safety and equivalences ---------------------------------------------------------------------------------------
def raw_sample(buf, B, counter, pad, fn, inds=None, status=0):
    """The C entry itself into outputs `pad` rows longer than B, prefilled with sentinels."""
    S, A = buf.state_dim, buf.action_dim
    f = [t.full((B + pad, w), SENT_F, dtype=t.float32, device="cuda") for w in (S, A, 1, 1, S)]
    ints = [t.full((B + pad,), SENT_I, dtype=t.int32, device="cuda") for _ in range(3 if fn.endswith("_mix") else 2)]
    idx = None if inds is None else t.as_tensor(inds).to(device="cuda", dtype=t.int64).contiguous()
    rc = getattr(_capi.load(), fn)(buf.handle, B, _capi.ptr(idx), buf.seed, counter, *[_capi.ptr(x) for x in f],
                                   *[_capi.ptr(x) for x in ints], _capi.current_stream())
    assert rc == status, (rc, _capi.load().oprl_last_error())
    t.cuda.synchronize()
    out = {k: x.cpu().numpy() for k, x in zip(KEYS, f)}
    out.update({k: x.cpu().numpy() for k, x in zip(INTS, ints)})
    return out


@pytest.mark.parametrize("B", [1, 17])
def test_nothing_is_written_past_the_batch_and_two_runs_agree(B):
    _prior, buf, _twin = trio(12, 2)
    set_share(buf, 0.5)
    a = raw_sample(buf, B, 8, 40, "oprl_replay_sample_mix")
    b = raw_sample(buf, B, 8, 40, "oprl_replay_sample_mix")
    for k in a:
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k
        tail = a[k][B:]
        assert np.all(tail == (SENT_I if tail.dtype == np.int32 else SENT_F)), k
    assert_same({k: v[:B] for k, v in a.items()}, oracle(buf, B, 8), "head")
    # the optional outputs are optional
    rows = [t.zeros((B, w), device="cuda") for w in (12, 2, 1, 1, 12)]
    _capi.check(_capi.load().oprl_replay_sample_mix(buf.handle, B, None, buf.seed, 8, *[_capi.ptr(x) for x in rows], None, None,
                                                    None, _capi.current_stream()), "oprl_replay_sample_mix")
    assert_same(as_numpy(rows), a, "no optional outputs", slice(0, B))


def test_oprl_replay_sample_forwards_to_the_mixed_gather():
    prior, buf, twin = trio(12, 2)
    set_share(buf, 0.5)
    via_plain = raw_sample(buf, 61, 6, 0, "oprl_replay_sample")            # EpisodicReplayBuffer.sample's entry
    direct = raw_sample(buf, 61, 6, 0, "oprl_replay_sample_mix")
    assert_same(via_plain, direct, "forward")
    twin.seed = buf.seed
    stored = raw_sample(twin, 61, 6, 0, "oprl_replay_sample")
    assert not np.array_equal(via_plain["s"][:31], stored["s"][:31]) and np.array_equal(via_plain["s"][31:], stored["s"][31:])


def test_rows_staged_in_the_prior_are_seen_by_the_next_mixed_sample():
    """add_transitions leaves its rows in the prior's host staging (fill_replay does): the mixed sample flushes both
    handles before its launch."""
    S, A, n = 12, 2, 9
    prior = make_buffer(4, 12, S, A, fill=False)
    buf = make_buffer(6, 5, S, A, prior=prior, share=1.0, fill=False)
    rows = np.random.RandomState(5).standard_normal((n, S + A + 2)).astype(np.float32)
    prior.add_transitions(rows)
    assert prior._lib is not None and len(prior) == n and len(buf) == 0
    got = sample(buf, n - 1, 0, np.arange(n - 1))
    assert np.array_equal(got["s"], rows[:-1, :S]) and np.array_equal(got["a"], rows[:-1, S:S + A])
    assert np.array_equal(got["r"][:, 0], rows[:-1, S + A]) and np.array_equal(got["d"][:, 0], rows[:-1, S + A + 1])
    assert np.array_equal(got["s2"], rows[1:, :S]) and np.all(got["src"] == 1) and np.all(got["ep"] == 0)
    # ... and rows staged in the online replay likewise
    more = np.random.RandomState(6).standard_normal((4, S + A + 2)).astype(np.float32)
    buf.add_transitions(more)
    set_share(buf, 0.5)
    got = sample(buf, 6, 1, np.array([0, 1, 2, 0, 1, 2]))
    assert list(got["src"]) == [1, 1, 1, 0, 0, 0]
    assert np.array_equal(got["s"], np.concatenate([rows[:3, :S], more[:3, :S]])) and np.array_equal(got["s2"][3:], more[1:4, :S])


# ---- refusals and round trips -----------------------------------------------------------------------------------------------
LS, LA, LB = 12, 3, 32


def make_algo(name, prec):
    return support.make_algo(name, prec, LS, LA, **(dict(max_batch=256) if name in ("tqc", "iql") else {}))


@pytest.fixture(scope="module")
def learner_replays():          # not twin_replays: two shapes, and one stream of draws runs through both tables
    """A prior of 20 x 12 steps and an online replay of 10 x 7 over it, at the learners' dims."""
    rs = np.random.RandomState(4)
    prior = make_buffer(20, 12, LS, LA)
    buf = make_buffer(10, 7, LS, LA, prior=prior)
    for b, (E, L) in ((prior, (20, 12)), (buf, (10, 7))):
        b._tensors["dones"].copy_(t.as_tensor((rs.rand(E, L, 1) < 0.1).astype(np.float32)))
        set_table(b, rs.randint(1, L + 1, size=E - 1))
    return prior, buf


def test_set_prior_refusals():
    from oprl_amd.buffers.prioritized_buffer import PrioritizedEpisodicReplayBuffer
    lib = _capi.load()
    prior, buf, twin = trio(12, 2)
    set_share(buf, 0.5)
    before = raw_sample(buf, 61, 2, 0, "oprl_replay_sample_mix")
    h, p = buf._handle, prior._handle
    nan, inf = float("nan"), float("inf")
    for share in (-0.1, 1.1, nan, inf, -inf):
        refused(lib.oprl_replay_set_prior(h, p, share), INVALID, b"share", **LONG)
    refused(lib.oprl_replay_set_prior(h, h, 0.5), INVALID, b"itself", **LONG)
    for S, A in ((13, 2), (12, 3)):
        other = make_buffer(4, 5, S, A, fill=False)
        refused(lib.oprl_replay_set_prior(h, other._handle, 0.5), INVALID, b"dims", **LONG)
        refused(lib.oprl_replay_set_prior(other._handle, p, 0.5), INVALID, b"dims", **LONG)
    # n-step, hindsight and prioritized handles, on either side
    x, y = make_buffer(4, 5, 12, 2, fill=False), make_buffer(4, 5, 12, 2, fill=False)
    for word, on, off in ((b"n-step", lambda r: lib.oprl_replay_set_nstep(r, 3, 0.99), lambda r: lib.oprl_replay_set_nstep(r, 1, 0.99)),
                          (b"hindsight", lambda r: lib.oprl_replay_set_her(r, 6, 9, 3, 0.8, 0, 0, 0.1),
                           lambda r: lib.oprl_replay_set_her(r, 0, 0, 0, 0.0, 0, 0, 0.0))):
        assert on(x._handle) == 0
        refused(lib.oprl_replay_set_prior(x._handle, y._handle, 0.5), STATE, word, **LONG)
        msg = refused(lib.oprl_replay_set_prior(y._handle, x._handle, 0.5), STATE, **LONG)
        assert word in msg and b"prior replay" in msg
        assert off(x._handle) == 0
    prio = PrioritizedEpisodicReplayBuffer(buffer_size_transitions=20, state_dim=12, action_dim=2, max_episode_lenth=5, device="cuda").create()
    refused(lib.oprl_replay_set_prior(prio._handle, y._handle, 0.5), STATE, b"prioritized", **LONG)
    msg = refused(lib.oprl_replay_set_prior(y._handle, prio._handle, 0.5), STATE, **LONG)
    assert b"prioritized" in msg and b"prior replay" in msg
    # one prior per batch
    refused(lib.oprl_replay_set_prior(y._handle, h, 0.5), STATE, b"prior of its own", **LONG)
    # ... and each of them changed nothing: x and y are still plain and without a prior, buf samples what it sampled
    rows = [t.zeros((4, w), device="cuda") for w in (12, 2, 1, 1, 12)]
    ptrs = [_capi.ptr(r) for r in rows]
    for r in (x, y):
        refused(lib.oprl_replay_sample_mix(r._handle, 4, None, 0, 0, *ptrs, None, None, None, _capi.current_stream()), STATE,
                b"no prior", **LONG)
    assert_same(raw_sample(buf, 61, 2, 0, "oprl_replay_sample_mix"), before, "after the refusals")
    # a handle with a prior takes no n-step returns, no hindsight goals and no sum tree
    assert lib.oprl_replay_set_prior(x._handle, y._handle, 0.0) == 0          # (share 0 is allowed: the mode is on)
    refused(lib.oprl_replay_set_nstep(x._handle, 3, 0.99), STATE, b"prior data", **LONG)
    assert lib.oprl_replay_set_nstep(x._handle, 1, 0.99) == 0                 # (n = 1 is the mode off: nothing to refuse)
    refused(lib.oprl_replay_set_her(x._handle, 6, 9, 3, 0.8, 0, 0, 0.1), STATE, b"prior data", **LONG)
    refused(lib.oprl_replay_prio_enable(x._handle, 0.6, 1e-6, None), STATE, b"prior data", **LONG)
    assert lib.oprl_replay_set_prior(x._handle, None, nan) == 0               # the mode off: the share is not read
    assert lib.oprl_replay_set_nstep(x._handle, 3, 0.99) == 0 and lib.oprl_replay_set_nstep(x._handle, 1, 0.99) == 0
    t.cuda.synchronize()


def test_sample_mix_refusals_and_the_way_back_to_the_plain_path():
    lib = _capi.load()
    prior, buf, twin = trio(12, 2)
    set_share(buf, 0.5)
    before = raw_sample(buf, 61, 2, 0, "oprl_replay_sample_mix")
    # the prior took on a mode after set_prior: found per call, and gone with the mode
    assert lib.oprl_replay_set_nstep(prior._handle, 3, 0.99) == 0
    for fn in ("oprl_replay_sample_mix", "oprl_replay_sample"):
        out = raw_sample(buf, 61, 2, 0, fn, status=STATE)
        assert b"n-step" in lib.oprl_last_error() and np.all(out["s"] == SENT_F) and np.all(out["ep"] == SENT_I)
    assert lib.oprl_replay_set_nstep(prior._handle, 1, 0.99) == 0
    assert lib.oprl_replay_set_her(prior._handle, 6, 9, 3, 0.8, 0, 0, 0.1) == 0
    raw_sample(buf, 61, 2, 0, "oprl_replay_sample_mix", status=STATE)
    assert b"hindsight" in lib.oprl_last_error()
    assert lib.oprl_replay_set_her(prior._handle, 0, 0, 0, 0.0, 0, 0, 0.0) == 0
    assert_same(raw_sample(buf, 61, 2, 0, "oprl_replay_sample_mix"), before, "the prior is plain again")
    # invalid arguments
    rows = [t.zeros((4, w), device="cuda") for w in (12, 2, 1, 1, 12)]
    ptrs = [_capi.ptr(r) for r in rows]
    assert lib.oprl_replay_sample_mix(buf.handle, 0, None, 0, 0, *ptrs, None, None, None, _capi.current_stream()) == INVALID
    assert lib.oprl_replay_sample_mix(buf.handle, 4, None, 0, 0, None, *ptrs[1:], None, None, None, _capi.current_stream()) == INVALID
    # a source that has to supply a row and holds none
    e_prior, e_own = make_buffer(4, 5, 12, 2, fill=False), make_buffer(4, 5, 12, 2, fill=False)
    assert lib.oprl_replay_set_prior(e_own._handle, prior._handle, 0.5) == 0
    out = raw_sample(e_own, 8, 0, 0, "oprl_replay_sample_mix", status=STATE)
    assert b"this replay is empty" in lib.oprl_last_error() and np.all(out["s"] == SENT_F)
    assert lib.oprl_replay_set_prior(e_own._handle, prior._handle, 1.0) == 0          # ... but no row is asked of it now
    prior.seed = e_own.seed
    assert_same(raw_sample(e_own, 8, 0, 0, "oprl_replay_sample_mix"), raw_sample(prior, 8, 0, 0, "oprl_replay_sample"), "share 1")
    assert lib.oprl_replay_set_prior(twin._handle, e_prior._handle, 0.5) == 0
    out = raw_sample(twin, 8, 0, 0, "oprl_replay_sample_mix", status=STATE)
    assert b"prior replay is empty" in lib.oprl_last_error() and np.all(out["s"] == SENT_F)
    assert lib.oprl_replay_set_prior(twin._handle, e_prior._handle, 0.0) == 0
    plain = raw_sample(twin, 8, 0, 0, "oprl_replay_sample_mix")               # ... nor of the empty prior now
    assert np.all(plain["src"] == 0)
    # set_prior(NULL): the plain path, bit for bit
    assert lib.oprl_replay_set_prior(twin._handle, None, 0.5) == 0
    raw_sample(twin, 8, 0, 0, "oprl_replay_sample_mix", status=STATE)
    assert b"no prior" in lib.oprl_last_error()
    back = raw_sample(twin, 8, 0, 0, "oprl_replay_sample")
    assert_same(back, plain, "share 0 is the plain sample")
    set_mode(buf, None, 0.5)
    twin.seed = buf.seed
    assert_same(raw_sample(buf, 61, 2, 0, "oprl_replay_sample"), raw_sample(twin, 61, 2, 0, "oprl_replay_sample"), "mode off")
    assert np.all(sample(buf, 16, 0)["src"] == 0)
    set_mode(buf, prior, 0.5)
    assert_same(raw_sample(buf, 61, 2, 0, "oprl_replay_sample"), before, "mode on again")


def test_group_step_n_refuses_a_mixed_replay(learner_replays):
    from oprl_amd.group import LearnerGroup
    _prior, buf = learner_replays
    members = [make_algo("ddpg", "f32") for _ in range(2)]
    g = LearnerGroup(members)
    seeds = (C.c_uint64 * 2)(1, 2)
    lib = _capi.load()
    refused(lib.oprl_group_step_n(g.handle, buf.handle, 1, LB, seeds, _capi.current_stream()), STATE, b"prior data", **LONG)
    assert members[0].update_step == 0 and members[1].update_step == 0


def test_checkpoint_round_trip():
    prior, buf, _twin = trio(12, 2)
    set_share(buf, 0.25)
    buf._sample_counter = 17
    sd = buf.state_dict()
    assert sd["prior_share"] == 0.25 and "prior" not in sd
    copy = make_buffer(6, 5, 12, 2, seed=99, prior=prior, share=0.9, fill=False)
    copy.load_state_dict(sd)
    assert (copy.prior_share, copy.seed, copy._sample_counter, copy.prior) == (0.25, buf.seed, 17, prior)
    a, b = sample(buf, 61, 17), sample(copy, 61, 17)
    assert_same(a, b, "round trip")
    assert a["src"].sum() == 15


# ---- learners ---------------------------------------------------------------------------------------------------------------
V_KEYS = ("value", "value_m", "value_v", "value_step")


def assert_same_state(a, b):        # kept: IQL's V, its moments and its step count ride along when either learner has them
    x, y = a.state_dict(), b.state_dict()
    support.assert_same_state(a, b, extra=tuple(k for k in V_KEYS if k in x or k in y))


@pytest.mark.parametrize("name,prec", [("ddpg", "f32"), ("td3", "x2"), ("sac", "f32"), ("tqc", "f32"), ("iql", "f32")])
def test_step_n_over_a_mixed_replay_equals_sample_then_update(learner_replays, name, prec):
    prior, buf = learner_replays
    set_share(buf, 0.5)
    fused, loop = make_algo(name, prec), make_algo(name, prec)
    assert_same_state(fused, loop)
    print(name, prec, "launch form at B = 32:", fused.debug_form(LB))
    fused.learner.step_n(buf.handle, 3, LB, seed=11)
    loop_updates(loop, buf, 3, 11, LB)
    assert_same_state(fused, loop)
    assert fused.update_step == 3
    # the batch is mixed (the comparison above is not vacuous): half of it is the prior's plain sample
    buf._sample_counter = prior._sample_counter = 0
    buf.seed = prior.seed = 11
    rows, src = buf.sample(LB, return_source=True)
    assert src.sum().item() == 16 and t.equal(rows[0][:16], prior.sample(LB)[0][:16])
    # update_from_buffer over the buffer class: one more update, alone and with the next observation's action riding
    fused.update_from_buffer(buf, LB)
    loop_updates(loop, buf, 1, 11, LB)
    assert_same_state(fused, loop)
    obs = np.linspace(-1, 1, LS).astype(np.float32)
    fused.update_from_buffer(buf, LB, act_next=obs)
    act = fused.actor.explore(obs)
    loop_updates(loop, buf, 1, 11, LB)
    assert_same_state(fused, loop)
    assert fused.update_step == 5 and np.all(np.isfinite(act)) and np.shape(act)[-1] == LA
    # no flag is left behind: step_n over a plain replay, against the learner that never saw the mixed handle
    fused.learner.step_n(prior.handle, 3, LB, seed=12)
    loop.learner.step_n(prior.handle, 3, LB, seed=12)
    assert_same_state(fused, loop)
    assert fused.update_step == 8
    assert not t.equal(fused.state_dict()["actor"], make_algo(name, prec).state_dict()["actor"])


# ---- end to end -------------------------------------------------------------------------------------------------------------
ENV, EPISODES, STEPS, B = "cheetah-run", 6, 50, 32


def make_env(seed):
    from oprl_amd.environment.synthetic import SyntheticEnv
    return SyntheticEnv(ENV, seed=seed, episode_length=STEPS)


@pytest.fixture(scope="module")
def data():
    """6 episodes x 50 steps under uniform actions, as tests/test_gpu_offline.py builds them: every episode ends in a
    timeout, and next_observations is kept so that no row is dropped."""
    from oprl_amd.buffers.offline_dataset import OfflineData
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


def record_batches(algo, log):
    """Before every update draw the update's own batch — the buffer's seed, the learner's update count — with
    return_source, and keep it."""
    update_from_buffer = algo.update_from_buffer

    def recording(replay_buffer, batch_size, **kw):
        counter = replay_buffer._sample_counter
        replay_buffer._sample_counter = algo.update_step
        rows, src = replay_buffer.sample(batch_size, return_source=True)
        replay_buffer._sample_counter = counter
        log.append((replay_buffer, len(replay_buffer), rows[0].cpu().numpy(), rows[1].cpu().numpy(), src.cpu().numpy()))
        return update_from_buffer(replay_buffer, batch_size, **kw)
    algo.update_from_buffer = recording


def check_batches(log, buf, dataset_obs, dataset_act, n_updates):
    """Every training batch: n_prior(B) prior rows in front, each prior row's (s, a) a row of the dataset as stored."""
    known = {row.tobytes() for row in np.concatenate([dataset_obs, dataset_act], axis=1).astype(np.float32)}
    assert len(log) == n_updates and buf.n_prior(B) == 16
    fresh = set()
    for replay_buffer, n_online, s, a, src in log:
        assert replay_buffer is buf and n_online >= B
        assert list(src) == [1] * 16 + [0] * 16
        sa = np.concatenate([s, a], axis=1)
        assert all(row.tobytes() in known for row in sa[:16])
        fresh.update(row.tobytes() for row in sa[16:])
    assert len(fresh) > 60 and not (fresh & known)      # the own rows are the run's fresh experience
    online_s = buf.states.cpu().numpy()
    stored = {online_s[e, k].tobytes() for e in range(buf.episodes_counter) for k in range(buf.ep_lens[e])}
    assert all(row[:dataset_obs.shape[1] * 4] in stored for row in fresh)


def test_iql_pretrained_offline_is_finetuned_online_on_mixed_batches(data):
    from oprl_amd.algos.iql import IQL
    from oprl_amd.buffers.episodic_buffer import EpisodicReplayBuffer
    from oprl_amd.buffers.offline_dataset import fill_replay
    from oprl_amd.buffers.prior_buffer import PriorDataReplayBuffer
    from oprl_amd.environment.normalized import NormalizedObsEnv
    from oprl_amd.logging import NullLogger
    from oprl_amd.trainers.finetune import finetune
    from oprl_amd.trainers.offline_trainer import OfflineTrainer
    S, A = data.observations.shape[1], data.actions.shape[1]
    prior = EpisodicReplayBuffer(buffer_size_transitions=(EPISODES + 1) * STEPS, state_dim=S, action_dim=A,
                                 max_episode_lenth=STEPS, device="cuda", seed=11).create()
    norm = fill_replay(prior, data)
    t.manual_seed(0)
    algo = IQL(logger=NullLogger(), state_dim=S, action_dim=A, max_batch=256, log_every=10 ** 9).create()
    OfflineTrainer(logger=NullLogger(), make_env_test=make_env, replay_buffer=prior, algo=algo, obs_norm=norm, num_updates=32,
                   updates_per_call=16, batch_size=B, eval_interval=0, save_policy_every=0, stdout_log_every=0, seed=5).train()
    assert algo.update_step == 32 and algo.learner.value_step == 32
    before = algo.state_dict()
    log = []
    record_batches(algo, log)
    np.random.seed(0)
    tr = finetune(algo=algo, prior_buffer=prior, obs_norm=norm, make_env=make_env, logger=NullLogger("/tmp/oprl_amd_test"),
                  num_steps=120, batch_size=B, prior_share=0.5, seed=5, eval_interval=10 ** 9, save_policy_every=0,
                  stdout_log_every=10 ** 9, num_eval_episodes=2)
    t.cuda.synchronize()
    algo.learner.check()
    buf = tr.replay_buffer
    assert type(buf) is PriorDataReplayBuffer and buf.prior is prior and buf.seed == prior.seed == 11
    assert isinstance(tr.env, NormalizedObsEnv) and isinstance(tr.make_env_test(0), NormalizedObsEnv) and tr.start_steps == 0
    assert len(buf) == 121 and live_lens(buf) == [50, 50, 21] and len(prior) == EPISODES * STEPS
    n_updates = 121 - (B - 1)
    assert algo.update_step == 32 + n_updates and algo.learner.value_step == 32 + n_updates      # IQL's own losses go on
    after = algo.state_dict()
    for k in ("actor", "critic", "value"):
        assert t.isfinite(after[k]).all() and not t.equal(before[k], after[k]), k
    check_batches(log, buf, norm(data.observations), data.actions, n_updates)
    # the online rows are normalised observations: the first stored state is the ObsNorm of the environment's first one
    first = make_env(5).reset()[0]
    assert np.array_equal(buf.states[0, 0].cpu().numpy(), norm(first))
    ret = tr.evaluate()["return"]
    print(f"IQL: 32 offline updates, {n_updates} online updates on mixed batches, evaluation return {ret:.3f}")
    assert np.isfinite(ret) and 0.0 < ret <= STEPS


def test_sac_from_scratch_through_the_prior_data_flag(data, tmp_path, monkeypatch):
    """configs/sac.py --prior-data: the script's own factories through run_training for 120 environment steps."""
    from oprl_amd.buffers.prior_buffer import PriorDataReplayBuffer
    from oprl_amd.logging import NullLogger
    from oprl_amd.runners.train import run_training
    path = tmp_path / "cheetah.npz"
    np.savez(path, observations=data.observations, actions=data.actions, rewards=data.rewards, terminals=data.terminals,
             timeouts=data.timeouts, next_observations=data.next_observations)
    mod = load_config(monkeypatch, "sac", ["--env", f"synthetic:{ENV}", "--prior-data", str(path), "--prior-share", "0.5"])
    made, log = {}, []

    def make_algo(logger):
        algo = made["algo"] = mod.make_algo(logger)
        made["start"] = algo.state_dict()
        record_batches(algo, log)
        return algo

    def make_replay_buffer():
        made["buf"] = mod.make_replay_buffer()
        return made["buf"]
    run_training(make_algo=make_algo, make_env=mod.make_env, make_replay_buffer=make_replay_buffer,
                 make_logger=lambda seed: NullLogger(tmp_path), config=dataclasses.replace(mod.config, num_steps=120),
                 start_steps=40, batch_size=B, save_policy_every=0)
    t.cuda.synchronize()
    algo, buf = made["algo"], made["buf"]
    algo.learner.check()
    assert type(buf) is PriorDataReplayBuffer and len(buf) == 121 and len(buf.prior) == EPISODES * STEPS
    n_updates = 121 - (B - 1)
    assert algo.update_step == n_updates
    after = algo.state_dict()
    for k in ("actor", "critic"):
        assert t.isfinite(after[k]).all() and not t.equal(made["start"][k], after[k]), k
    check_batches(log, buf, data.observations, data.actions, n_updates)       # the dataset is stored as it is
    env = mod.make_env(3)
    obs, _ = env.reset()
    assert np.all(np.isfinite(algo.actor.exploit(obs)))
