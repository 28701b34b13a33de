"""GPU tests of the returns-to-go primitive (csrc/replay_returns.hip) against tests/calql_oracle.py: the
float64 definition within the tolerance counted from the kernel's summation order, and that order restated in numpy
float32 bit for bit; over a plain, an n-step, a prioritized and a prior-data handle; slots from the samplers and injected
ones that cover every slot of the table, t = len_e and slots outside the storage; sentinels behind the output, two runs,
rows staged and not yet flushed, and every refusal.

The storage: E = 8, L = 150 with lengths [150, 129, 128, 65, 64, 63, 1, 0], so that tails cross no, one and two chunk
boundaries of 64 steps and end on and next to them; dones mid-episode at steps 70 and 128 of episode 0 and on the last
steps of episodes 1, 3 and 5; the never-written steps hold random rewards and non-zero dones, which nothing may read as part
of a return."""
from __future__ import annotations

import numpy as np
import pytest
import torch as t

from oprl_amd import _capi
from tests import calql_oracle as cal
from tests import prior_oracle as po
from tests.support import INVALID, STATE, fill_random, refused, set_table

pytestmark = pytest.mark.gpu
E, L, S, A = 8, 150, 5, 2
LENS = [150, 129, 128, 65, 64, 63, 1, 0]
PE, PL, P_LENS = 3, 12, [12, 5, 1]
GAMMAS = (1.0, 0.99, 0.5)
BATCHES = (1, 4, 5, 61, 256)
SENT = 12345.0


@pytest.fixture(scope="module", autouse=True)
def generators_as_found():
    """The global generators leave this module as they entered it (DESIGN.md §20's lesson)."""
    import random
    state = random.getstate(), np.random.get_state(), t.get_rng_state(), t.cuda.get_rng_state_all()
    yield
    random.setstate(state[0])
    np.random.set_state(state[1])
    t.set_rng_state(state[2])
    t.cuda.set_rng_state_all(state[3])


def contents(n_e, n_l, lens, seed, dones_at=()):
    """rewards and dones [n_e, n_l] of a storage: random rewards of both signs everywhere, dones 0 inside the live steps
    but at `dones_at`, and non-zero outside them."""
    rs = np.random.RandomState(seed)
    r = (rs.standard_normal((n_e, n_l)) * 2).astype(np.float32)
    d = (1.0 + rs.rand(n_e, n_l)).astype(np.float32)
    for e, n in enumerate(lens):
        d[e, :n] = 0
    for e, k in dones_at:
        d[e, k] = 1
    return r, d


R, D = contents(E, L, LENS, 1, dones_at=((0, 70), (0, 128), (1, 128), (3, 64), (5, 62)))
PR, PD = contents(PE, PL, P_LENS, 2, dones_at=((0, 4), (1, 4)))
_cache: dict = {}


def fill(buf, r, d, lens):
    fill_random(buf, ("states", "actions"), gen_seed=77)
    buf._tensors["rewards"].copy_(t.as_tensor(r).reshape(buf._tensors["rewards"].shape))
    buf._tensors["dones"].copy_(t.as_tensor(d).reshape(buf._tensors["dones"].shape))
    set_table(buf, lens)
    return buf


def handle(kind):
    """One replay per kind over the same contents, built once."""
    if kind in _cache:
        return _cache[kind]
    from oprl_amd.buffers.episodic_buffer import EpisodicReplayBuffer
    from oprl_amd.buffers.nstep_buffer import NStepEpisodicReplayBuffer
    from oprl_amd.buffers.prior_buffer import PriorDataReplayBuffer
    from oprl_amd.buffers.prioritized_buffer import PrioritizedEpisodicReplayBuffer
    kw = dict(buffer_size_transitions=E * L, state_dim=S, action_dim=A, max_episode_lenth=L, device="cuda", seed=7)
    if kind == "plain":
        buf = EpisodicReplayBuffer(**kw).create()
    elif kind == "nstep":
        buf = NStepEpisodicReplayBuffer(n_step=3, gamma=0.9, **kw).create()
    elif kind == "prio":
        buf = PrioritizedEpisodicReplayBuffer(**kw).create()
    else:
        prior = fill(EpisodicReplayBuffer(buffer_size_transitions=PE * PL, state_dim=S, action_dim=A, max_episode_lenth=PL,
                                          device="cuda", seed=7).create(), PR, PD, P_LENS)
        buf = PriorDataReplayBuffer(prior=prior, prior_share=0.5, **kw).create()
    _cache[kind] = fill(buf, R, D, LENS)
    return _cache[kind]


def check(got, ep, step, gamma, what, r=R, d=D, lens=LENS, want=None, tol=None, exact=None):
    """float64 within the counted tolerance, and the restated float32 order bit for bit; each worst figure printed first."""
    got = got.cpu().numpy()
    want = cal.returns_to_go(r, d, lens, ep, step, gamma) if want is None else want
    tol = cal.tolerance(r, d, lens, ep, step, gamma) if tol is None else tol
    exact = cal.returns_f32(r, d, lens, ep, step, gamma) if exact is None else exact
    err = np.abs(got.astype(np.float64) - want)
    print(f"{what}: worst |G - G64| / tolerance {float(np.max(err / np.maximum(tol, 1e-300))):.3f}, "
          f"rows differing from the float32 restatement {int(np.sum(got.view(np.uint32) != exact.view(np.uint32)))}")
    assert got.dtype == np.float32 and np.all(np.isfinite(got))
    assert np.all(err <= tol), (what, int(np.argmax(err - tol)), float(np.max(err - tol)))
    assert np.array_equal(got.view(np.uint32), exact.view(np.uint32)), (what, np.flatnonzero(got != exact)[:5].tolist())


@pytest.mark.parametrize("gamma", GAMMAS)
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("kind", ["plain", "nstep", "prio"])
def test_sampled_slots_on_one_storage(kind, B, gamma):
    """Slots from sample(return_indices=True) — on the prioritized handle from the uniform sampler and from the sum tree —
    at three discounts; G depends on (e, t) alone, so an n-step and a prioritized handle give the plain handle's values."""
    from oprl_amd.buffers.episodic_buffer import EpisodicReplayBuffer
    buf = handle(kind)
    buf._sample_counter = 3 + B
    if kind == "prio":
        _rows, (ep, step) = EpisodicReplayBuffer.sample(buf, B, return_indices=True)
        buf.sample(B)
        slots = buf.last_slots.to(t.int32)
        ep, step = t.cat([ep, slots // L]), t.cat([step, slots % L])
    else:
        _rows, (ep, step) = buf.sample(B, return_indices=True)
        e0, s0 = cal.drawn_slots(LENS, buf.seed, 3 + B, B)
        assert np.array_equal(ep.cpu().numpy(), e0) and np.array_equal(step.cpu().numpy(), s0)
    got = buf.returns_to_go(ep, step, gamma)
    assert got.shape == (ep.numel(),) and got.dtype == t.float32 and got.is_cuda
    check(got, ep.cpu().numpy(), step.cpu().numpy(), gamma, f"{kind} B={B} gamma={gamma}")
    if gamma == 0.99 and kind == "plain":
        buf.gamma = 0.99
        assert t.equal(buf.returns_to_go(ep, step), got)           # the buffer's own gamma is the default


@pytest.mark.parametrize("gamma", GAMMAS)
def test_every_slot_of_the_table_and_slots_outside_it(gamma):
    """Injected: every (e, t) of the storage once — the live steps, t = len_e and beyond (the single stored term), the
    empty episode — and e, t outside the storage (0, nothing read)."""
    ep = np.concatenate([np.repeat(np.arange(E), L), [-1, E, 1000, 0, 0, 0, -5, 2 ** 31 - 1, -2 ** 31]]).astype(np.int32)
    step = np.concatenate([np.tile(np.arange(L), E), [0, 0, 3, -1, L, 10 ** 6, -5, 2 ** 31 - 1, -2 ** 31]]).astype(np.int32)
    buf = handle("plain")
    got = buf.returns_to_go(ep, step, gamma)
    check(got, ep, step, gamma, f"all slots gamma={gamma}")
    g = got.cpu().numpy()
    assert np.all(g[E * L:] == 0)
    # the corners by hand: t >= len_e is the stored reward itself; a done ends the sum at its own step
    for e, n in enumerate(LENS):
        if n < L:
            assert g[e * L + n] == R[e, n], (e, n)
    assert g[0 * L + 70] == R[0, 70] and g[0 * L + 128] == R[0, 128] and g[1 * L + 128] == R[1, 128]
    assert g[6 * L] == R[6, 0] and np.array_equal(g[7 * L:8 * L], R[7])
    if gamma == 1.0:
        assert g[0] == pytest.approx(float(R[0, :71].astype(np.float64).sum()), abs=1e-4)
        assert g[0 * L + 71] == pytest.approx(float(R[0, 71:129].astype(np.float64).sum()), abs=1e-4)
        assert g[2 * L] == pytest.approx(float(R[2, :128].astype(np.float64).sum()), abs=1e-4)


def mixed_check(buf, ep, step, gamma, what):
    p = buf.prior
    args = ((None, None, PR, PD), P_LENS, (None, None, R, D), LENS, buf.prior_share, ep, step, gamma)
    tol = cal.mixed_returns(*args, fn=cal.tolerance)
    check(buf.returns_to_go(ep, step, gamma), ep, step, gamma, what, want=cal.mixed_returns(*args), tol=tol,
          exact=cal.mixed_returns(*args, fn=cal.returns_f32))
    assert p is not None


@pytest.mark.parametrize("gamma", GAMMAS)
@pytest.mark.parametrize("share", [0.0, 0.5, 0.8, 1.0])
@pytest.mark.parametrize("B", BATCHES)
def test_a_prior_data_handle_splits_by_row_index(B, share, gamma):
    """Rows [0, B_p) are slots of the prior (E = 3, L = 12), the rest of the online replay; B_p inside a workgroup's four
    rows (B = 5, 61 at 0.5; 61, 256 at 0.8) and on their boundary (B = 256 at 0.5, B = 5 at 0.8), all and none."""
    buf = handle("prior")
    buf.prior_share = share
    buf._set_prior()
    Bp = buf.n_prior(B)
    assert Bp == po.n_prior(B, share)
    buf._sample_counter = 11 + B
    _rows, (ep, step) = buf.sample(B, return_indices=True)
    ep, step = ep.cpu().numpy(), step.cpu().numpy()
    assert np.all(ep[:Bp] < PE) and np.all(step[:Bp] < PL)
    mixed_check(buf, ep, step, gamma, f"prior-data B={B} share={share} gamma={gamma}")
    if B == 256 and gamma == 0.5:
        # injected: slots that exist in one source only, on both sides — a prior row past the prior's storage gives 0,
        # the same slot as an own row gives the online replay's value
        ep2 = np.where(np.arange(B) % 2 == 0, 5, 1).astype(np.int32)
        step2 = np.where(np.arange(B) % 2 == 0, 40, 3).astype(np.int32)
        mixed_check(buf, ep2, step2, gamma, f"prior-data injected share={share}")
        g = buf.returns_to_go(ep2, step2, gamma).cpu().numpy()
        assert np.all(g[:Bp][np.arange(Bp) % 2 == 0] == 0) and np.all(g[Bp:] != 0)


@pytest.mark.parametrize("B", [1, 5, 61])
def test_nothing_is_written_past_the_batch_and_two_runs_agree(B):
    buf = handle("plain")
    lib = _capi.load()
    rs = np.random.RandomState(B)
    ep = t.as_tensor(rs.randint(0, E, size=B + 9).astype(np.int32)).cuda()
    step = t.as_tensor(rs.randint(0, L, size=B + 9).astype(np.int32)).cuda()
    outs = []
    for _ in range(2):
        out = t.full((B + 9,), SENT, dtype=t.float32, device="cuda")
        _capi.check(lib.oprl_replay_returns(buf.handle, B, _capi.ptr(ep), _capi.ptr(step), 0.99, _capi.ptr(out),
                                            _capi.current_stream()), "oprl_replay_returns")
        t.cuda.synchronize()
        outs.append(out.cpu().numpy())
    assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32))
    assert np.all(outs[0][B:] == SENT)
    check(t.as_tensor(outs[0][:B]), ep[:B].cpu().numpy(), step[:B].cpu().numpy(), 0.99, f"head B={B}")


def test_rows_staged_and_not_yet_flushed_are_seen():
    """add_transitions leaves its rows in host staging: the call flushes the handle — and its prior — before its launch."""
    from oprl_amd.buffers.episodic_buffer import EpisodicReplayBuffer
    from oprl_amd.buffers.prior_buffer import PriorDataReplayBuffer
    kw = dict(state_dim=S, action_dim=A, device="cuda")
    rs = np.random.RandomState(9)

    def staged(buf, lens, done_last):
        n_e, n_l = buf._max_episodes, buf.max_episode_lenth
        r, d = np.zeros((n_e, n_l), np.float32), np.zeros((n_e, n_l), np.float32)
        for e, n in enumerate(lens):
            rows = rs.standard_normal((n, S + A + 2)).astype(np.float32)
            rows[:, S + A + 1] = 0
            if done_last[e]:
                rows[-1, S + A + 1] = 1
            buf.add_transitions(rows, episode_done=e + 1 < len(lens))        # the last episode stays open: the running tail
            r[e, :n], d[e, :n] = rows[:, S + A], rows[:, S + A + 1]
        return r, d

    buf = EpisodicReplayBuffer(buffer_size_transitions=4 * 70, max_episode_lenth=70, **kw).create()
    lens = [70, 3, 66]
    r, d = staged(buf, lens, [True, False, False])
    ep = np.repeat(np.arange(3), 70).astype(np.int32)
    step = np.tile(np.arange(70), 3).astype(np.int32)
    check(buf.returns_to_go(ep, step, 0.9), ep, step, 0.9, "staged rows", r=r, d=d, lens=lens)
    prior = EpisodicReplayBuffer(buffer_size_transitions=3 * 6, max_episode_lenth=6, **kw).create()
    p_lens = [6, 2]
    pr, pd = staged(prior, p_lens, [False, False])
    mix = PriorDataReplayBuffer(buffer_size_transitions=4 * 70, max_episode_lenth=70, prior=prior, prior_share=0.5, **kw).create()
    m_lens = [5]
    mr, md = staged(mix, m_lens, [False])
    ep = np.array([0, 0, 1, 1, 0, 0, 0, 0], np.int32)
    step = np.array([0, 5, 0, 1, 0, 1, 4, 5], np.int32)
    args = ((None, None, pr, pd), p_lens, (None, None, mr, md), m_lens, 0.5, ep, step, 0.9)
    check(mix.returns_to_go(ep, step, 0.9), ep, step, 0.9, "staged rows, both sources", want=cal.mixed_returns(*args),
          tol=cal.mixed_returns(*args, fn=cal.tolerance), exact=cal.mixed_returns(*args, fn=cal.returns_f32))


def test_refusals():
    """Every refusal with its status and a word of its message; the output is untouched and a following call is right."""
    from oprl_amd.buffers.episodic_buffer import EpisodicReplayBuffer
    from oprl_amd.buffers.prior_buffer import PriorDataReplayBuffer
    lib = _capi.load()
    buf = handle("plain")
    h, st = buf.handle, _capi.current_stream()
    B = 5
    ep = t.zeros(B, dtype=t.int32, device="cuda")
    step = t.arange(B, dtype=t.int32, device="cuda")
    out = t.full((B,), SENT, dtype=t.float32, device="cuda")
    call = lambda hh=h, b=B, e=ep, s=step, g=0.99, o=out: lib.oprl_replay_returns(hh, b, _capi.ptr(e), _capi.ptr(s), g, _capi.ptr(o), st)   # noqa: E731
    refused(call(hh=None), INVALID, b"null")
    refused(call(e=None), INVALID, b"null")
    refused(call(s=None), INVALID, b"null")
    refused(call(o=None), INVALID, b"null")
    for b in (0, -3):
        refused(call(b=b), INVALID, b"B >= 1")
    for g in (0.0, -0.5, 1.0000001, float("nan"), float("inf")):
        refused(call(g=g), INVALID, b"gamma")
    # a source in hindsight mode: its rewards are relabelled per sample
    her = fill(EpisodicReplayBuffer(buffer_size_transitions=E * L, state_dim=S, action_dim=A, max_episode_lenth=L,
                                    device="cuda").create(), R, D, LENS)
    assert lib.oprl_replay_set_her(her.handle, 0, 2, 2, 0.8, 0, 0, 0.1) == 0
    refused(call(hh=her.handle), STATE, b"hindsight")
    with pytest.raises(RuntimeError, match="hindsight"):
        her.returns_to_go(ep, step)
    assert lib.oprl_replay_set_her(her.handle, 0, 0, 0, 0.0, 0, 0, 0.0) == 0
    # a source that must supply a row but holds no transitions
    kw = dict(state_dim=S, action_dim=A, device="cuda")
    empty = EpisodicReplayBuffer(buffer_size_transitions=4 * 6, max_episode_lenth=6, **kw).create()
    refused(call(hh=empty.handle), STATE, b"empty")
    prior = EpisodicReplayBuffer(buffer_size_transitions=3 * 6, max_episode_lenth=6, **kw).create()
    mix = PriorDataReplayBuffer(buffer_size_transitions=4 * 6, max_episode_lenth=6, prior=prior, prior_share=0.5, **kw).create()
    refused(call(hh=mix.handle), STATE, b"prior replay is empty")
    prior.add_transitions(np.ones((3, S + A + 2), np.float32))
    refused(call(hh=mix.handle), STATE, b"this replay is empty")
    mix.prior_share = 1.0
    mix._set_prior()
    assert call(hh=mix.handle, g=1.0) == 0                # the online replay supplies no row: it may be empty
    t.cuda.synchronize()
    assert out.cpu().tolist() == [1.0, 1.0, 1.0, 0.0, 0.0]          # three stored steps of reward 1 and done 1, then t >= len_e
    out.fill_(SENT)
    for bad in (lambda: call(hh=None), lambda: call(g=0.0), lambda: call(hh=empty.handle)):
        bad()
    t.cuda.synchronize()
    assert bool((out == SENT).all())
    assert call() == 0
    t.cuda.synchronize()
    check(out, ep.cpu().numpy(), step.cpu().numpy(), 0.99, "after the refusals")
