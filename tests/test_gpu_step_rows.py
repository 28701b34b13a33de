"""Where step_n's rows come from, held across calls (csrc/learner_internal.h StepRows / RowStager).

A learner alternates step_n calls of odd and even K with a plain update() on the caller's rows, at B = 40 (three 16-row
slices, the last one ragged) over a small replay of uneven episodes; its twin only ever sees buf.sample(B) + update() with
the sampler's seed and counter set as tests/test_gpu_bench_parity.py sets them.  After every call every arena, both
optimizers' moments, the targets, the temperature and the counters are compared bit for bit: a staging set read out of
turn, rows staged by one call and read by the next, or a gather flag that outlives its call all change the bits.  Each case
first asserts the launch form, so that it is on the row path it names."""
from __future__ import annotations

import pytest
import torch as t

from oprl_amd import _capi
from tests.test_gpu_nstep import assert_same_state, make_buffer, set_table

pytestmark = pytest.mark.gpu

S, A, B = 24, 6, 40
E, L = 10, 30
LENS = [7, 30, 1, 12, 25, 3, 18, 30, 9, 14]
INVALID, STATE = -1, -3


def _fill(buf):
    """Ten closed episodes of uneven length over random storage; episodes 0, 3 and 6 end in done = 1, episode 4 has one
    in its middle."""
    dones = t.zeros((E, L, 1))
    for e in (0, 3, 6):
        dones[e, LENS[e] - 1] = 1
    dones[4, 11] = 1
    buf._tensors["dones"].copy_(dones)
    set_table(buf, LENS)
    return buf


@pytest.fixture(scope="module")
def replay():
    from oprl_amd.buffers.episodic_buffer import EpisodicReplayBuffer
    return _fill(make_buffer(E, L, S, A, cls=EpisodicReplayBuffer))


def make_algo(name, prec, monkeypatch, env=None):
    """A learner at walker dims; `env`: OPRL_AMD_* switches that hold while it is created (they are read once, there)."""
    from oprl_amd.algos.ddpg import DDPG
    from oprl_amd.algos.sac import SAC
    from oprl_amd.algos.td3 import TD3
    from oprl_amd.algos.tqc import TQC
    from oprl_amd.logging import NullLogger
    cls = dict(ddpg=DDPG, td3=TD3, sac=SAC, tqc=TQC)[name]
    kw = {} if name == "ddpg" else dict(log_every=10 ** 9)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    t.manual_seed(0)
    algo = cls(logger=NullLogger("/tmp/oprl_amd_test"), state_dim=S, action_dim=A, device="cuda", max_batch=B,
               precision=prec, **kw).create()
    for k in env or {}:
        monkeypatch.delenv(k)
    return algo


def interleave(fused, loop, buf):
    """step_n(K = 5, seed 1), a plain update on sampled rows, step_n(K = 1), step_n(K = 4, seed 2) on `fused`; the same
    eleven updates as sample() + update() pairs on `loop`; equal bits after every call."""
    def step_n(K, seed):
        fused.learner.step_n(buf.handle, K, B, seed=seed)
        buf.seed = seed
        for _ in range(K):
            buf._sample_counter = loop.update_step
            loop.update(*buf.sample(B))
        assert_same_state(fused, loop)

    step_n(5, 1)
    buf.seed, buf._sample_counter = 9, fused.update_step
    batch = buf.sample(B)
    fused.update(*batch)
    loop.update(*batch)
    assert_same_state(fused, loop)
    step_n(1, 1)
    step_n(4, 2)
    assert fused.update_step == loop.update_step == 11


# (name, precision, switches at create, the debug_form fields that name the row path)
CASES = [
    # k_ddpg_chain launches of 2, 2, 1 updates and then 2, 2: an odd U flips the set parity, pf_last takes both values
    ("ddpg", "f32", {"OPRL_AMD_CHAIN": "2"}, dict(fused=1, form=4, updates_per_chain_launch=2)),
    # TD3 at policy_freq 2: the odd K ends on a critic-only update.  Merged phase 1 only (exact fp32: the r06-15 rows) and
    # both merged launches (x2) stage from phase 1 into alternating sets ...
    ("td3", "f32", {}, dict(fused=1, form=2)),
    ("td3", "x2", {}, dict(fused=1, form=3)),
    # ... without the phase-1 rows phase 2 stages, and a critic-only update leaves nothing staged
    ("td3", "f32", {"OPRL_AMD_NO_P1_ROWS": "1"}, dict(fused=1, form=2)),
    ("sac", "f32", {}, dict(fused=1, form=1)),      # phase 2 stages into the set it reads
    ("tqc", "f32", {}, dict(fused=0)),              # the generic path: the riders of k_lw_dact fill the other set
]


@pytest.mark.parametrize("name,prec,env,form", CASES, ids=["-".join([n, p, *e]) for n, p, e, _ in CASES])
def test_interleaved_calls_equal_sample_then_update(name, prec, env, form, replay, monkeypatch):
    fused, loop = make_algo(name, prec, monkeypatch, env), make_algo(name, prec, monkeypatch, env)
    got = fused.debug_form(B)
    assert {k: got[k] for k in form} == form, got
    if name == "td3":
        assert fused.policy_freq == 2
    assert_same_state(fused, loop)
    interleave(fused, loop, replay)


def test_a_refused_step_n_leaves_nothing_behind(replay, monkeypatch):
    from oprl_amd.buffers.episodic_buffer import EpisodicReplayBuffer
    lib = _capi.load()
    fused, loop = make_algo("ddpg", "f32", monkeypatch), make_algo("ddpg", "f32", monkeypatch)
    empty = make_buffer(E, L, S, A, cls=EpisodicReplayBuffer)
    other = make_buffer(4, 10, 3, 2, cls=EpisodicReplayBuffer)
    set_table(other, [5, 5])
    nstep = _fill(make_buffer(E, L, S, A, n_step=3, gamma=0.9))
    assert fused.gamma != 0.9

    def refused(buf, status, word):
        rc = lib.oprl_learner_step_n(fused.learner.handle, buf.handle, 5, B, 1, _capi.current_stream())
        msg = lib.oprl_last_error()
        assert rc == status and word in msg, (rc, msg)

    refused(empty, STATE, b"empty")
    refused(other, INVALID, b"dims")
    refused(nstep, INVALID, b"gamma")
    assert fused.update_step == 0
    interleave(fused, loop, replay)


def test_group_members_read_the_callers_rows_afterwards(replay, monkeypatch):
    from oprl_amd.group import LearnerGroup
    members = [make_algo("ddpg", "f32", monkeypatch) for _ in range(2)]
    solo = [make_algo("ddpg", "f32", monkeypatch) for _ in range(2)]
    seeds = [5, 6]
    g = LearnerGroup(members)
    g.step_n(replay.handle, 3, B, seeds)
    gen = t.Generator(device="cuda").manual_seed(77)
    rows = [t.randn((B, n), device="cuda", generator=gen) for n in (S, A, 1, 1, S)]      # (in no replay)
    rows[3] = (rows[3] > 1).float()
    for m, s, seed in zip(members, solo, seeds):
        assert s.learner.lib.oprl_learner_set_cluster(s.learner.handle, 1) == 0          # (the members' launch form)
        s.learner.step_n(replay.handle, 3, B, seed=seed)
        assert_same_state(m, s)
        m.update(*rows)
        s.update(*rows)
        assert_same_state(m, s)
        assert m.update_step == 4
    g.close()
