"""DDPG through step_n at the shapes where the chain launch's index arithmetic takes another path.

k_ddpg_chain reads (grid row, update) off the block index and forms its row / column / tile indices from multipliers
the host writes (csrc/idiv.h) — no division.  The shapes:

    B = 16,  S = 3,  A = 1    one slice: the tile-only grid rows carry every tile the roles cannot
    B = 40,  S = 11, A = 5    a ragged last slice; S + A = 16, exactly one layer-0 step
    B = 176, S = 17, A = 6    eleven slices — the first batch without tile-only rows — and two layer-0 steps
    B = 64,  S = 67, A = 21   88 inputs: all six layer-0 steps.  21 actions are more than the chain launch's tiles and the
                              cluster-of-eight passes take: this learner runs the phase launches on clusters of four, where
                              of the divide-free quotients only the 16 x 64 tiles' coordinates can occur — the shape guards
                              the step_n path beside the chain more than the chain's own index arithmetic

each with K = 3 (one chain launch) and K = 33 (32 + 1: the launch boundary), in f32, x2 and bf16:
  * step_n equals the same number of update() calls on the sampler's rows, bit for bit;
  * the last updates against the float64 CPU oracle, from the twin learner's own state, within the suite's gates: f32
    and x2 those of tests/test_gpu_bench_parity.py; bf16 those tests/test_gpu_bf16.py holds the mode to against the
    fp32 reference (operands of 8 mantissa bits: 2^-9 relative each).  Those gates are wide: a subtle bf16-only error
    would pass them, and the bitwise equality does not catch an index error either — step_n and update() run the same
    kernel.  What checks the index arithmetic is the f32 and x2 cases: the bf16 kernel is the same text with another
    precision policy.  (The bf16 emulation's own gate — 2e-5, set at B = 256 by tests/test_gpu_bf16.py — is not one for
    these shapes: measured at B = 16, A = 1, K = 3, pi is 3.3e-5 from the float32 emulation — one hidden activation on
    the other side of a bf16 rounding boundary moves a one-column output by 2^-9 of one of its 256 terms.)
Two more cases put another writer of the masters between two chain calls: load_state_dict of another learner's state, and
a learner of a non-chain launch form."""
from __future__ import annotations

import numpy as np
import pytest
import torch as t

from oracle import fixtures as fx
from tests import hip_adapters as ha
from tests import scenarios as sc

pytestmark = pytest.mark.gpu

SHAPES = [(16, 3, 1), (40, 11, 5), (176, 17, 6), (64, 67, 21)]
PRECS = ("f32", "x2", "bf16")
KS = (3, 33)
WINDOW = 4                   # updates the oracle runs up to the end, from the twin learner's state
SEED = 7
TOL, X2_MOMENT_TOL = 2e-5, 5e-3                  # tests/test_gpu_bench_parity.py
TOL_REF_OUT, TOL_REF_PARAM, TOL_REF_GRAD = 2e-2, 5e-2, 0.2               # tests/test_gpu_bf16.py: bf16 against fp32
PROBE_B = 64
PARAMS = ("actor", "critic", "actor_target", "critic_target")


def _buffer(S, A, n_eps=6, L=50, seed=3):
    """n_eps - 1 finished episodes of L, L - 1, ... transitions, the last transition of each a real terminal."""
    from oprl_amd.buffers.episodic_buffer import EpisodicReplayBuffer
    buf = EpisodicReplayBuffer(buffer_size_transitions=n_eps * L, state_dim=S, action_dim=A,
                               max_episode_lenth=L, device="cuda", seed=seed).create()
    rs = np.random.RandomState(S * 100 + A)
    for e in range(n_eps - 1):
        for i in range(L - e):
            last = i == L - e - 1
            buf.add_transition(rs.standard_normal(S).astype(np.float32), rs.uniform(-1, 1, A),
                               float(rs.uniform()), last, episode_done=last)
    return buf


@pytest.fixture(scope="module")
def buffers():
    cache = {}

    def get(S, A):
        if (S, A) not in cache:
            cache[(S, A)] = _buffer(S, A)
        return cache[(S, A)]

    yield get
    cache.clear()


def _nets(S, A):
    return fx.make_net(101, fx.actor_dims(S, A)), fx.make_net(102, fx.critic_dims(S, A))


def _equal_state(a, b):
    x, y = a.state_dict(), b.state_dict()
    for k in ("actor", "actor_m", "actor_v", "critic", "critic_m", "critic_v"):
        assert t.equal(x[k], y[k]), (k, (x[k] - y[k]).abs().max().item())
    for i, (p, q) in enumerate(zip(x["targets"], y["targets"])):
        assert t.equal(p, q), (f"targets[{i}]", (p - q).abs().max().item())
    assert x["counters"] == y["counters"], (x["counters"], y["counters"])


def _snapshot(ad, tag, probe):
    s, a = probe
    snap = {f"{tag}.out.q": ad.q(s, a), f"{tag}.out.q_target": ad.q_target_pi(s), f"{tag}.out.pi": ad.pi(s)}
    snap = {k: np.asarray(v.detach().cpu().numpy(), np.float64) for k, v in snap.items()}
    for name in PARAMS:
        for i, x in enumerate(ad.params(name)):
            snap[f"{tag}.{name}.{i}"] = x.detach().cpu().numpy().copy()
    for w in ("critic", "actor"):
        m, v = ad.adam(w)
        for i, (mi, vi) in enumerate(zip(m, v)):
            snap[f"{tag}.m_{w}.{i}"] = mi.detach().cpu().numpy().copy()
            snap[f"{tag}.v_{w}.{i}"] = vi.detach().cpu().numpy().copy()
    return snap


def _oracle_from(hip, S, A, nets, dtype):
    """The CPU oracle standing where the learner stands: parameters, targets, both optimizers' moments and step counts."""
    ora = sc.OracleDDPG(S, A, *[[x.to(dtype) for x in n] for n in nets])
    o = ora.o
    with t.no_grad():
        for name in PARAMS:
            for dst, src in zip(getattr(o, name), hip.params(name), strict=True):
                dst.copy_(src)
    for w, opt in (("critic", o.opt_critic), ("actor", o.opt_actor)):
        m, v = hip.adam(w)
        opt.m, opt.v = [x.to(dtype) for x in m], [x.to(dtype) for x in v]
    n_upd, o.opt_critic.step_count, o.opt_actor.step_count, _ = hip.algo.learner.state_dict()["counters"]
    if hasattr(o, "update_step"):
        o.update_step = n_upd
    return ora


def _check_oracle(got, want, prec):
    if prec != "bf16":
        return sc.compare(got, want, TOL, param_tol=sc.PARAM_TOL, moment_tol=X2_MOMENT_TOL if prec == "x2" else None)
    # (across arithmetics: no element-count bound; the Adam moments are gradient-like keys)
    return sc.compare(got, want, TOL_REF_OUT, param_tol=TOL_REF_PARAM, moment_tol=TOL_REF_GRAD, moment_off_frac=None)


CASES = [(B, S, A, p, K) for (B, S, A) in SHAPES for p in PRECS for K in KS]


@pytest.mark.parametrize("B,S,A,prec,K", CASES, ids=[f"B{B}-S{S}-A{A}-{p}-K{K}" for B, S, A, p, K in CASES])
def test_step_n_at_the_index_edges(B, S, A, prec, K, buffers):
    buf = buffers(S, A)
    nets = _nets(S, A)
    hip, loop = (ha.HipDDPG(S, A, *nets, precision=prec, max_batch=B) for _ in range(2))
    L = hip.algo.learner
    form = L.debug_form(B)
    # the chain launch where its tiles take the action size (kDuLd = 8 du granules per row), 32 updates per launch
    assert (form["form"] == 4) == (A <= 8), form
    if A <= 8:
        assert form["updates_per_chain_launch"] == 32, form
    probe = fx.make_batch(999, PROBE_B, S, A)[:2]
    dtype = t.float64

    L.step_n(buf.handle, K, B, seed=SEED)
    buf.seed = SEED
    ora = None
    for k in range(K):
        if k == max(K - WINDOW, 0):
            t.cuda.synchronize()
            ora = _oracle_from(loop, S, A, nets, dtype)
            first = k
        buf._sample_counter = k
        batch = buf.sample(B)
        loop.algo.update(*batch)
        if ora is not None:
            rows = [x.cpu().to(dtype) for x in batch]
            ora.update(*rows)
    t.cuda.synchronize()
    L.check()
    loop.algo.learner.check()
    _equal_state(hip.algo, loop.algo)
    assert hip.algo.update_step == loop.algo.update_step == K

    probe_o = tuple(x.to(dtype) for x in probe)
    got, want = _snapshot(hip, f"after{K}", probe), _snapshot(ora, f"after{K}", probe_o)
    assert _oracle_counters(ora) == L.state_dict()["counters"][:3]
    worst = _check_oracle(got, want, prec)
    print(f"\nB={B} S={S} A={A} [{prec}] K={K}: form {form['form']}, oracle window {first}..{K}, worst {worst[1]:.2e} ({worst[0]})")


def _oracle_counters(ora):
    o = ora.o
    return [getattr(o, "update_step", o.opt_critic.step_count), o.opt_critic.step_count, o.opt_actor.step_count]


def test_load_state_between_two_step_n_calls(buffers):
    """Something other than a chain launch writes the masters — biases included — between two chain launches: the next
    launch's first update must read what was loaded."""
    B, S, A = 40, 11, 5
    buf = buffers(S, A)
    nets = _nets(S, A)
    other = ha.HipDDPG(S, A, *nets, precision="f32", max_batch=B)
    other.algo.learner.step_n(buf.handle, 5, B, seed=11)
    t.cuda.synchronize()
    state = other.algo.state_dict()
    hip, loop = (ha.HipDDPG(S, A, *nets, precision="f32", max_batch=B) for _ in range(2))
    hip.algo.learner.step_n(buf.handle, 3, B, seed=SEED)
    buf.seed = SEED
    for k in range(3):
        buf._sample_counter = k
        loop.algo.update(*buf.sample(B))
    t.cuda.synchronize()
    _equal_state(hip.algo, loop.algo)
    hip.algo.load_state_dict(state)
    loop.algo.load_state_dict(state)
    assert hip.algo.update_step == loop.algo.update_step == 5
    hip.algo.learner.step_n(buf.handle, 3, B, seed=SEED)
    for k in range(5, 8):
        buf._sample_counter = k
        loop.algo.update(*buf.sample(B))
    t.cuda.synchronize()
    hip.algo.learner.check()
    _equal_state(hip.algo, loop.algo)
    assert not t.equal(hip.algo.state_dict()["critic"], state["critic"])


@pytest.mark.parametrize("prec", PRECS)
def test_a_non_chain_form_between_two_chain_calls(prec, buffers, monkeypatch):
    """A learner of another launch form (OPRL_AMD_FORM=two at create: the merged phase launches, no k_ddpg_chain) writes
    the masters, the biases and the actor's output layer between two chain calls; the state crosses with state_dict /
    load_state_dict.  Update 0 of the chain launch that follows must read what that form left — the masters' biases,
    the row-major output layer — not what its own tiles left in their uncached copies three updates earlier.  The
    reference walks the same forms with update() on the sampler's rows: bit for bit after every leg."""
    B, S, A = 40, 11, 5
    buf = buffers(S, A)
    nets = _nets(S, A)

    def make(env):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        ad = ha.HipDDPG(S, A, *nets, precision=prec, max_batch=B)
        for k in env:
            monkeypatch.delenv(k)
        return ad

    chain, chain_ref = make({}), make({})
    two, two_ref = make({"OPRL_AMD_FORM": "two"}), make({"OPRL_AMD_FORM": "two"})
    assert chain.algo.learner.debug_form(B)["form"] == 4, chain.algo.learner.debug_form(B)
    assert two.algo.learner.debug_form(B)["form"] != 4, two.algo.learner.debug_form(B)
    buf.seed = SEED
    legs = ((chain, chain_ref), (two, two_ref), (chain, chain_ref))
    state = None
    for leg, (fused, ref) in enumerate(legs):
        if state is not None:
            fused.algo.load_state_dict(state)
            ref.algo.load_state_dict(state)
        assert fused.algo.update_step == ref.algo.update_step == 3 * leg
        fused.algo.learner.step_n(buf.handle, 3, B, seed=SEED)
        for k in range(3 * leg, 3 * leg + 3):
            buf._sample_counter = k
            ref.algo.update(*buf.sample(B))
        t.cuda.synchronize()
        fused.algo.learner.check()
        ref.algo.learner.check()
        _equal_state(fused.algo, ref.algo)
        state = fused.algo.state_dict()
    # (the second chain call started from the other form's state, not from where the first one ended)
    assert chain.algo.update_step == 9
