"""REDQ on the MI355X learner against tests/redq_oracle.py (float64, autograd, written from the spec), and the
properties the spec fixes: the target subset, the actor's cadence against the targets' Polyak step, step_n against
sample() + update(), resume in the middle of a group, and the configurations create() refuses."""
from __future__ import annotations

import ctypes as C

import pytest
import torch as t

from oprl_amd import _capi
from oprl_amd.algos.redq import REDQ
from oprl_amd.logging import NullLogger
from oracle import fixtures as fx
from tests import scenarios as sc
from tests.hip_adapters import cpu_params
from tests.redq_oracle import REDQOracle
from tests.support import (as_np, assert_same_state, check_step_n_equals_loop, fill_full_episodes, pair_adam, pair_nets, pair_q_y,
                           run_pair, to_double, worst_ratio)

pytestmark = pytest.mark.gpu

S, A, N, G = 24, 6, 10, 3          # walker dims, the default ensemble, an actor step every third update
TOL = 2e-5                          # network outputs (tests/test_gpu_algos.py)
SEED, RANK = 7, 0


def subset(n, m, seed=SEED, rank=RANK):
    lib = _capi.load()

    def draw(u):
        out = (C.c_int32 * m)()
        _capi.check(lib.oprl_redq_subset(seed, rank, u, n, m, out), "oprl_redq_subset")
        return list(out)
    return draw


def make(n_min, B, **kw):
    algo = REDQ(logger=NullLogger(), state_dim=S, action_dim=A, n_critics=kw.pop("n_critics", N), n_min=n_min,
                utd_ratio=kw.pop("utd_ratio", G), log_every=10 ** 9, max_batch=max(B, 256), **kw).create()
    algo.set_seed(SEED, RANK)
    return algo


def oracle_for(algo, n_min, **kw):
    L = algo.learner
    return REDQOracle(S, A, cpu_params(algo.actor), [cpu_params(n) for n in algo.critic.nets],
                      [cpu_params(n) for n in algo.critic_target.nets], subset(algo.n_critics, n_min), n_min,
                      algo.utd_ratio, tau=algo.target_update_coef, alpha_init=algo.alpha_init, **kw)


def batches(B, n):
    out = []
    for k in range(n):
        s, a, r, d, s2 = fx.make_batch(100 + k, B, S, A)
        g = t.Generator().manual_seed(500 + k)
        out.append((s, a, r, d, s2, t.randn(B, A, generator=g), t.randn(B, A, generator=g)))
    return out


def step(algo, x):
    algo.update(*(v.cuda() for v in x[:5]), noise=(x[5].cuda(), x[6].cuda()))


def got_and_want(algo, o, B):
    L = algo.learner
    got, want = {}, {}
    for i in range(algo.n_critics):
        pair_nets(got, want, f"critic.{i}", algo.critic.nets[i], o.critics[i])
        pair_nets(got, want, f"critic_target.{i}", algo.critic_target.nets[i], o.targets[i])
    pair_nets(got, want, "actor", algo.actor, o.actor)
    pair_adam(got, want, algo, "critic", o.opt_critic)
    pair_adam(got, want, algo, "actor", o.opt_actor)
    got["u.log_alpha"], want["u.log_alpha"] = L.log_alpha.cpu().reshape(1), o.log_alpha.reshape(1)
    got["u.log_alpha_m"], want["u.log_alpha_m"] = L.log_alpha_m.cpu().reshape(1), o.opt_alpha.m[0]
    got["u.log_alpha_v"], want["u.log_alpha_v"] = L.log_alpha_v.cpu().reshape(1), o.opt_alpha.v[0]
    pair_q_y(got, want, algo, B, o.last["q"], o.last["y"])
    return as_np(got), as_np(want)


PARITY = [(256, 2), (256, 1), (256, 3), (100, 2)]


@pytest.mark.parametrize("B,n_min", PARITY, ids=[f"B{b}-M{m}" for b, m in PARITY])
def test_redq_matches_the_oracle(B, n_min):
    """Four updates with G = 3 (critic-only updates before and after an actor step): every critic, target, the actor,
    both optimizers' moments, log alpha and its moments, and the last update's q / y rows within the suite's gates.
    M = 3 takes the minimum through k_redq_min; B = 100 is a ragged batch."""
    algo = make(n_min, B)
    o = oracle_for(algo, n_min)
    run_pair(algo, [o], batches(B, 4), step, to_double)
    assert algo.learner.update_count == 4
    got, want = got_and_want(algo, o, B)
    sc.compare(got, want, TOL, param_tol=sc.PARAM_TOL)


def test_the_comparison_discriminates():
    """The same oracle, given the subset of u + 1, the mean instead of the minimum, or the Polyak step on actor steps
    only, misses the gates by a factor of ten or more (tau = 0.5 here so that a missing Polyak step shows in y at once)."""
    B = 256
    algo = make(2, B, target_update_coef=0.5)
    right = oracle_for(algo, 2)
    wrong = {"subset of u+1": oracle_for(algo, 2, subset_shift=1), "mean": oracle_for(algo, 2, use_mean=True),
             "polyak on actor steps": oracle_for(algo, 2, polyak_on_actor_steps=True)}
    run_pair(algo, [right, *wrong.values()], batches(B, 4), step, to_double)
    got, want = got_and_want(algo, right, B)
    sc.compare(got, want, TOL, param_tol=sc.PARAM_TOL)
    for name, o in wrong.items():
        r, _key = worst_ratio(*got_and_want(algo, o, B), TOL)
        assert r >= 10.0, f"{name}: the learner is only {r:.1f} gates away from the wrong oracle"


def test_actor_cadence_and_targets_every_update():
    """Across updates 0 .. G-2 the actor arena is bitwise unchanged while the critic targets move on every update; update
    G-1 moves the actor."""
    B = 256
    algo = make(2, B)
    L = algo.learner
    data = batches(B, G)
    actor0 = L.actor_arena.detach().clone()
    for k, (s, a, r, d, s2, e1, e2) in enumerate(data):
        tgt = L.target_arenas()[0].detach().clone()
        algo.update(*(x.cuda() for x in (s, a, r, d, s2)), noise=(e1.cuda(), e2.cuda()))
        t.cuda.synchronize()
        assert not t.equal(L.target_arenas()[0], tgt), f"targets did not move at update {k}"
        if k < G - 1:
            assert t.equal(L.actor_arena, actor0), f"the actor moved at update {k}"
    assert not t.equal(L.actor_arena, actor0), "the actor did not move at update G-1"


def _replay(dev, seed=0, E=40, Lep=100):
    from oprl_amd.buffers.episodic_buffer import EpisodicReplayBuffer
    buf = EpisodicReplayBuffer(buffer_size_transitions=E * Lep, state_dim=S, action_dim=A, device=str(dev),
                               seed=seed, max_episode_lenth=Lep).create()
    fill_full_episodes(buf, E, Lep)
    return buf


def test_step_n_equals_sample_then_update_bitwise():
    """step_n(K = G) over a replay with 2 % done rows is bit for bit G times sample() + update() with the sampler's rows."""
    B, dev = 256, t.device("cuda", 0)
    buf = _replay(dev)
    fused, _loop, n_done = check_step_n_equals_loop(lambda: (make(2, B), make(2, B)), buf, B, K=G)
    assert n_done > 0 and "log_alpha" in fused.state_dict()


def test_resume_in_the_middle_of_a_group():
    """state_dict() after update 1 of a G group, loaded into a fresh learner, continues bit for bit."""
    B = 256
    data = batches(B, 5)
    a = make(2, B)
    for x in data[:1]:
        step(a, x)
    b = make(2, B)
    b.load_state_dict(a.state_dict())
    for x in data[1:]:
        for algo in (a, b):
            step(algo, x)
    assert a.update_step == 5
    assert_same_state(a, b)
    assert "log_alpha" in a.state_dict()


@pytest.mark.parametrize("kw,msg", [
    (dict(n_min=3, n_critics=2), "n_min=3"),
    (dict(n_critics=11), "n_critics=11"),
    (dict(precision="bf16"), "f32 only"),
    (dict(precision="x2"), "f32 only"),
    (dict(export_grads=True), "export_grads"),
], ids=["n_min>n_critics", "n_critics=11", "bf16", "x2", "export_grads"])
def test_create_refuses(kw, msg):
    n_min = kw.pop("n_min", 2)
    with pytest.raises((RuntimeError, ValueError), match=msg):
        make(n_min, 256, **kw)


def test_learner_group_refuses_redq_members():
    from oprl_amd.group import LearnerGroup
    members = [make(2, 256), make(2, 256)]
    with pytest.raises(RuntimeError, match="fused"):
        LearnerGroup(members)
