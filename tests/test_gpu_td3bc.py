"""TD3+BC on the MI355X learner against tests/td3bc_oracle.py (float64, written from the formulas of DESIGN.md §16):
parity over four updates at four shapes, oracle variants that must miss, the bitwise links to a plain no_fuse TD3
learner, step_n against sample() + update() over a plain and an n-step replay, resume, every refusal, and no effect on a
TD3 learner of the same process.

The parity runs start from fixture nets (oracle/fixtures.py make_net, as the TD3 scenario does).  Their seed, 300 for
both environments, was fixed with the oracle alone, before any GPU run: its float32 run on the CPU stays within 1.0e-6
(walker, B = 256), 2.0e-6 (walker, 100), 5.8e-6 (cheetah, 256) and 3.0e-6 (cheetah, 100) of its float64 run, max-norm per
tensor over parameters, targets and moments after these four updates — a twentieth of the parameter gate at worst, so a
miss here says something about the kernels.  (Seed 500 for walker, 3.8e-5 on these batches, and seeds 200 / 400 for
cheetah, up to 1.2e-2 — the one-row ReLU flip tests/scenarios.py compare describes — were passed over.)  In the same
runs the oracle without the cloning term is 0.2 .. 0.4 away and the one with lambda = 1 about 1.0: thousands of gates."""
from __future__ import annotations

import ctypes as C

import pytest
import torch as t

from oprl_amd import _capi
from oprl_amd.algos.td3 import TD3
from oprl_amd.algos.td3_bc import TD3BC
from oprl_amd.logging import NullLogger
from oracle import fixtures as fx
from tests import scenarios as sc
from tests.hip_adapters import load_params
from tests.support import (INVALID, STATE, as_np, assert_same_state, check_resume, check_step_n_equals_loop, counters, pair_adam,
                           pair_nets, pair_q_y, random_replay, refused, run_pair, worst_ratio)
from tests.td3bc_oracle import TD3BCOracle

pytestmark = pytest.mark.gpu

TOL = 2e-5                          # network outputs (tests/test_gpu_algos.py)
NET_SEED = 300
GAMMA = 0.99


def make(env, B, cls=TD3BC, fixture_nets=False, **kw):
    S, A = fx.ENVS[env]
    t.manual_seed(0)
    if cls is TD3:
        kw.setdefault("no_fuse", True)
    algo = cls(logger=NullLogger(), state_dim=S, action_dim=A, max_batch=max(B, 256), log_every=10 ** 9, **kw).create()
    if fixture_nets:
        actor, c1, c2 = fixture(env)
        load_params(algo.actor, actor); load_params(algo.actor_target, actor)
        load_params(algo.critic, c1 + c2); load_params(algo.critic_target, c1 + c2)
    return algo


def fixture(env):
    S, A = fx.ENVS[env]
    return (fx.make_net(NET_SEED + 1, fx.actor_dims(S, A)), fx.make_net(NET_SEED + 2, fx.critic_dims(S, A)),
            fx.make_net(NET_SEED + 3, fx.critic_dims(S, A)))


def oracle_for(env, algo, **kw):
    S, A = fx.ENVS[env]
    return TD3BCOracle(S, A, *fixture(env), bc_alpha=algo.bc_alpha, gamma=algo.gamma, tau=algo.tau,
                       policy_noise=algo.policy_noise, noise_clip=algo.noise_clip, policy_freq=algo.policy_freq, **kw)


def batches(env, B, n):
    S, A = fx.ENVS[env]
    return [(*fx.make_batch(100 + k, B, S, A), fx.make_noise(150 + k, (B, A))) for k in range(n)]


def step(algo, x):
    algo.update(*(v.cuda() for v in x[:5]), noise=x[5].cuda())


def got_and_want(algo, o, B):
    got, want = {}, {}
    for name in ("critic", "critic_target", "actor", "actor_target"):
        pair_nets(got, want, name, getattr(algo, name), getattr(o, name))
    pair_adam(got, want, algo, "critic", o.opt_critic)
    pair_adam(got, want, algo, "actor", o.opt_actor)
    pair_q_y(got, want, algo, B, o.last["q1"], o.last["y"])
    bc = algo.learner.read_bc()
    for k in ("bc_lambda", "q_abs_mean", "bc_mse"):
        got[f"u.{k}"], want[f"u.{k}"] = t.tensor([bc[k]]), o.last_actor[k].reshape(1)
    return as_np(got), as_np(want)


PARITY = [("walker", 256), ("walker", 100), ("cheetah", 256), ("cheetah", 100)]


@pytest.mark.parametrize("env,B", PARITY, ids=[f"{e}-B{b}" for e, b in PARITY])
def test_td3bc_matches_the_oracle(env, B):
    """Four updates with injected target noise (actor steps at updates 0 and 2): critics, actor, all targets, both
    optimizers' moments, the last update's q1 and y rows, and lambda, mean |Q1(s, pi)| and the cloning term of the last
    actor step within the suite's gates; the same oracle without the cloning term, or with lambda = 1, misses them by more
    than ten gates."""
    data = batches(env, B, 4)
    algo = make(env, B, fixture_nets=True)
    o = oracle_for(env, algo)
    wrong = {"no_bc": oracle_for(env, algo, no_bc=True), "no_lambda": oracle_for(env, algo, no_lambda=True)}
    run_pair(algo, [o, *wrong.values()], data, step)
    assert algo.learner.update_count == 4 and algo.learner.state_dict()["counters"][:3] == [4, 4, 2]
    got, want = got_and_want(algo, o, B)
    for k in ("bc_lambda", "q_abs_mean", "bc_mse"):
        print(f"{env} B={B}: {k} {got['u.' + k][0]:.6g} (oracle {want['u.' + k][0]:.6g})")
    worst = sc.compare(got, want, TOL, param_tol=sc.PARAM_TOL)
    print(f"{env} B={B}: worst key {worst[0]} rel dev {worst[1]:.2e}")
    scal = algo.learner.read_scalars()
    assert scal["actor_loss"] == pytest.approx(float(o.last_actor["actor_loss"]), rel=1e-4)       # TD3's meaning: -mean Q1(s, pi)
    assert scal["critic_loss"] == pytest.approx(float(o.last["critic_loss"]), rel=1e-4)
    for name, w in wrong.items():
        # (the parameter, target and moment keys only: lambda and the cloning term themselves, which a wrong oracle misses
        # trivially, do not count)
        r, _key = worst_ratio(*got_and_want(algo, w, B), TOL, params_only=True)
        print(f"{env} B={B}: {name} is {r:.0f} gates away")
        assert r >= 10.0, f"{name}: the learner is only {r:.1f} gates away from the wrong oracle"


# ---- bitwise links -----------------------------------------------------------------------------------------------------
def test_the_critic_step_of_update_0_is_plain_td3s():
    """The critic steps before the actor: after update 0 the critics, their moments and (Polyak of the stepped critics)
    their targets equal a plain no_fuse TD3's from the same nets, batch and noise, bit for bit; the actors do not."""
    env, B = "cheetah", 100
    bc, plain = make(env, B, fixture_nets=True), make(env, B, cls=TD3, fixture_nets=True)
    x = batches(env, B, 1)[0]
    step(bc, x)
    step(plain, x)
    assert_same_state(bc, plain, keys=("critic", "critic_m", "critic_v"), targets=(0,))
    assert not t.equal(bc.learner.actor_arena, plain.learner.actor_arena)


def test_with_the_mode_off_it_is_plain_td3_again():
    """After set_bc(0), further updates equal a plain no_fuse TD3 continued from the same state; turned on again, the
    mode is back."""
    env, B = "walker", 100
    data = batches(env, B, 6)
    bc, plain = make(env, B), make(env, B, cls=TD3)
    for x in data[:2]:
        step(bc, x)
    plain.load_state_dict(bc.state_dict())
    bc.learner.set_bc(0.0)
    for x in data[2:5]:
        step(bc, x)
        step(plain, x)
    assert_same_state(bc, plain)
    bc.learner.set_bc(2.5)
    step(bc, data[5])           # (update 5: critic only)
    step(plain, data[5])
    assert_same_state(bc, plain)
    step(bc, data[0])           # (update 6: an actor step)
    step(plain, data[0])
    t.cuda.synchronize()
    assert not t.equal(bc.learner.actor_arena, plain.learner.actor_arena)


RB, NSTEP = 64, 3


@pytest.mark.parametrize("nstep", [False, True], ids=["plain", "nstep3"])
def test_step_n_equals_sample_then_update_bitwise(nstep):
    """step_n(3) is bit for bit three sample() + update() pairs (the target noise drawn on the device in both), over a
    plain replay and over an n-step replay (n = 3)."""
    env = "cheetah"
    buf = random_replay(env, NSTEP if nstep else None, GAMMA)
    fused, loop, _ = check_step_n_equals_loop(lambda: (make(env, RB), make(env, RB)), buf, RB)
    assert fused.update_step == 6
    assert not t.equal(fused.learner.actor_arena, make(env, RB).learner.actor_arena)   # (it trained)
    assert fused.learner.read_bc() == loop.learner.read_bc() and fused.learner.read_bc()["bc_lambda"] > 0


def test_resume():
    """A checkpoint taken after three updates, loaded into a fresh learner, gives bit-identical state after three more."""
    env, B = "walker", 100
    a, _b, _sd = check_resume(lambda: make(env, B), step, batches(env, B, 6), 3)
    assert a.update_step == 6


def test_a_td3_learner_of_the_same_process_is_untouched():
    """A TD3 learner (fused, the default) stepped before and after a TD3BC learner was created and stepped ends with the
    parameters, targets and moments, bit for bit, of one stepped straight through."""
    env, B = "cheetah", 256
    data = batches(env, B, 4)
    straight, around = make(env, B, cls=TD3, no_fuse=False), make(env, B, cls=TD3, no_fuse=False)
    around.load_state_dict(straight.state_dict())
    for x in data:
        step(straight, x)
    for x in data[:2]:
        step(around, x)
    bc = make(env, B)
    for x in data[:2]:
        step(bc, x)
    t.cuda.synchronize()
    bc.learner.check()
    for x in data[2:]:
        step(around, x)
    assert_same_state(straight, around)


# ---- refusals ----------------------------------------------------------------------------------------------------------
def test_refusals():
    """Every case DESIGN.md §16 lists as refused returns its status with a message that names the reason; the update
    count and the Adam step counts stay where they were, and a refused learner goes on as what it was."""
    from oprl_amd.algos.ddpg import DDPG
    lib = _capi.load()
    env, B = "cheetah", 64
    S, A = fx.ENVS[env]
    x = batches(env, B, 1)[0]
    set_bc = lambda algo, alpha: lib.oprl_learner_set_bc(algo.learner.handle, C.c_double(alpha))   # noqa: E731

    # any algorithm but TD3
    ddpg = DDPG(logger=NullLogger(), state_dim=S, action_dim=A, max_batch=256, no_fuse=True).create()
    ddpg.update(*(v.cuda() for v in x[:5]))
    before = counters(ddpg)
    refused(set_bc(ddpg, 2.5), INVALID, b"DDPG")
    out = (C.c_float * 4)()
    refused(lib.oprl_learner_read_bc(ddpg.learner.handle, out, _capi.current_stream()), STATE, b"never on")
    assert counters(ddpg) == before
    # a precision other than f32 (said before the fused form is)
    for prec in ("bf16", "x2"):
        other = make(env, B, cls=TD3, no_fuse=False, precision=prec)
        refused(set_bc(other, 2.5), INVALID, b"f32")
    # a negative or non-finite alpha: the mode stays as it was, on with alpha = 2.5
    bc = make(env, B)
    step(bc, x)
    before, lam = counters(bc), bc.learner.read_bc()
    for alpha in (-1.0, float("nan"), float("inf"), float("-inf"), 1e300):
        refused(set_bc(bc, alpha), INVALID, b"alpha")
    assert counters(bc) == before and bc.learner.read_bc() == lam
    # a fused learner
    fused = make(env, B, cls=TD3, no_fuse=False)
    step(fused, x)
    before = counters(fused)
    assert fused.debug_form(B)["fused"] == 1
    refused(set_bc(fused, 2.5), STATE, b"no_fuse")
    assert counters(fused) == before
    # a gradient-exporting (data-parallel) learner
    exporting = make(env, B, cls=TD3, no_fuse=True, export_grads=True)
    refused(set_bc(exporting, 2.5), STATE, b"export_grads")
    # a member of a group
    members = [fused, make(env, B, cls=TD3, no_fuse=False)]
    handles = (C.c_void_p * 2)(*[m.learner.handle for m in members])
    g = C.c_void_p()
    _capi.check(lib.oprl_group_create(handles, 2, C.byref(g)), "oprl_group_create")
    refused(set_bc(fused, 2.5), STATE, b"group")
    assert counters(fused) == before
    lib.oprl_group_destroy(g)
    # oprl_group_create refuses a learner with the mode on
    handles = (C.c_void_p * 2)(bc.learner.handle, make(env, B).learner.handle)
    g = C.c_void_p()
    refused(lib.oprl_group_create(handles, 2, C.byref(g)), STATE, b"behaviour-cloning")
    assert not g.value
    # ... and after all that the BC learner steps as one that was never asked
    twin = make(env, B)
    step(twin, x)
    for algo in (bc, twin):
        step(algo, batches(env, B, 2)[1])
    assert_same_state(bc, twin)


def test_the_weighted_critic_step_is_orthogonal():
    """update_weighted with unit weights on a BC learner equals update(): the importance-weighted critic step and the BC
    actor branch do not meet (they share qpi one after the other)."""
    env, B = "walker", 100
    data = batches(env, B, 3)
    a, b = make(env, B), make(env, B)
    for x in data:
        step(a, x)
        b.update(*(v.cuda() for v in x[:5]), noise=x[5].cuda(), weights=t.ones(B, device="cuda"))
    assert_same_state(a, b)
    assert a.learner.read_bc() == b.learner.read_bc()
