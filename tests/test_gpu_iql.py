"""IQL on the MI355X learner against tests/iql_oracle.py (float64, written from the formulas of DESIGN.md §17): parity over
four updates at walker dims with B = 256 and the ragged B = 100, oracle variants that must miss, the bitwise links to a
plain no_fuse TD3 learner, step_n against sample() + update() over a plain and a 3-step replay, the offline trainer,
resume, every refusal, and no effect on a TD3 learner of the same process.

The parity runs start from fixture nets (oracle/fixtures.py make_net; V from seed + 4) with tau = 0.7, beta = 3 and the
clip lowered to c = 1.0: with these batches |u| stays below 0.4, so the default c = 100 would never bind.  Seed and clip
were fixed with the oracle alone, on the CPU, before any GPU run.  For net seed 400 the oracle's float32 run stays within
5.9e-6 (B = 256) and 7.8e-6 (B = 100) of its float64 run, max-norm per tensor over parameters, targets and moments of
actor, critics and V after these four updates — under a tenth of the parameter gate, so a miss here says something about
the kernels.  (Of the fourteen seeds 300, 310, ... 430 tried, 300, 370, 390 and 410 came to 4.5e-5 .. 9.1e-5 at one of the
two batch sizes and were passed over, as were those whose clip share left 10 % .. 90 % in some update.)  The share of rows
at the clip in the four updates is 0.63, 0.25, 0.21, 0.25 (B = 256) and 0.61, 0.22, 0.29, 0.33 (B = 100), and no row's
beta u comes nearer to log c than 3.1e-4, three orders above float32's rounding of it, so the count is the oracle's.
In the same runs the variant oracles end 0.78 / 1.68 (tau = 0.5), 0.21 / 0.14 (V(s') and u after the V step), 0.65 / 0.79
(no clip) and 0.20 / 0.28 (beta = 1) away in their worst key: more than a thousand gates."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest
import torch as t

from oprl_amd import _capi
from oprl_amd.algos.iql import IQL
from oprl_amd.algos.td3 import TD3
from oprl_amd.algos.td3_bc import TD3BC
from oprl_amd.logging import NullLogger
from oracle import fixtures as fx
from tests import scenarios as sc
from tests import support
from tests.hip_adapters import load_params, split_like
from tests.iql_oracle import IQLOracle
from tests.support import (INVALID, STATE, as_np, assert_same_state, check_resume, check_step_n_equals_loop, pair_adam, pair_nets,
                           pair_q_y, random_replay, refused, worst_ratio)

pytestmark = pytest.mark.gpu

TOL = 2e-5                          # network outputs (tests/test_gpu_algos.py)
NET_SEED = 400
CLIP = 1.0                          # (the parity runs: see the docstring)
GAMMA = 0.99
ENV = "walker"
V_KEYS = ("value", "value_m", "value_v")


def fixture():
    S, A = fx.ENVS[ENV]
    return (fx.make_net(NET_SEED + 1, fx.actor_dims(S, A)), fx.make_net(NET_SEED + 2, fx.critic_dims(S, A)),
            fx.make_net(NET_SEED + 3, fx.critic_dims(S, A)), fx.make_net(NET_SEED + 4, [S, 256, 256, 1]))


def make(B, cls=IQL, fixture_nets=False, env=ENV, **kw):
    S, A = fx.ENVS[env]
    t.manual_seed(0)
    if cls is not IQL:
        kw.setdefault("no_fuse", True)
        kw.setdefault("policy_freq", 1)
    algo = cls(logger=NullLogger(), state_dim=S, action_dim=A, max_batch=max(B, 256), log_every=10 ** 9, **kw).create()
    if fixture_nets:
        actor, c1, c2, v = fixture()
        load_params(algo.actor, actor); load_params(algo.actor_target, actor)
        load_params(algo.critic, c1 + c2); load_params(algo.critic_target, c1 + c2)
        load_params(algo.value, v)
    return algo


def oracle_for(algo, **kw):
    S, A = fx.ENVS[ENV]
    kw.setdefault("beta", algo.beta)
    return IQLOracle(S, A, *fixture(), expectile=algo.expectile, adv_clip=algo.adv_clip, gamma=algo.gamma, tau=algo.tau, **kw)


def batches(B, n, env=ENV):
    S, A = fx.ENVS[env]
    return [fx.make_batch(100 + k, B, S, A) for k in range(n)]


def step(algo, x):
    algo.update(*(v.cuda() for v in x[:5]))


def got_and_want(algo, o, B):
    """(everything but V, V's parameters and moments): the second pair falls under the parameter gate as a whole"""
    got, want, got_v, want_v = {}, {}, {}, {}
    for name in ("critic", "critic_target", "actor", "actor_target"):
        pair_nets(got, want, name, getattr(algo, name), getattr(o, name))
    pair_adam(got, want, algo, "critic", o.opt_critic)
    pair_adam(got, want, algo, "actor", o.opt_actor)
    L = algo.learner
    pair_nets(got_v, want_v, "value", algo.value, o.value)
    m, v = split_like(L.value_m, algo.value), split_like(L.value_v, algo.value)
    for l in range(len(m)):
        got_v[f"u.m_value.{l}"], want_v[f"u.m_value.{l}"] = m[l], o.opt_value.m[l]
        got_v[f"u.v_value.{l}"], want_v[f"u.v_value.{l}"] = v[l], o.opt_value.v[l]
    pair_q_y(got, want, algo, B, o.last["q1"], o.last["y"])
    return as_np(got), as_np(want), as_np(got_v), as_np(want_v)


def gates_away(got, want, got_v, want_v):
    """max over the parameter, target and moment keys, V's included (every V key is one), of (deviation / the parameter
    gate)"""
    return max(worst_ratio(got, want, TOL, params_only=True)[0], worst_ratio(got_v, want_v, sc.PARAM_TOL)[0])


@pytest.mark.parametrize("B", [256, 100], ids=["B256", "B100"])
def test_iql_matches_the_oracle(B):
    """Four updates: critics, actor, their targets, V, all three optimizers' moments and the last update's q1 and y rows
    within the suite's gates (outputs 2e-5; parameters, targets and moments 1e-4, V's among them); the losses and
    means read back agree with the oracle's; the clip binds on 10 % .. 90 % of the rows in every update; each variant
    oracle misses by more than ten gates."""
    data = batches(B, 4)
    algo = make(B, fixture_nets=True, adv_clip=CLIP)
    assert (algo.expectile, algo.beta, algo.policy_freq, algo.no_fuse) == (0.7, 3.0, 1, True)
    o = oracle_for(algo)
    wrong = {"tau = 0.5": oracle_for(algo, sym=True), "late": oracle_for(algo, late=True),
             "no clip": oracle_for(algo, no_clip=True), "beta = 1": oracle_for(algo, beta=1.0)}
    for k, x in enumerate(data):
        step(algo, x)
        for p in (o, *wrong.values()):
            p.update(*x)
        q = algo.learner.read_iql()
        frac = float(o.last["clip_frac"])
        print(f"B={B} update {k}: at the clip {q['clip_frac']:.4f} (oracle {frac:.4f}), V loss {q['v_loss']:.6g} "
              f"(oracle {float(o.last['v_loss']):.6g}), max |u| {float(o.last['u'].abs().max()):.3f}")
        assert 0.1 <= frac <= 0.9
        assert round(q["clip_frac"] * B) == round(frac * B)                 # the count of rows at the clip is exact
    t.cuda.synchronize()
    algo.learner.check()
    assert algo.learner.update_count == 4 and algo.learner.state_dict()["counters"][:3] == [4, 4, 4]
    assert algo.learner.value_step == 4
    got, want, got_v, want_v = got_and_want(algo, o, B)
    worst = sc.compare(got, want, TOL, param_tol=sc.PARAM_TOL)
    worst_v = sc.compare(got_v, want_v, sc.PARAM_TOL)
    print(f"B={B}: worst key {worst[0]} rel dev {worst[1]:.2e}; worst V key {worst_v[0]} rel dev {worst_v[1]:.2e}")
    q, scal = algo.learner.read_iql(), algo.learner.read_scalars()
    for k in ("v_loss", "v_mean", "adv_mean", "w_mean", "actor_loss"):
        print(f"B={B}: {k} {q[k]:.6g} (oracle {float(o.last[k]):.6g})")
    assert q["v_loss"] == pytest.approx(float(o.last["v_loss"]), rel=1e-4)
    assert q["actor_loss"] == pytest.approx(float(o.last["actor_loss"]), rel=1e-4)
    assert q["w_mean"] == pytest.approx(float(o.last["w_mean"]), rel=1e-4)
    assert scal["actor_loss"] == pytest.approx(float(o.last["actor_loss"]), rel=1e-4)      # in this mode: the weighted cloning loss
    assert scal["critic_loss"] == pytest.approx(float(o.last["critic_loss"]), rel=1e-4)
    # (means of rows of both signs: the output gate on the rows they average, 2e-5 of the largest)
    assert abs(q["v_mean"] - float(o.last["v_mean"])) <= TOL * float(o.last["v"].abs().max())
    assert abs(q["adv_mean"] - float(o.last["adv_mean"])) <= TOL * max(float(o.last["u"].abs().max()), float(o.last["v"].abs().max()))
    for name, w in wrong.items():
        r = gates_away(*got_and_want(algo, w, B))
        print(f"B={B}: {name} is {r:.0f} gates away")
        assert r >= 10.0, f"{name}: the learner is only {r:.1f} gates away from the wrong oracle"


# ---- bitwise links -----------------------------------------------------------------------------------------------------
WITH_V = dict(extra=V_KEYS + ("value_step",))            # V, its moments and its step count ride along


def test_with_the_mode_off_it_is_plain_td3_again():
    """After set_iql(None), two further updates equal a plain no_fuse TD3 (policy_freq 1) continued from the same state,
    V and its step count stay where they were, and turned on again the mode is back."""
    B = 100
    data = batches(B, 5)
    iql, plain = make(B), make(B, cls=TD3)
    for x in data[:2]:
        step(iql, x)
    sd = iql.state_dict()
    plain.load_state_dict(sd)
    value = iql.value
    iql.learner.set_iql(None)
    assert "value" not in iql.state_dict()
    for x in data[2:4]:
        step(iql, x)
        step(plain, x)
    assert_same_state(iql, plain)
    assert t.equal(value._oprl_arena.cpu(), sd["value"])
    iql.learner.set_iql(value, iql.expectile, iql.beta, iql.adv_clip, iql.lr_value)
    assert iql.learner.value_step == 2
    step(iql, data[4])
    step(plain, data[4])
    t.cuda.synchronize()
    assert iql.learner.value_step == 3 and not t.equal(value._oprl_arena.cpu(), sd["value"])
    assert not t.equal(iql.learner.actor_arena, plain.learner.actor_arena)


def test_a_td3_learner_of_the_same_process_is_untouched():
    """A TD3 learner (fused, the default) stepped before and after an IQL learner was created and stepped ends with the
    parameters, targets and moments, bit for bit, of one stepped straight through."""
    B = 256
    data = batches(B, 4)
    noise = [fx.make_noise(150 + k, (B, fx.ENVS[ENV][1])) for k in range(4)]
    td3_step = lambda algo, k: algo.update(*(v.cuda() for v in data[k]), noise=noise[k].cuda())    # noqa: E731
    straight, around = make(B, cls=TD3, no_fuse=False, policy_freq=2), make(B, cls=TD3, no_fuse=False, policy_freq=2)
    around.load_state_dict(straight.state_dict())
    for k in range(4):
        td3_step(straight, k)
    for k in range(2):
        td3_step(around, k)
    iql = make(B)
    for x in data[:2]:
        step(iql, x)
    t.cuda.synchronize()
    iql.learner.check()
    for k in range(2, 4):
        td3_step(around, k)
    assert_same_state(straight, around)


RB, NSTEP = 64, 3


@pytest.mark.parametrize("nstep", [False, True], ids=["plain", "nstep3"])
def test_step_n_equals_sample_then_update_bitwise(nstep):
    """step_n(3) is bit for bit three sample() + update() pairs, over a plain replay and over an n-step replay (n = 3),
    V, its moments and its step count included."""
    buf = random_replay(ENV, NSTEP if nstep else None, GAMMA)
    fused, loop, _ = check_step_n_equals_loop(lambda: (make(RB), make(RB)), buf, RB, **WITH_V)
    assert fused.update_step == 6 and fused.learner.value_step == 6
    fresh = make(RB).state_dict()
    assert not t.equal(fused.learner.actor_arena.cpu(), fresh["actor"]) and not t.equal(fused.state_dict()["value"], fresh["value"])
    assert fused.learner.read_iql() == loop.learner.read_iql() and fused.learner.read_iql()["w_mean"] > 0


def test_the_offline_trainer_equals_sample_and_update_pairs_bitwise():
    """A small dataset rolled from the synthetic environment, fill_replay'd into an HBM replay: OfflineTrainer over an
    IQL learner (one step_n(16) per call) against 32 sample() + update() pairs from the same start."""
    from oprl_amd.buffers.episodic_buffer import EpisodicReplayBuffer
    from oprl_amd.buffers.offline_dataset import OfflineData, fill_replay
    from oprl_amd.environment.synthetic import SyntheticEnv
    from oprl_amd.trainers.offline_trainer import OfflineTrainer
    episodes, steps, B = 4, 40, 64
    make_env = lambda seed: SyntheticEnv("cheetah-run", seed=seed, episode_length=steps)     # noqa: E731
    env = make_env(3)
    cols = [[] for _ in range(6)]
    for _ in range(episodes):
        obs, _ = env.reset()
        over = False
        while not over:
            a = env.sample_action()
            nxt, r, term, trunc, _ = env.step(a)
            for c, v in zip(cols, (obs, a, r, term, trunc, nxt)):
                c.append(v)
            obs, over = nxt, term or trunc
    o, a, r, term, tout, nxt = cols
    data = OfflineData(np.asarray(o, np.float32), np.asarray(a, np.float32), np.asarray(r, np.float32), np.asarray(term, bool),
                       np.asarray(tout, bool), np.asarray(nxt, np.float32))
    S, A = data.observations.shape[1], data.actions.shape[1]
    buf = EpisodicReplayBuffer(buffer_size_transitions=(episodes + 1) * steps, state_dim=S, action_dim=A,
                               max_episode_lenth=steps, device="cuda", seed=11).create()
    norm = fill_replay(buf, data)

    def learner():
        t.manual_seed(0)
        return IQL(logger=NullLogger(), state_dim=S, action_dim=A, max_batch=256, log_every=10 ** 9).create()
    algo, loop = learner(), learner()
    loop.load_state_dict(algo.state_dict())
    OfflineTrainer(logger=NullLogger(), make_env_test=make_env, replay_buffer=buf, algo=algo, obs_norm=norm, num_updates=32,
                   updates_per_call=16, batch_size=B, eval_interval=0, save_policy_every=0, stdout_log_every=0,
                   num_eval_episodes=1, seed=5).train()
    assert algo.update_step == 32
    for _ in range(32):
        buf._sample_counter = loop.update_step
        loop.update(*buf.sample(B))
    assert_same_state(algo, loop, **WITH_V)
    assert algo.state_dict()["counters"][:3] == [32, 32, 32] and algo.learner.value_step == 32
    assert algo.learner.read_iql() == loop.learner.read_iql()
    assert not t.equal(algo.state_dict()["actor"], learner().state_dict()["actor"])


def test_resume():
    """A checkpoint taken after two updates, loaded into a fresh learner, gives bit-identical state after two more — V,
    its moments and its step count included; a checkpoint without them is refused by name."""
    B = 100

    def partial_checkpoint_is_refused(b, sd):
        assert sd["value_step"] == 2 and all(k in sd for k in V_KEYS)
        with pytest.raises(ValueError, match="value_m"):
            b.load_state_dict({k: v for k, v in sd.items() if k != "value_m"})

    a, _b, sd = check_resume(lambda: make(B), step, batches(B, 4), 2, before_load=partial_checkpoint_is_refused, **WITH_V)
    assert a.update_step == 4
    assert not t.equal(a.state_dict()["value"], sd["value"])


# ---- refusals ----------------------------------------------------------------------------------------------------------
def counters(algo):
    return support.counters(algo, "value_step")


class ValueNet:
    """A value net of the caller's with its moments, and the descriptor oprl_learner_set_iql takes."""

    def __init__(self, dims, moments=True, pack=True):
        from oprl_amd.algos.nn_models import MLP, flatten_module_
        self.mlp = MLP(dims[0], dims[-1], tuple(dims[1:-1]), t.nn.ReLU(inplace=True)).cuda()
        flatten_module_(self.mlp)
        self.m, self.v = t.zeros_like(self.mlp._oprl_arena), t.zeros_like(self.mlp._oprl_arena)
        d = _capi.OprlNet()
        d.n_layers = len(dims) - 1
        for i, x in enumerate(dims):
            d.dims[i] = x
        d.theta = self.mlp.theta_ptr()
        d.pack = self.mlp.pack_tensor().data_ptr() if pack else None
        d.adam_m, d.adam_v = (self.m.data_ptr(), self.v.data_ptr()) if moments else (None, None)
        self.desc = d


def test_refusals():
    """Every case DESIGN.md §17 lists as refused returns its status with a message that names the reason; the update
    count and all Adam step counts, V's included, stay where they were, and a refused learner goes on as what it was."""
    from oprl_amd.algos.ddpg import DDPG
    from oprl_amd.buffers.episodic_buffer import EpisodicReplayBuffer
    lib = _capi.load()
    B = 64
    S, A = fx.ENVS[ENV]
    x = batches(B, 2)
    good = ValueNet([S, 256, 256, 1])

    def set_iql(algo, net=good, tau=0.7, beta=3.0, clip=100.0, lr=3e-4):
        return lib.oprl_learner_set_iql(algo.learner.handle, C.byref(net.desc), C.c_double(tau), C.c_double(beta),
                                        C.c_double(clip), C.c_double(lr))

    # any algorithm but TD3
    ddpg = DDPG(logger=NullLogger(), state_dim=S, action_dim=A, max_batch=256, no_fuse=True).create()
    ddpg.update(*(v.cuda() for v in x[0]))
    before = counters(ddpg)
    refused(set_iql(ddpg), INVALID, b"TD3")
    out = (C.c_float * 8)()
    refused(lib.oprl_learner_read_iql(ddpg.learner.handle, out, _capi.current_stream()), STATE, b"never on")
    assert counters(ddpg) == before
    # a precision other than f32 (said before the fused form is)
    for prec in ("bf16", "x2"):
        refused(set_iql(make(B, cls=TD3, no_fuse=False, precision=prec)), INVALID, b"f32")
    # policy_freq != 1
    refused(set_iql(make(B, cls=TD3, policy_freq=2)), INVALID, b"policy_freq")
    # hyper-parameters and value nets, on a learner whose mode is on and stays as it was
    iql, twin = make(B), make(B)
    twin.load_state_dict(iql.state_dict())
    step(iql, x[0])
    step(twin, x[0])
    before = counters(iql)
    nan, inf = float("nan"), float("inf")
    for kw, word in [(dict(tau=v), b"expectile") for v in (0.0, 1.0, -0.1, 1.5, nan, inf)] + \
                    [(dict(beta=v), b"beta") for v in (-1.0, nan, inf, 1e300)] + \
                    [(dict(clip=v), b"adv_clip") for v in (0.0, -1.0, nan, inf, 1e300)] + \
                    [(dict(lr=v), b"lr_value") for v in (0.0, -1e-3, nan, inf)]:
        refused(set_iql(iql, **kw), INVALID, word)
    for net, word in ((ValueNet([S + 1, 256, 256, 1]), b"state_dim"), (ValueNet([S, 256, 256, 2]), b"one output"),
                      (ValueNet([S, 1]), b"n_layers"), (ValueNet([S, 128, 128, 1]), b"width"),
                      (ValueNet([S, 256, 512, 1]), b"widths"), (ValueNet([S, 256, 256, 1], moments=False), b"moments"),
                      (ValueNet([S, 256, 256, 1], pack=False), b"pack")):
        refused(set_iql(iql, net=net), INVALID, word)
    # ... set_bc, a group, importance weights: refused while the mode is on
    refused(lib.oprl_learner_set_bc(iql.learner.handle, C.c_double(2.5)), STATE, b"implicit-Q-learning")
    handles = (C.c_void_p * 2)(iql.learner.handle, make(B).learner.handle)
    g = C.c_void_p()
    refused(lib.oprl_group_create(handles, 2, C.byref(g)), STATE, b"implicit-Q-learning")
    assert not g.value
    dev = [v.cuda().contiguous() for v in x[1]]
    w, td = t.ones(B, device="cuda"), t.zeros(B, device="cuda")
    refused(lib.oprl_learner_update_weighted(iql.learner.handle, *(_capi.ptr(v) for v in dev), _capi.ptr(w), B, None, None,
                                             _capi.ptr(td), _capi.current_stream()), STATE, b"importance weights")
    buf = EpisodicReplayBuffer(buffer_size_transitions=4 * 30, state_dim=S, action_dim=A, max_episode_lenth=30, device="cuda").create()
    refused(lib.oprl_learner_step_n_prio(iql.learner.handle, buf.handle, 1, B, 0, C.c_double(0.4), C.c_double(100.0),
                                         _capi.current_stream()), STATE, b"importance weights")
    assert counters(iql) == before
    # ... and after all that the learner steps as one that was never asked
    step(iql, x[1])
    step(twin, x[1])
    assert_same_state(iql, twin, **WITH_V)
    # a fused learner
    fused = make(B, cls=TD3, no_fuse=False)
    step(fused, x[0])
    before = counters(fused)
    assert fused.debug_form(B)["fused"] == 1
    refused(set_iql(fused), STATE, b"no_fuse")
    assert counters(fused) == before
    # a gradient-exporting (data-parallel) learner
    refused(set_iql(make(B, cls=TD3, export_grads=True)), STATE, b"export_grads")
    # a learner with the behaviour-cloning mode on
    bc = make(B, cls=TD3BC)
    refused(set_iql(bc), STATE, b"behaviour-cloning")
    assert bc.learner.read_bc is not None and counters(bc)[:4] == [0, 0, 0, 0]
    # a member of a group
    members = [fused, make(B, cls=TD3, no_fuse=False)]
    handles = (C.c_void_p * 2)(*[m.learner.handle for m in members])
    g = C.c_void_p()
    _capi.check(lib.oprl_group_create(handles, 2, C.byref(g)), "oprl_group_create")
    refused(set_iql(fused), STATE, b"group")
    assert counters(fused) == before
    lib.oprl_group_destroy(g)
