"""CQL on the MI355X learner against tests/cql_oracle.py (float64, written from the formulas of DESIGN.md §19): parity over
four updates at walker dims with supplied draws at the ragged B = 100, N = 2 (700 wide rows) and at B = 16, N = 16 (784 wide
rows: one data slice, the widest entry count), with the temperature fixed and learned; oracle variants that must miss; the
bitwise links to a plain no_fuse SAC learner, step_n against sample() + update() over a plain and a 3-step replay, the
offline trainer, resume, no effect on a fused SAC learner of the same process; and every refusal.

The parity runs start from fixture nets (oracle/fixtures.py make_net, seed 600 + 1 .. 3) with cql_alpha = 5.0, the class's
default.  Both were fixed with the oracle alone, on the CPU, before any GPU run — the first pair tried.  With them the
oracle's float32 run stays within 1.13e-5 (B = 100, N = 2) and 2.4e-6 (B = 16, N = 16) of its float64 run, max-norm per
tensor over parameters, targets, moments and log_alpha after these four updates, and within 8.0e-7 / 8.9e-7 on the last
update's q1 and y rows: under half of the parameter gate 1e-4 and of the output gate 2e-5, so a miss here says something
about the kernels.  In the same runs the variant oracles end, in their worst critic key, 373 / 370 gates (cql_alpha = 0),
277 / 289 (no log-density correction), 356 / 356 (the third kind evaluated at s') and 21 / 73 (seeds scaled by 1/Bw) away."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest
import torch as t

from oprl_amd import _capi
from oprl_amd.algos.cql import CQL
from oprl_amd.algos.sac import SAC
from oprl_amd.logging import NullLogger
from oracle import fixtures as fx
from tests import cql_oracle as co
from tests import scenarios as sc
from tests import support
from tests.hip_adapters import cpu_params, hip_adam, load_params
from tests.support import INVALID, STATE, check_resume, check_step_n_equals_loop, counters, random_replay, refused  # noqa: F401

pytestmark = pytest.mark.gpu

TOL = 2e-5                          # network outputs (tests/test_gpu_algos.py)
GAMMA = 0.99
ENV = co.ENV
NSTEP = 3


def make(B, N=2, cls=CQL, fixture_nets=False, env=ENV, **kw):
    S, A = fx.ENVS[env]
    t.manual_seed(0)
    if cls is CQL:
        kw.setdefault("cql_n_actions", N)
        kw.setdefault("cql_alpha", co.CQL_ALPHA)
    else:
        kw.setdefault("no_fuse", True)
    algo = cls(logger=NullLogger(), state_dim=S, action_dim=A, batch_size=B, log_every=10 ** 9, **kw).create()
    if fixture_nets:
        actor, c1, c2 = co.fixture_nets()
        load_params(algo.actor, actor)
        load_params(algo.critic, c1 + c2); load_params(algo.critic_target, c1 + c2)
    return algo


def step(algo, item):
    """One update with every draw supplied."""
    batch, en, ec, eps, uni = item
    algo.learner.set_cql_noise(eps, uni)
    algo.update(*(v.cuda() for v in batch), noise=(en.cuda(), ec.cuda()))


def plain_step(algo, batch):
    algo.update(*(v.cuda() for v in batch))


def batches(B, n, env=ENV):
    S, A = fx.ENVS[env]
    return [fx.make_batch(100 + k, B, S, A) for k in range(n)]


def learner_state(algo, B):
    got = {}
    for name, mod in (("critic", algo.critic), ("critic_target", algo.critic_target), ("actor", algo.actor)):
        for l, x in enumerate(cpu_params(mod)):
            got[f"u.{name}.{l}"] = x
    for which in ("critic", "actor"):
        m, v = hip_adam(algo, which)
        for l in range(len(m)):
            got[f"u.m_{which}.{l}"], got[f"u.v_{which}.{l}"] = m[l], v[l]
    if algo.tune_alpha:
        got["u.critic.log_alpha"] = algo.log_alpha.detach().cpu().reshape(1)
    q, y = algo.learner.debug_q_y(B)
    got["u.q"], got["u.y"] = q.cpu(), y.cpu()
    return {k: np.asarray(v.detach().cpu().double().numpy()) for k, v in got.items()}


def oracle_state(o):
    want = co.oracle_state(o)
    want["u.q"], want["u.y"] = o.last["q1"].reshape(-1).double().numpy(), o.last["y"].reshape(-1).double().numpy()
    return want


def critic_gates(got, want):
    """max over the critics' parameter and target keys of (deviation / the parameter gate)"""
    return max(sc.rel_dev(got[k], v) / sc.PARAM_TOL for k, v in want.items() if ".critic." in k or ".critic_target." in k)


@pytest.mark.parametrize("tune", [False, True], ids=["alpha-fixed", "alpha-tuned"])
@pytest.mark.parametrize("B,N", co.SHAPES, ids=[f"B{b}-N{n}" for b, n in co.SHAPES])
def test_cql_matches_the_oracle(B, N, tune):
    """Four updates: critics, actor, the critics' targets, both optimizers' moments, log_alpha and the last update's q1 and
    y rows within the suite's gates (outputs 2e-5; parameters, targets, moments and log_alpha 1e-4); what read_cql and
    read_scalars give agrees with the oracle's; each variant oracle misses by more than ten gates."""
    S, A = fx.ENVS[ENV]
    data = co.parity_data(B, N)
    algo = make(B, N, fixture_nets=True, tune_alpha=tune)
    assert (algo.cql_alpha, algo.cql_n_actions, algo.no_fuse) == (co.CQL_ALPHA, N, True)
    mk = lambda ca=co.CQL_ALPHA, **kw: co.CQLOracle(S, A, *co.fixture_nets(), cql_alpha=ca, n_actions=N, tune_alpha=tune,    # noqa: E731
                                                    gamma=algo.gamma, tau=algo.target_update_coef, alpha_init=algo.alpha_init, **kw)
    o = mk()
    wrong = {"cql_alpha = 0": mk(0.0), "no log-density": mk(no_logd=True), "third kind at s'": mk(at_next=True),
             "seeds / Bw": mk(scale_bw=True)}
    for item in data:
        step(algo, item)
        for p in (o, *wrong.values()):
            p.update(*item[0], *item[1:])
    t.cuda.synchronize()
    algo.learner.check()
    assert algo.learner.update_count == 4 and algo.learner.state_dict()["counters"] == [4, 4, 4, 4 if tune else 0]
    got, want = learner_state(algo, B), oracle_state(o)
    worst = sc.compare(got, want, TOL, param_tol=sc.PARAM_TOL)
    print(f"B={B} N={N} tune={tune}: worst key {worst[0]} rel dev {worst[1]:.2e}")
    q, scal = algo.learner.read_cql(), algo.learner.read_scalars()
    for k in ("gap1", "gap2", "q_rand1", "q_rand2", "q_pi1", "q_pi2", "penalty"):
        print(f"B={B} N={N}: {k} {q[k]:.6g} (oracle {float(o.last[k]):.6g})")
        assert q[k] == pytest.approx(float(o.last[k]), rel=1e-4)
    assert scal["critic_loss"] == pytest.approx(float(o.last["critic_loss"]), rel=1e-4)
    assert scal["q1_mean"] == pytest.approx(float(o.last["q1"].mean()), rel=1e-4)
    assert scal["q_target_mean"] == pytest.approx(float(o.last["y"].mean()), rel=1e-4)
    for name, w in wrong.items():
        r = critic_gates(got, oracle_state(w))
        print(f"B={B} N={N}: {name} is {r:.0f} gates away")
        assert r >= 10.0, f"{name}: the learner is only {r:.1f} gates away from the wrong oracle"


# ---- bitwise links -----------------------------------------------------------------------------------------------------
def assert_same_state(a, b, **kw):       # kept: the shared check plus SAC's "exactly one target list" at this call site
    assert len(a.state_dict()["targets"]) == 1          # (SAC: the critics' targets; the actor has none)
    support.assert_same_state(a, b, **kw)


@pytest.mark.parametrize("tune", [False, True], ids=["alpha-fixed", "alpha-tuned"])
def test_with_the_mode_off_it_is_plain_sac_again(tune):
    """After set_cql(..., 0), two further updates (Philox draws) equal a plain no_fuse SAC continued from the same state;
    turned on again the penalty is back."""
    B = 100
    data = batches(B, 5)
    cql, plain = make(B, tune_alpha=tune), make(B, cls=SAC, tune_alpha=tune)
    for x in data[:2]:
        plain_step(cql, x)
    plain.load_state_dict(cql.state_dict())
    cql.learner.set_cql(cql.cql_alpha, 0)
    for x in data[2:4]:
        plain_step(cql, x)
        plain_step(plain, x)
    assert_same_state(cql, plain)
    cql.learner.set_cql(cql.cql_alpha, cql.cql_n_actions)
    plain_step(cql, data[4])
    plain_step(plain, data[4])
    t.cuda.synchronize()
    assert not t.equal(cql.learner.critic_arena, plain.learner.critic_arena)
    assert cql.learner.read_cql()["gap1"] != 0


def test_a_fused_sac_learner_of_the_same_process_is_untouched():
    """A SAC learner (fused, the default) stepped before and after a CQL learner was created and stepped ends with the
    parameters, targets and moments, bit for bit, of one stepped straight through."""
    B = 256
    data = batches(B, 4)
    A = fx.ENVS[ENV][1]
    noise = [(fx.make_noise(150 + k, (B, A)), fx.make_noise(160 + k, (B, A))) for k in range(4)]
    sac_step = lambda algo, k: algo.update(*(v.cuda() for v in data[k]), noise=tuple(n.cuda() for n in noise[k]))    # noqa: E731
    straight, around = make(B, cls=SAC, no_fuse=False), make(B, cls=SAC, no_fuse=False)
    assert straight.debug_form(B)["fused"] == 1
    around.load_state_dict(straight.state_dict())
    for k in range(4):
        sac_step(straight, k)
    for k in range(2):
        sac_step(around, k)
    cql = make(64)
    for x in batches(64, 2):
        plain_step(cql, x)
    t.cuda.synchronize()
    cql.learner.check()
    for k in range(2, 4):
        sac_step(around, k)
    assert_same_state(straight, around)


RB = 64


def replay(nstep):
    return random_replay(ENV, NSTEP if nstep else None, GAMMA)


@pytest.mark.parametrize("nstep", [False, True], ids=["plain", "nstep3"])
def test_step_n_equals_sample_then_update_bitwise(nstep):
    """step_n(3) is bit for bit three sample() + update() pairs (Philox draws at the same counters), over a plain replay
    and over an n-step replay (n = 3)."""
    buf = replay(nstep)
    fused, loop, _ = check_step_n_equals_loop(lambda: (make(RB, tune_alpha=True), make(RB, tune_alpha=True)), buf, RB)
    assert fused.update_step == 6 and len(fused.state_dict()["targets"]) == 1
    assert not t.equal(fused.learner.critic_arena.cpu(), make(RB, tune_alpha=True).state_dict()["critic"])
    assert fused.learner.read_cql() == loop.learner.read_cql() and fused.learner.read_cql()["gap1"] != 0


def test_the_offline_trainer_equals_sample_and_update_pairs_bitwise():
    """A small dataset rolled from the synthetic environment, fill_replay'd into an HBM replay: OfflineTrainer over a
    CQL learner (one step_n(16) per call) against 32 sample() + update() pairs from the same start."""
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
        return CQL(logger=NullLogger(), state_dim=S, action_dim=A, batch_size=B, cql_n_actions=2, log_every=10 ** 9).create()
    algo, loop = learner(), learner()
    loop.load_state_dict(algo.state_dict())
    OfflineTrainer(logger=NullLogger(), make_env_test=make_env, replay_buffer=buf, algo=algo, obs_norm=norm, num_updates=32,
                   updates_per_call=16, batch_size=B, eval_interval=0, save_policy_every=0, stdout_log_every=0,
                   num_eval_episodes=1, seed=5).train()
    assert algo.update_step == 32
    for _ in range(32):
        buf._sample_counter = loop.update_step
        loop.update(*buf.sample(B))
    assert_same_state(algo, loop)
    assert algo.state_dict()["counters"][:2] == [32, 32]
    assert algo.learner.read_cql() == loop.learner.read_cql()
    assert not t.equal(algo.state_dict()["critic"], learner().state_dict()["critic"])


def test_resume():
    """A checkpoint taken after two updates, loaded into a fresh learner, gives bit-identical state after two more: the
    mode has no state of its own."""
    B = 100
    a, _b, sd = check_resume(lambda: make(B, tune_alpha=True), plain_step, batches(B, 4), 2)
    assert a.update_step == 4 and len(sd["targets"]) == 1
    assert not t.equal(a.state_dict()["critic"], sd["critic"])


# ---- refusals ----------------------------------------------------------------------------------------------------------
def test_refusals():
    """Every case DESIGN.md §19 lists as refused returns its status with a message that names the reason; the update
    count and all Adam step counts stay where they were, and a refused learner goes on as what it was."""
    from oprl_amd.algos.td3 import TD3
    from oprl_amd.buffers.episodic_buffer import EpisodicReplayBuffer
    lib = _capi.load()
    B = 64
    S, A = fx.ENVS[ENV]
    x = batches(B, 2)
    set_cql = lambda algo, ca=5.0, n=2: lib.oprl_learner_set_cql(algo.learner.handle, C.c_double(ca), n)     # noqa: E731
    # a learner that is not SAC
    td3 = TD3(logger=NullLogger(), state_dim=S, action_dim=A, max_batch=256, no_fuse=True).create()
    plain_step(td3, x[0])
    before = counters(td3)
    refused(set_cql(td3), INVALID, b"SAC")
    out = (C.c_float * 8)()
    refused(lib.oprl_learner_read_cql(td3.learner.handle, out, _capi.current_stream()), STATE, b"never on")
    assert counters(td3) == before
    # a precision other than f32 (said before the fused form is)
    for prec in ("bf16", "x2"):
        refused(set_cql(make(B, cls=SAC, no_fuse=False, precision=prec)), INVALID, b"f32")
    # hyper-parameters, on a learner whose mode is on and stays as it was
    cql, twin = make(B), make(B)
    twin.load_state_dict(cql.state_dict())
    plain_step(cql, x[0])
    plain_step(twin, x[0])
    before = counters(cql)
    for ca in (-1.0, float("nan"), float("inf"), 1e300):
        refused(set_cql(cql, ca=ca), INVALID, b"cql_alpha")
    for n in (-1, 17, 100):
        refused(set_cql(cql, n=n), INVALID, b"n_actions")
    # ... importance weights: refused while the mode is on
    dev = [v.cuda().contiguous() for v in x[1]]
    w, td = t.ones(B, device="cuda"), t.zeros(B, device="cuda")
    refused(lib.oprl_learner_update_weighted(cql.learner.handle, *(_capi.ptr(v) for v in dev), _capi.ptr(w), B, None, None,
                                             _capi.ptr(td), _capi.current_stream()), STATE, b"importance weights")
    buf = EpisodicReplayBuffer(buffer_size_transitions=4 * 30, state_dim=S, action_dim=A, max_episode_lenth=30, device="cuda").create()
    refused(lib.oprl_learner_step_n_prio(cql.learner.handle, buf.handle, 1, B, 0, C.c_double(0.4), C.c_double(100.0),
                                         _capi.current_stream()), STATE, b"importance weights")
    assert counters(cql) == before
    # ... and after all that the learner steps as one that was never asked
    plain_step(cql, x[1])
    plain_step(twin, x[1])
    assert_same_state(cql, twin)
    # more wide rows than the workspace holds, at update time: update and step_n
    small = make(B, N=2, max_batch=7 * B)            # (create() sizes max_batch for batch_size (1 + 3 N) = 448 rows)
    assert small.max_batch == 448
    plain_step(small, x[0])
    before = counters(small)
    _capi.check(set_cql(small, n=3), "oprl_learner_set_cql")          # 64 x 10 = 640 rows
    refused(lib.oprl_learner_update(small.learner.handle, *(_capi.ptr(v) for v in dev), B, None, None, _capi.current_stream()),
            INVALID, b"max_batch=448")
    refused(lib.oprl_learner_step_n(small.learner.handle, buf.handle, 1, B, 0, _capi.current_stream()), INVALID, b"max_batch=448")
    assert counters(small) == before
    _capi.check(set_cql(small, n=2), "oprl_learner_set_cql")
    plain_step(small, x[1])
    assert counters(small)[0] == before[0] + 1
    # a fused learner
    fused = make(B, cls=SAC, no_fuse=False, max_batch=256)      # (a group's members: clusters of four for every slice of max_batch)
    plain_step(fused, x[0])
    before = counters(fused)
    assert fused.debug_form(B)["fused"] == 1
    refused(set_cql(fused), STATE, b"no_fuse")
    assert counters(fused) == before
    # a gradient-exporting (data-parallel) learner
    refused(set_cql(make(B, cls=SAC, export_grads=True)), STATE, b"export_grads")
    # a member of a group
    members = [fused, make(B, cls=SAC, no_fuse=False, max_batch=256)]
    handles = (C.c_void_p * 2)(*[m.learner.handle for m in members])
    g = C.c_void_p()
    _capi.check(lib.oprl_group_create(handles, 2, C.byref(g)), "oprl_group_create")
    refused(set_cql(fused), STATE, b"group")
    assert counters(fused) == before
    lib.oprl_group_destroy(g)
