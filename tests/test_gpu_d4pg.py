"""D4PG on the MI355X learner against tests/d4pg_oracle.py (float64, autograd, written from the spec of DESIGN.md §15):
parity over four updates, oracle variants that must miss, step_n against sample() + update() over a plain and an n-step
replay, resume, every refusal, and no effect on a DDPG learner of the same process.

The atoms of the parity runs come from the fixture's reward scale: oracle/fixtures.py draws r uniform in [0, 1) and
gamma is 0.99, so returns lie in [0, 100); the support [20, 60] sits inside that range on purpose, so that one batch has
rows whose atoms are clamped at the lower end (d = 0, r < (1 - gamma) v_min = 0.2), at the upper end (d = 0,
r > (1 - gamma) v_max = 0.6), at neither (0.2 <= r <= 0.6), and terminal rows (d = 1: every atom lands on r < v_min).
The replay-driven tests store N(0, 1) rewards and use the support [-5, 5].

The parity runs start from fixture nets (oracle/fixtures.py make_net, as the DDPG / TD3 / SAC scenarios do), not from
create()'s own initialisation: that zeroes the actor's biases, and a parameter key is gated relative to its largest
entry — four Adam steps from zero leave a bias key 1e-3 across, and 1e-4 of that is 0.04 % of one Adam step, which no
float32 run reproduces.  The nets' seed was fixed with the oracle alone: its float32 run on the CPU stays within about a
third of the parameter gate of its float64 run at all four parity shapes (Adam turns float32 summation noise in a small
gradient element into a few percent of a step: tests/scenarios.py compare), so a miss here says something about the
kernels."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest
import torch as t

from oprl_amd import _capi
from oprl_amd.algos.d4pg import D4PG
from oprl_amd.logging import NullLogger
from oracle import fixtures as fx
from tests import nstep_oracle as no
from tests import scenarios as sc
from tests.d4pg_oracle import D4PGOracle
from tests.hip_adapters import cpu_params, load_params
from tests.support import (INVALID, as_np, assert_same_state, check_resume, check_step_n_equals_loop, loop_updates, pair_adam,
                           pair_nets, pair_q_y, random_replay, refused, run_pair, to_double, worst_ratio)

pytestmark = pytest.mark.gpu

S, A = 24, 6                        # walker dims
TOL = 2e-5                          # network outputs (tests/test_gpu_algos.py)
V_MIN, V_MAX = 20.0, 60.0
GAMMA = 0.99
NET_SEED = 500


def make(B, N, fixture_nets=False, **kw):
    kw.setdefault("v_min", V_MIN)
    kw.setdefault("v_max", V_MAX)
    t.manual_seed(0)
    algo = D4PG(logger=NullLogger(), state_dim=S, action_dim=A, n_atoms=N, max_batch=max(B, 256), **kw).create()
    if fixture_nets:
        actor = fx.make_net(NET_SEED + 1, fx.actor_dims(S, A))
        critic = fx.make_net(NET_SEED + 2, fx.critic_dims(S, A, out=N))
        for mod, params in ((algo.actor, actor), (algo.actor_target, actor), (algo.critic, critic), (algo.critic_target, critic)):
            load_params(mod, params)
    return algo


def oracle_for(algo, **kw):
    return D4PGOracle(S, A, cpu_params(algo.actor), cpu_params(algo.critic), algo.n_atoms, algo.v_min, algo.v_max,
                      gamma=algo.gamma, tau=algo.tau, **kw)


def batches(B, n):
    return [fx.make_batch(100 + k, B, S, A) for k in range(n)]


def assert_the_batches_reach_every_case(data, v_min, v_max):
    """Rows with d = 1, rows with atoms clamped at each end, rows with no clamped atom — in every batch."""
    for s, a, r, d, s2 in data:
        r, d = r.double().reshape(-1), d.double().reshape(-1)
        g = (1 - d) * GAMMA
        low, high = r + g * v_min < v_min, r + g * v_max > v_max
        assert int((d == 1).sum()) >= 1
        assert int((low & (d == 0)).sum()) >= 1 and int((high & (d == 0)).sum()) >= 1
        assert int((~low & ~high).sum()) >= 1


def step(algo, batch):
    algo.update(*(x.cuda() for x in batch))


def got_and_want(algo, o, B):
    got, want = {}, {}
    for name in ("critic", "critic_target", "actor", "actor_target"):
        pair_nets(got, want, name, getattr(algo, name), getattr(o, name))
    pair_adam(got, want, algo, "critic", o.opt_critic)
    pair_adam(got, want, algo, "actor", o.opt_actor)
    pair_q_y(got, want, algo, B, o.last["q"], o.last["y"])
    return as_np(got), as_np(want)


PARITY = [(256, 41), (256, 48), (100, 41), (100, 5)]


@pytest.mark.parametrize("B,N", PARITY, ids=[f"B{b}-N{n}" for b, n in PARITY])
def test_d4pg_matches_the_oracle(B, N):
    """Four updates: critic, critic target, actor, actor target, both optimizers' moments and the last update's
    Q(s, a) = sum z p and sum z m rows within the suite's gates; the scalars read_scalars reports are the oracle's."""
    data = batches(B, 4)
    assert_the_batches_reach_every_case(data, V_MIN, V_MAX)
    algo = make(B, N, fixture_nets=True)
    o = oracle_for(algo)
    run_pair(algo, [o], data, step, to_double)
    assert algo.learner.update_count == 4
    got, want = got_and_want(algo, o, B)
    worst = sc.compare(got, want, TOL, param_tol=sc.PARAM_TOL)
    print(f"B={B} N={N}: worst key {worst[0]} rel dev {worst[1]:.2e}")
    scal = algo.learner.read_scalars()
    assert scal["critic_loss"] == pytest.approx(float(o.last["critic_loss"]), rel=1e-4)
    assert scal["actor_loss"] == pytest.approx(float(o.last["actor_loss"]), rel=1e-4)
    assert scal["q_mean"] == pytest.approx(float(o.last["q"].mean()), rel=1e-4)
    assert scal["q_target_mean"] == pytest.approx(float(o.last["y"].mean()), rel=1e-4)


def test_the_comparison_discriminates():
    """The same oracle without the (1 - d) factor, or without the Polyak steps, misses the gates by a factor of ten or
    more (tau = 0.5 here so that a missing Polyak step shows in the targets at once)."""
    B, N = 256, 41
    algo = make(B, N, fixture_nets=True, tau=0.5)
    right = oracle_for(algo)
    wrong = {"no (1 - d)": oracle_for(algo, no_done=True), "no polyak": oracle_for(algo, skip_polyak=True)}
    run_pair(algo, [right, *wrong.values()], batches(B, 4), step, to_double)
    got, want = got_and_want(algo, right, B)
    sc.compare(got, want, TOL, param_tol=sc.PARAM_TOL)
    for name, o in wrong.items():
        r, _key = worst_ratio(*got_and_want(algo, o, B), TOL)
        assert r >= 10.0, f"{name}: the learner is only {r:.1f} gates away from the wrong oracle"


# ---- step_n over replays ---------------------------------------------------------------------------------------------
RB, RN, RV = 64, 41, 5.0            # batch, atoms and support [-5, 5] of the replay-driven tests
NSTEP = 3


def replay(nstep):
    return random_replay((S, A), NSTEP if nstep else None, GAMMA)


@pytest.mark.parametrize("nstep", [False, True], ids=["plain", "nstep3"])
def test_step_n_equals_sample_then_update_bitwise(nstep):
    """step_n(3) is bit for bit three sample() + update() pairs, over a plain replay and over an n-step replay (n = 3)."""
    buf = replay(nstep)
    pair = lambda: (make(RB, RN, v_min=-RV, v_max=RV), make(RB, RN, v_min=-RV, v_max=RV))       # noqa: E731
    fused, _loop, n_done = check_step_n_equals_loop(pair, buf, RB)
    assert n_done > 0 and fused.update_step == 6
    assert not t.equal(fused.learner.actor_arena, make(RB, RN, v_min=-RV, v_max=RV).learner.actor_arena)   # (it trained)


def test_the_nstep_target_is_the_oracles():
    """The first update of step_n over the n-step replay: sum_j z_j m_j per row against the float64 oracle fed the rows
    tests/nstep_oracle.py gathers for the drawn slots; fed the one-step rows of the same slots it misses the gate."""
    nbuf = replay(True)
    algo = make(RB, RN, v_min=-RV, v_max=RV)
    o = oracle_for(algo)
    algo.learner.step_n(nbuf.handle, 1, RB, seed=5)
    _q, y = algo.learner.debug_q_y(RB)
    algo.learner.check()
    nbuf.seed, nbuf._sample_counter = 5, 0
    _rows, (ep, st), m = nbuf.sample(RB, return_indices=True, return_steps=True)
    lens = nbuf.ep_lens[:nbuf.episodes_counter]
    starts = np.concatenate([[0], np.cumsum(lens)[:-1]])
    inds = starts[ep.cpu().numpy()] + st.cpu().numpy()
    store = [getattr(nbuf, k).cpu().numpy() for k in ("states", "actions", "rewards", "dones")]
    devs = {}
    for n in (NSTEP, 1):
        w = no.nstep_gather(*store, lens, inds, n, GAMMA)
        r, d, s2 = (t.from_numpy(w[k]).double() for k in ("r", "d", "s2"))
        devs[n] = sc.rel_dev(y.cpu().numpy(), (o.target_distribution(r, d, s2) * o.z).sum(1).numpy())
    print(f"sum z m vs the oracle on {NSTEP}-step rows {devs[NSTEP]:.2e}, on one-step rows {devs[1]:.2e}; steps taken {t.bincount(m.cpu()).tolist()}")
    assert int(m.max()) == NSTEP and int(m.min()) == 1
    assert devs[NSTEP] < TOL
    assert not devs[1] < TOL


def test_lanes_replay_trains():
    """A replay with one open episode per environment (open_lanes) feeds step_n like any other."""
    from oprl_amd.buffers.episodic_buffer import EpisodicReplayBuffer
    buf = EpisodicReplayBuffer(buffer_size_transitions=8 * 20, state_dim=S, action_dim=A, max_episode_lenth=20,
                               device="cuda", seed=1).create()
    buf.open_lanes(4)
    rs = np.random.RandomState(2)
    for _ in range(12):
        buf.add_step_rows(rs.standard_normal((4, S)).astype(np.float32), rs.uniform(-1, 1, (4, A)).astype(np.float32),
                     rs.standard_normal(4).astype(np.float32), np.zeros(4, np.float32),
                     rs.standard_normal((4, S)).astype(np.float32), np.zeros(4, bool))
    fused, loop = make(RB, RN, v_min=-RV, v_max=RV), make(RB, RN, v_min=-RV, v_max=RV)
    loop.load_state_dict(fused.state_dict())
    fused.learner.step_n(buf.handle, 2, RB, seed=9)
    loop_updates(loop, buf, 2, 9, RB)
    assert_same_state(fused, loop)


def test_resume():
    """A checkpoint taken after two updates, loaded into a fresh learner, gives bit-identical state after two more."""
    B, N = 100, 41
    a, _b, _sd = check_resume(lambda: make(B, N), step, batches(B, 4), 2)
    assert a.update_step == 4


# ---- refusals ----------------------------------------------------------------------------------------------------------
def test_refusals():
    """Every configuration and call DESIGN.md §15 lists as refused returns its status with a message; the update count
    and the Adam step counts stay where they were."""
    lib = _capi.load()
    B = 64
    algo = make(B, 41)
    L = algo.learner
    algo.update(*(x.cuda() for x in batches(B, 1)[0]))
    t.cuda.synchronize()
    counters = L.state_dict()["counters"]

    def create_with(change):
        cfg = _capi.OprlLearnerConfig.from_buffer_copy(L._cfg)
        change(cfg)
        h = C.c_void_p()
        rc = lib.oprl_learner_create(C.byref(cfg), C.byref(h))
        assert not h.value
        return rc

    def atoms(n):
        def f(cfg):
            cfg.critics[0].dims[cfg.critics[0].n_layers] = n
        return f

    msg = refused(create_with(atoms(51)), INVALID)
    assert b"48" in msg and b"atoms" in msg, msg
    refused(create_with(atoms(49)), INVALID)
    refused(create_with(atoms(1)), INVALID)
    for lo, hi in ((1.0, 1.0), (2.0, -2.0)):
        def f(cfg, lo=lo, hi=hi):
            cfg.hp.v_min, cfg.hp.v_max = lo, hi
        assert b"v_max" in refused(create_with(f), INVALID)
    for prec in ("bf16", "x2"):
        def f(cfg, prec=prec):
            cfg.precision = _capi.PRECISION[prec]
        assert b"f32" in refused(create_with(f), INVALID)

    def f(cfg):
        cfg.export_grads = 1
    assert b"export_grads" in refused(create_with(f), INVALID)

    def f(cfg):
        cfg.n_critics = 2
    refused(create_with(f), INVALID)
    # group membership
    other = make(B, 41)
    handles = (C.c_void_p * 2)(L.handle, other.learner.handle)
    g = C.c_void_p()
    refused(lib.oprl_group_create(handles, 2, C.byref(g)), INVALID)
    assert not g.value
    # importance weights
    s, a, r, d, s2 = (x.cuda() for x in batches(B, 1)[0])
    w, td = t.ones(B, device="cuda"), t.zeros(B, device="cuda")
    msg = refused(lib.oprl_learner_update_weighted(L.handle, _capi.ptr(s), _capi.ptr(a), _capi.ptr(r), _capi.ptr(d),
                                                   _capi.ptr(s2), _capi.ptr(w), B, None, None, _capi.ptr(td),
                                                   _capi.current_stream()), INVALID)
    assert b"D4PG" in msg
    buf = replay(False)
    msg = refused(lib.oprl_learner_step_n_prio(L.handle, buf.handle, 1, B, 0, 0.4, 1000.0, _capi.current_stream()), INVALID)
    assert b"D4PG" in msg
    # an n-step replay whose gamma is not the learner's
    nbuf = replay(True)
    nbuf.n_step, nbuf.gamma = NSTEP, 0.95
    nbuf._set_nstep()
    assert b"gamma" in refused(lib.oprl_learner_step_n(L.handle, nbuf.handle, 1, B, 0, _capi.current_stream()), INVALID)
    with pytest.raises(ValueError, match="gamma"):
        algo.update_from_buffer(nbuf, B)
    t.cuda.synchronize()
    L.check()
    assert L.state_dict()["counters"] == counters and algo.update_step == 1
    assert algo.debug_form(B)["fused"] == 0 and algo.debug_form(B)["form"] == 0


def test_a_ddpg_learner_of_the_same_process_is_untouched():
    """A DDPG learner stepped before and after a D4PG learner was created and stepped ends with the parameters, targets
    and moments, bit for bit, of one stepped straight through."""
    from oprl_amd.algos.ddpg import DDPG
    B = 256
    data = batches(B, 4)

    def ddpg():
        t.manual_seed(0)
        return DDPG(logger=NullLogger(), state_dim=S, action_dim=A, max_batch=B).create()

    straight, around = ddpg(), ddpg()
    around.load_state_dict(straight.state_dict())
    for x in data:
        straight.update(*(v.cuda() for v in x))
    for x in data[:2]:
        around.update(*(v.cuda() for v in x))
    d4 = make(B, 41)
    for x in data[:2]:
        d4.update(*(v.cuda() for v in x))
    t.cuda.synchronize()
    d4.learner.check()
    for x in data[2:]:
        around.update(*(v.cuda() for v in x))
    assert_same_state(straight, around)
