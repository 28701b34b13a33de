"""Cal-QL on the MI355X learner against tests/calql_oracle.py's CalQLOracle (float64): parity over four
updates at walker dims with supplied draws and returns at B = 16 and the ragged B = 37, N = 2, with the temperature fixed
and learned, at the gates of tests/test_gpu_cql.py; the bitwise links — returns of -inf are CQL's plain update, the mode
turned off is CQL again, step_n is sample(return_indices=True) + returns_to_go + update(returns=) over a plain, a 3-step
and a prior-data replay, resume; every refusal; and CalQL end to end through OfflineTrainer and finetune.

The parity runs use tests/cql_oracle.py's nets, rows and draws.  Their returns are g = r - 0.55 with r the rows' own
rewards in (0, 1): the fixture critics' values at the policy's actions lie in about [-0.2, 0.14] at the first update, so
some policy entries are at the bound and some are not (shares 0.70, 0.33, 0.42, 0.14 over the four updates at B = 16 and
0.50, 0.38, 0.29, 0.33 at B = 37) — asserted on the oracle, on the CPU, before the comparison.  The formula was fixed with
the oracle alone on the CPU, before any GPU run, among six tried: with it the oracle's float32 run stays within 0.08
parameter gates of its float64 run at both shapes (worst key an actor layer), so a miss says something about the kernels;
with 0.4 (r - 0.5), the first tried, float32 arithmetic alone was 1.7 gates off in an actor layer at B = 37.  The plain
CQL oracle on the same rows ends about 350 gates away in its worst critic key."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest
import torch as t

from oprl_amd import _capi
from oprl_amd.algos.calql import CalQL
from oprl_amd.algos.cql import CQL
from oprl_amd.algos.sac import SAC
from oprl_amd.logging import NullLogger
from oracle import fixtures as fx
from tests import calql_oracle as cal
from tests import cql_oracle as co
from tests import scenarios as sc
from tests.support import INVALID, STATE, check_resume, check_step_n_equals_loop, counters, refused
from tests.test_gpu_cql import (ENV, GAMMA, TOL, assert_same_state, batches, critic_gates, learner_state, make, oracle_state,
                                plain_step, replay)

pytestmark = pytest.mark.gpu
SHAPES = ((16, 2), (37, 2))
NEG_INF = -float("inf")


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


def make_cal(B, N=2, **kw):
    return make(B, N, cls=CalQL, cql_n_actions=N, cql_alpha=co.CQL_ALPHA, **kw)


def returns_of(batch):
    return batch[2].reshape(-1) - 0.55


def cal_step(algo, batch, g=None):
    """One calibrated update on Philox draws."""
    algo.update(*(v.cuda() for v in batch), returns=(returns_of(batch) if g is None else g).cuda())


@pytest.mark.parametrize("tune", [False, True], ids=["alpha-fixed", "alpha-tuned"])
@pytest.mark.parametrize("B,N", SHAPES, ids=[f"B{b}-N{n}" for b, n in SHAPES])
def test_calql_matches_the_oracle(B, N, tune):
    """Four updates: every parameter, target, moment, log_alpha and the last update's q1 and y rows within the suite's gates;
    read_cql's bound rate is the oracle's share; the plain CQL oracle on the same rows is more than ten gates away."""
    S, A = fx.ENVS[ENV]
    data = co.parity_data(B, N)
    algo = make_cal(B, N, fixture_nets=True, tune_alpha=tune)
    mk = lambda cls: cls(S, A, *co.fixture_nets(), cql_alpha=co.CQL_ALPHA, n_actions=N, tune_alpha=tune, gamma=algo.gamma,     # noqa: E731
                         tau=algo.target_update_coef, alpha_init=algo.alpha_init)
    o, plain = mk(cal.CalQLOracle), mk(co.CQLOracle)
    rates = []
    for item in data:
        batch, en, ec, eps, uni = item
        g = returns_of(batch)
        o.update(*batch, en, ec, eps, uni, g)
        plain.update(*batch, en, ec, eps, uni)
        rates.append(o.last["bound_rate"])
        if len(rates) == 1:
            assert 0.1 < rates[0] < 0.9, rates       # some entries at the bound and some not, at the first update
        algo.learner.set_cql_noise(eps, uni)
        algo.update(*(v.cuda() for v in batch), returns=g.cuda(), noise=(en.cuda(), ec.cuda()))
        got_rate = algo.learner.read_cql()["bound_rate"]
        print(f"B={B} N={N} tune={tune}: bound rate {got_rate:.6f} (oracle {rates[-1]:.6f})")
        assert got_rate == pytest.approx(rates[-1], abs=1e-6)
    t.cuda.synchronize()
    algo.learner.check()
    assert algo.learner.update_count == 4 and algo.learner.state_dict()["counters"] == [4, 4, 4, 4 if tune else 0]
    got, want = learner_state(algo, B), oracle_state(o)
    worst = sc.compare(got, want, TOL, param_tol=sc.PARAM_TOL)
    print(f"B={B} N={N} tune={tune}: worst key {worst[0]} rel dev {worst[1]:.2e}")
    q = algo.learner.read_cql()
    for k in ("gap1", "gap2", "q_rand1", "q_rand2", "q_pi1", "q_pi2", "penalty"):
        assert q[k] == pytest.approx(float(o.last[k]), rel=1e-4), k
    r = critic_gates(got, oracle_state(plain))
    print(f"B={B} N={N}: the uncalibrated oracle is {r:.0f} gates away")
    assert r >= 10.0


# ---- bitwise links -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tune", [False, True], ids=["alpha-fixed", "alpha-tuned"])
def test_returns_of_minus_infinity_are_the_plain_cql_update(tune):
    B = 37
    data = batches(B, 3)
    calq, cql = make_cal(B, tune_alpha=tune), make(B, tune_alpha=tune)
    cql.load_state_dict(calq.state_dict())
    for x in data:
        cal_step(calq, x, t.full((B,), NEG_INF))
        plain_step(cql, x)
    assert_same_state(calq, cql)
    a, b = calq.learner.read_cql(), cql.learner.read_cql()
    assert a == b and a["bound_rate"] == 0 and a["gap1"] != 0
    cal_step(calq, data[0])            # ... and real returns move it away
    plain_step(cql, data[0])
    t.cuda.synchronize()
    assert not t.equal(calq.learner.critic_arena, cql.learner.critic_arena) and calq.learner.read_cql()["bound_rate"] > 0


def test_with_the_form_off_it_is_cql_again():
    B = 37
    data = batches(B, 5)
    calq, cql = make_cal(B, tune_alpha=True), make(B, tune_alpha=True)
    for x in data[:2]:
        cal_step(calq, x)
    cql.load_state_dict(calq.state_dict())
    calq.learner.set_calql(False)
    for x in data[2:4]:
        SAC.update(calq, *(v.cuda() for v in x))          # (CalQL.update insists on returns; the learner no longer does)
        plain_step(cql, x)
    assert_same_state(calq, cql)
    assert calq.learner.read_cql() == cql.learner.read_cql() and calq.learner.read_cql()["bound_rate"] == 0
    calq.learner.set_calql(True)
    cal_step(calq, data[4])
    plain_step(cql, data[4])
    t.cuda.synchronize()
    assert not t.equal(calq.learner.critic_arena, cql.learner.critic_arena)


RB = 64


def prior_replay():
    """tests/test_gpu_cql.py's replay as the online side, over a prior of 12 x 20 steps with other contents."""
    from oprl_amd.buffers.episodic_buffer import EpisodicReplayBuffer
    from oprl_amd.buffers.prior_buffer import PriorDataReplayBuffer
    S, A = fx.ENVS[ENV]
    own = replay(False)
    prior = EpisodicReplayBuffer(buffer_size_transitions=12 * 20, state_dim=S, action_dim=A, max_episode_lenth=20, device="cuda", seed=7).create()
    gen = t.Generator(device="cuda").manual_seed(2000)
    for v in prior._tensors.values():
        v.copy_(t.randn(v.shape, device="cuda", generator=gen))
    prior._tensors["dones"].copy_(t.as_tensor((np.random.RandomState(16).rand(12, 20, 1) < 0.1).astype(np.float32)))
    lens = [int(x) for x in np.random.RandomState(14).randint(1, 21, size=11)]
    prior.ep_lens, prior.episodes_counter, prior._number_transitions, prior._lens_dirty = lens + [0], 11, sum(lens), True
    buf = PriorDataReplayBuffer(buffer_size_transitions=own.buffer_size_transitions, state_dim=S, action_dim=A,
                                max_episode_lenth=own.max_episode_lenth, device="cuda", seed=7, prior=prior, prior_share=0.5).create()
    for k, v in own._tensors.items():
        buf._tensors[k].copy_(v)
    buf.ep_lens, buf.episodes_counter, buf._number_transitions, buf._lens_dirty = list(own.ep_lens), own.episodes_counter, len(own), True
    return buf


@pytest.mark.parametrize("kind", ["plain", "nstep3", "prior-data"])
def test_step_n_equals_sample_returns_update_bitwise(kind):
    """step_n(3) is bit for bit three rounds of sample(return_indices=True) + returns_to_go (the learner's gamma) +
    update(returns=) at the same counters, and the returns are not trivial."""
    buf = prior_replay() if kind == "prior-data" else replay(kind == "nstep3")

    def sample_returns_update(loop, buf, B):
        rows, (ep, step) = buf.sample(B, return_indices=True)[:2]
        g = buf.returns_to_go(ep, step, gamma=loop.gamma)
        assert float(g.abs().max()) > 0 and bool(t.isfinite(g).all())
        loop.update(*rows, returns=g)
        return rows

    fused, loop, _ = check_step_n_equals_loop(lambda: (make_cal(RB, tune_alpha=True), make_cal(RB, tune_alpha=True)), buf, RB,
                                              one=sample_returns_update)
    assert fused.update_step == 6 and loop.gamma == GAMMA and len(fused.state_dict()["targets"]) == 1
    a = fused.learner.read_cql()
    assert a == loop.learner.read_cql() and a["gap1"] != 0 and 0 < a["bound_rate"] < 1
    # update_from_buffer reaches step_n: one more round each
    fused.update_from_buffer(buf, RB)
    buf._sample_counter = loop.update_step
    rows, (ep, step) = buf.sample(RB, return_indices=True)[:2]
    loop.update(*rows, returns=buf.returns_to_go(ep, step, gamma=loop.gamma))
    assert_same_state(fused, loop)


def test_resume():
    """A checkpoint after two calibrated updates, loaded into a fresh CalQL, gives bit-identical state after two more: the
    form has no state of its own, and create() turns it on."""
    B = 37
    data = batches(B, 4)
    a, b, sd = check_resume(lambda: make_cal(B, tune_alpha=True), cal_step, data, 2)
    assert a.update_step == 4 and len(sd["targets"]) == 1
    assert not t.equal(a.state_dict()["critic"], sd["critic"])
    with pytest.raises(RuntimeError, match="returns"):
        b.learner.update(*(v.cuda() for v in data[0]))


# ---- refusals ------------------------------------------------------------------------------------------------------------
def test_refusals():
    """Every refusal of DESIGN.md §21's learner mode with its status and a word of its message; the update count and the
    Adam step counts stay where they were, and the learner then steps as a twin that was never asked."""
    from oprl_amd.buffers.episodic_buffer import EpisodicReplayBuffer
    lib = _capi.load()
    B = 37
    S, A = fx.ENVS[ENV]
    x = batches(B, 3)
    st = _capi.current_stream()
    set_calql = lambda algo, on=1: lib.oprl_learner_set_calql(algo.learner.handle, on)      # noqa: E731
    # the CQL mode is off: a plain SAC learner, a fused one, one that exports gradients (none of them can have it on)
    for sac in (make(B, cls=SAC), make(B, cls=SAC, no_fuse=False, max_batch=256), make(B, cls=SAC, export_grads=True)):
        refused(set_calql(sac), STATE, b"conservative")
        assert set_calql(sac, 0) == 0
    # ... and turning CQL off turns the calibrated form off with it
    calq, twin = make_cal(B), make_cal(B)
    twin.load_state_dict(calq.state_dict())
    cal_step(calq, x[0])
    cal_step(twin, x[0])
    before = counters(calq)
    dev = [v.cuda().contiguous() for v in x[1]]
    ptrs = [_capi.ptr(v) for v in dev]
    g = returns_of(x[1]).cuda().contiguous()
    # the plain entry points: the rows carry no returns
    refused(lib.oprl_learner_update(calq.learner.handle, *ptrs, B, None, None, st), STATE, b"returns")
    for phase in (0, 1):
        refused(lib.oprl_learner_update_phase(calq.learner.handle, phase, *ptrs, B, None, None, st), STATE, b"returns")
    refused(lib.oprl_learner_update_calql(calq.learner.handle, *ptrs, None, B, None, None, st), INVALID, b"null")
    refused(lib.oprl_learner_update_calql(None, *ptrs, _capi.ptr(g), B, None, None, st), INVALID, b"null")
    # importance weights, as under the CQL mode
    w, td = t.ones(B, device="cuda"), t.zeros(B, device="cuda")
    refused(lib.oprl_learner_update_weighted(calq.learner.handle, *ptrs, _capi.ptr(w), B, None, None, _capi.ptr(td), st), STATE,
            b"importance weights")
    buf = replay(False)
    refused(lib.oprl_learner_step_n_prio(calq.learner.handle, buf.handle, 1, B, 0, C.c_double(0.4), C.c_double(100.0), st), STATE,
            b"importance weights")
    # a hindsight replay has no stored returns: step_n, step_act and step_act_rows through it, before anything is launched
    her = EpisodicReplayBuffer(buffer_size_transitions=4 * 30, state_dim=S, action_dim=A, max_episode_lenth=30, device="cuda").create()
    her.add_transitions(np.ones((20, S + A + 2), np.float32))
    assert lib.oprl_replay_set_her(her.handle, 0, 2, 2, 0.8, 0, 0, 0.1) == 0
    refused(lib.oprl_learner_step_n(calq.learner.handle, her.handle, 2, B, 0, st), STATE, b"hindsight")
    obs = np.zeros((3, S), np.float32)
    refused(lib.oprl_learner_step_act(calq.learner.handle, her.handle, B, 0, obs.ctypes.data_as(C.c_void_p), st), STATE, b"hindsight")
    refused(lib.oprl_learner_step_act_rows(calq.learner.handle, her.handle, 1, B, 0, obs.ctypes.data_as(C.c_void_p), 3, st), STATE,
            b"hindsight")
    # ... and an empty one is refused by the sampler as ever
    empty = EpisodicReplayBuffer(buffer_size_transitions=4 * 30, state_dim=S, action_dim=A, max_episode_lenth=30, device="cuda").create()
    refused(lib.oprl_learner_step_n(calq.learner.handle, empty.handle, 1, B, 0, st), STATE, b"empty")
    assert counters(calq) == before
    # after all that the learner steps as one that was never asked
    cal_step(calq, x[1])
    cal_step(twin, x[1])
    assert_same_state(calq, twin)
    # returns for a learner whose form is off; set_cql(.., 0) turns it off
    cql = make(B)
    plain_step(cql, x[0])
    before = counters(cql)
    refused(lib.oprl_learner_update_calql(cql.learner.handle, *ptrs, _capi.ptr(g), B, None, None, st), STATE, b"off")
    assert counters(cql) == before
    calq.learner.set_cql(calq.cql_alpha, 0)
    refused(lib.oprl_learner_update_calql(calq.learner.handle, *ptrs, _capi.ptr(g), B, None, None, st), STATE, b"off")
    calq.learner.set_cql(calq.cql_alpha, calq.cql_n_actions)
    SAC.update(calq, *(v.cuda() for v in x[2]))        # CQL on, the calibrated form still off: the plain update is accepted again
    assert counters(calq)[0] == 3


# ---- end to end -----------------------------------------------------------------------------------------------------------
def test_calql_pretrained_offline_is_finetuned_online():
    """6 x 50 steps of the synthetic environment: CalQL through OfflineTrainer for 32 updates (step_n over the dataset's
    replay), then finetune for 120 environment steps at batch 32 on mixed batches (step_act over the prior-data replay,
    the fresh rows' returns those of the episodes as far as they have run)."""
    from oprl_amd.buffers.episodic_buffer import EpisodicReplayBuffer
    from oprl_amd.buffers.offline_dataset import OfflineData, fill_replay
    from oprl_amd.buffers.prior_buffer import PriorDataReplayBuffer
    from oprl_amd.environment.synthetic import SyntheticEnv
    from oprl_amd.trainers.finetune import finetune
    from oprl_amd.trainers.offline_trainer import OfflineTrainer
    episodes, steps, B = 6, 50, 32
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
    prior = EpisodicReplayBuffer(buffer_size_transitions=(episodes + 1) * steps, state_dim=S, action_dim=A,
                                 max_episode_lenth=steps, device="cuda", seed=11).create()
    norm = fill_replay(prior, data)
    t.manual_seed(0)
    algo = CalQL(logger=NullLogger(), state_dim=S, action_dim=A, batch_size=B, cql_n_actions=2, log_every=10 ** 9).create()
    OfflineTrainer(logger=NullLogger(), make_env_test=make_env, replay_buffer=prior, algo=algo, obs_norm=norm, num_updates=32,
                   updates_per_call=16, batch_size=B, eval_interval=0, save_policy_every=0, stdout_log_every=0, seed=5).train()
    assert algo.update_step == 32
    rate = algo.learner.read_cql()["bound_rate"]
    assert 0.0 <= rate <= 1.0
    # the dataset's returns as the replay gives them: every episode is 50 stored steps with no done (timeouts)
    g = prior.returns_to_go([0, 0, 5], [0, 49, 10], gamma=algo.gamma).cpu().numpy()
    rew = data.rewards.astype(np.float64)
    assert g[0] == pytest.approx(float(np.sum(algo.gamma ** np.arange(50) * rew[:50])), rel=1e-5, abs=1e-4)
    assert g[1] == pytest.approx(float(rew[49]), rel=1e-6)
    assert g[2] == pytest.approx(float(np.sum(algo.gamma ** np.arange(40) * rew[260:300])), rel=1e-5, abs=1e-4)
    before = algo.state_dict()
    np.random.seed(0)
    tr = finetune(algo=algo, prior_buffer=prior, obs_norm=norm, make_env=make_env, logger=NullLogger("/tmp/oprl_amd_test"),
                  num_steps=120, batch_size=B, prior_share=0.5, seed=5, eval_interval=10 ** 9, save_policy_every=0,
                  stdout_log_every=10 ** 9, num_eval_episodes=2)
    t.cuda.synchronize()
    algo.learner.check()
    buf = tr.replay_buffer
    assert type(buf) is PriorDataReplayBuffer and buf.prior is prior and len(buf) == 121
    n_updates = 121 - (B - 1)
    assert algo.update_step == 32 + n_updates
    after = algo.state_dict()
    for k in ("actor", "critic"):
        assert t.isfinite(after[k]).all() and not t.equal(before[k], after[k]), k
    rate2 = algo.learner.read_cql()["bound_rate"]
    ret = tr.evaluate()["return"]
    print(f"CalQL: 32 offline updates (bound rate {rate:.3f}), {n_updates} online updates on mixed batches (bound rate {rate2:.3f}), "
          f"evaluation return {ret:.3f}")
    assert 0.0 <= rate2 <= 1.0 and np.isfinite(ret)
