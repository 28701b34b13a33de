"""Acting for many environments per launch: k_policy_act_rows through oprl_mlp_act_rows /
oprl_learner_act_rows / step_act_rows / act_rows_wait, the policies' explore_rows / exploit_rows, and VecTrainer.

The arithmetic gate is `scenarios.rel_dev` over the WHOLE output array < 2e-6 against a float64 restatement of the MLP
— the gate test_policy_io_matches_the_reference_vectors_on_the_hip_path holds the single-row kernels to.  Margin: fp32
evaluation with 1, 4, 16 and 64 interleaved accumulation chains stayed within 6e-7 of float64 on these shapes (37 rows,
4 to 6 seeds per shape), so the gate has about a 3x margin over summation order alone.  Not normalised per row: a
one-output row near zero reaches 1.6e-5 from rounding alone."""
import ctypes as C

import numpy as np
import pytest
import torch as t
from torch import nn

from oracle import fixtures as fx
from tests import hip_adapters as ha
from tests import scenarios as sc

pytestmark = pytest.mark.gpu

GATE = 2e-6
ERR_INVALID, ERR_STATE = -1, -3


def ref64(params, x):
    """float64 restatement of the MLP: ReLU hidden layers, identity output; params = [W0, b0, W1, b1, ...]."""
    h = np.asarray(x, np.float64)
    ps = [np.asarray(p.detach().cpu().numpy() if isinstance(p, t.Tensor) else p, np.float64) for p in params]
    n = len(ps) // 2
    for l in range(n):
        h = h @ ps[2 * l].T + ps[2 * l + 1]
        if l + 1 < n:
            h = np.maximum(h, 0.0)
    return h


def rows_of(seed, n, S):
    return np.random.RandomState(seed).standard_normal((n, S)).astype(np.float32)


def make_mlp(seed, dims):
    from oprl_amd.algos.nn_models import MLP
    params = fx.make_net(seed, dims)
    mlp = MLP(dims[0], dims[-1], tuple(dims[1:-1]), nn.ReLU()).to("cuda")
    ha.load_params(mlp, params)
    return mlp, params


def _ddpg(**kw):
    from oprl_amd.algos.ddpg import DDPG
    from oprl_amd.logging import NullLogger
    t.manual_seed(0)
    return DDPG(logger=NullLogger("/tmp/oprl_amd_test"), state_dim=24, action_dim=6, device="cuda", **kw).create()


def _filled_buffer(n_eps=6, L=50, seed=3, S=24, A=6):
    from oprl_amd.buffers.episodic_buffer import EpisodicReplayBuffer
    buf = EpisodicReplayBuffer(buffer_size_transitions=n_eps * L, state_dim=S, action_dim=A,
                               max_episode_lenth=L, device="cuda", seed=seed).create()
    rs = np.random.RandomState(0)
    for e in range(n_eps - 1):
        for i in range(L - e):
            last = i == L - e - 1
            buf.add_transition(rs.standard_normal(S).astype(np.float32), rs.uniform(-1, 1, A),
                               float(rs.uniform()), last, episode_done=last)
    return buf


# (S, outputs): deterministic walker; cheetah (input width not a multiple of 4); Gaussian humanoid (input wider than 64,
# 42 outputs); cartpole; quadruped
SHAPES = [(24, 6), (17, 6), (67, 42), (5, 1), (78, 12)]


@pytest.mark.parametrize("S,n_out", SHAPES)
def test_rows_match_the_float64_mlp(S, n_out):
    mlp, params = make_mlp(11 + S, [S, 256, 256, n_out])
    for n in (1, 16, 17, 37, 256):
        x = rows_of(100 + n, n, S)
        got = mlp.hip_act_rows(x)
        assert got.shape == (n, n_out) and got.dtype == np.float32
        dev = sc.rel_dev(got, ref64(params, x))
        print(f"act_rows S={S} out={n_out} N={n}: rel_dev {dev:.2e}")
        assert dev < GATE, (S, n_out, n, dev)


@pytest.mark.parametrize("dims", [[33, 512, 100, 512, 7],      # four layers, 512 wide, a hidden width that is no multiple of 16
                                  [33, 101, 256, 7]])           # odd hidden width: the next layers' rows are not 16-byte aligned
def test_rows_match_the_float64_mlp_on_other_layer_shapes(dims):
    mlp, params = make_mlp(5, dims)
    x = rows_of(7, 37, dims[0])
    dev = sc.rel_dev(mlp.hip_act_rows(x), ref64(params, x))
    print(f"act_rows dims={dims}: rel_dev {dev:.2e}")
    assert dev < GATE, (dims, dev)


@pytest.mark.parametrize("S,n_out", [(24, 6), (17, 6), (67, 42)])
def test_a_rows_bits_do_not_depend_on_the_batch(S, n_out):
    """Row i alone (N = 1), inside a batch of 37, and at another position of a permuted batch of 256: the same bits."""
    mlp, _ = make_mlp(3, [S, 256, 256, n_out])
    x = rows_of(21, 256, S)
    perm = np.random.RandomState(22).permutation(256)
    big = t.from_numpy(mlp.hip_act_rows(x[perm]))
    mid = t.from_numpy(mlp.hip_act_rows(x[:37]))
    for i in (0, 5, 15, 16, 36):
        alone = t.from_numpy(mlp.hip_act_rows(x[i:i + 1]))[0]
        pos = int(np.nonzero(perm == i)[0][0])
        assert t.equal(alone, mid[i]), i
        assert t.equal(alone, big[pos]), (i, pos)


def test_rows_reproduce_the_reference_policy_vectors(monkeypatch):
    """tests/golden/policy_io.npz with the fixture's observation at rows 0 and 20 of a 37-row batch: exploit / explore
    of both policy classes (the reference's noise injected; DeterministicPolicy.explore applies NO tanh), and
    exploit_rows(X)[i] against exploit(X[i])."""
    from oprl_amd.algos.sac import SAC
    from oprl_amd.logging import NullLogger
    gold = sc.load_golden("policy_io")
    S, A, seed = (int(x) for x in gold["meta"])
    obs = np.random.RandomState(seed + 3).standard_normal(S).astype(np.float32)
    x = rows_of(31, 37, S)
    x[0] = obs
    x[20] = obs
    from oprl_amd.algos.ddpg import DDPG
    t.manual_seed(0)
    d = DDPG(logger=NullLogger("/tmp/oprl_amd_test"), state_dim=S, action_dim=A, device="cuda").create()
    ha.load_params(d.actor, fx.make_net(seed + 1, fx.actor_dims(S, A)))
    got = d.actor.exploit_rows(x)
    assert got.shape == (37, A)
    for i in (0, 20):
        assert sc.rel_dev(got[i], gold["det.exploit"]) < GATE
    for i in (1, 7, 16, 20, 36):
        assert sc.rel_dev(got[i], d.actor.exploit(x[i])) < GATE, i
    real_randn = t.randn
    noise = fx.make_noise(seed + 4, (A,))
    monkeypatch.setattr(t, "randn", lambda *a, **k: noise.repeat(37, 1))
    raw_explore = d.actor.explore_rows(x)
    monkeypatch.setattr(t, "randn", real_randn)
    for i in (0, 20):
        assert sc.rel_dev(raw_explore[i], gold["det.explore"]) < GATE
        assert sc.rel_dev(np.tanh(raw_explore[i]), gold["det.explore"]) > 1e-3      # the quirk: tanh would miss
    s = SAC(logger=NullLogger(), state_dim=S, action_dim=A, device="cuda").create()
    ha.load_params(s.actor, fx.make_net(seed + 2, fx.actor_dims(S, A, gaussian=True)))
    got = s.actor.exploit_rows(x)
    for i in (0, 20):
        assert sc.rel_dev(got[i], gold["ga.exploit"]) < GATE
    for i in (1, 7, 16, 20, 36):
        assert sc.rel_dev(got[i], s.actor.exploit(x[i])) < GATE, i
    s.actor.train()
    eps = fx.make_noise(seed + 5, (1, A))
    monkeypatch.setattr(t, "randn", lambda *a, **k: eps.repeat(37, 1))
    sampled = s.actor.explore_rows(x)
    monkeypatch.setattr(t, "randn", real_randn)
    for i in (0, 20):
        assert sc.rel_dev(sampled[i], gold["ga.explore"]) < GATE
    s.actor.eval()
    assert sc.rel_dev(s.actor.explore_rows(x)[20], gold["ga.exploit"]) < GATE       # eval mode: tanh(mean)
    s.actor.train()


@pytest.mark.parametrize("precision", ["f32", "x2", "bf16"])
def test_rows_read_the_masters_not_the_packs(precision):
    """After 3 updates in every arithmetic mode the rows are the fp32 evaluation of the actor arena's CURRENT contents
    (no repack in between), and differ from the rows taken before the updates."""
    algo, buf = _ddpg(max_batch=64, precision=precision), _filled_buffer()
    x = rows_of(41, 37, 24)
    mlp = algo.actor.mlp
    before = mlp.hip_act_rows(x)
    algo.learner.step_n(buf.handle, 3, 64, seed=5)
    after = mlp.hip_act_rows(x)
    t.cuda.synchronize()
    params = [p.detach().cpu() for p in algo.actor.parameters()]
    dev = sc.rel_dev(after, ref64(params, x))
    print(f"act_rows after 3 {precision} updates: rel_dev {dev:.2e}")
    assert dev < GATE, (precision, dev)
    assert not np.array_equal(before, after)


def _state(algo):
    L = algo.learner
    t.cuda.synchronize()
    arenas = [algo.actor._oprl_arena, algo.actor_target._oprl_arena, algo.critic._oprl_arena,
              algo.critic_target._oprl_arena, L.actor_m, L.actor_v, L.critic_m, L.critic_v]
    return [a.clone() for a in arenas], L.state_dict()["counters"], L.update_count


def test_rows_ride_behind_the_updates_and_beside_a_pending_row():
    """step_act_rows(K = 3) leaves parameters, targets, moments and counters bit-identical to step_n(3) on a twin; the
    collected rows are bit-identical to a later stand-alone act_rows of the same array; a step_act row pending at the
    same time is collected unharmed."""
    B = 64
    a1, a2 = _ddpg(max_batch=B), _ddpg(max_batch=B)
    b1, b2 = _filled_buffer(), _filled_buffer()
    obs1 = rows_of(51, 1, 24)[0]
    x = rows_of(52, 37, 24)
    a2.learner.step_act(b2.handle, B, 9, obs1)
    row2 = a2.learner.act_wait(6)
    a2.learner.step_n(b2.handle, 3, B, seed=9)
    a1.learner.step_act(b1.handle, B, 9, obs1)            # one update; its row stays pending ...
    a1.learner.step_act_rows(b1.handle, 3, B, 9, x)       # ... while three more updates and 37 rows are enqueued
    rows = a1.learner.act_rows_wait(37, 6)
    row1 = a1.learner.act_wait(6)
    assert t.equal(t.from_numpy(row1), t.from_numpy(row2))
    s1, s2 = _state(a1), _state(a2)
    for u, v in zip(s1[0], s2[0]):
        assert t.equal(u, v)
    assert s1[1] == s2[1] and s1[2] == s2[2] == 4
    a1.learner.act_rows(x)
    again = a1.learner.act_rows_wait(37, 6)
    assert t.equal(t.from_numpy(rows), t.from_numpy(again))
    assert t.equal(t.from_numpy(rows), t.from_numpy(a1.actor.mlp.hip_act_rows(x)))      # (and the stand-alone entry point)
    params = [p.detach().cpu() for p in a1.actor.parameters()]
    assert sc.rel_dev(rows, ref64(params, x)) < GATE
    # through the Python layer: a 2-D act_next rides as rows, and explore_rows with that very array collects them
    a1.update_from_buffer(b1, B, act_next=x, n_updates=2)
    assert a1.actor.mlp.__dict__.get("_pending_rows") is not None
    got = a1.actor.exploit_rows(x)
    assert a1.actor.mlp.__dict__.get("_pending_rows") is None and a1.learner.update_count == 6
    params = [p.detach().cpu() for p in a1.actor.parameters()]
    assert sc.rel_dev(got, np.tanh(ref64(params, x))) < GATE


def test_refusals_return_their_codes_and_change_nothing():
    from oprl_amd import _capi
    B = 64
    algo, buf = _ddpg(max_batch=B), _filled_buffer()
    other = _filled_buffer(S=17, A=6)                      # a replay of other dims
    L = algo.learner
    lib, h, st = L.lib, L.handle, _capi.current_stream()
    x = rows_of(61, 37, 24)
    xp = x.ctypes.data_as(C.c_void_p)
    out = np.empty((256, 6), np.float32)
    op = out.ctypes.data_as(C.c_void_p)
    algo.learner.step_n(buf.handle, 2, B, seed=1)
    handle, bad = buf.handle, other.handle
    before = _state(algo)

    def unchanged():
        now = _state(algo)
        return all(t.equal(u, v) for u, v in zip(before[0], now[0])) and before[1:] == now[1:]

    # nothing pending yet
    assert lib.oprl_learner_act_rows_wait(h, op, 37, 6, 1000) == ERR_STATE
    # act_rows
    assert lib.oprl_learner_act_rows(None, xp, 37, st) == ERR_INVALID
    assert lib.oprl_learner_act_rows(h, None, 37, st) == ERR_INVALID
    assert lib.oprl_learner_act_rows(h, xp, 0, st) == ERR_INVALID
    assert lib.oprl_learner_act_rows(h, xp, 257, st) == ERR_INVALID
    # step_act_rows
    assert lib.oprl_learner_step_act_rows(None, handle, 1, B, 1, xp, 37, st) == ERR_INVALID
    assert lib.oprl_learner_step_act_rows(h, None, 1, B, 1, xp, 37, st) == ERR_INVALID
    assert lib.oprl_learner_step_act_rows(h, handle, 1, B, 1, None, 37, st) == ERR_INVALID
    assert lib.oprl_learner_step_act_rows(h, handle, 1, B, 1, xp, 0, st) == ERR_INVALID
    assert lib.oprl_learner_step_act_rows(h, handle, 1, B, 1, xp, 257, st) == ERR_INVALID
    assert lib.oprl_learner_step_act_rows(h, handle, -1, B, 1, xp, 37, st) == ERR_INVALID
    assert lib.oprl_learner_step_act_rows(h, handle, 1, 0, 1, xp, 37, st) == ERR_INVALID
    assert lib.oprl_learner_step_act_rows(h, handle, 1, B + 1, 1, xp, 37, st) == ERR_INVALID
    assert lib.oprl_learner_step_act_rows(h, bad, 1, B, 1, xp, 37, st) == ERR_INVALID
    assert lib.oprl_learner_act_rows_wait(h, op, 37, 6, 1000) == ERR_STATE      # (still nothing pending)
    assert unchanged()
    # a pending batch survives refused calls
    L.act_rows(x)
    assert lib.oprl_learner_act_rows_wait(None, op, 37, 6, 1000) == ERR_INVALID
    assert lib.oprl_learner_act_rows_wait(h, None, 37, 6, 1000) == ERR_INVALID
    assert lib.oprl_learner_act_rows_wait(h, op, 36, 6, 1000) == ERR_STATE      # not the pending n_rows
    assert lib.oprl_learner_act_rows_wait(h, op, 37, 5, 1000) == ERR_INVALID    # not the actor's outputs
    assert lib.oprl_learner_act_rows(h, xp, 257, st) == ERR_INVALID
    assert lib.oprl_learner_step_act_rows(h, handle, 1, B + 1, 1, xp, 37, st) == ERR_INVALID
    rows = L.act_rows_wait(37, 6)
    params = [p.detach().cpu() for p in algo.actor.parameters()]
    assert sc.rel_dev(rows, ref64(params, x)) < GATE
    assert lib.oprl_learner_act_rows_wait(h, op, 37, 6, 1000) == ERR_STATE      # collected: nothing pending again
    assert unchanged()
    # the stand-alone entry point
    mlp = algo.actor.mlp
    desc = mlp._packed_desc()[1]
    assert lib.oprl_mlp_act_rows(None, xp, 37, 24, op, 6, st) == ERR_INVALID
    assert lib.oprl_mlp_act_rows(C.byref(desc), None, 37, 24, op, 6, st) == ERR_INVALID
    assert lib.oprl_mlp_act_rows(C.byref(desc), xp, 37, 24, None, 6, st) == ERR_INVALID
    assert lib.oprl_mlp_act_rows(C.byref(desc), xp, 0, 24, op, 6, st) == ERR_INVALID
    assert lib.oprl_mlp_act_rows(C.byref(desc), xp, 257, 24, op, 6, st) == ERR_INVALID
    assert lib.oprl_mlp_act_rows(C.byref(desc), xp, 37, 23, op, 6, st) == ERR_INVALID
    assert lib.oprl_mlp_act_rows(C.byref(desc), xp, 37, 24, op, 7, st) == ERR_INVALID
    assert unchanged()


def test_a_pending_device_error_refuses_the_row_calls():
    """The learner's error word is checked as in step_n: once a bounded wait has been reported (forced through the test
    hook of tests/test_gpu_errors.py), act_rows and step_act_rows return OPRL_ERR_STATE and enqueue nothing."""
    from oprl_amd import _capi
    B = 256
    algo = _ddpg(max_batch=B)
    buf = _filled_buffer()
    L = algo.learner
    batch = [v.cuda() for v in fx.make_batch(3, B, 24, 6)]
    algo.update(*batch)
    t.cuda.synchronize()
    L.check()
    good = L.state_dict()
    x = rows_of(71, 37, 24)
    xp = x.ctypes.data_as(C.c_void_p)
    handle = buf.handle
    assert L.lib.oprl_learner_debug_expire(L.handle, 2) == 0
    algo.update(*batch)
    t.cuda.synchronize()
    count = L.update_count
    assert L.lib.oprl_learner_act_rows(L.handle, xp, 37, _capi.current_stream()) == ERR_STATE
    assert L.lib.oprl_learner_step_act_rows(L.handle, handle, 1, 64, 1, xp, 37, _capi.current_stream()) == ERR_STATE
    out = np.empty((37, 6), np.float32)
    assert L.lib.oprl_learner_act_rows_wait(L.handle, out.ctypes.data_as(C.c_void_p), 37, 6, 1000) == ERR_STATE
    assert L.update_count == count
    assert L.lib.oprl_learner_debug_expire(L.handle, 0) == 0
    L.clear_error()
    L.load_state_dict(good)
    L.act_rows(x)
    rows = L.act_rows_wait(37, 6)
    params = [p.detach().cpu() for p in algo.actor.parameters()]
    assert sc.rel_dev(rows, ref64(params, x)) < GATE


def test_vec_trainer_end_to_end():
    from oprl_amd.buffers.episodic_buffer import EpisodicReplayBuffer
    from oprl_amd.environment.synthetic import SyntheticEnv
    from oprl_amd.logging import NullLogger
    from oprl_amd.trainers.base_trainer import BaseTrainer
    from oprl_amd.trainers.vec_trainer import VecTrainer
    N, B, L, steps, start = 4, 32, 25, 400, 100
    algo = _ddpg(max_batch=B)
    buf = EpisodicReplayBuffer(buffer_size_transitions=1000, state_dim=24, action_dim=6, max_episode_lenth=L,
                               device="cuda", seed=0).create()

    def make_env(seed):
        return SyntheticEnv("walker-walk", seed, episode_length=L)

    kw = dict(logger=NullLogger("/tmp/oprl_amd_test"), make_env_test=make_env, replay_buffer=buf, algo=algo, num_steps=steps,
              start_steps=start, batch_size=B, eval_interval=10 ** 9, save_policy_every=0, stdout_log_every=10 ** 9,
              num_eval_episodes=3, seed=0)
    trainer = VecTrainer(envs=[make_env(100 + i) for i in range(N)], **kw)
    trainer.train()
    t.cuda.synchronize()
    # 16 closed episodes of 25 steps and nothing open (episodes_counter, the reference's quirk, counts the open slot too)
    lens = list(buf.ep_lens[:buf.episodes_counter])
    assert lens == [L] * 16 + [0] and buf.episodes_counter == 17 and len(buf) == 400
    # the same rule: an iteration learns when, after its N steps (whole episodes only), the buffer holds a batch
    learn_iterations = sum(1 for it in range(steps // N) if ((it + 1) // L) * L * N >= B)
    assert learn_iterations == 76
    assert algo.learner.update_count == N * learn_iterations
    for m in (algo.actor, algo.critic, algo.actor_target, algo.critic_target):
        assert bool(t.isfinite(m._oprl_arena).all())
    algo.learner.check()
    batched = trainer.evaluate()["return"]
    single = BaseTrainer(env=make_env(0), **kw).evaluate()["return"]
    print(f"evaluate: batched {batched!r}, one by one {single!r}")
    assert abs(batched - single) <= sc.PARAM_TOL * max(abs(single), 1e-30)
