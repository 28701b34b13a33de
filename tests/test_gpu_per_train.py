"""Training from prioritized replay on the MI355X ("Training from it"): the weighted update
with w = 1 against today's update bit for bit, with real weights against tests/per_train_oracle.py (float64,
autograd), step_n_prio against the calls it stands for, the refusals, and the trainer end to end."""
from __future__ import annotations

import numpy as np
import pytest
import torch as t

from oprl_amd.algos.ddpg import DDPG
from oprl_amd.algos.redq import REDQ
from oprl_amd.algos.sac import SAC
from oprl_amd.algos.td3 import TD3
from oprl_amd.logging import NullLogger
from oracle import fixtures as fx
from tests import per_oracle as po
from tests import scenarios as sc
from tests.hip_adapters import cpu_params
from tests.per_train_oracle import WeightedOracle, WeightedREDQOracle
from tests.support import (as_np, assert_same_state, fill_full_episodes, pair_adam, pair_nets, pair_q_y, run_pair, to_double,
                           worst_ratio)

pytestmark = pytest.mark.gpu

S, A = 24, 6
N, M, G = 10, 2, 3                 # REDQ: the default ensemble, two target critics, an actor step every third update
TOL = 2e-5                          # network outputs (tests/test_gpu_algos.py)
SEED, RANK = 7, 0
ALGOS = ["ddpg", "td3", "sac", "redq"]
BATCHES = [256, 100]                # 100: six full 16-row slices plus four rows
CASES = [(n, b) for n in ALGOS for b in BATCHES]
IDS = [f"{n}-B{b}" for n, b in CASES]


def make(name, B=256, **kw):
    """A learner of the named algorithm; the same call gives the same initial parameters."""
    t.manual_seed(11)
    common = dict(logger=NullLogger(), state_dim=S, action_dim=A, max_batch=max(B, 256), **kw)
    if name == "ddpg":
        algo = DDPG(**common)
    elif name == "td3":
        algo = TD3(log_every=10 ** 9, **common)
    elif name == "sac":
        algo = SAC(tune_alpha=True, log_every=10 ** 9, **common)
    else:
        algo = REDQ(n_critics=N, n_min=M, utd_ratio=G, log_every=10 ** 9, **common)
    algo.create()
    algo.set_seed(SEED, RANK)
    return algo


def critic_nets(name, algo, target=False):
    c = algo.critic_target if target else algo.critic
    return [c.q1] if name == "ddpg" else [c.q1, c.q2] if name in ("td3", "sac") else list(c.nets)


def batches(B, n, weights="drawn"):
    """n minibatches with the two noise draws and the weights: drawn in [0.05, 1] with one row at 1 (what the replay's
    normalisation by the batch maximum gives), or all ones."""
    out = []
    for k in range(n):
        s, a, r, d, s2 = fx.make_batch(100 + k, B, S, A)
        g = t.Generator().manual_seed(500 + k)
        e1, e2 = t.randn(B, A, generator=g), t.randn(B, A, generator=g)
        w = 0.05 + 0.95 * t.rand(B, 1, generator=g)
        w[int(t.randint(B, (1,), generator=g))] = 1.0
        out.append((s, a, r, d, s2, t.ones(B, 1) if weights == "ones" else w, e1, e2))
    return out


def update(name, algo, x, weighted=True):
    s, a, r, d, s2, w, e1, e2 = (v.cuda() for v in x)
    kw = dict(weights=w) if weighted else {}
    if name == "td3":
        kw["noise"] = e1
    elif name != "ddpg":
        kw["noise"] = (e1, e2)
    algo.update(s, a, r, d, s2, **kw)


# ---------------------------------------------------------------- 1. w = 1 is today's update
@pytest.mark.parametrize("name,B", CASES, ids=IDS)
def test_unit_weights_are_todays_update_bitwise(name, B):
    """Four updates with weights = 1 on a prioritized learner against the same four plain updates on an identically
    initialised no_fuse learner: parameters, targets, both optimizers' moments, alpha, counters and the q / y rows of
    every update bit for bit (forward | seed kernel | backward run the same kernels on the same operands as the one
    forward + seed + backward launch), and |TD| = mean_j |q_j - y| for the rows the plain learner reports."""
    wl, pl = make(name, B, prioritized=True), make(name, B, no_fuse=True)
    pl.load_state_dict(wl.state_dict())
    for k, x in enumerate(batches(B, 4, weights="ones")):
        update(name, wl, x)
        update(name, pl, x, weighted=False)
        t.cuda.synchronize()
        (q1, y1), (q2, y2) = wl.learner.debug_q_y(B), pl.learner.debug_q_y(B)
        assert t.equal(q1, q2) and t.equal(y1, y2), f"update {k}: q / y rows differ"
        assert wl.last_td_abs.shape == (B,) and bool(t.isfinite(wl.last_td_abs).all())
        if name == "ddpg":
            assert t.equal(wl.last_td_abs, (q1 - y1).abs())
        assert_same_state(wl, pl, what=f"update {k}")
    wl.learner.check()
    assert wl.update_step == 4


# ---------------------------------------------------------------- 2. / 3. against float64
def oracle_for(name, algo, **knobs):
    if name == "redq":
        from tests.test_gpu_redq import subset
        return WeightedREDQOracle(S, A, cpu_params(algo.actor), [cpu_params(n) for n in algo.critic.nets],
                                  [cpu_params(n) for n in algo.critic_target.nets], subset(N, M, SEED, RANK), M, G,
                                  tau=algo.target_update_coef, alpha_init=algo.alpha_init, **knobs)
    kw = dict(tau=algo.target_update_coef, alpha_init=algo.alpha_init, lr_alpha=algo.lr_alpha) if name == "sac" else dict(tau=algo.tau)
    if name == "td3":
        kw.update(policy_noise=algo.policy_noise, noise_clip=algo.noise_clip, policy_freq=algo.policy_freq, max_action=algo.max_action)
    return WeightedOracle(name, S, A, cpu_params(algo.actor), [cpu_params(n) for n in critic_nets(name, algo)], **kw, **knobs)


def got_and_want(name, algo, o, B):
    L = algo.learner
    got, want = {}, {}
    nets, tnets = critic_nets(name, algo), critic_nets(name, algo, target=True)
    for i in range(len(nets)):
        pair_nets(got, want, f"critic.{i}", nets[i], o.critics[i])
        pair_nets(got, want, f"critic_target.{i}", tnets[i], o.targets[i])
    pair_nets(got, want, "actor", algo.actor, o.actor)
    if name in ("ddpg", "td3"):
        pair_nets(got, want, "actor_target", algo.actor_target, o.actor_target)
    pair_adam(got, want, algo, "critic", o.opt_critic)
    pair_adam(got, want, algo, "actor", o.opt_actor)
    if L.log_alpha is not None:
        got["u.log_alpha"], want["u.log_alpha"] = L.log_alpha.cpu().reshape(1), o.log_alpha.reshape(1)
        got["u.log_alpha_m"], want["u.log_alpha_m"] = L.log_alpha_m.cpu().reshape(1), o.opt_alpha.m[0]
        got["u.log_alpha_v"], want["u.log_alpha_v"] = L.log_alpha_v.cpu().reshape(1), o.opt_alpha.v[0]
    pair_q_y(got, want, algo, B, o.last["q"], o.last["y"])
    return as_np(got), as_np(want)


def td_ratio(algo, o):
    """max |td_abs - oracle| over its gate 2e-5 * max(max|q|, max|y|): the gate q and y meet, through one subtraction"""
    scale = max(float(o.last["q"].abs().max()), float(o.last["y"].abs().max()))
    dev = float((algo.last_td_abs.cpu().double() - o.last["td_abs"]).abs().max())
    return dev / (TOL * scale), dev, scale


@pytest.mark.parametrize("name,B", CASES, ids=IDS)
def test_weighted_updates_match_float64(name, B):
    """Four weighted updates: every net, target, both optimizers' moments, the temperature, and the last update's q / y
    rows within the suite's gates, and its |TD| within 2e-5 of max(max|q|, max|y|)."""
    algo = make(name, B, prioritized=True)
    o = oracle_for(name, algo)
    run_pair(algo, [o], batches(B, 4), lambda a, x: update(name, a, x), to_double)
    assert algo.update_step == 4
    got, want = got_and_want(name, algo, o, B)
    worst = sc.compare(got, want, TOL, param_tol=sc.PARAM_TOL)
    r, dev, scale = td_ratio(algo, o)
    print(f"{name} B={B}: worst key {worst[0]} {worst[1]:.3e}; td_abs dev {dev:.3e} at scale {scale:.3e} ({r:.3f} of its gate)")
    assert r <= 1.0, f"td_abs: {dev:.3e} > 2e-5 * {scale:.3e}"


@pytest.mark.parametrize("name", ALGOS)
def test_the_comparison_discriminates(name):
    """An oracle that ignores the weights, one that weights the actor loss too and one that normalises by sum(w)
    instead of B each miss the gates the right oracle meets by a factor of ten or more."""
    B = 256
    algo = make(name, B, prioritized=True)
    right = oracle_for(name, algo)
    wrong = {"ignores the weights": oracle_for(name, algo, ignore_weights=True),
             "weights the actor loss": oracle_for(name, algo, weight_actor=True),
             "normalises by sum(w)": oracle_for(name, algo, normalise_by_sum=True)}
    run_pair(algo, [right, *wrong.values()], batches(B, 4), lambda a, x: update(name, a, x), to_double)
    got, want = got_and_want(name, algo, right, B)
    sc.compare(got, want, TOL, param_tol=sc.PARAM_TOL)
    for what, o in wrong.items():
        r, _key = worst_ratio(*got_and_want(name, algo, o, B), TOL)
        print(f"{name}: oracle that {what}: {r:.1f} gates away")
        assert r >= 10.0, f"{what}: the learner is only {r:.1f} gates away from the wrong oracle"


# ---------------------------------------------------------------- 4. step_n_prio
def prio_replay(seed=3, E=40, Lep=100, fill=True):
    from oprl_amd.buffers.prioritized_buffer import PrioritizedEpisodicReplayBuffer
    dev = t.device("cuda", 0)
    buf = PrioritizedEpisodicReplayBuffer(buffer_size_transitions=E * Lep, state_dim=S, action_dim=A, device="cuda",
                                          seed=seed, max_episode_lenth=Lep).create()
    if not fill:
        return buf
    g = fill_full_episodes(buf, E, Lep)
    td0 = t.rand(E * Lep, device=dev, generator=g) * 2       # random initial priorities on every slot
    buf.update_priorities(t.arange(E * Lep, dtype=t.int32, device=dev), td0)
    return buf


@pytest.mark.parametrize("name", ["ddpg", "redq"])
def test_step_n_prio_equals_the_calls_it_stands_for(name):
    """step_n_prio(K = 5) against a Python loop of sample(beta(u)) at counter u, update(weights), update_priorities:
    learner state, the whole tree and p_max bit for bit; each update's sampled leaves are (td_abs + eps)^alpha."""
    B, K = 256, 5
    one, loop = make(name, B, prioritized=True), make(name, B, prioritized=True)
    loop.load_state_dict(one.state_dict())
    b1, b2 = prio_replay(), prio_replay()
    E_L = 40 * 100
    tree0, pm0 = b1.tree()
    assert t.equal(tree0, b2.tree()[0])
    one.learner.step_n_prio(b1.handle, K, B, seed=b1.seed, beta0=b1.beta0, beta_steps=b1.beta_steps)
    for _ in range(K):
        u = loop.update_step
        b2._sample_counter = u
        batch = b2.sample(B, beta=b2.beta(u))
        loop.update(*batch, weights=b2.last_weights)
        b2.update_priorities(b2.last_slots, loop.last_td_abs)
        leaves = b2.tree()[0][:E_L].cpu().numpy()
        want = {}
        for slot, td in zip(b2.last_slots.cpu().numpy(), loop.last_td_abs.cpu().numpy()):
            want[int(slot)] = po.priority(float(td), b2.alpha, b2.eps)       # (a slot listed twice: the later row)
        for slot, p in want.items():
            assert leaves[slot] == p, (slot, leaves[slot], p)
    t.cuda.synchronize()
    one.learner.check()
    assert one.update_step == K
    assert_same_state(one, loop)
    (tree1, pm1), (tree2, pm2) = b1.tree(), b2.tree()
    assert t.equal(tree1, tree2) and pm1 == pm2
    assert not t.equal(tree1[:E_L], tree0[:E_L]), "no leaf changed"


# ---------------------------------------------------------------- 5. refusals
def _weighted_call(algo, B=32):
    s, a, r, d, s2 = (x.cuda() for x in fx.make_batch(1, B, S, A))
    return algo.learner.update_weighted(s, a, r, d, s2, t.ones(B, device="cuda"))


@pytest.mark.parametrize("which", ["fused", "tqc", "x2", "bf16", "export_grads"])
def test_update_weighted_refuses(which):
    from oprl_amd.algos.tqc import TQC
    if which == "tqc":
        algo = TQC(logger=NullLogger(), state_dim=S, action_dim=A, max_batch=256).create()
    else:
        kw = dict(fused={}, x2=dict(precision="x2"), bf16=dict(precision="bf16"), export_grads=dict(export_grads=True, no_fuse=True))[which]
        algo = DDPG(logger=NullLogger(), state_dim=S, action_dim=A, max_batch=256, **kw).create()
    before = algo.update_step
    with pytest.raises(RuntimeError, match="oprl_learner_update_weighted") as e:
        _weighted_call(algo)
    assert len(str(e.value)) > 60 and algo.update_step == before
    with pytest.raises(RuntimeError, match="oprl_learner_step_n_prio"):
        algo.learner.step_n_prio(prio_replay().handle, 1, 32, seed=0, beta0=0.4, beta_steps=1e6)
    assert algo.update_step == before


def test_step_n_prio_refuses_bad_replays_and_plain_algorithms_refuse_prioritized_buffers():
    from oprl_amd.buffers.episodic_buffer import EpisodicReplayBuffer
    from oprl_amd.buffers.prioritized_buffer import PrioritizedEpisodicReplayBuffer
    algo = make("ddpg", prioritized=True)
    L = algo.learner
    plain = EpisodicReplayBuffer(buffer_size_transitions=400, state_dim=S, action_dim=A, device="cuda", max_episode_lenth=100).create()
    other = PrioritizedEpisodicReplayBuffer(buffer_size_transitions=400, state_dim=S + 1, action_dim=A, device="cuda",
                                            max_episode_lenth=100).create()
    empty = prio_replay(fill=False)
    for buf, msg in ((plain, "sum tree"), (other, "dims"), (empty, "empty")):
        with pytest.raises(RuntimeError, match=msg) as e:
            L.step_n_prio(buf.handle, 1, 32, seed=0, beta0=0.4, beta_steps=1e6)
        assert len(str(e.value)) > 40 and algo.update_step == 0
    state = algo.state_dict()
    assert state["counters"] == make("ddpg", prioritized=True).state_dict()["counters"]      # (Adam step counts too)
    full = prio_replay()
    for plain_algo in (make("ddpg"), make("redq")):
        with pytest.raises(ValueError, match="importance weights"):
            plain_algo.update_from_buffer(full, 32)
        assert plain_algo.update_step == 0
    # a prioritized learner over a plain buffer trains uniformly through today's path
    filled = prio_replay()
    plain._tensors["states"].copy_(filled._tensors["states"][:4])
    plain._tensors["actions"].copy_(filled._tensors["actions"][:4])
    plain.ep_lens, plain.episodes_counter, plain._number_transitions, plain._lens_dirty = [100] * 4, 4, 400, True
    ref = make("ddpg", no_fuse=True)
    ref.load_state_dict(algo.state_dict())
    algo.update_from_buffer(plain, 32)
    ref.update_from_buffer(plain, 32)
    t.cuda.synchronize()
    assert_same_state(algo, ref)


# ---------------------------------------------------------------- 6. the trainer
def _trainer(fused, seed=1):
    from oprl_amd.buffers.prioritized_buffer import PrioritizedEpisodicReplayBuffer
    from oprl_amd.environment.synthetic import SyntheticEnv
    from oprl_amd.trainers.base_trainer import BaseTrainer
    t.manual_seed(0)
    algo = DDPG(logger=NullLogger(), state_dim=S, action_dim=A, max_batch=32, prioritized=True).create()
    buf = PrioritizedEpisodicReplayBuffer(buffer_size_transitions=4000, state_dim=S, action_dim=A, max_episode_lenth=40,
                                          device="cuda", seed=seed).create()
    tr = BaseTrainer(logger=NullLogger("/tmp/oprl_amd_test"), env=SyntheticEnv("walker-walk", seed=0, episode_length=40),
                     make_env_test=lambda s: SyntheticEnv("walker-walk", seed=s, episode_length=40),
                     replay_buffer=buf, algo=algo, num_steps=200, start_steps=60, batch_size=32,
                     eval_interval=10 ** 9, save_policy_every=0, stdout_log_every=10 ** 9, fused_sample_update=fused)
    return tr, algo, buf


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "two-call"])
def test_trainer_end_to_end_and_resume(fused, tmp_path):
    """BaseTrainer with DDPG(prioritized=True) over a prioritized buffer: 200 environment steps, a checkpoint, 100 more
    updates; a fresh trainer that loads the checkpoint and runs the same 100 reaches the same learner state and tree."""
    tr, algo, buf = _trainer(fused)
    np.random.seed(0)
    t.manual_seed(1)
    tr.train()
    t.cuda.synchronize()
    algo.learner.check()
    assert algo.update_step == 201 - 31
    sc_ = algo.learner.read_scalars()
    assert all(np.isfinite(v) for v in sc_.values()), sc_
    leaves = buf.priorities()
    live = leaves[leaves > 0]
    assert live.numel() == len(buf) and float(live.min()) < float(live.max()), "the live leaves are all equal"
    tr.save_checkpoint(tmp_path / "mid.ckpt", 200)
    tr2, algo2, buf2 = _trainer(fused)
    assert tr2.load_checkpoint(tmp_path / "mid.ckpt") == 200
    for k in range(100):
        tr._learn(201 + k)
        tr2._learn(201 + k)
    t.cuda.synchronize()
    algo2.learner.check()
    assert algo.update_step == algo2.update_step == 201 - 31 + 100
    assert_same_state(algo, algo2)
    (tree1, pm1), (tree2, pm2) = buf.tree(), buf2.tree()
    assert t.equal(tree1, tree2) and pm1 == pm2
