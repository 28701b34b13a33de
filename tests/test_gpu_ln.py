"""SAC and REDQ with LayerNorm critics (``layer_norm=True``) against tests/ln_oracle.py (float64, autograd,
written from the definitions): parity within the suite's gates, three wrong oracles it is at least ten gates away from,
the launch counts the round rule gives, step_n against sample() + update(), resume in the middle of a group, the class
untouched with the field off, the modules' torch forward against the learner's q rows, and the C-level refusals."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest
import torch as t

from oprl_amd import _capi
from oprl_amd.algos.cql import CQL
from oprl_amd.algos.redq import REDQ
from oprl_amd.algos.sac import SAC
from oprl_amd.algos.td3 import TD3
from oprl_amd.logging import NullLogger
from tests import ln_oracle as lno
from tests import scenarios as sc
from tests import support
from tests.hip_adapters import cpu_params, hip_adam, load_params
from tests.support import INVALID, STATE, check_step_n_equals_loop, fill_full_episodes, run_pair, to_double, worst_ratio

pytestmark = pytest.mark.gpu

S, A, N, G = lno.S, lno.A, lno.N, lno.G
TOL = 2e-5                          # network outputs (tests/test_gpu_algos.py)
SEED, RANK = 7, 0
LN_KEYS = ("critic_ln", "critic_ln_target", "critic_ln_m", "critic_ln_v")


def subset(n, m):
    lib = _capi.load()

    def draw(u):
        out = (C.c_int32 * m)()
        _capi.check(lib.oprl_redq_subset(SEED, RANK, u, n, m, out), "oprl_redq_subset")
        return list(out)
    return draw


def nets_of(algo):
    if isinstance(algo, REDQ):
        return algo.critic.nets, algo.critic_target.nets
    return [algo.critic.q1, algo.critic.q2], [algo.critic_target.q1, algo.critic_target.q2]


def make(name, B, n_min=2, scenario=True, **kw):
    """The learner of a scenario: the fixture nets and gamma / beta of tests/ln_oracle.py loaded into it."""
    kw.setdefault("layer_norm", True)
    common = dict(logger=NullLogger(), state_dim=S, action_dim=A, log_every=10 ** 9, max_batch=max(B, 256))
    if name == "redq":
        algo = REDQ(n_critics=N, n_min=n_min, utd_ratio=G, **common, **kw).create()
    else:
        algo = SAC(tune_alpha=True, **common, **kw).create()
    algo.set_seed(SEED, RANK)
    if scenario:
        actor, critics, ln = lno.scenario_params(name)
        load_params(algo.actor, [x.cuda() for x in actor])
        flat = [x.cuda() for c in critics for x in c]
        load_params(algo.critic, flat)
        load_params(algo.critic_target, flat)
        if algo.layer_norm:
            with t.no_grad():
                algo.critic_ln.theta.data.copy_(ln.cuda())
                algo.critic_ln.target.copy_(ln.cuda())
    return algo


def step(algo, x):
    algo.update(*(v.cuda() for v in x[:5]), noise=(x[5].cuda(), x[6].cuda()))


def state_of(algo, B):
    """The learner's state under the oracle digest's key names."""
    L = algo.learner
    got = {}
    nets, targets = nets_of(algo)
    th, tg, lm, lv = (x.cpu() for x in algo.critic_ln.tensors())
    for i, (c, ct) in enumerate(zip(nets, targets)):
        for l, x in enumerate(cpu_params(c)):
            got[f"u.critic.{i}.{l}"] = x
        for l, x in enumerate(cpu_params(ct)):
            got[f"u.critic_target.{i}.{l}"] = x
        got[f"u.critic.{i}.ln"], got[f"u.critic_target.{i}.ln"] = th[i], tg[i]
    for l, x in enumerate(cpu_params(algo.actor)):
        got[f"u.actor.{l}"] = x
    for which in ("critic", "actor"):
        m, v = hip_adam(algo, which)
        for l in range(len(m)):
            got[f"u.m_{which}.{l}"], got[f"u.v_{which}.{l}"] = m[l], v[l]
    got["u.m_critic.ln"], got["u.v_critic.ln"] = lm, lv
    got["u.log_alpha"] = L.log_alpha.cpu().reshape(1)
    got["u.log_alpha_m"], got["u.log_alpha_v"] = L.log_alpha_m.cpu().reshape(1), L.log_alpha_v.cpu().reshape(1)
    q, y = L.debug_q_y(B)
    got["u.q"], got["u.y"] = q.cpu(), y.cpu()
    return {k: np.asarray(v.detach().cpu().double().numpy()) for k, v in got.items()}


@pytest.mark.parametrize("name,B,n_min,seed", lno.SCENARIOS, ids=[f"{a}-B{b}-M{m}" for a, b, m, _ in lno.SCENARIOS])
def test_layer_norm_learners_match_the_oracle(name, B, n_min, seed):
    """Four updates (REDQ: G = 3, critic-only updates before and after an actor step; M = 3 takes the minimum through
    k_redq_min; B = 100 is a ragged batch; SAC: a tuned temperature): every critic, target, the actor, both optimisers'
    moments, log alpha and its moments, the last q / y rows, and gamma / beta, their targets and their moments."""
    algo = make(name, B, n_min)
    o = lno.scenario_oracle(name, subset(N, n_min), n_min)
    run_pair(algo, [o], lno.scenario_batches(seed, B, 4), step, to_double)
    assert algo.learner.update_count == 4
    got, want = state_of(algo, B), lno.digest(o)
    assert "u.critic.0.ln" in want and "u.m_critic.ln" in want and "u.log_alpha_m" in want
    print("worst: %.3f gates at %s" % worst_ratio(got, want, TOL))
    sc.compare(got, want, TOL, param_tol=sc.PARAM_TOL)


def test_the_comparison_discriminates():
    """One REDQ learner at tau = 0.5 (so that a missing Polyak step of the target gamma / beta shows in y at once) meets
    the right oracle and is ten gates or more away from plain critics, frozen gamma / beta, and targets that never move."""
    B = 256
    algo = make("redq", B, 2, target_update_coef=0.5)
    right = lno.scenario_oracle("redq", subset(N, 2), 2, tau=0.5)
    wrong = {k: lno.scenario_oracle("redq", subset(N, 2), 2, tau=0.5, **{k: True}) for k in ("no_ln", "freeze_ln", "no_ln_polyak")}
    run_pair(algo, [right, *wrong.values()], lno.scenario_batches(100, B, 4), step, to_double)
    got = state_of(algo, B)
    sc.compare(got, lno.digest(right), TOL, param_tol=sc.PARAM_TOL)
    for k, o in wrong.items():
        r, key = worst_ratio(got, lno.digest(o), TOL)
        print(f"{k}: {r:.1f} gates at {key}")
        assert r >= 10.0, f"{k}: the learner is only {r:.1f} gates away from the wrong oracle"


def slice_launches(algo, batch):
    """Kind-0 (slice kernel) launches of one update."""
    lib = algo.learner.lib
    cnt, ms = (C.c_int64 * 6)(), (C.c_double * 6)()
    t.cuda.synchronize()
    lib.oprl_profile_enable(1)
    try:
        assert lib.oprl_profile_read(cnt, ms, 1) == 0
        algo.update(*batch[:5], noise=(batch[5], batch[6]))
        assert lib.oprl_profile_read(cnt, ms, 1) == 0
    finally:
        lib.oprl_profile_enable(0)
    return int(cnt[0])


def test_launch_counts():
    """A round of n LN nets is ceil(n / 5) multi launches.  REDQ N = 10, M = 2: critic-only 4 (actor on s' 1, targets 1,
    critics 2), actor-step 8 (+ actor forward 1, critics on (s, pi) 2, actor backward 1); SAC: 7 every update."""
    B = 256
    data = [tuple(x.cuda() for x in b) for b in lno.scenario_batches(100, B, G)]
    redq = make("redq", B, 2)
    assert [slice_launches(redq, b) for b in data] == [4, 4, 8]
    sac = make("sac", B)
    assert [slice_launches(sac, b) for b in data[:2]] == [7, 7]
    t.cuda.synchronize()
    redq.learner.check()
    sac.learner.check()


def _replay(dev, seed=0, E=40, Lep=100):
    from oprl_amd.buffers.episodic_buffer import EpisodicReplayBuffer
    buf = EpisodicReplayBuffer(buffer_size_transitions=E * Lep, state_dim=S, action_dim=A, device=str(dev),
                               seed=seed, max_episode_lenth=Lep).create()
    fill_full_episodes(buf, E, Lep)
    return buf


def assert_same_state(a, b, ln=True):     # kept: gamma / beta ride along, present exactly when asked for, and stepped
    x = a.state_dict()
    assert ln == ("critic_ln" in x) and "log_alpha" in x
    if ln:
        assert float(x["critic_ln_v"].abs().max()) > 0.0
    support.assert_same_state(a, b, extra=LN_KEYS if ln else ())


def test_step_n_equals_sample_then_update_bitwise():
    """step_n(K = G) over a replay with 2 % done rows is bit for bit G times sample() + update() with the sampler's rows."""
    B, dev = 256, t.device("cuda", 0)
    buf = _replay(dev)
    fused, loop, n_done = check_step_n_equals_loop(lambda: (make("redq", B), make("redq", B)), buf, B, K=G, extra=LN_KEYS)
    assert_same_state(fused, loop)
    assert n_done > 0


def test_resume_in_the_middle_of_a_group():
    """state_dict() after update 1 of a G group, loaded into a fresh learner, continues bit for bit — gamma / beta, their
    target copy and their moments with the rest."""
    B = 256
    data = lno.scenario_batches(100, B, 5)
    a = make("redq", B)
    for x in data[:1]:
        step(a, x)
    b = make("redq", B, scenario=False)
    b.load_state_dict(a.state_dict())
    for x in data[1:]:
        for algo in (a, b):
            step(algo, x)
    assert a.update_step == 5
    assert_same_state(a, b)
    plain = make("redq", B, layer_norm=False)
    with pytest.raises(ValueError, match="critic_ln"):
        plain.load_state_dict(a.state_dict())
    with pytest.raises(ValueError, match="critic_ln"):
        a.load_state_dict(plain.state_dict())


@pytest.mark.parametrize("name", ["sac", "redq"])
def test_the_field_off_changes_nothing(name):
    """layer_norm=False and a learner built without the field: the same launch form and, after two updates, the same bits."""
    B = 256
    common = dict(logger=NullLogger(), state_dim=S, action_dim=A, log_every=10 ** 9, max_batch=B)
    cls, kw = (REDQ, dict(n_critics=N, n_min=2, utd_ratio=2)) if name == "redq" else (SAC, dict(tune_alpha=True))
    a, b = cls(**common, **kw, layer_norm=False).create(), cls(**common, **kw).create()
    for algo in (a, b):
        algo.set_seed(SEED, RANK)
    b.load_state_dict(a.state_dict())
    assert a.learner.debug_form(B) == b.learner.debug_form(B)
    assert not hasattr(a, "critic_ln") and a.learner._ln is None
    for x in lno.scenario_batches(100, B, 2):
        for algo in (a, b):
            step(algo, x)
    assert_same_state(a, b, ln=False)


@pytest.mark.parametrize("name", ["sac", "redq"])
def test_the_modules_forward_is_what_the_learner_computes(name):
    """critic.forward in torch on the device (before the update's step: on a copy of the parameters) against the q rows
    of the learner's critic step."""
    B = 100
    algo = make(name, B)
    s, a, r, d, s2, e1, e2 = (x.cuda() for x in lno.scenario_batches(100, B, 1)[0])
    with t.no_grad():
        out = algo.critic(s, a)
        q_torch = (out[0] if name == "sac" else out[:, :1]).reshape(-1).cpu()
    algo.update(s, a, r, d, s2, noise=(e1, e2))
    q, _ = algo.learner.debug_q_y(B)
    assert sc.rel_dev(q.cpu().double().numpy(), q_torch.double().numpy()) <= TOL


# ---- the C-level refusals ---------------------------------------------------------------------------------------------------
def hand_built_sac(hidden):
    """A SAC learner over critics of another shape than the classes build (``hidden``), on the generic launch sequence:
    (the HipLearner, its modules)."""
    import math
    from torch import nn
    from oprl_amd.algos.base_algorithm import HipLearner
    from oprl_amd.algos.nn_functions import make_target_
    from oprl_amd.algos.nn_models import DoubleCritic, GaussianActor, flatten_module_
    dev = t.device("cuda", t.cuda.current_device())
    actor = GaussianActor(S, A, (256, 256), nn.ReLU(inplace=True), device="cuda").to(dev)
    c = DoubleCritic(S, A, hidden, nn.ReLU(inplace=True)).to(dev)
    ct = DoubleCritic(S, A, hidden, nn.ReLU(inplace=True)).to(dev).eval()
    for m in (actor, c, ct):
        flatten_module_(m)
    make_target_(ct, c)
    log_alpha = t.tensor(math.log(0.2), dtype=t.float64, device=dev)
    hp = dict(gamma=0.99, tau=5e-3, lr_actor=3e-4, lr_critic=3e-4, lr_alpha=1e-3, beta1=0.9, beta2=0.999, adam_eps=1e-8,
              alpha_init=0.2, tune_alpha=1, target_entropy=-float(A), policy_freq=1)
    L = HipLearner("sac", S, A, dev, actor_group=actor, actor_mlp=actor.net, actor_target_mlp=None, critic_group=c,
                   critic_mlps=[c.q1, c.q2], critic_target_group=ct, critic_target_mlps=[ct.q1, ct.q2], hp=hp, max_batch=256,
                   log_alpha=log_alpha, no_fuse=True)
    return L, (actor, c, ct)


def test_critics_of_another_shape_are_refused_and_stay_plain_sac():
    """OPRL_ERR_INVALID for critics that are not three layers of hidden width 256 with one output — what keeps a kernel
    built for 256 x 256 from a differently shaped pack — and the refused learner still updates as plain SAC."""
    from oprl_amd.algos.nn_models import CriticLayerNorm
    lib = _capi.load()
    B = 256
    batch = [x.cuda() for x in lno.scenario_batches(100, B, 1)[0]]
    for hidden in ((512, 512), (256,)):
        L, keep = hand_built_sac(hidden)
        holder = CriticLayerNorm(2).cuda().make_state()
        rc = lib.oprl_learner_set_layernorm(L.handle, C.byref(_ln_desc(holder)))
        msg = lib.oprl_last_error()
        assert rc == INVALID and b"three-layer net of hidden width 256 with one output" in msg, (hidden, rc, msg)
        assert L._ln is None
        if hidden == (512, 512):
            before = L.critic_arena.detach().clone()
            L.update(*batch[:5], noise0=batch[5], noise1=batch[6])
            t.cuda.synchronize()
            L.check()
            assert L.update_count == 1 and not t.equal(L.critic_arena, before)
            assert bool(t.isfinite(L.critic_arena).all()) and bool(t.isfinite(L.actor_arena).all())
            assert float(holder.m.abs().max()) == 0.0 and bool((holder.theta[:, :, 0] == 1).all())      # (nothing of the holder was stepped)
        L.close()


def test_a_replaced_holder_tensor_is_caught_before_the_next_update():
    """The library keeps the raw pointers of the holder's four tensors: check_bound() watches them with the arenas."""
    B = 256
    algo = make("sac", B)
    batch = [x.cuda() for x in lno.scenario_batches(100, B, 1)[0]]
    algo.update(*batch[:5], noise=(batch[5], batch[6]))
    old = algo.critic_ln.tensors()                      # (kept alive: the library still points at them)
    algo.critic_ln.make_state()                         # a new target copy and new moments
    with pytest.raises(RuntimeError, match="re-allocated"):
        algo.update(*batch[:5], noise=(batch[5], batch[6]))
    assert algo.learner.update_count == 1 and len(old) == 4


def _ln_desc(holder, **kw):
    d = _capi.OprlLayerNorm()
    d.theta, d.theta_target, d.adam_m, d.adam_v = (x.data_ptr() for x in holder.tensors())
    d.eps = 1e-5
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _refused(algo, code, word, **kw):
    from oprl_amd.algos.nn_models import CriticLayerNorm
    lib = _capi.load()
    holder = CriticLayerNorm(len(nets_of(algo)[0]) if not isinstance(algo, TD3) else 2).cuda().make_state()
    support.refused(lib.oprl_learner_set_layernorm(algo.learner.handle, C.byref(_ln_desc(holder, **kw))), code, word)


def test_set_layernorm_refuses_with_its_codes_and_leaves_the_learner_usable():
    B = 256
    common = dict(logger=NullLogger(), state_dim=S, action_dim=A, log_every=10 ** 9, max_batch=B)
    batch = [x.cuda() for x in lno.scenario_batches(100, B, 1)[0]]
    lib = _capi.load()
    # OPRL_ERR_INVALID
    _refused(TD3(**common, no_fuse=True).create(), INVALID, b"SAC and REDQ")
    _refused(SAC(**common, precision="bf16").create(), INVALID, b"f32")
    plain = SAC(**common, no_fuse=True, tune_alpha=True).create()
    _refused(plain, INVALID, b"null parameter array", adam_v=None)
    _refused(plain, INVALID, b"eps", eps=0.0)
    _refused(plain, INVALID, b"eps", eps=float("inf"))
    assert lib.oprl_learner_set_layernorm(plain.learner.handle, None) == INVALID
    # OPRL_ERR_STATE
    _refused(SAC(**common).create(), STATE, b"no_fuse")
    from oprl_amd.group import LearnerGroup
    members = [SAC(**common).create(), SAC(**common).create()]
    group = LearnerGroup(members)
    _refused(members[1], STATE, b"member of a group")
    group.close()
    _refused(SAC(**common, no_fuse=True, export_grads=True).create(), STATE, b"export_grads")
    _refused(CQL(**common, batch_size=8, cql_n_actions=2).create(), STATE, b"conservative")
    on = make("sac", B)
    _refused(on, STATE, b"already on")
    plain.update(*batch[:5], noise=(batch[5], batch[6]))          # (the refused calls above left it a plain SAC learner)
    t.cuda.synchronize()
    plain.learner.check()
    assert plain.learner.update_count == 1
    _refused(plain, STATE, b"before the first")
    # while the mode is on
    h = on.learner.handle
    assert lib.oprl_learner_set_cql(h, 5.0, 2) == STATE and b"layer normalisation" in lib.oprl_last_error()
    assert lib.oprl_learner_set_calql(h, 1) == STATE and b"layer normalisation" in lib.oprl_last_error()
    g = C.c_void_p()
    handles = (C.c_void_p * 1)(h)
    assert lib.oprl_group_create(handles, 1, C.byref(g)) == STATE and b"layer normalisation" in lib.oprl_last_error()
    w = t.ones(B, device="cuda")
    td = t.zeros(B, device="cuda")
    rc = lib.oprl_learner_update_weighted(h, *(_capi.ptr(x) for x in batch[:5]), _capi.ptr(w), B, None, None, _capi.ptr(td),
                                          _capi.current_stream())
    assert rc == STATE and b"layer normalisation" in lib.oprl_last_error()
    buf = _replay(t.device("cuda", 0))
    rc = lib.oprl_learner_step_n_prio(h, buf.handle, 1, B, 3, 0.4, 1000.0, _capi.current_stream())
    assert rc == STATE and b"layer normalisation" in lib.oprl_last_error()
    # the data-parallel entry points need an export_grads learner, which the mode refuses: OPRL_ERR_STATE for this one
    ident = C.create_string_buffer(128)                 # OPRL_COMM_ID_BYTES
    assert lib.oprl_comm_init(h, None, 0, 1, ident) == STATE and b"export_grads" in lib.oprl_last_error()
    window = C.create_string_buffer(64)                # OPRL_P2P_HANDLE_BYTES
    assert lib.oprl_p2p_create(h, 0, 1, window) == STATE and b"export_grads" in lib.oprl_last_error()
    assert lib.oprl_learner_dp_update(h, *(_capi.ptr(x) for x in batch[:5]), B, None, None, _capi.current_stream()) == STATE
    # ... and the refused calls changed nothing: the learner with the mode on still meets the oracle
    o = lno.scenario_oracle("sac", None)
    run_pair(on, [o], lno.scenario_batches(600, B, 2), step, to_double)
    sc.compare(state_of(on, B), lno.digest(o), TOL, param_tol=sc.PARAM_TOL)
