"""DroQ, and REDQ / SAC with ``dropout > 0``, through the learner against tests/droq_oracle.py (float64,
autograd, the kernel's Philox mask restated in numpy — no noise injection is needed for it): parity within the suite's gates,
the wrong oracles it is at least ten gates away from, the launch counts (dropout adds none), step_n against sample() +
update(), resume in the middle of a group, ``dropout=0.0`` against a learner built without the field, and the C-level
refusals."""
from __future__ import annotations

import pytest
import torch as t

from oprl_amd import _capi
from oprl_amd.algos.droq import DroQ
from oprl_amd.algos.redq import REDQ
from oprl_amd.algos.sac import SAC
from oprl_amd.logging import NullLogger
from tests import droq_oracle as do
from tests import ln_oracle as lno
from tests import scenarios as sc
from tests import support
from tests.hip_adapters import load_params
from tests.support import INVALID, STATE, check_step_n_equals_loop, run_pair, to_double, worst_ratio
from tests.test_gpu_ln import LN_KEYS, RANK, SEED, _replay, slice_launches, state_of, step, subset

pytestmark = pytest.mark.gpu

S, A, N, G = do.S, do.A, do.N, do.G
TOL = 2e-5                          # network outputs (tests/test_gpu_algos.py)


def n_critics(name):
    return N if name == "redq" else 2


def make(name, B, rate, scenario=True, **kw):
    """The learner of a scenario ("droq": N = 2, M = 2, G = 3; "redq": N = 10, M = 2, G = 3; "sac": a tuned temperature)
    with the fixture nets and gamma / beta of tests/ln_oracle.py loaded into it."""
    common = dict(logger=NullLogger(), state_dim=S, action_dim=A, log_every=10 ** 9, max_batch=max(B, 256))
    if rate is not None:
        kw["dropout"] = rate
    if name == "droq":
        algo = DroQ(utd_ratio=G, **common, **kw).create()
    elif name == "redq":
        algo = REDQ(n_critics=N, n_min=2, utd_ratio=G, layer_norm=True, **common, **kw).create()
    else:
        algo = SAC(tune_alpha=True, layer_norm=True, **common, **kw).create()
    algo.set_seed(SEED, RANK)
    if scenario:
        actor, critics, ln = lno.scenario_params("redq" if name == "redq" else "sac")
        load_params(algo.actor, [x.cuda() for x in actor])
        flat = [x.cuda() for c in critics for x in c]
        load_params(algo.critic, flat)
        load_params(algo.critic_target, flat)
        with t.no_grad():
            algo.critic_ln.theta.data.copy_(ln.cuda())
            algo.critic_ln.target.copy_(ln.cuda())
    return algo


def oracle(name, rate, **kw):
    return do.scenario_oracle(name, subset(n_critics(name), 2), rate, **kw)


@pytest.mark.parametrize("name,B,rate,seed", do.SCENARIOS, ids=[f"{n}-B{b}-p{r}" for n, b, r, _ in do.SCENARIOS])
def test_dropout_learners_match_the_oracle(name, B, rate, seed):
    """Four updates (G = 3: critic-only updates before and after an actor step; B = 100 is a ragged batch; REDQ's ten
    critics go out as two 5-net launches, j up to 9; SAC's actor phase is a forward-only and a backward-only launch that
    draw the same mask): every critic, target, the actor, both optimisers' moments, log alpha and its moments, the last
    q / y rows, and gamma / beta, their targets and their moments."""
    algo = make(name, B, rate)
    assert algo.learner.state_dict()["critic_dropout"] == rate
    o = oracle(name, rate)
    run_pair(algo, [o], lno.scenario_batches(seed, B, 4), step, to_double)
    assert algo.learner.update_count == 4
    got, want = state_of(algo, B), lno.digest(o)
    assert "u.critic.0.ln" in want and "u.m_critic.ln" in want and "u.log_alpha_m" in want
    print("worst: %.3f gates at %s" % worst_ratio(got, want, TOL))
    sc.compare(got, want, TOL, param_tol=sc.PARAM_TOL)


def test_the_comparison_discriminates():
    """One DroQ learner at rate 0.1 meets the right oracle and is ten gates or more away from plain LN critics, one mask per
    update, targets without dropout and rows numbered inside their slice.  The fifth knob, ``no_scale``, is printed and NOT
    asserted: LayerNorm cancels a common factor of its input up to eps / var, forward and backward, so the scale reaches no
    parameter of a learner (measured on the CPU between the two float64 oracles: 0.34 gates here); tests/test_gpu_droq_slice.py
    holds it on rstd and dz, where it shows."""
    B = 256
    algo = make("droq", B, 0.1)
    right = oracle("droq", 0.1)
    wrong = {k: oracle("droq", 0.1, **{k: True}) for k in do.KNOBS}
    run_pair(algo, [right, *wrong.values()], lno.scenario_batches(100, B, 4), step, to_double)
    got = state_of(algo, B)
    print("right: %.3f gates at %s" % worst_ratio(got, lno.digest(right), TOL))
    sc.compare(got, lno.digest(right), TOL, param_tol=sc.PARAM_TOL)
    for k, o in wrong.items():
        r, key = worst_ratio(got, lno.digest(o), TOL)
        print(f"{k}: {r:.1f} gates at {key}")
        if k != "no_scale":
            assert r >= 10.0, f"{k}: the learner is only {r:.1f} gates away from the wrong oracle"


def test_launch_counts():
    """Section 24's counts, to which dropout adds nothing.  DroQ (N = 2, M = 2): critic-only 3 (actor on s' 1, targets 1,
    critics 1), actor step 6 (+ actor forward 1, critics on (s, pi) 1, actor backward 1); REDQ N = 10: 4, 4, 8; SAC: 7."""
    B = 256
    data = [tuple(x.cuda() for x in b) for b in lno.scenario_batches(100, B, G)]
    droq = make("droq", B, 0.1)
    assert [slice_launches(droq, b) for b in data] == [3, 3, 6]
    redq = make("redq", B, 0.1)
    assert [slice_launches(redq, b) for b in data] == [4, 4, 8]
    sac = make("sac", B, 0.1)
    assert [slice_launches(sac, b) for b in data[:2]] == [7, 7]
    t.cuda.synchronize()
    for algo in (droq, redq, sac):
        algo.learner.check()


def assert_same_state(a, b):
    x = a.state_dict()
    assert "critic_ln" in x and "log_alpha" in x and float(x["critic_ln_v"].abs().max()) > 0.0
    assert x.get("critic_dropout") == b.state_dict().get("critic_dropout")
    support.assert_same_state(a, b, extra=LN_KEYS)


def test_step_n_equals_sample_then_update_bitwise():
    """step_n(K = G) over a replay with 2 % done rows is bit for bit G times sample() + update() with the sampler's rows:
    the masks follow the update count, which both paths advance alike."""
    B, dev = 256, t.device("cuda", 0)
    buf = _replay(dev)
    fused, loop, n_done = check_step_n_equals_loop(lambda: (make("droq", B, 0.1), make("droq", B, 0.1)), buf, B, K=G, extra=LN_KEYS)
    assert_same_state(fused, loop)
    assert n_done > 0


def test_resume_in_the_middle_of_a_group():
    """state_dict() after update 1 of a G group, loaded into a fresh learner, continues bit for bit: nothing of the masks
    is state beyond the update count.  The rate rides in the dict, and only a learner of that rate loads it."""
    B = 256
    data = lno.scenario_batches(100, B, 5)
    a = make("droq", B, 0.1)
    for x in data[:1]:
        step(a, x)
    b = make("droq", B, 0.1, scenario=False)
    b.load_state_dict(a.state_dict())
    for x in data[1:]:
        for algo in (a, b):
            step(algo, x)
    assert a.update_step == 5
    assert_same_state(a, b)
    plain = make("droq", B, 0.0)
    assert "critic_dropout" not in plain.state_dict()
    with pytest.raises(ValueError, match="critic_dropout"):
        plain.load_state_dict(a.state_dict())
    with pytest.raises(ValueError, match="critic_dropout"):
        a.load_state_dict(plain.state_dict())


@pytest.mark.parametrize("name", ["sac", "redq"])
def test_rate_zero_changes_nothing(name):
    """dropout=0.0 and a learner built without the field: after three updates the same bits."""
    B = 100
    a, b = make(name, B, 0.0), make(name, B, None)
    assert a.learner._dropout == 0.0 and "critic_dropout" not in a.state_dict()
    for x in lno.scenario_batches(100, B, 3):
        for algo in (a, b):
            step(algo, x)
    support.assert_same_state(a, b, extra=LN_KEYS)
    # ... and a rate below 2^-32 leaves the mode off through the C call too
    c = make(name, B, None)
    c.learner.set_dropout(1e-12)
    assert c.learner._dropout == 0.0
    for x in lno.scenario_batches(100, B, 3):
        step(c, x)
    support.assert_same_state(a, c, extra=LN_KEYS)


def test_set_dropout_refuses_with_its_codes_and_leaves_the_learner_usable():
    B = 100
    lib = _capi.load()
    common = dict(logger=NullLogger(), state_dim=S, action_dim=A, log_every=10 ** 9, max_batch=256)
    batch = [x.cuda() for x in lno.scenario_batches(100, B, 1)[0]]
    call = lambda algo, rate: lib.oprl_learner_set_dropout(algo.learner.handle, rate)      # noqa: E731
    # OPRL_ERR_STATE: before oprl_learner_set_layernorm — and the learner stays plain SAC
    plain = SAC(**common, no_fuse=True, tune_alpha=True).create()
    support.refused(call(plain, 0.1), STATE, b"oprl_learner_set_layernorm comes first")
    plain.update(*batch[:5], noise=(batch[5], batch[6]))
    t.cuda.synchronize()
    plain.learner.check()
    assert plain.learner.update_count == 1
    # OPRL_ERR_INVALID: the rates, on a learner whose LN mode is on
    ln = make("sac", B, None)
    for rate in (1.0, 1.5, -0.1, float("nan"), float("inf")):
        support.refused(call(ln, rate), INVALID, b"[0, 1)")
    assert lib.oprl_learner_set_dropout(None, 0.1) == INVALID
    # ... which is still an LN learner without dropout: it meets the rate-0 oracle
    o = oracle("sac", 0.0)
    run_pair(ln, [o], lno.scenario_batches(100, B, 2), step, to_double)
    sc.compare(state_of(ln, B), lno.digest(o), TOL, param_tol=sc.PARAM_TOL)
    # OPRL_ERR_STATE: after an update; a second call
    support.refused(call(ln, 0.1), STATE, b"before the first")
    on = make("sac", B, 0.1)
    support.refused(call(on, 0.1), STATE, b"already on")
    support.refused(call(on, 0.2), STATE, b"already on")
    with pytest.raises(RuntimeError, match="already on"):
        on.learner.set_dropout(0.2)
    assert on.learner._dropout == 0.1
    # everything the LN mode refuses stays refused
    h = on.learner.handle
    assert lib.oprl_learner_set_cql(h, 5.0, 2) == STATE and b"layer normalisation" in lib.oprl_last_error()
    w, td = t.ones(B, device="cuda"), t.zeros(B, device="cuda")
    rc = lib.oprl_learner_update_weighted(h, *(_capi.ptr(x) for x in batch[:5]), _capi.ptr(w), B, None, None, _capi.ptr(td),
                                          _capi.current_stream())
    assert rc == STATE and b"layer normalisation" in lib.oprl_last_error()
    # ... and the refused calls changed nothing: the learner with the mode on still meets the oracle at ITS rate
    o = oracle("sac", 0.1)
    run_pair(on, [o], lno.scenario_batches(100, B, 2), step, to_double)
    sc.compare(state_of(on, B), lno.digest(o), TOL, param_tol=sc.PARAM_TOL)
