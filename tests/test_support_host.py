"""The comparison discriminates, for the shared helpers of tests/support.py themselves: each assertion fails when it
should, on stub learners that expose only state_dict(), learner.check() and update_step, and passes when the difference
lies outside what the caller narrowed it to."""
from __future__ import annotations

import numpy as np
import pytest
import torch as t

from tests import support


class Stub:
    """A learner as assert_same_state sees it."""

    class _Learner:
        def __init__(self):
            self.checks = 0

        def check(self):
            self.checks += 1

    def __init__(self, n_targets=2, log_alpha=False, **extra):
        g = t.Generator().manual_seed(3)
        self.sd = {k: t.randn(8, generator=g) for k in support.STATE_KEYS}
        self.sd["targets"] = [t.randn(8, generator=g) for _ in range(n_targets)]
        self.sd["counters"] = [4, 4, 2, 0]
        if log_alpha:
            self.sd["log_alpha"] = [t.randn(1, generator=g) for _ in range(3)]
        self.sd.update(extra)
        self.learner = self._Learner()
        self.update_step = 4

    def state_dict(self):
        return self.sd


def flip_a_bit(x):
    x.view(t.int32)[0] ^= 1


def test_equal_states_pass_and_both_learners_are_checked():
    a, b = Stub(log_alpha=True, value_step=4), Stub(log_alpha=True, value_step=4)
    support.assert_same_state(a, b, extra=("value_step",))
    assert a.learner.checks == 1 and b.learner.checks == 1


@pytest.mark.parametrize("key", [*support.STATE_KEYS, "value"])
def test_a_flipped_bit_in_one_key_fails(key):
    a, b = Stub(value=t.ones(4)), Stub(value=t.ones(4))
    flip_a_bit(b.sd[key])
    extra = ("value",) if key == "value" else ()
    with pytest.raises(AssertionError, match=key):
        support.assert_same_state(a, b, extra=extra)
    if key == "value":
        support.assert_same_state(a, b)            # (not named: not compared)


def test_a_flipped_bit_in_a_target_fails():
    a, b = Stub(), Stub()
    flip_a_bit(b.sd["targets"][1])
    with pytest.raises(AssertionError, match=r"targets\[1\]"):
        support.assert_same_state(a, b)
    with pytest.raises(AssertionError, match=r"targets\[1\]"):
        support.assert_same_state(a, b, targets=(0, 1))


def test_a_missing_target_fails():
    a, b = Stub(n_targets=2), Stub(n_targets=1)
    with pytest.raises(AssertionError, match="targets"):
        support.assert_same_state(a, b)
    with pytest.raises(AssertionError, match="targets"):
        support.assert_same_state(b, a)


def test_log_alpha_on_one_side_only_fails_and_so_does_an_unequal_one():
    a, b = Stub(log_alpha=True), Stub()
    for x, y in ((a, b), (b, a)):
        with pytest.raises(AssertionError, match="log_alpha on one side only"):
            support.assert_same_state(x, y)
    c = Stub(log_alpha=True)
    flip_a_bit(c.sd["log_alpha"][2])
    with pytest.raises(AssertionError, match=r"log_alpha\[2\]"):
        support.assert_same_state(a, c)


def test_unequal_counters_fail_unless_told_not_to_compare_them():
    a, b = Stub(), Stub()
    b.sd["counters"] = [4, 4, 3, 0]
    with pytest.raises(AssertionError, match="counters"):
        support.assert_same_state(a, b)
    support.assert_same_state(a, b, counters=False)


def test_an_unequal_or_missing_extra_scalar_fails():
    a, b = Stub(value_step=4), Stub(value_step=5)
    with pytest.raises(AssertionError, match="value_step"):
        support.assert_same_state(a, b, extra=("value_step",))
    with pytest.raises(AssertionError, match="missing"):
        support.assert_same_state(a, Stub(), extra=("value_step",))


def test_the_narrowed_call_passes_when_the_difference_lies_outside_it():
    """The TD3+BC update-0 call: the critics, their moments and the first target list."""
    a, b = Stub(), Stub()
    narrow = dict(keys=("critic", "critic_m", "critic_v"), targets=(0,))
    for k in ("actor", "actor_m", "actor_v"):
        flip_a_bit(b.sd[k])
    flip_a_bit(b.sd["targets"][1])
    support.assert_same_state(a, b, **narrow)
    with pytest.raises(AssertionError):
        support.assert_same_state(a, b)
    flip_a_bit(b.sd["critic_v"])
    with pytest.raises(AssertionError, match="critic_v"):
        support.assert_same_state(a, b, **narrow)


def test_what_is_in_the_failure_message():
    a, b = Stub(), Stub()
    flip_a_bit(b.sd["critic"])
    with pytest.raises(AssertionError, match="update 3"):
        support.assert_same_state(a, b, what="update 3")


# ---- refused ---------------------------------------------------------------------------------------------------------------
def null_handle_call():
    """A real refusal without a GPU: OPRL_ERR_INVALID and a message that says 'null'."""
    from oprl_amd import _capi
    return _capi.load().oprl_learner_set_calql(None, 1)


def test_refused_returns_the_message_of_a_real_refusal():
    msg = support.refused(null_handle_call(), support.INVALID, b"null")
    assert isinstance(msg, bytes) and b"null" in msg
    assert support.refused(null_handle_call(), support.INVALID) == msg
    assert support.refused(null_handle_call(), support.INVALID, min_len=len(msg)) == msg


def test_refused_fails_on_a_wrong_status_a_missing_word_and_a_short_message():
    with pytest.raises(AssertionError):
        support.refused(null_handle_call(), support.STATE, b"null")
    with pytest.raises(AssertionError):
        support.refused(0, support.INVALID)
    with pytest.raises(AssertionError, match="no such word"):
        support.refused(null_handle_call(), support.INVALID, b"no such word")
    with pytest.raises(AssertionError):
        support.refused(null_handle_call(), support.INVALID, b"null", min_len=10 ** 4)


# ---- worst_ratio -----------------------------------------------------------------------------------------------------------
def test_worst_ratio_names_the_right_key_under_each_gate():
    from tests import scenarios as sc
    want = {"u.critic.0": np.ones(4), "u.m_actor.1": np.ones(4), "u.q": np.ones(4), "u.bc_lambda": np.ones(1)}
    got = {k: v.copy() for k, v in want.items()}
    assert support.worst_ratio(got, want, 2e-5)[0] == 0.0
    got["u.critic.0"][1] += 3 * sc.PARAM_TOL            # three parameter gates
    got["u.m_actor.1"][0] -= 2 * sc.PARAM_TOL           # two
    r, k = support.worst_ratio(got, want, 2e-5)
    assert k == "u.critic.0" and r == pytest.approx(3.0)
    got["u.q"][2] += 5 * 2e-5                           # five output gates: smaller in size, larger in gates
    r, k = support.worst_ratio(got, want, 2e-5)
    assert k == "u.q" and r == pytest.approx(5.0)
    got["u.bc_lambda"][0] = 2.0                         # a scalar key far off: counted at the output gate ...
    r, k = support.worst_ratio(got, want, 2e-5)
    assert k == "u.bc_lambda" and r == pytest.approx(1.0 / 2e-5)
    r, k = support.worst_ratio(got, want, 2e-5, params_only=True)          # ... and not at all with params_only
    assert k == "u.critic.0" and r == pytest.approx(3.0)
