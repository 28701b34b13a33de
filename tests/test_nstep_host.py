"""CPU tests of the n-step replay's host side: the C-ABI surface and its argument checks, the Python buffer's fields and
checks, the alias, the command-line flag, the gamma-mismatch refusal, and the properties of tests/nstep_oracle.py on
hand-written episodes (no GPU needed)."""
from __future__ import annotations

import sys

import numpy as np
import pytest

from oprl_amd import _capi
from tests import nstep_oracle as no
from tests import support

NSTEP_FUNCS = ["oprl_replay_set_nstep", "oprl_replay_sample_nstep"]


def cpu_buffer(**kw):
    from oprl_amd.buffers.nstep_buffer import NStepEpisodicReplayBuffer
    return support.cpu_buffer(NStepEpisodicReplayBuffer, **{**dict(state_dim=3, action_dim=1), **kw})


def test_nstep_functions_are_declared_bound_and_exported():
    support.assert_abi_bound(NSTEP_FUNCS)


def test_nstep_functions_refuse_null_handles_without_a_gpu():
    lib = _capi.load()
    assert lib.oprl_replay_set_nstep(None, 3, 0.99) == -1
    assert b"null replay handle" in lib.oprl_last_error()
    assert lib.oprl_replay_sample_nstep(None, 4, None, 0, 0, *([None] * 8), None) == -1
    assert len(lib.oprl_last_error()) > 0


def test_alias_and_defaults():
    from oprl.buffers.nstep_buffer import NStepEpisodicReplayBuffer as Aliased
    from oprl_amd.buffers.episodic_buffer import EpisodicReplayBuffer
    from oprl_amd.buffers.nstep_buffer import NStepEpisodicReplayBuffer
    assert Aliased is NStepEpisodicReplayBuffer and issubclass(Aliased, EpisodicReplayBuffer)
    b = cpu_buffer().create()
    assert (b.n_step, b.gamma) == (3, 0.99) and len(b) == 0
    assert not getattr(b, "prioritized", False)
    sd = b.state_dict()
    assert sd["n_step"] == 3
    c = cpu_buffer(n_step=5).create()
    c.load_state_dict(sd)
    assert c.n_step == 3


@pytest.mark.parametrize("kw", [dict(n_step=0), dict(n_step=17), dict(n_step=-1), dict(n_step=2.5), dict(gamma=0.0),
                                dict(gamma=1.5), dict(gamma=-0.9), dict(gamma=float("nan"))])
def test_bad_fields_are_refused(kw):
    with pytest.raises(ValueError):
        cpu_buffer(**kw).create()


@pytest.mark.parametrize("kw", [dict(n_step=1), dict(n_step=16), dict(gamma=1.0), dict(gamma=1e-3)])
def test_edge_fields_are_accepted(kw):
    cpu_buffer(**kw).create()


def test_cpu_buffer_is_a_host_container_without_a_sampler():
    b = cpu_buffer().create()
    b.add_transition(np.ones(3), np.zeros(1), 2.0, False)
    assert len(b) == 1 and float(b.rewards[0, 0, 0]) == 2.0
    with pytest.raises(RuntimeError, match="MI355X"):
        b.sample(4)


def test_n_step_flag(monkeypatch):
    from oprl_amd.parse_args import parse_args, parse_args_distrib
    monkeypatch.setattr(sys, "argv", ["x"])
    assert parse_args().n_step == 1 and parse_args_distrib().n_step == 1
    monkeypatch.setattr(sys, "argv", ["x", "--n-step", "5"])
    assert parse_args().n_step == 5 and parse_args_distrib().n_step == 5


def test_gamma_mismatch_is_refused_by_learners_and_trainer():
    from oprl_amd.algos.base_algorithm import OffPolicyAlgorithm
    from oprl_amd.algos.redq import REDQ
    from oprl_amd.trainers.base_trainer import BaseTrainer
    buf = cpu_buffer(n_step=3, gamma=0.95).create()

    class Algo:                     # update_from_buffer refuses before it touches the learner
        gamma = 0.99

        def check_created(self):
            pass
    with pytest.raises(ValueError, match="gamma"):
        OffPolicyAlgorithm.update_from_buffer(Algo(), buf, 4)
    with pytest.raises(ValueError, match="gamma"):
        REDQ.update_from_buffer(Algo(), buf, 4)
    tr = BaseTrainer.__new__(BaseTrainer)
    tr.algo, tr.replay_buffer = Algo(), buf
    with pytest.raises(ValueError, match="gamma"):
        tr.train()
    # n_step = 1 is one-step sampling: its gamma is never used, and is not checked
    from oprl_amd.algos.base_algorithm import check_nstep_gamma
    check_nstep_gamma(Algo(), cpu_buffer(n_step=1, gamma=0.5).create())
    check_nstep_gamma(Algo(), cpu_buffer(n_step=3, gamma=0.99).create())


# ---- the oracle on hand-written episodes ----------------------------------------------------------------------------
def storage():
    """E = 4, L = 6, S = 2, A = 1.  Episode 0: 6 steps, done at its last.  Episode 1: 4 steps, a done at step 1.
    Episode 2: 3 steps, never done (truncated).  Episode 3 is dead (its rows hold poison)."""
    E, L, S, A = 4, 6, 2, 1
    states = np.arange(E * (L + 1) * S, dtype=np.float32).reshape(E, L + 1, S)
    actions = -np.arange(E * L * A, dtype=np.float32).reshape(E, L, A)
    rewards = (1 + np.arange(E * L, dtype=np.float32)).reshape(E, L)
    dones = np.zeros((E, L), np.float32)
    dones[0, 5] = 1
    dones[1, 1] = 1
    rewards[2, 3:] = 1e9            # beyond episode 2's stored steps
    dones[2, 3:] = 1
    rewards[3], dones[3] = 1e9, 1
    return states, actions, rewards, dones, [6, 4, 3]


def test_oracle_m_stops_at_a_done_and_at_the_stored_end():
    st, ac, rw, dn, lens = storage()
    g = no.nstep_gather(st, ac, rw, dn, lens, np.arange(13), 3, 0.5)
    #            episode 0 (t = 0..5)  episode 1 (t = 0..3)  episode 2 (t = 0..2)
    assert list(g["m"]) == [3, 3, 3, 3, 2, 1, 2, 1, 2, 1, 3, 2, 1]
    assert list(g["ep"]) == [0] * 6 + [1] * 4 + [2] * 3 and list(g["step"]) == [0, 1, 2, 3, 4, 5, 0, 1, 2, 3, 0, 1, 2]
    # R: plain sums at gamma = 0.5 (exact in float32)
    assert g["r"][0, 0] == 1 + 0.5 * 2 + 0.25 * 3
    assert g["r"][4, 0] == 5 + 0.5 * 6 and g["r"][5, 0] == 6
    assert g["r"][6, 0] == 7 + 0.5 * 8                    # stops AFTER the done step, which is included
    assert g["r"][10, 0] == 13 + 0.5 * 14 + 0.25 * 15     # stops at the stored end: the poison is never read
    assert np.all(g["r"] < 1e3)
    # d': 1 where the last step is terminal, 1 - gamma^(m-1) where it is not
    assert g["d"][3, 0] == 1.0 and g["d"][4, 0] == 1.0 and g["d"][5, 0] == 1.0 and g["d"][6, 0] == 1.0
    assert g["d"][0, 0] == 1 - 0.25 and g["d"][11, 0] == 1 - 0.5 and g["d"][12, 0] == 0.0
    # s' = s_{t+m}, in the same episode row
    assert np.array_equal(g["s2"], st[g["ep"], g["step"] + g["m"]])
    assert np.array_equal(g["s"], st[g["ep"], g["step"]]) and np.array_equal(g["a"], ac[g["ep"], g["step"]])


def test_oracle_n1_is_the_identity():
    st, ac, rw, dn, lens = storage()
    dn[2, 1] = 0.5                                        # a non-binary done travels verbatim
    g = no.nstep_gather(st, ac, rw, dn, lens, np.arange(13), 1, 0.9)
    ep, t = g["ep"], g["step"]
    assert np.all(g["m"] == 1)
    assert np.array_equal(g["r"][:, 0], rw[ep, t]) and np.array_equal(g["d"][:, 0], dn[ep, t])
    assert np.array_equal(g["s2"], st[ep, t + 1])


def test_oracle_index_past_every_end_takes_one_step_of_episode_zero():
    st, ac, rw, dn, lens = storage()
    g = no.nstep_gather(st, ac, rw, dn, [2, 1], [4], 5, 0.9)     # 3 live transitions: index 4 is past every end
    assert (g["ep"][0], g["step"][0], g["m"][0]) == (0, 4, 1)    # the reference's all-True argmin, as the plain gather
    assert g["r"][0, 0] == rw[0, 4] and np.array_equal(g["s2"][0], st[0, 5])


@pytest.mark.parametrize("gamma", [0.9, 0.99, 1.0])
def test_effective_discount_is_within_half_an_ulp_of_one(gamma):
    """What the learner forms, gamma * fl(1 - d'), against gamma^m (1 - d_last), for d in {0, 1} and every m <= 16."""
    pw = no.powers(gamma)
    for m in range(1, 17):
        for d_last in (0.0, 1.0):
            r = np.ones(m, np.float32)
            d = np.zeros(m, np.float32)
            d[-1] = d_last
            _R, m_got, d_out = no.scan(r, d, m, pw)
            assert m_got == m
            eff = gamma * float(np.float32(1) - d_out)
            assert abs(eff - gamma ** m * (1 - d_last)) <= 2.0 ** -24, (gamma, m, d_last)
