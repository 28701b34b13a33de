"""Host side of D4PG (no GPU): the C-ABI additions are declared, exported and bound, the build lists the new source,
configs/d4pg.py parses its flags, what the Python class refuses it refuses before the GPU is touched, and the oracle's
scatter projection is the kernel's gather formula."""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np
import pytest
import torch as t

from oprl_amd import _capi
from oprl_amd.algos.d4pg import D4PG
from oprl_amd.logging import NullLogger
from tests import d4pg_oracle as do
from tests.config_scripts import load_config
from tests.support import assert_abi_bound, assert_class_refuses, assert_source_built

ROOT = Path(__file__).resolve().parents[1]


def test_the_abi_additions_are_bound():
    assert _capi.ALGO["d4pg"] == 5
    lib, header = assert_abi_bound({"oprl_c51_seed": 14})
    assert "OPRL_D4PG = 5" in header
    names = [f[0] for f in _capi.OprlHparams._fields_]
    assert names[-2:] == ["v_min", "v_max"] and names[-3] == "n_min"          # appended: no earlier field moved
    assert _capi.OprlHparams.v_min.offset == _capi.OprlHparams.n_min.offset + 8   # (the int32 tail is padded to 8)
    assert _capi.OprlLearnerConfig._fields_[-1][0] == "hp"
    # null arguments are refused without a GPU
    assert lib.oprl_c51_seed(None, None, None, None, 0.99, -1.0, 1.0, 5, 4, 8, None, None, None, None) == -1
    assert b"null" in lib.oprl_last_error()


def test_the_build_lists_the_new_source():
    assert_source_built("c51_seed")


def test_exports():
    import oprl.algos.d4pg
    import oprl_amd.algos
    assert oprl.algos.d4pg.D4PG is D4PG and oprl_amd.algos.D4PG is D4PG
    from oprl_amd.algos.nn_models import CategoricalCritic
    c = CategoricalCritic(3, 2, n_atoms=5, v_min=-1.0, v_max=1.0)
    s, a = t.randn(7, 3), t.randn(7, 2)
    with t.no_grad():
        logits = c(s, a)
        q = c.Q1(s, a)
    assert logits.shape == (7, 5)
    assert q.shape == (7, 1) and float(q.abs().max()) <= 1.0
    assert t.allclose(q[:, 0], (t.softmax(logits, 1) * t.linspace(-1, 1, 5)).sum(1))


def test_the_config_script_parses_its_flags(monkeypatch):
    mod = load_config(monkeypatch, "d4pg", ["--env", "walker-walk"])
    assert (mod.script.args.atoms, mod.script.args.v_min, mod.script.args.v_max) == (41, -150.0, 150.0)
    assert mod.atoms_of(mod.script.args) == dict(n_atoms=41, v_min=-150.0, v_max=150.0)
    mod = load_config(monkeypatch, "d4pg", ["--env", "walker-walk", "--atoms", "31", "--v-min", "-10", "--v-max", "90",
                                            "--n-step", "3", "--num-envs", "4", "--open-episodes"])
    args = mod.script.args
    assert (args.atoms, args.v_min, args.v_max, args.n_step, args.num_envs, args.open_episodes) == (31, -10.0, 90.0, 3, 4, True)
    assert mod.config.state_dim == 24 and mod.config.action_dim == 6
    assert mod.script.algo_cls is D4PG and not mod.script.takes_per
    with pytest.raises(ValueError, match="--per"):
        load_config(monkeypatch, "d4pg", ["--env", "walker-walk", "--per"])
    # the other scripts still parse as before
    from oprl_amd.parse_args import parse_args
    monkeypatch.setattr(sys, "argv", ["ddpg.py"])
    assert not hasattr(parse_args(), "atoms")


@pytest.mark.parametrize("kw,msg", [
    (dict(n_atoms=51), "48"),
    (dict(n_atoms=1), "n_atoms"),
    (dict(v_min=1.0, v_max=1.0), "v_max"),
    (dict(v_min=2.0, v_max=-2.0), "v_max"),
    (dict(precision="x2"), "f32"),
    (dict(precision="bf16"), "f32"),
    (dict(prioritized=True), "priorit"),
    (dict(export_grads=True), "export_grads"),
], ids=["51-atoms", "1-atom", "empty-support", "reversed-support", "x2", "bf16", "prioritized", "export_grads"])
def test_the_class_refuses_before_any_gpu_call(kw, msg, monkeypatch):
    """ValueError at construction; and again from create() for fields set afterwards — before require_gpu, which a
    machine without a GPU would fail with RuntimeError instead."""
    import oprl_amd.algos.d4pg as mod
    assert_class_refuses(D4PG, mod, kw, msg, monkeypatch)


def test_the_prioritized_refusal_names_the_follow_up():
    with pytest.raises(ValueError, match="follow-up"):
        D4PG(logger=NullLogger(), state_dim=4, action_dim=2, prioritized=True)


def test_a_prioritized_buffer_is_refused():
    from oprl_amd.algos.base_algorithm import refuse_prioritized

    class Buf:
        prioritized = True
    with pytest.raises(ValueError, match="importance weights"):
        refuse_prioritized(D4PG(logger=NullLogger(), state_dim=4, action_dim=2), Buf())


def gather_projection(p, b):
    """The kernel's form in numpy float64: m_j = sum_i p_i max(0, 1 - |b_i - j|), i in index order."""
    B, N = p.shape
    m = np.zeros((B, N))
    j = np.arange(N, dtype=np.float64)
    for i in range(N):
        m += p[:, i:i + 1] * np.maximum(0.0, 1.0 - np.abs(b[:, i:i + 1] - j[None, :]))
    return m


def offset_projection(p, r, d, gamma, v_min, v_max):
    """The kernel's arithmetic in numpy float64: the fractional index as an offset from the atom's own index,
    b_i - i = (r - (1 - g) v_min) / delta - (1 - g) i clamped to [-i, N - 1 - i], and 1 - |(b_i - i) + (i - j)|."""
    B, N = p.shape
    delta = (v_max - v_min) / (N - 1)
    omg = 1.0 - (1.0 - d) * gamma
    i = np.arange(N, dtype=np.float64)[None, :]
    off = np.clip((r - omg * v_min)[:, None] / delta - omg[:, None] * i, -i, (N - 1) - i)
    m = np.zeros((B, N))
    for k in range(N):
        m += p[:, k:k + 1] * np.maximum(0.0, 1.0 - np.abs(off[:, k:k + 1] + (k - i)))
    return m


@pytest.mark.parametrize("N", [2, 5, 41, 48])
def test_scatter_and_gather_projections_agree(N):
    """Random rows (fractional b, clamped ends, terminal rows) and rows whose b is an integer everywhere: the oracle's
    floor / ceil scatter equals the gather over triangular weights to float64 rounding, and both conserve the mass."""
    rs = np.random.RandomState(N)
    B, v_min, delta = 64, -4.0, 0.5
    v_max = v_min + (N - 1) * delta
    p = rs.dirichlet(np.ones(N), B)
    r = rs.uniform(v_min - 2, v_max + 2, B)
    d = (rs.uniform(0, 1, B) < 0.3).astype(np.float64)
    r[:8] = v_min + rs.randint(0, N, 8) * delta          # terminal rows on an atom: integer b
    d[:8] = 1.0
    r[8:12], d[8:12] = 0.0, 0.0                          # gamma = 1 below: the grid maps onto itself, integer b
    zs = do.atoms(N, v_min, v_max)
    for gamma in (0.99, 1.0):
        b = do.fractional_index(t.from_numpy(r), t.from_numpy(d), gamma, zs, v_min, v_max)
        if gamma == 1.0:
            assert t.equal(b[8:12], b[8:12].round()) and t.equal(b[:8], b[:8].round())
        m_s = do.project_scatter(t.from_numpy(p), b).numpy()
        m_g = gather_projection(p, b.numpy())
        assert np.abs(m_s - m_g).max() < 1e-14
        assert np.abs(m_s - offset_projection(p, r, d, gamma, v_min, v_max)).max() < 1e-13
        assert np.abs(m_s.sum(1) - 1).max() < 1e-13 and m_s.min() >= 0
        if gamma == 1.0:
            assert np.array_equal(m_s[8:12], p[8:12])        # the identity map: every atom keeps its mass
            assert np.allclose(np.sort(m_s[:8], 1)[:, -1], 1.0)   # a terminal row on an atom: all mass there
