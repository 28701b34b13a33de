"""Training from prioritized replay, the parts that need no GPU: the new entry points are declared, exported and bound
and refuse null handles; ``--per`` parses and its bad pairings are refused; the algorithms' ``prioritized`` field is
checked before anything touches the GPU; ``refuse_prioritized`` lets a prioritized algorithm through."""
from __future__ import annotations

import sys
from pathlib import Path

import pytest

from oprl_amd import _capi, parse_args as pa

ROOT = Path(__file__).resolve().parents[1]
NEW = ("oprl_learner_update_weighted", "oprl_learner_step_n_prio")


def test_new_entry_points_are_declared_exported_and_bound():
    header = (ROOT / "include" / "oprl_amd.h").read_text()
    lib = _capi.load()
    assert _capi.OPRL_ABI_VERSION == 4 and lib.oprl_abi_version() == 4       # additive: the version stays
    for name in NEW:
        assert f"int {name}(" in header, name
        assert name in _capi.SIGNATURES and hasattr(lib, name), name
    assert len(_capi.SIGNATURES["oprl_learner_update_weighted"][1]) == 12
    assert len(_capi.SIGNATURES["oprl_learner_step_n_prio"][1]) == 8
    assert "per_seed.hip" in __import__("oprl_amd.build", fromlist=["SOURCES"]).SOURCES


def test_null_handles_are_refused_with_a_message():
    lib = _capi.load()
    assert lib.oprl_learner_update_weighted(*([None] * 7), 4, *([None] * 4)) == -1
    assert b"oprl_learner_update_weighted" in lib.oprl_last_error()
    assert lib.oprl_learner_step_n_prio(None, None, 1, 4, 0, 0.4, 1e6, None) == -1
    assert b"oprl_learner_step_n_prio" in lib.oprl_last_error()


@pytest.mark.parametrize("parse", [pa.parse_args, pa.parse_args_distrib], ids=["single", "distrib"])
def test_per_flag_parses_and_bad_pairings_are_refused(parse, monkeypatch):
    monkeypatch.setattr(sys, "argv", ["prog"])
    args = parse()
    assert args.per is False and pa.check_per(args) is False
    monkeypatch.setattr(sys, "argv", ["prog", "--per"])
    args = parse()
    assert args.per is True and pa.check_per(args) is True
    monkeypatch.setattr(sys, "argv", ["prog", "--per", "--n-step", "3"])
    with pytest.raises(ValueError, match="n-step"):
        pa.check_per(parse())
    monkeypatch.setattr(sys, "argv", ["prog", "--n-step", "3"])
    assert pa.check_per(parse()) is False


def test_prioritized_field_is_checked_before_any_gpu_call():
    from oprl_amd.algos.ddpg import DDPG
    from oprl_amd.algos.redq import REDQ
    from oprl_amd.algos.sac import SAC
    from oprl_amd.algos.td3 import TD3
    from oprl_amd.algos.tqc import TQC
    from oprl_amd.logging import NullLogger
    with pytest.raises(ValueError, match="follow-up"):
        TQC(logger=NullLogger(), state_dim=3, action_dim=1, prioritized=True)
    assert TQC(logger=NullLogger(), state_dim=3, action_dim=1).prioritized is False
    for cls in (DDPG, TD3, SAC, REDQ):
        assert cls(logger=NullLogger(), state_dim=3, action_dim=1).prioritized is False
        # (device="cpu" would raise RuntimeError from require_gpu: the ValueError comes first)
        with pytest.raises(ValueError, match="precision='f32'"):
            cls(logger=NullLogger(), state_dim=3, action_dim=1, prioritized=True, precision="x2", device="cpu").create()
        with pytest.raises(ValueError, match="export"):
            cls(logger=NullLogger(), state_dim=3, action_dim=1, prioritized=True, export_grads=True, device="cpu").create()


def test_refuse_prioritized_lets_a_prioritized_algorithm_through():
    from oprl_amd.algos.base_algorithm import refuse_prioritized, trains_prioritized

    class Algo:
        prioritized = False

    class Buf:
        prioritized = True
        handle = None
    with pytest.raises(ValueError, match="importance weights"):
        refuse_prioritized(Algo(), Buf())
    algo = Algo()
    algo.prioritized = True
    refuse_prioritized(algo, Buf())                     # no exception
    refuse_prioritized(Algo(), object())                # a plain buffer: nothing to refuse
    assert not trains_prioritized(algo, Buf())          # (no device handle: no weighted path)
    assert not trains_prioritized(algo, object())
