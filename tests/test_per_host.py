"""CPU tests of prioritized replay's host side: the C-ABI surface and its argument checks, the Python buffer's fields,
checks and beta schedule, the tree layout, the refusal of a prioritized buffer by the learners and the trainer, and the
restatement of tests/per_oracle.py against the spec's properties (no GPU needed)."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from oprl_amd import _capi
from tests import per_oracle as po
from tests import support

PRIO_FUNCS = ["oprl_replay_prio_enable", "oprl_replay_prio_sample", "oprl_replay_prio_update",
              "oprl_replay_prio_read", "oprl_replay_prio_load"]


def cpu_buffer(**kw):
    from oprl_amd.buffers.prioritized_buffer import PrioritizedEpisodicReplayBuffer
    return support.cpu_buffer(PrioritizedEpisodicReplayBuffer, **{**dict(state_dim=3, action_dim=1), **kw})


def test_prio_functions_are_exported_and_bound():
    support.assert_abi_bound(PRIO_FUNCS)


def test_prio_functions_refuse_bad_arguments_without_a_gpu():
    lib = _capi.load()
    assert lib.oprl_replay_prio_enable(None, 0.6, 1e-6, None) == -1
    assert lib.oprl_replay_prio_sample(None, 4, 0, 0, 0.4, *([None] * 7), None) == -1
    assert lib.oprl_replay_prio_update(None, 4, None, None, None) == -1
    n = C.c_int64()
    assert lib.oprl_replay_prio_read(None, None, 0, C.byref(n), None, None) == -1
    assert lib.oprl_replay_prio_load(None, None, 1.0, None) == -1
    assert b"null replay handle" in lib.oprl_last_error()


def test_alias_and_defaults():
    from oprl.buffers.prioritized_buffer import PrioritizedEpisodicReplayBuffer as Aliased
    from oprl_amd.buffers.prioritized_buffer import PrioritizedEpisodicReplayBuffer
    assert Aliased is PrioritizedEpisodicReplayBuffer
    b = cpu_buffer().create()
    assert (b.alpha, b.beta0, b.beta_steps, b.eps) == (0.6, 0.4, 1e6, 1e-6)
    assert b.prioritized and len(b) == 0


@pytest.mark.parametrize("kw", [dict(alpha=-0.1), dict(beta0=-0.01), dict(beta0=1.5), dict(eps=0.0), dict(eps=-1e-6),
                                dict(beta_steps=0)])
def test_bad_hyperparameters_are_refused(kw):
    with pytest.raises(ValueError):
        cpu_buffer(**kw).create()


def test_beta_anneals_linearly_to_one():
    b = cpu_buffer(beta0=0.4, beta_steps=1000).create()
    assert b.beta(0) == 0.4
    assert b.beta(500) == 0.4 + 0.6 * 500 / 1000
    assert b.beta(1000) == 1.0 and b.beta(10 ** 9) == 1.0


def test_cpu_buffer_has_no_sampler():
    b = cpu_buffer().create()
    b.add_transition(np.zeros(3), np.zeros(1), 0.0, False)
    with pytest.raises(RuntimeError, match="MI355X"):
        b.sample(4)
    with pytest.raises(RuntimeError, match="MI355X"):
        b.update_priorities([0], [1.0])


def test_tree_layout():
    assert po.tree_layout(350) == ([350, 2, 1], [0, 512, 768, 1024])
    counts, offs = po.tree_layout(10 ** 6)
    assert counts == [10 ** 6, 3907, 16, 1] and offs[-1] == 1000192 + 4096 + 256 + 256
    assert po.tree_layout(1) == ([1, 1], [0, 256, 512])


def test_learners_and_trainer_refuse_a_prioritized_buffer():
    from oprl_amd.algos.base_algorithm import OffPolicyAlgorithm
    from oprl_amd.algos.redq import REDQ
    from oprl_amd.trainers.base_trainer import BaseTrainer
    buf = cpu_buffer().create()

    class Algo:                     # update_from_buffer refuses before it touches the learner
        pass
    with pytest.raises(ValueError, match="prioritized"):
        OffPolicyAlgorithm.update_from_buffer(Algo(), buf, 4)
    with pytest.raises(ValueError, match="prioritized"):
        REDQ.update_from_buffer(Algo(), buf, 4)

    class Created:
        def check_created(self):
            pass
    tr = BaseTrainer.__new__(BaseTrainer)
    tr.algo, tr.replay_buffer = Created(), buf
    with pytest.raises(ValueError, match="prioritized"):
        tr.train()


def test_restated_nodes_are_sums_of_their_children():
    rng = np.random.default_rng(0)
    leaves = (rng.random(5000) * (rng.random(5000) < 0.7)).astype(np.float32)
    tree = po.build(leaves)
    counts, offs = po.tree_layout(len(leaves))
    root = tree[offs[-2]]
    assert abs(float(root) - leaves.astype(np.float64).sum()) < 1e-5 * leaves.sum()
    assert np.all(tree[offs[1] + counts[1]:offs[2]] == 0)          # padding


def test_restated_descent_is_proportional_and_never_returns_a_zero_leaf():
    rng = np.random.default_rng(1)
    n = 700
    leaves = rng.random(n).astype(np.float32) + 0.05
    leaves[::3] = 0                                                 # zeros interleaved with the mass
    leaves[-40:] = 0
    tree = po.build(leaves)
    B = 2000
    slots = np.array(po.descend(tree, n, B, seed=5, counter=3))
    assert np.all(leaves[slots] > 0)
    # stratified: draw j lies in segment j, so the slots are non-decreasing and every leaf with more than a segment's
    # mass is drawn
    assert np.all(np.diff(slots) >= 0)
    seg = leaves.astype(np.float64).sum() / B
    assert set(np.nonzero(leaves > seg)[0]) <= set(slots.tolist())
    counts = np.bincount(slots, minlength=n)
    expect = B * leaves / leaves.astype(np.float64).sum()
    assert np.all(np.abs(counts - expect) <= 2)                     # at most one boundary draw off per side


def test_restated_descent_of_an_empty_tree():
    tree = po.build(np.zeros(300, np.float32))
    assert po.descend(tree, 300, 4, 0, 0) == [-1] * 4


def test_model_update_rules():
    m = po.TreeModel(2, 4, alpha=0.5, eps=1e-6)
    m.enable([3, 2], 2)
    assert list(m.leaves) == [1, 1, 1, 0, 1, 1, 0, 0]
    m.update([0, 0, 5, 6], [3.0, 8.0, 0.25, 99.0])                  # slot 0 twice: the later row; slot 6 is dead
    assert m.leaves[0] == po.priority(8.0, 0.5, 1e-6) and m.leaves[5] == po.priority(0.25, 0.5, 1e-6)
    assert m.leaves[6] == 0 and m.p_max == po.priority(8.0, 0.5, 1e-6)
    m.flush([(1, 0), (1, 1), (1, 2)], [3, 3], 2)                    # episode 1 evicted and refilled to 3 steps
    assert list(m.leaves[4:]) == [m.p_max] * 3 + [0]
