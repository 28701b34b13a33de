"""CPU tests of REDQ's host side: the target-subset draw of the C-ABI (oprl_redq_subset) against a short Python
restatement of its documented algorithm, its statistics and argument checks; the Python class's import path and CPU
refusal; the trainer's update-to-data ratio."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from oprl_amd import _capi

M32 = 0xFFFFFFFF
M64 = (1 << 64) - 1


def lib():
    return _capi.load()


def draw(seed, rank, counter, n, m):
    out = (C.c_int32 * max(m, 1))()
    rc = lib().oprl_redq_subset(seed, rank, counter, n, m, out)
    return rc, list(out)[:m]


# ---- the documented draw, restated (include/oprl_amd.h oprl_redq_subset; csrc/philox.h; learner.hip noise_key)
def noise_key(seed, rank, stream):
    x = (seed ^ ((rank * 0x9E3779B97F4A7C15) & M64)) & M64
    if x:
        x = (x + 0x9E3779B97F4A7C15) & M64
        x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
        x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
        x ^= x >> 31
    return (0x0B5E55ED + stream + x) & M64


def philox4x32_10(ctr, k0, k1):
    x, y, z, w = ctr
    for _ in range(10):
        p0, p1 = 0xD2511F53 * x, 0xCD9E8D57 * z
        x, y, z, w = ((p1 >> 32) ^ y ^ k0) & M32, p1 & M32, ((p0 >> 32) ^ w ^ k1) & M32, p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return x, y, z, w


def py_subset(seed, rank, counter, n, m):
    key = noise_key(seed, rank, 3)
    perm = list(range(n))
    words = []
    for i in range(m):
        if i % 4 == 0:
            words = philox4x32_10((counter & M32, (counter >> 32) & M32, i // 4, 0), key & M32, key >> 32)
        j = i + ((words[i % 4] * (n - i)) >> 32)
        perm[i], perm[j] = perm[j], perm[i]
    return perm[:m]


def test_redq_subset_is_exported_and_bound():
    assert "oprl_redq_subset" in _capi.SIGNATURES
    assert hasattr(lib(), "oprl_redq_subset")
    assert _capi.ALGO["redq"] == 4 and _capi.OPRL_MAX_CRITICS == 10


@pytest.mark.parametrize("n,m", [(10, 2), (10, 1), (10, 3), (10, 10), (7, 5), (1, 1), (10, 9)])
def test_redq_subset_distinct_in_range_deterministic(n, m):
    for counter in (0, 1, 2, 17, 2 ** 33 + 5):
        rc, a = draw(7, 0, counter, n, m)
        assert rc == 0
        assert len(set(a)) == m and all(0 <= i < n for i in a), a
        assert draw(7, 0, counter, n, m)[1] == a
        if m == n:
            assert sorted(a) == list(range(n))


def test_redq_subset_changes_with_counter_seed_and_rank():
    base = [draw(7, 0, u, 10, 3)[1] for u in range(64)]
    assert len({tuple(x) for x in base}) > 32                      # the counter moves the draw
    assert base != [draw(8, 0, u, 10, 3)[1] for u in range(64)]    # the seed does
    assert base != [draw(7, 1, u, 10, 3)[1] for u in range(64)]    # and the rank


@pytest.mark.parametrize("m", [1, 2, 3])
def test_redq_subset_frequencies(m):
    """Over 20,000 counters every index turns up M/N of the time, within 5 sigma."""
    n, trials = 10, 20_000
    counts = np.zeros(n)
    for u in range(trials):
        for i in draw(11, 0, u, n, m)[1]:
            counts[i] += 1
    p = m / n
    sigma = np.sqrt(trials * p * (1 - p))
    assert np.all(np.abs(counts - trials * p) <= 5 * sigma), counts


@pytest.mark.parametrize("seed,rank", [(0, 0), (7, 0), (7, 3), (2 ** 63 + 12345, 1)])
def test_redq_subset_matches_the_documented_draw(seed, rank):
    for n, m in ((10, 2), (10, 5), (10, 10), (6, 4)):
        for counter in (0, 1, 99, 2 ** 32 + 1):
            assert draw(seed, rank, counter, n, m)[1] == py_subset(seed, rank, counter, n, m), (seed, rank, n, m, counter)


@pytest.mark.parametrize("n,m", [(10, 0), (10, 11), (11, 2), (0, 0), (3, 4), (-1, 1)])
def test_redq_subset_refuses_bad_sizes(n, m):
    out = (C.c_int32 * 16)()
    assert lib().oprl_redq_subset(0, 0, 0, n, m, out) == -1        # OPRL_ERR_INVALID
    assert b"oprl_redq_subset" in lib().oprl_last_error()


def test_redq_imports_and_has_no_cpu_path():
    from oprl.algos.redq import REDQ
    from oprl_amd.logging import NullLogger
    algo = REDQ(logger=NullLogger(), state_dim=24, action_dim=6, device="cpu")
    assert (algo.n_critics, algo.n_min, algo.utd_ratio, algo.tune_alpha, algo.alpha_init) == (10, 2, 20, True, 1.0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        algo.create()


class _Algo:
    def __init__(self, utd=None):
        self.calls = []
        self._created = True
        self.actor = self
        if utd is not None:
            self.utd_ratio = utd

    def check_created(self): pass
    def explore(self, s): return np.zeros(6, np.float32)
    def update(self, *batch): self.calls.append("update")
    def update_from_buffer(self, buf, B, act_next=None): self.calls.append("update_from_buffer")


class _Buffer:
    def __init__(self): self.n, self.calls, self.episodes_counter, self.last_episode_length = 0, [], 1, 0
    def check_created(self): pass
    def add_transition(self, *a, **k): self.n += 1
    def sample(self, B):
        import torch as t
        self.calls.append("sample")
        return tuple(t.zeros(B, 1) for _ in range(5))
    def __len__(self): return self.n


def _train(algo, buf, fused):
    from oprl_amd.environment import make_env
    from oprl_amd.logging import NullLogger
    from oprl_amd.trainers.base_trainer import BaseTrainer
    tr = BaseTrainer(logger=NullLogger("/tmp/oprl_amd_test"), env=make_env("walker-walk", 0),
                     make_env_test=lambda s: make_env("walker-walk", s), replay_buffer=buf, algo=algo,
                     num_steps=20, start_steps=100, batch_size=8, eval_interval=10 ** 9, save_policy_every=0,
                     stdout_log_every=10 ** 9, fused_sample_update=fused)
    tr.train()
    return 21 - 7          # environment steps with a full batch in the buffer


def test_trainer_runs_utd_ratio_updates_per_env_step():
    algo, buf = _Algo(utd=5), _Buffer()
    steps = _train(algo, buf, fused=False)
    assert algo.calls.count("update") == buf.calls.count("sample") == 5 * steps
    plain, buf2 = _Algo(), _Buffer()
    assert plain.calls == [] and _train(plain, buf2, fused=False) == plain.calls.count("update")


def test_fused_trainer_calls_update_from_buffer_once_per_env_step():
    algo, buf = _Algo(utd=5), _Buffer()
    steps = _train(algo, buf, fused=True)
    assert algo.calls.count("update_from_buffer") == steps and algo.calls.count("update") == 0
