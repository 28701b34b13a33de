"""Which learner calls ``update_from_buffer`` makes (no GPU): DDPG, SAC and REDQ objects that were never created, over a
learner, an actor MLP, a logger and replay buffers that only record what is called on them.  Every case's call list —
``step_n``, ``step_act``, ``step_act_rows``, ``step_n_prio``, ``update``, ``read_scalars``, the actor's ``set_pending`` /
``set_pending_rows`` and the logger's steps — must be the one tests/golden/update_dispatch.json holds, or the same refusal.

The file was recorded with ``python -m tests.test_update_dispatch_host --record`` at the commit before the algorithm
classes came to share ``OffPolicyAlgorithm.update_from_buffer`` (REDQ had a copy of it with a hand-written search for
the logged step): what it holds is that commit's behaviour, REDQ's logged step included, and it is not regenerated.
A learner that exports gradients is a case of DDPG and SAC only: REDQ's copy had no test for it, and the learner refuses
to create a REDQ that does."""
from __future__ import annotations

import inspect
import json
import sys
from itertools import product
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

from oprl_amd.algos.ddpg import DDPG
from oprl_amd.algos.redq import REDQ
from oprl_amd.algos.sac import SAC

GOLDEN = Path(__file__).resolve().parent / "golden" / "update_dispatch.json"
S, A, B = 4, 2, 8
ALGOS = {"ddpg": (DDPG, {}), "sac": (SAC, dict(log_every=4)), "redq": (REDQ, dict(utd_ratio=3, log_every=4))}
ACT_NEXT = {"none": None, "1d": np.zeros(S, np.float32), "2d": np.zeros((3, S), np.float32)}


def plain(x):
    """An argument as JSON holds it."""
    if isinstance(x, np.ndarray):
        return {"shape": list(x.shape)}
    if isinstance(x, (RecordingLearner, RecordingMLP)):
        return type(x).__name__
    return x


def recorded(fn):
    """The method records its name and its arguments by name (however the caller passed them), then runs."""
    sig = inspect.signature(fn)

    def call(self, *a, **kw):
        bound = sig.bind(self, *a, **kw)
        bound.apply_defaults()
        self.calls.append([fn.__name__, {k: plain(v) for k, v in list(bound.arguments.items())[1:]}])
        return fn(self, *a, **kw)
    return call


class RecordingLearner:
    """The learner's surface ``update_from_buffer`` and ``update`` reach; the update count advances as the real one's."""

    def __init__(self, calls, start: int, export_grads: bool):
        self.calls, self.update_count, self.export_grads = calls, start, export_grads

    @recorded
    def step_n(self, replay_handle, K, B, seed):
        self.update_count += K

    @recorded
    def step_n_prio(self, replay_handle, K, B, seed, beta0, beta_steps):
        self.update_count += K

    @recorded
    def step_act(self, replay_handle, B, seed, obs):
        self.update_count += 1

    @recorded
    def step_act_rows(self, replay_handle, K, B, seed, obs):
        self.update_count += K

    @recorded
    def update(self, state, action, reward, done, next_state, noise0=None, noise1=None):
        self.update_count += 1

    @recorded
    def update_weighted(self, state, action, reward, done, next_state, weights, noise0=None, noise1=None):
        self.update_count += 1

    @recorded
    def read_scalars(self):
        return dict.fromkeys(("critic_loss", "actor_loss", "q_mean", "q_target_mean", "alpha", "update_step", "q1_mean",
                              "log_pi_mean", "gauss_actor_loss", "alpha_loss"), 0.0)


class RecordingMLP:
    def __init__(self, calls, gpu: bool):
        self.calls, self.gpu = calls, gpu

    def on_gpu(self):
        return self.gpu

    @recorded
    def set_pending(self, obs, learner):
        pass

    @recorded
    def set_pending_rows(self, obs, learner):
        pass


class RecordingLogger:
    def __init__(self, calls):
        self.calls = calls

    def log_scalar(self, tag, value, step):
        self.calls.append(["log", {"tags": 1, "step": step}])

    def log_scalars(self, values, step):
        self.calls.append(["log", {"tags": len(values), "step": step}])


def make_buffer(kind: str, calls):
    """``handle``: a device replay; ``host``: neither handle nor seed; ``nstep``: 3-step rows with the algorithm's gamma;
    ``gamma``: ... with another; ``prio``: a sum tree on the device."""
    def sample(batch_size):
        calls.append(["sample", {"batch_size": batch_size}])
        return "state", "action", "reward", "done", "next_state"
    buf = SimpleNamespace(sample=sample)
    if kind != "host":
        buf.handle, buf.seed = "replay", 7
    if kind in ("nstep", "gamma"):
        buf.n_step, buf.gamma = 3, 0.99 if kind == "nstep" else 0.9
    if kind == "prio":
        buf.prioritized, buf.beta0, buf.beta_steps = True, 0.4, 1000.0
    return buf


def cases():
    for name, n, act, buf, start, prio in product(ALGOS, (1, 5), ACT_NEXT, ("handle", "host", "nstep", "prio"), (0, 6), (False, True)):
        yield dict(algo=name, n_updates=n, act_next=act, buffer=buf, start=start, prioritized=prio)
    for name in ALGOS:
        yield dict(algo=name, n_updates=0, act_next="none", buffer="handle", start=0, prioritized=False)      # refused
        yield dict(algo=name, n_updates=1, act_next="none", buffer="gamma", start=0, prioritized=False)       # refused
        yield dict(algo=name, n_updates=5, act_next="1d", buffer="handle", start=6, prioritized=False, mlp_on_gpu=False)
    for name, act in product(("ddpg", "sac"), ACT_NEXT):
        yield dict(algo=name, n_updates=5, act_next=act, buffer="handle", start=6, prioritized=False, export_grads=True)


def case_id(case) -> str:
    return "-".join(f"{k}={v}" for k, v in case.items())


CASES = {case_id(c): c for c in cases()}


def run_case(case) -> dict:
    calls: list = []
    cls, kw = ALGOS[case["algo"]]
    algo = cls(logger=RecordingLogger(calls), state_dim=S, action_dim=A, prioritized=case["prioritized"], **kw)
    algo.learner = RecordingLearner(calls, case["start"], case.get("export_grads", False))
    mlp = RecordingMLP(calls, case.get("mlp_on_gpu", True))
    algo.actor = SimpleNamespace(mlp=mlp) if case["algo"] == "ddpg" else SimpleNamespace(net=mlp)
    algo._created = True
    try:
        algo.update_from_buffer(make_buffer(case["buffer"], calls), B, act_next=ACT_NEXT[case["act_next"]],
                                n_updates=case["n_updates"])
    except ValueError as e:
        return {"refused": str(e), "calls": calls}
    return {"calls": calls, "update_count": algo.update_step}


@pytest.fixture(scope="module")
def golden():
    return json.loads(GOLDEN.read_text())


def test_the_golden_file_holds_these_cases(golden):
    assert sorted(golden) == sorted(CASES)
    assert sum("refused" in g for g in golden.values()) >= 2 * len(ALGOS)
    # REDQ logs the first multiple of log_every = 4 among the K = n_updates x utd_ratio = 3, 15 updates of one call
    for n, start, step in ((1, 0, 0), (1, 6, 8), (5, 0, 0), (5, 6, 8)):
        g = golden[f"algo=redq-n_updates={n}-act_next=none-buffer=handle-start={start}-prioritized=False"]
        assert g["calls"][0] == ["step_n", dict(replay_handle="replay", K=3 * n, B=B, seed=7)]
        assert [c[1]["step"] for c in g["calls"] if c[0] == "log"] == [step] * 3


@pytest.mark.parametrize("cid", sorted(CASES))
def test_update_from_buffer_makes_the_recorded_calls(cid, golden):
    assert json.loads(json.dumps(run_case(CASES[cid]))) == golden[cid]


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: python -m tests.test_update_dispatch_host --record")
    GOLDEN.write_text("{\n" + ",\n".join(f"{json.dumps(cid)}: {json.dumps(run_case(c))}" for cid, c in sorted(CASES.items())) + "\n}\n")
    print(f"{len(CASES)} cases -> {GOLDEN}")
