"""Host time of acting in rows against acting row by row, to be run on the MI355X:

  python tools/probe_act_rows.py            # both parts, one JSON line each

rows:      host time per call of ``exploit_rows(N)`` against N x ``exploit`` for N = 1, 10, 16, 64, 256 at walker dims
           (S = 24, A = 6, DDPG actor): 2000 calls each, two alternating passes, the best of the two.
evaluate:  wall time of ``BaseTrainer.evaluate`` against ``VecTrainer.evaluate`` at 10 episodes x 1000 steps of the
           synthetic walker.
The yardstick is the existing single-row path in the same build; no speed-up is fixed in advance."""
from __future__ import annotations

import json
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

import numpy as np  # noqa: E402
import torch as t  # noqa: E402

CALLS = 2000


def _algo():
    from oprl_amd.algos.ddpg import DDPG
    from oprl_amd.logging import NullLogger
    t.manual_seed(0)
    return DDPG(logger=NullLogger("/tmp/oprl_amd_probe"), state_dim=24, action_dim=6, device="cuda").create()


def _time(fn, calls: int) -> float:
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    return (time.perf_counter() - t0) / calls * 1e6


def rows(algo) -> dict:
    actor = algo.actor
    out = {}
    for n in (1, 10, 16, 64, 256):
        x = np.random.RandomState(n).standard_normal((n, 24)).astype(np.float32)

        def batched():
            actor.exploit_rows(x)

        def one_by_one():
            for r in x:
                actor.exploit(r)

        single_calls = max(CALLS // n, 20)          # (N x exploit per call: fewer calls, the same number of rows or more)
        batched(), one_by_one()
        best = [float("inf"), float("inf")]
        for _ in range(2):
            best[0] = min(best[0], _time(batched, CALLS))
            best[1] = min(best[1], _time(one_by_one, single_calls))
        out[str(n)] = {"exploit_rows_us": round(best[0], 2), "n_x_exploit_us": round(best[1], 2),
                       "ratio": round(best[1] / best[0], 2)}
    return out


def evaluate(algo) -> dict:
    from oprl_amd.environment.synthetic import SyntheticEnv
    from oprl_amd.logging import NullLogger
    from oprl_amd.trainers.base_trainer import BaseTrainer
    from oprl_amd.trainers.vec_trainer import VecTrainer

    def make_env(seed):
        return SyntheticEnv("walker-walk", seed, episode_length=1000)

    kw = dict(logger=NullLogger("/tmp/oprl_amd_probe"), make_env_test=make_env, replay_buffer=None, algo=algo,
              num_eval_episodes=10, seed=0)
    base, vec = BaseTrainer(env=make_env(0), **kw), VecTrainer(envs=[make_env(0)], **kw)
    res = {}
    for name, tr in (("base", base), ("vec", vec), ("base", base), ("vec", vec)):
        t0 = time.perf_counter()
        ret = tr.evaluate()["return"]
        dt = time.perf_counter() - t0
        if name not in res or dt < res[name]["seconds"]:
            res[name] = {"seconds": round(dt, 4), "return": ret}
    res["ratio"] = round(res["base"]["seconds"] / res["vec"]["seconds"], 2)
    return res


if __name__ == "__main__":
    assert t.cuda.is_available(), "this probe measures the GPU path"
    algo = _algo()
    print(json.dumps({"probe": "act_rows.rows", "device": t.cuda.get_device_name(0), "calls": CALLS, "rows": rows(algo)}), flush=True)
    print(json.dumps({"probe": "act_rows.evaluate", "episodes": 10, "steps": 1000, **evaluate(algo)}), flush=True)
