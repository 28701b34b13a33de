"""Host time of writing one step of N open episodes, to be run on the MI355X:

  python tools/probe_open_episodes.py       # one JSON line per N

At walker dims (S = 24, A = 6), a replay of 1000 episodes x 1000 steps, N = 16, 64, 256 environments:

lanes:      host time per ``add_step_rows`` call — 2000 calls (every lane closes its episode at step 1000), the stream
            synchronised once at the end and that wait counted.
assembler:  what the path it replaces costs per iteration in the same build: N ``EpisodeAssembler.add`` calls per
            iteration and, every 1000 iterations, N ``add_transitions(1000 rows, episode_done=True)`` — 2000 iterations,
            synchronised at the end; the share of the ``add_transitions`` calls is reported on its own.
Two alternating passes, the best of the two.  The assembler path is the yardstick; no figure is fixed in advance."""
from __future__ import annotations

import json
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

import numpy as np  # noqa: E402
import torch as t  # noqa: E402

CALLS, S, A, E, L = 2000, 24, 6, 1000, 1000


def _buffer():
    from oprl_amd.buffers.episodic_buffer import EpisodicReplayBuffer
    return EpisodicReplayBuffer(buffer_size_transitions=E * L, state_dim=S, action_dim=A, max_episode_lenth=L,
                                device="cuda").create()


def _data(n: int):
    rs = np.random.RandomState(n)
    return (rs.standard_normal((n, S)).astype(np.float32), rs.uniform(-1, 1, (n, A)).astype(np.float32),
            rs.standard_normal(n).astype(np.float32), np.zeros(n, np.float32), rs.standard_normal((n, S)).astype(np.float32))


def lanes_pass(buf, n: int, data, first_call: int) -> float:
    never, all_of_them = np.zeros(n, bool), np.ones(n, bool)
    t.cuda.synchronize()
    t0 = time.perf_counter()
    for call in range(first_call, first_call + CALLS):
        buf.add_step_rows(*data, all_of_them if (call + 1) % L == 0 else never)
    t.cuda.synchronize()
    return (time.perf_counter() - t0) / CALLS * 1e6


def assembler_pass(buf, n: int, data) -> tuple[float, float]:
    from oprl_amd.trainers.vec_trainer import EpisodeAssembler
    asm = EpisodeAssembler(n)
    s, a, r, _d, _s2 = data
    in_buffer = 0.0
    t.cuda.synchronize()
    t0 = time.perf_counter()
    for call in range(CALLS):
        over = (call + 1) % L == 0
        for i in range(n):
            rows = asm.add(i, s[i], a[i], float(r[i]), False, over)
            if rows is not None:
                t1 = time.perf_counter()
                buf.add_transitions(rows, episode_done=True)
                in_buffer += time.perf_counter() - t1
    t.cuda.synchronize()
    return (time.perf_counter() - t0) / CALLS * 1e6, in_buffer / CALLS * 1e6


def probe(n: int) -> dict:
    data = _data(n)
    lanes, classic = _buffer(), _buffer()
    lanes.open_lanes(n)
    best = {"lanes": float("inf"), "assembler": float("inf"), "add_transitions": float("inf")}
    for k in range(2):
        best["lanes"] = min(best["lanes"], lanes_pass(lanes, n, data, k * CALLS))
        whole, share = assembler_pass(classic, n, data)
        best["assembler"], best["add_transitions"] = min(best["assembler"], whole), min(best["add_transitions"], share)
    return {"add_step_rows_us_per_call": round(best["lanes"], 2), "assembler_us_per_iteration": round(best["assembler"], 2),
            "of_which_add_transitions_us": round(best["add_transitions"], 2),
            "floats_per_launch": n * (2 * S + A + 4)}


if __name__ == "__main__":
    assert t.cuda.is_available(), "this probe measures the GPU path"
    for n in (16, 64, 256):
        print(json.dumps({"probe": "open_episodes", "device": t.cuda.get_device_name(0), "calls": CALLS, "n": n,
                          **probe(n)}), flush=True)
