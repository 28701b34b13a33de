"""What Cal-QL costs (needs a GPU).  Walker dims, a 1000 x 1000 replay with every slot live and no
done, so that a slot at step 0 has a full-length tail of 1000 steps (16 chunks of 64).  Every step that uses the GPU runs
under a time limit of its own, and the steps are chained so that a failure ends the chain:

    timeout -k 10 300 rocprofv3 --kernel-trace --stats -d DIR -o calql --output-format csv -- python tools/probe_calql.py returns \\
      && timeout -k 10 60 python tools/probe_calql.py parse DIR/.../calql_kernel_trace.csv
        kernel time of k_replay_returns at B = 256 and 1024, full-length tails (t = 0) and the uniform sampler's slots
        (mean tail 500 steps): `returns` issues ITERS launches per configuration in a fixed order, `parse` cuts the trace
        into those runs
    timeout -k 10 120 python tools/probe_calql.py events
        the same configurations timed with device events around ITERS back-to-back launches (launch gaps included: an
        upper bound on the kernel time, for a run without a profiler)
    timeout -k 10 300 python tools/probe_calql.py rate
        step_n in updates/s of CQL and of CalQL on the same learner shape (walker dims, B = 256, N = 10, f32), alternating"""
import csv
import sys
import time
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

ITERS = 300
CONFIGS = [(B, tails) for B in (256, 1024) for tails in ("full", "sampled")]
GAMMA = 0.99


def _slots(buf, B, tails, dev):
    import torch as t
    if tails == "full":
        return (t.arange(B, dtype=t.int32, device=dev) % len(buf.ep_lens)).contiguous(), t.zeros(B, dtype=t.int32, device=dev)
    _rows, (ep, step) = buf.sample(B, return_indices=True)
    return ep, step


def _launches(timed):
    import torch as t
    import bench
    from oprl_amd import _capi
    dev = t.device("cuda", 0)
    buf = bench.make_replay(dev, 0)
    lib, h, st = buf._lib, buf.handle, _capi.current_stream()
    for B, tails in CONFIGS:
        ep, step = _slots(buf, B, tails, dev)
        out = t.empty(B, dtype=t.float32, device=dev)
        ev = [t.cuda.Event(enable_timing=True) for _ in range(2)]
        t.cuda.synchronize()
        for i in range(ITERS + 20):
            if i == 20:
                ev[0].record()
            _capi.check(lib.oprl_replay_returns(h, B, _capi.ptr(ep), _capi.ptr(step), GAMMA, _capi.ptr(out), st), "oprl_replay_returns")
        ev[1].record()
        t.cuda.synchronize()
        mean_tail = float((buf.max_episode_lenth - step.float()).mean())
        if timed:
            print(f"B={B:5d} {tails:7s} (mean tail {mean_tail:.0f} steps): {ev[0].elapsed_time(ev[1]) / ITERS * 1e3:.2f} us per launch, "
                  f"back to back; G[0] = {float(out[0]):.4f}", flush=True)
        else:
            print(f"B={B} {tails}: {ITERS + 20} launches", flush=True)


def parse(path):
    import numpy as np
    rows = [r for r in csv.DictReader(open(path)) if "k_replay_returns" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    n = ITERS + 20
    assert len(rows) == n * len(CONFIGS), (len(rows), n * len(CONFIGS))
    for j, (B, tails) in enumerate(CONFIGS):
        us = np.array([int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in rows[j * n:(j + 1) * n][20:]]) / 1e3
        print(f"B={B:5d} {tails:7s} k_replay_returns: median {np.median(us):.2f} us, mean {us.mean():.2f}, min {us.min():.2f}, "
              f"p90 {np.percentile(us, 90):.2f}")


def rate():
    import torch as t
    import bench
    from oprl_amd.algos.calql import CalQL
    from oprl_amd.algos.cql import CQL
    from oprl_amd.logging import NullLogger
    dev = t.device("cuda", 0)
    buf = bench.make_replay(dev, 0)
    learners = {}
    for name, cls in (("CQL", CQL), ("CalQL", CalQL)):
        t.manual_seed(0)
        learners[name] = cls(logger=NullLogger(), state_dim=24, action_dim=6, device="cuda", max_batch=256, log_every=10 ** 9).create().learner
    K = 1000
    best = {k: 1e9 for k in learners}
    for rep in range(3):
        for name, L in learners.items():
            L.step_n(buf.handle, 100, 256, seed=rep)
            t.cuda.synchronize()
            t0 = time.perf_counter()
            L.step_n(buf.handle, K, 256, seed=rep)
            t.cuda.synchronize()
            dt = time.perf_counter() - t0
            best[name] = min(best[name], dt)
            print(f"rep {rep} {name:5s}: {dt / K * 1e6:.2f} us/update ({K / dt:.0f} updates/s)", flush=True)
    for name, L in learners.items():
        L.check()
        print(f"{name}: read_cql {L.read_cql()}", flush=True)
    print("best: " + ", ".join(f"{k} {K / v:.0f} updates/s ({v / K * 1e6:.2f} us)" for k, v in best.items()), flush=True)


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "rate"
    if mode == "parse":
        parse(sys.argv[2])
    else:
        {"returns": lambda: _launches(False), "events": lambda: _launches(True), "rate": rate}[mode]()
