"""The hindsight sampler's cost (needs a GPU).  Walker dims, a 1000 x 1000 replay, every slot live;
the goals are the last 3 + 3 columns of the 24-float state row, ratio 0.8, strategy future, sparse reward.

    rocprofv3 --kernel-trace --stats -d DIR -o her --output-format csv -- python tools/probe_her.py gather
    python tools/probe_her.py parse DIR/.../her_kernel_trace.csv
        kernel time of k_replay_gather and of k_replay_gather_her at B = 256 and 1024: `gather` issues ITERS launches
        per configuration in a fixed order, `parse` cuts the trace into those runs
    python tools/probe_her.py events
        the same four configurations timed with device events around ITERS back-to-back launches (launch gaps
        included: an upper bound on the kernel time, for a run without a profiler)
    python tools/probe_her.py rate
        DDPG B = 256 f32 step_n in updates/s over a plain and a hindsight replay, alternating"""
import csv
import sys
import time
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

ITERS = 300
CONFIGS = [(B, her) for B in (256, 1024) for her in (False, True)]
LAYOUT = (18, 21, 3, 0.8, 0, 0, 0.5)      # ag_off, g_off, G, ratio, strategy, reward, threshold


def _set_her(buf, on):
    from oprl_amd import _capi
    args = LAYOUT if on else (0, 0, 0, 0.0, 0, 0, 0.0)
    _capi.check(buf._lib.oprl_replay_set_her(buf.handle, *args), "oprl_replay_set_her")


def _launches(timed):
    import torch as t
    import bench
    from oprl_amd import _capi
    dev = t.device("cuda", 0)
    buf = bench.make_replay(dev, 0)
    lib, h, S, A = buf._lib, buf.handle, buf.state_dim, buf.action_dim
    st = _capi.current_stream()
    for B, her in CONFIGS:
        out = [t.empty((B, w), dtype=t.float32, device=dev) for w in (S, A, 1, 1, S)]
        p = [_capi.ptr(x) for x in out]
        _set_her(buf, her)
        ev = [t.cuda.Event(enable_timing=True) for _ in range(2)]
        for i in range(ITERS + 20):
            if i == 20:
                ev[0].record()
            if her:
                _capi.check(lib.oprl_replay_sample_her(h, B, None, 0, i, *p, None, None, None, st), "oprl_replay_sample_her")
            else:
                _capi.check(lib.oprl_replay_sample(h, B, None, 0, i, *p, None, None, st), "oprl_replay_sample")
        ev[1].record()
        t.cuda.synchronize()
        name = "k_replay_gather_her" if her else "k_replay_gather    "
        if timed:
            print(f"B={B:5d} {name}: {ev[0].elapsed_time(ev[1]) / ITERS * 1e3:.2f} us per launch, back to back", flush=True)
        else:
            print(f"B={B} her={her}: {ITERS + 20} launches", flush=True)
    _set_her(buf, False)


def parse(path):
    import numpy as np
    rows = [r for r in csv.DictReader(open(path)) if "k_replay_gather" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    n = ITERS + 20
    assert len(rows) == n * len(CONFIGS), (len(rows), n * len(CONFIGS))
    for j, (B, her) in enumerate(CONFIGS):
        run = rows[j * n:(j + 1) * n]
        names = {("her" if "gather_her" in r["Kernel_Name"] else "plain") for r in run}
        assert names == ({"her"} if her else {"plain"}), (B, her, names)
        us = np.array([int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in run[20:]]) / 1e3
        print(f"B={B:5d} {'k_replay_gather_her' if her else 'k_replay_gather    '}: median {np.median(us):.2f} us, "
              f"mean {us.mean():.2f}, min {us.min():.2f}, p90 {np.percentile(us, 90):.2f}")


def rate():
    import torch as t
    import bench
    dev = t.device("cuda", 0)
    plain = bench.make_replay(dev, 0)
    her = bench.make_replay(dev, 0)
    _set_her(her, True)
    t.manual_seed(0)
    L = bench._make_algo("DDPG", 24, 6, 256, {}, dev, "f32").learner
    K = 4000
    best = {"plain": 1e9, "her": 1e9}
    for rep in range(4):
        for name, buf in (("plain", plain), ("her", her)):
            L.step_n(buf.handle, 200, 256, seed=rep)
            t.cuda.synchronize()
            t0 = time.perf_counter()
            L.step_n(buf.handle, K, 256, seed=rep)
            t.cuda.synchronize()
            dt = time.perf_counter() - t0
            best[name] = min(best[name], dt)
            print(f"rep {rep} {name:5s}: {dt / K * 1e6:.2f} us/update ({K / dt / 1e3:.1f}k updates/s)", flush=True)
    L.check()
    print("best: " + ", ".join(f"{k} {K / v / 1e3:.1f}k updates/s ({v / K * 1e6:.2f} us)" for k, v in best.items()), flush=True)


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "rate"
    if mode == "parse":
        parse(sys.argv[2])
    else:
        {"gather": lambda: _launches(False), "events": lambda: _launches(True), "rate": rate}[mode]()
