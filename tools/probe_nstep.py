"""The n-step sampler's cost (needs a GPU).  Walker dims, a 1000 x 1000 replay, every slot live.

    rocprofv3 --kernel-trace --stats -d DIR -o nstep --output-format csv -- python tools/probe_nstep.py gather
    python tools/probe_nstep.py parse DIR/.../nstep_kernel_trace.csv
        kernel time of k_replay_gather and of k_replay_gather_nstep at n = 1, 3, 5, B = 256 and 1024: `gather` issues
        ITERS launches per configuration in a fixed order, `parse` cuts the trace into those runs
    python tools/probe_nstep.py rate
        DDPG B = 256 f32 step_n in updates/s over the replay without n-step and with n = 3, alternating"""
import csv
import sys
import time
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

ITERS = 300
CONFIGS = [(B, n) for B in (256, 1024) for n in (0, 1, 3, 5)]      # n = 0: the plain gather


def gather():
    import torch as t
    import bench
    from oprl_amd import _capi
    dev = t.device("cuda", 0)
    buf = bench.make_replay(dev, 0)
    lib, h, S, A = buf._lib, buf.handle, buf.state_dim, buf.action_dim
    st = _capi.current_stream()
    for B, n in CONFIGS:
        out = [t.empty((B, w), dtype=t.float32, device=dev) for w in (S, A, 1, 1, S)]
        p = [_capi.ptr(x) for x in out]
        _capi.check(lib.oprl_replay_set_nstep(h, max(n, 1), 0.99), "oprl_replay_set_nstep")
        for i in range(ITERS):
            if n == 0:
                _capi.check(lib.oprl_replay_sample(h, B, None, 0, i, *p, None, None, st), "oprl_replay_sample")
            else:
                _capi.check(lib.oprl_replay_sample_nstep(h, B, None, 0, i, *p, None, None, None, st), "oprl_replay_sample_nstep")
        t.cuda.synchronize()
        print(f"B={B} n={n}: {ITERS} launches", flush=True)


def parse(path):
    import numpy as np
    rows = [r for r in csv.DictReader(open(path)) if "k_replay_gather" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    assert len(rows) == ITERS * len(CONFIGS), (len(rows), ITERS * len(CONFIGS))
    for j, (B, n) in enumerate(CONFIGS):
        run = rows[j * ITERS:(j + 1) * ITERS]
        names = {("nstep" if "nstep" in r["Kernel_Name"] else "plain") for r in run}
        assert names == ({"plain"} if n == 0 else {"nstep"}), (B, n, names)
        us = np.array([int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in run[20:]]) / 1e3
        print(f"B={B:5d} {'k_replay_gather        ' if n == 0 else f'k_replay_gather_nstep n={n}'}: median {np.median(us):.2f} us, "
              f"mean {us.mean():.2f}, min {us.min():.2f}, p90 {np.percentile(us, 90):.2f}")


def rate():
    import torch as t
    import bench
    dev = t.device("cuda", 0)
    plain = bench.make_replay(dev, 0)
    nstep = bench.make_replay(dev, 0)
    from oprl_amd import _capi
    _capi.check(nstep._lib.oprl_replay_set_nstep(nstep.handle, 3, 0.99), "oprl_replay_set_nstep")
    t.manual_seed(0)
    L = bench._make_algo("DDPG", 24, 6, 256, {}, dev, "f32").learner
    K = 4000
    best = {"plain": 1e9, "n=3": 1e9}
    for rep in range(4):
        for name, buf in (("plain", plain), ("n=3", nstep)):
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
        {"gather": gather, "rate": rate}[mode]()
