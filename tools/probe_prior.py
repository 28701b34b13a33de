"""The mixed sampler's cost (needs a GPU).  Walker dims, a 1000 x 1000 online replay and a
200 x 1000 prior, every slot live, share 0.5.

    rocprofv3 --kernel-trace --stats -d DIR -o prior --output-format csv -- python tools/probe_prior.py gather
    python tools/probe_prior.py parse DIR/.../prior_kernel_trace.csv
        kernel time of k_replay_gather and of k_replay_gather_mix at B = 256 and 1024: `gather` issues ITERS launches
        per configuration in a fixed order, `parse` cuts the trace into those runs
    python tools/probe_prior.py events
        the same four configurations timed with device events around ITERS back-to-back launches (launch gaps
        included: an upper bound on the kernel time, for a run without a profiler)
    python tools/probe_prior.py rate
        DDPG B = 256 f32 step_n in updates/s over the plain and the mixed replay, alternating"""
import csv
import sys
import time
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

ITERS = 300
CONFIGS = [(B, mix) for B in (256, 1024) for mix in (False, True)]
PRIOR_EPISODES, SHARE = 200, 0.5


def _replays(dev):
    """(plain online replay, mixed replay of the same contents over a 200-episode prior)."""
    import torch as t
    import bench
    from oprl_amd.buffers.episodic_buffer import EpisodicReplayBuffer
    from oprl_amd.buffers.prior_buffer import PriorDataReplayBuffer
    plain = bench.make_replay(dev, 0)
    S, A, L = plain.state_dim, plain.action_dim, plain.max_episode_lenth
    prior = EpisodicReplayBuffer(buffer_size_transitions=PRIOR_EPISODES * L, state_dim=S, action_dim=A, device=str(dev)).create()
    mixed = PriorDataReplayBuffer(buffer_size_transitions=plain.buffer_size_transitions, state_dim=S, action_dim=A,
                                  device=str(dev), prior=prior, prior_share=SHARE).create()
    g = t.Generator(device=dev).manual_seed(99)
    for k, v in prior._tensors.items():
        v.copy_(t.zeros_like(v) if k == "dones" else t.rand(v.shape, device=dev, generator=g) * 2 - 1)
    for k, v in mixed._tensors.items():
        v.copy_(plain._tensors[k])
    for buf, E in ((prior, PRIOR_EPISODES), (mixed, len(plain.ep_lens))):
        buf.ep_lens = [L] * E
        buf.episodes_counter = E
        buf._number_transitions = E * L
        buf._lens_dirty = True
    return plain, mixed


def _launches(timed):
    import torch as t
    from oprl_amd import _capi
    dev = t.device("cuda", 0)
    plain, mixed = _replays(dev)
    lib, S, A = plain._lib, plain.state_dim, plain.action_dim
    hp, hm = plain.handle, mixed.handle
    st = _capi.current_stream()
    for B, mix in CONFIGS:
        out = [t.empty((B, w), dtype=t.float32, device=dev) for w in (S, A, 1, 1, S)]
        p = [_capi.ptr(x) for x in out]
        ev = [t.cuda.Event(enable_timing=True) for _ in range(2)]
        for i in range(ITERS + 20):
            if i == 20:
                ev[0].record()
            if mix:
                _capi.check(lib.oprl_replay_sample_mix(hm, B, None, 0, i, *p, None, None, None, st), "oprl_replay_sample_mix")
            else:
                _capi.check(lib.oprl_replay_sample(hp, B, None, 0, i, *p, None, None, st), "oprl_replay_sample")
        ev[1].record()
        t.cuda.synchronize()
        name = "k_replay_gather_mix" if mix else "k_replay_gather    "
        if timed:
            print(f"B={B:5d} {name}: {ev[0].elapsed_time(ev[1]) / ITERS * 1e3:.2f} us per launch, back to back", flush=True)
        else:
            print(f"B={B} mix={mix}: {ITERS + 20} launches", flush=True)


def parse(path):
    import numpy as np
    rows = [r for r in csv.DictReader(open(path)) if "k_replay_gather" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    n = ITERS + 20
    assert len(rows) == n * len(CONFIGS), (len(rows), n * len(CONFIGS))
    for j, (B, mix) in enumerate(CONFIGS):
        run = rows[j * n:(j + 1) * n]
        names = {("mix" if "gather_mix" in r["Kernel_Name"] else "plain") for r in run}
        assert names == ({"mix"} if mix else {"plain"}), (B, mix, names)
        us = np.array([int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in run[20:]]) / 1e3
        print(f"B={B:5d} {'k_replay_gather_mix' if mix else 'k_replay_gather    '}: median {np.median(us):.2f} us, "
              f"mean {us.mean():.2f}, min {us.min():.2f}, p90 {np.percentile(us, 90):.2f}")


def rate():
    import torch as t
    import bench
    dev = t.device("cuda", 0)
    plain, mixed = _replays(dev)
    t.manual_seed(0)
    L = bench._make_algo("DDPG", 24, 6, 256, {}, dev, "f32").learner
    K = 4000
    best = {"plain": 1e9, "mixed": 1e9}
    for rep in range(4):
        for name, buf in (("plain", plain), ("mixed", mixed)):
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
