"""What training from prioritized replay costs (needs a GPU; DESIGN.md section 11, "Training from it").  DDPG, B = 256,
f32, walker dims, a 1000 x 1000 replay with every slot live, ONE no_fuse learner (DDPG(prioritized=True)):

    python tools/probe_per_train.py [K]
        updates/s of step_n over a uniform replay (the generic launch sequence, one gather launch per update) and of
        step_n_prio over a prioritized replay with random priorities (sample by priority, weighted update, priority
        update), alternating, best of two passes, host clock around K updates ending in a synchronise."""
import sys
import time
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parents[1]))


def prioritized_replay(dev, seed):
    """bench.make_replay's rows in a PrioritizedEpisodicReplayBuffer, a random priority on every slot"""
    import torch as t
    import bench
    from oprl_amd.buffers.prioritized_buffer import PrioritizedEpisodicReplayBuffer
    E, L, S, A = bench.E, bench.L, bench.S, bench.A
    buf = PrioritizedEpisodicReplayBuffer(buffer_size_transitions=E * L, state_dim=S, action_dim=A, device=str(dev),
                                          seed=seed).create()
    g = t.Generator(device=dev).manual_seed(1234 + seed)
    buf._tensors["states"].copy_(t.randn((E, L + 1, S), device=dev, generator=g))
    buf._tensors["actions"].copy_(t.rand((E, L, A), device=dev, generator=g) * 2 - 1)
    buf._tensors["rewards"].copy_(t.rand((E, L, 1), device=dev, generator=g))
    buf._tensors["dones"].zero_()
    buf.ep_lens = [L] * E
    buf.episodes_counter = E
    buf._number_transitions = E * L
    buf._lens_dirty = True
    buf.update_priorities(t.arange(E * L, dtype=t.int32, device=dev), t.rand(E * L, device=dev, generator=g) * 2)
    return buf


def main(K=4000):
    import torch as t
    import bench
    dev = t.device("cuda", 0)
    uniform, prio = bench.make_replay(dev, 0), prioritized_replay(dev, 0)
    L = bench._make_algo("DDPG", bench.S, bench.A, 256, {"prioritized": True}, dev, "f32").learner
    assert L.debug_form(256)["fused"] == 0

    def run(name, n, seed):
        if name == "uniform":
            L.step_n(uniform.handle, n, 256, seed=seed)
        else:
            L.step_n_prio(prio.handle, n, 256, seed=seed, beta0=prio.beta0, beta_steps=prio.beta_steps)

    best = {"uniform": 1e9, "prioritized": 1e9}
    for rep in range(2):
        for name in best:
            run(name, 200, rep)
            t.cuda.synchronize()
            t0 = time.perf_counter()
            run(name, K, rep)
            t.cuda.synchronize()
            dt = time.perf_counter() - t0
            best[name] = min(best[name], dt)
            print(f"pass {rep} {name:11s}: {dt / K * 1e6:.2f} us/update ({K / dt / 1e3:.2f}k updates/s)", flush=True)
    L.check()
    print("best of two: " + ", ".join(f"{k} {K / v:.0f} updates/s ({v / K * 1e6:.2f} us)" for k, v in best.items()), flush=True)
    print(f"prioritized - uniform: {(best['prioritized'] - best['uniform']) / K * 1e6:.2f} us per update", flush=True)


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 4000)
