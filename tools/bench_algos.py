"""update() throughput of the algorithms at the BASELINE.json configs
(parity-test cases 2-4 + DDPG, REDQ, D4PG, TD3BC, IQL, CQL, LayerNorm critics), fixed synthetic minibatch resident in HBM, noise
drawn on device — one Python call per update, so the fast paths are bound by the
call rate — and, second column, oprl_learner_step_n (sampling from an HBM replay +
update, K steps per call).  Not the headline bench (bench.py); numbers for DESIGN.md.

    python tools/bench_algos.py [n] [name filter] [precisions]      one case after the other
    python tools/bench_algos.py 2000 D4PG DDPG                      a comparison on the GENERIC launch sequence
    python tools/bench_algos.py 2000 TD3BC TD3                      
    python tools/bench_algos.py 2000 IQL TD3-walker TD3BC-walker    (all three at walker dims)
    python tools/bench_algos.py 2000 CQL SAC-walker                 (the penalty's cost over SAC)
    python tools/bench_algos.py 2000 REDQ REDQ-LN SAC-walker SAC-LN (LayerNorm critics' cost)

Two or more algorithm names: each names the first case that starts with it, created as a ``no_fuse`` learner so that
all of them take the generic launch sequence (D4PG has no other), and the timed passes alternate
between the learners; best of two passes each."""
import sys
import time
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import torch as t
from oprl_amd.algos.cql import CQL
from oprl_amd.algos.d4pg import D4PG
from oprl_amd.algos.ddpg import DDPG
from oprl_amd.algos.droq import DroQ
from oprl_amd.algos.iql import IQL
from oprl_amd.algos.redq import REDQ
from oprl_amd.algos.sac import SAC
from oprl_amd.algos.td3 import TD3
from oprl_amd.algos.td3_bc import TD3BC
from oprl_amd.algos.tqc import TQC
from oprl_amd.buffers.episodic_buffer import EpisodicReplayBuffer
from oprl_amd.logging import NullLogger

CASES = [("DDPG walker B=256", DDPG, 24, 6, 256, {}),
         ("TD3 cheetah B=256", TD3, 17, 6, 256, dict(log_every=10 ** 9)),
         ("SAC humanoid B=1024", SAC, 67, 21, 1024, dict(log_every=10 ** 9)),
         ("SAC walker tuned B=256", SAC, 24, 6, 256, dict(log_every=10 ** 9, tune_alpha=True)),
         ("TQC walker B=256", TQC, 24, 6, 256, dict(log_every=10 ** 9)),
         ("REDQ walker N=10 M=2 B=256", REDQ, 24, 6, 256, dict(log_every=10 ** 9)),
         ("D4PG walker N=41 B=256", D4PG, 24, 6, 256, {}),
         ("TD3BC cheetah B=256", TD3BC, 17, 6, 256, dict(log_every=10 ** 9)),
         ("IQL walker B=256", IQL, 24, 6, 256, dict(log_every=10 ** 9)),
         ("TD3-walker pf=1 B=256", TD3, 24, 6, 256, dict(log_every=10 ** 9, policy_freq=1)),      # (an actor step on every update, as IQL)
         ("TD3BC-walker pf=1 B=256", TD3BC, 24, 6, 256, dict(log_every=10 ** 9, policy_freq=1)),
         ("CQL walker N=10 B=256", CQL, 24, 6, 256, dict(log_every=10 ** 9)),      # (7936 wide rows in the critic step)
         ("SAC-walker B=256", SAC, 24, 6, 256, dict(log_every=10 ** 9)),           # (the fixed temperature, as CQL's default)
         ("SAC-LN walker B=256", SAC, 24, 6, 256, dict(log_every=10 ** 9, layer_norm=True)),      # (LayerNorm critics: the single-CU LN slice kernels)
         ("REDQ-LN walker N=10 M=2 B=256", REDQ, 24, 6, 256, dict(log_every=10 ** 9, layer_norm=True)),
         ("REDQ-LN-drop walker N=10 M=2 p=0.01 B=256", REDQ, 24, 6, 256, dict(log_every=10 ** 9, layer_norm=True, dropout=0.01)),      # (dropout's cost over REDQ-LN)
         ("DroQ walker N=2 M=2 p=0.01 B=256", DroQ, 24, 6, 256, dict(log_every=10 ** 9))]      # (two LN critics with dropout: one 2-net launch per round)
PRECISIONS = ("f32", "bf16", "x2")


class Bench:
    """One case: the learner, its fixed minibatch and a replay of its dims, warmed up."""

    def __init__(self, name, cls, S, A, B, kw):
        self.name, self.B = name, B
        t.manual_seed(0)
        algo = cls(logger=NullLogger(), state_dim=S, action_dim=A, device="cuda", max_batch=B, **kw).create()
        self.algo, self.L = algo, algo.learner
        self.batch = [t.randn(B, S, device="cuda"), t.rand(B, A, device="cuda") * 2 - 1, t.rand(B, 1, device="cuda"),
                      t.zeros(B, 1, device="cuda"), t.randn(B, S, device="cuda")]
        for _ in range(100):
            self.L.update(*self.batch)
        # step_n: device-side sampling from a replay of the same dims
        E, LEN = 200, 1000
        buf = EpisodicReplayBuffer(buffer_size_transitions=E * LEN, state_dim=S, action_dim=A, device="cuda", seed=0).create()
        g = t.Generator(device="cuda").manual_seed(5)
        buf._tensors["states"].copy_(t.randn((E, LEN + 1, S), device="cuda", generator=g))
        buf._tensors["actions"].copy_(t.rand((E, LEN, A), device="cuda", generator=g) * 2 - 1)
        buf._tensors["rewards"].copy_(t.rand((E, LEN, 1), device="cuda", generator=g))
        buf._tensors["dones"].zero_()
        buf.ep_lens = [LEN] * E
        buf.episodes_counter = E
        buf._number_transitions = E * LEN
        buf._lens_dirty = True
        self.buf = buf
        self.L.step_n(buf.handle, 100, B, seed=1)
        self.dt = self.dt2 = 1e9

    def time_update(self, n):
        t.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            self.L.update(*self.batch)
        t.cuda.synchronize()
        self.dt = min(self.dt, time.perf_counter() - t0)

    def time_step_n(self, n):
        t.cuda.synchronize()
        t0 = time.perf_counter()
        self.L.step_n(self.buf.handle, n, self.B, seed=2)
        t.cuda.synchronize()
        self.dt2 = min(self.dt2, time.perf_counter() - t0)

    def report(self, n):
        print(f"{self.name:32s} update(): {n / self.dt:9.1f}/s {self.dt / n * 1e6:7.1f} us   "
              f"step_n: {n / self.dt2:9.1f}/s {self.dt2 / n * 1e6:7.1f} us", flush=True)


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 2000
    words = sys.argv[2:]
    is_precs = lambda w: all(p in PRECISIONS for p in w.split(","))      # noqa: E731
    names = [w for w in words if not is_precs(w)]
    precs = next((w.split(",") for w in words if is_precs(w)), ["f32"])      # e.g. f32,bf16
    if len(names) >= 2:
        # the comparison: generic launch sequence for all, the passes alternating (best of two; the first still sees clock ramp-up)
        picked = []
        for w in names:
            case = next((c for c in CASES if c[0].split()[0] == w), None)
            if case is None:
                sys.exit(f"no case starts with {w!r}: {[c[0] for c in CASES]}")
            picked.append(Bench(f"{case[0]} no_fuse [{precs[0]}]", *case[1:5], dict(case[5], precision=precs[0], no_fuse=True)))
        for _rep in range(2):
            for b in picked:
                b.time_update(n)
        for _rep in range(2):
            for b in picked:
                b.time_step_n(n)
        for b in picked:
            b.report(n)
        return
    only = names[0] if names else ""     # substring filter on the case name
    for name, cls, S, A, B, kw in [(f"{c[0]} [{p}]", *c[1:5], dict(c[5], precision=p)) for c in CASES for p in precs]:
        if only and only not in name:
            continue
        if (cls in (D4PG, TD3BC, IQL, CQL, DroQ) or kw.get("layer_norm")) and kw["precision"] != "f32":
            continue                    # (f32 only)
        b = Bench(name, cls, S, A, B, kw)
        for _rep in range(2):           # best of two passes (the first one still sees clock ramp-up)
            b.time_update(n)
        for _rep in range(2):
            b.time_step_n(n)
        b.report(n)
        del b


if __name__ == "__main__":
    main()
