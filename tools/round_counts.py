"""Prints the launch counts of the generic (per-net) launch sequence that tests/test_gpu_rounds.py holds (needs a GPU): for
every case K = 4 updates with oprl_profile_enable on, then oprl_profile_read's per-kind launch counts (include/oprl_amd.h:
0 k_mlp_slice and everything launched in its place, 1 k_dw_adam, 3 everything else) and the SHA-256 of the actor and critic
arenas.  How a round of nets goes out — twin critics as one launch, five quantile critics layer by layer or as one multi
launch, an ensemble in pairs or over the side streams — changes the counts and no bit of the result; the hash is there to
compare two builds of the library on the same cases (OPRL_AMD_LIB).

`python tools/round_counts.py` prints the table; `--json PATH [note]` writes it as tests/golden/round_counts.json holds it."""
import ctypes as C
import hashlib
import json
import os
import sys
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import torch as t

S, A, B, K = 17, 6, 64, 4
KINDS = 6                            # OPRL_PROFILE_KINDS
E, L = 8, 40                         # the small replay of the step_n cases
NO_LEAN = {"OPRL_AMD_NO_LEAN": "1"}             # no cluster launches: every net pass is a k_mlp_slice launch
NO_LAYERWISE = {"OPRL_AMD_NO_LAYERWISE": "1"}   # TQC's five critics as one k_mlp_slice_multi launch
SWITCHES = ("OPRL_AMD_NO_LEAN", "OPRL_AMD_NO_LAYERWISE")

# (id, algorithm, constructor arguments, switches that hold while the learner is created, how the K updates run)
CASES = [
    ("ddpg-no_fuse", "ddpg", dict(no_fuse=True), {}, "update"),                       # rounds of one net
    ("td3-no_fuse", "td3", dict(no_fuse=True), {}, "update"),                         # twin rounds: one tp2 launch each
    ("sac-no_fuse-tuned", "sac", dict(no_fuse=True, tune_alpha=True), {}, "update"),  # ... the actor phase has two
    ("sac-no_fuse-tuned-NO_LEAN", "sac", dict(no_fuse=True, tune_alpha=True), NO_LEAN, "update"),
    # 5 x 512 critics layer by layer: every rider by update(), and the row prefetch by step_n
    ("tqc-f32-update", "tqc", dict(precision="f32"), {}, "update"),
    ("tqc-f32-step_n", "tqc", dict(precision="f32"), {}, "step_n"),
    ("tqc-bf16-update", "tqc", dict(precision="bf16"), {}, "update"),
    ("tqc-bf16-step_n", "tqc", dict(precision="bf16"), {}, "step_n"),
    ("tqc-f32-update-NO_LAYERWISE", "tqc", dict(precision="f32"), NO_LAYERWISE, "update"),
    ("tqc-f32-step_n-NO_LAYERWISE", "tqc", dict(precision="f32"), NO_LAYERWISE, "step_n"),
    ("tqc-bf16-update-NO_LAYERWISE", "tqc", dict(precision="bf16"), NO_LAYERWISE, "update"),
    ("tqc-bf16-step_n-NO_LAYERWISE", "tqc", dict(precision="bf16"), NO_LAYERWISE, "step_n"),
    # N = 10 in pairs; the target round a pair, or three cluster launches and k_redq_min; the side-stream fork / join
    ("redq-N10-M2", "redq", dict(n_critics=10, n_min=2, utd_ratio=3), {}, "update"),
    ("redq-N10-M3", "redq", dict(n_critics=10, n_min=3, utd_ratio=3), {}, "update"),
    ("redq-N10-M2-NO_LEAN", "redq", dict(n_critics=10, n_min=2, utd_ratio=3), NO_LEAN, "update"),
    # the weighted critic step: forward | seed kernel | backward per grouping
    ("ddpg-prioritized", "ddpg", dict(prioritized=True), {}, "weighted"),
    ("td3-prioritized", "td3", dict(prioritized=True), {}, "weighted"),
    # the learner's modes, all on the generic sequence: a seed kernel between a forward-only and a backward-only launch
    ("d4pg", "d4pg", {}, {}, "update"),                                               # critic and actor step
    ("td3bc", "td3bc", {}, {}, "update"),                                             # the actor step, with k_bc_mix behind it
    ("iql", "iql", {}, {}, "update"),                                                 # V's step and dW launch, k_iql_actor_seed
    ("cql", "cql", dict(cql_n_actions=2, batch_size=B), {}, "update"),                # the critic step on B (1 + 3 N) = 448 rows
    ("calql", "calql", dict(cql_n_actions=2, batch_size=B), {}, "returns"),           # ... with returns-to-go to update()
]
# algorithms whose module and class are not `name` and `name.upper()`
CLASSES = {"td3bc": ("td3_bc", "TD3BC"), "calql": ("calql", "CalQL")}


def make_algo(name, kw):
    """(the environment switches are read once, at create: the caller sets them around this call; CQL.create raises
    max_batch to its wide rows itself)"""
    import importlib
    from oprl_amd.logging import NullLogger
    module, cls_name = CLASSES.get(name, (name, name.upper()))
    cls = getattr(importlib.import_module(f"oprl_amd.algos.{module}"), cls_name)
    extra = {} if name in ("ddpg", "d4pg") else dict(log_every=10 ** 9)
    t.manual_seed(0)
    algo = cls(logger=NullLogger(), state_dim=S, action_dim=A, device="cuda", max_batch=B, **extra, **kw).create()
    algo.set_seed(7, 0)
    return algo


def make_replay():
    from oprl_amd.buffers.episodic_buffer import EpisodicReplayBuffer
    buf = EpisodicReplayBuffer(buffer_size_transitions=E * L, state_dim=S, action_dim=A, max_episode_lenth=L,
                               device="cuda", seed=3).create()
    g = t.Generator(device="cuda").manual_seed(1234)
    buf._tensors["states"].copy_(t.randn((E, L + 1, S), device="cuda", generator=g))
    buf._tensors["actions"].copy_(t.rand((E, L, A), device="cuda", generator=g) * 2 - 1)
    buf._tensors["rewards"].copy_(t.rand((E, L, 1), device="cuda", generator=g))
    buf.ep_lens = [L] * E
    buf.episodes_counter = E
    buf._number_transitions = E * L
    buf._lens_dirty = True
    return buf


def run_case(case):
    """The case's K updates on a fresh learner -> (launch counts per kind, sha256 of the actor and critic arenas)."""
    from oracle import fixtures as fx
    _, name, kw, _, how = case
    algo = make_algo(name, kw)
    lib = algo.learner.lib
    replay = make_replay() if how == "step_n" else None
    if replay is not None:
        replay.sample(B)                      # (the table and the handle's first use stay outside the counted region)
    batches = []
    for k in range(K):
        g = t.Generator().manual_seed(500 + k)
        rows = [x.cuda() for x in fx.make_batch(100 + k, B, S, A)]
        w = (0.05 + 0.95 * t.rand(B, 1, generator=g)).cuda()
        batches.append((rows, w, (20.0 * t.rand(B, 1, generator=g) - 10.0).cuda()))
    t.cuda.synchronize()
    cnt, ms = (C.c_int64 * KINDS)(), (C.c_double * KINDS)()
    lib.oprl_profile_enable(1)
    try:
        assert lib.oprl_profile_read(cnt, ms, 1) == 0
        if how == "step_n":
            algo.learner.step_n(replay.handle, K, B, seed=5)
        else:
            for rows, w, ret in batches:
                algo.update(*rows, **(dict(weights=w) if how == "weighted" else dict(returns=ret) if how == "returns" else {}))
        assert lib.oprl_profile_read(cnt, ms, 1) == 0
    finally:
        lib.oprl_profile_enable(0)
    t.cuda.synchronize()
    algo.learner.check()
    assert algo.update_step == K
    h = hashlib.sha256()
    for m in ("actor", "critic"):
        h.update(getattr(algo, m)._oprl_arena.cpu().numpy().tobytes())
    return [int(x) for x in cnt], h.hexdigest()


def run_case_with_env(case):
    saved = {k: os.environ.pop(k) for k in SWITCHES if k in os.environ}
    os.environ.update(case[3])
    try:
        return run_case(case)
    finally:
        for k in case[3]:
            os.environ.pop(k, None)
        os.environ.update(saved)


if __name__ == "__main__":
    rows = []
    for case in CASES:
        counts, sha = run_case_with_env(case)
        rows.append(dict(id=case[0], counts=counts))
        print(f"{case[0]:32s} counts {counts}  sha256 {sha[:16]}", flush=True)
    if len(sys.argv) > 2 and sys.argv[1] == "--json":
        note = sys.argv[3] if len(sys.argv) > 3 else "tools/round_counts.py on MI355X (256 compute units)"
        with open(sys.argv[2], "w") as f:
            f.write('{\n"shape": ' + json.dumps(dict(S=S, A=A, B=B, K=K)) + ',\n"generated_by": ' + json.dumps(note) + ',\n"rows": [\n')
            f.write(",\n".join(json.dumps(r) for r in rows))
            f.write("\n]\n}\n")
        print(f"{len(rows)} rows -> {sys.argv[2]}")
