"""step_n at the configurations bench.py times, over the replay it builds, with the noise the kernels draw on the device.

Every case runs the benchmark's own call sequence — step_n(K = 20, seed 1), then step_n(K = 13, seed 2): 33 updates over
two sampler seeds — over bench.make_replay's 1000 x 1000 transitions ("bench"), and over the same replay with a seeded 2 %
of its `dones` set in place ("bench+dones"), so that a row gather that loses or misreads the `d` column (the chain's staged
rows, the phase-1 / phase-2 prefetch rows, TD3's merged twin launch, the batch_rows.h riders) changes the numbers.  Each
case first asserts it runs the launch form the benchmark times (tests/golden/launch_forms.json), so that it cannot quietly
test another path; it is then held bit for bit to a twin learner driven the way the reference's trainer calls it —
buf.seed / _sample_counter, then update(*buf.sample(B)) (k_replay_gather's rows) with the device's own noise — in every
arithmetic.

Configurations come from bench.BASELINE_CONFIGS (imported inside a fixture: CPU-only collection never imports bench),
plus SAC humanoid B = 1024 with a learned temperature (the temperature step and the riders together); TD3, SAC and TQC
also run once keyed by set_seed(11, rank = 3)."""
from __future__ import annotations

import json
from dataclasses import dataclass
from pathlib import Path

import numpy as np
import pytest
import torch as t

from oracle import fixtures as fx
from tests import hip_adapters as ha
from tests import scenarios as sc

pytestmark = pytest.mark.gpu

CALLS = ((1, 20), (2, 13))  # (sampler seed, K) of each step_n call: the bench's warm-up and timed seeds
N_UPDATES = 33
DONE_FRAC = 0.02
SET_SEED = (11, 3)

TABLE = json.loads((Path(__file__).parent / "golden" / "launch_forms.json").read_text())
# the fields that name the form the benchmark times, and what they must be
FORM_EXPECT = {"DDPG": {"form": 4, "updates_per_chain_launch": 32},
               "TD3": {"twin_split": 1, "form": {"f32": 2, "x2": 3, "bf16": 2}},
               "SAC": {"rt2": 2}, "TQC": {"fused": 0}}


@dataclass(frozen=True)
class Case:
    id: str
    bench_name: str
    tune_alpha: bool = False
    seeded: bool = False


CASES = [
    Case("ddpg_b256", "DDPG walker-walk B=256"),
    Case("ddpg_b128", "DDPG walker-walk B=128 (the reference scripts' batch)"),
    Case("td3_b256", "TD3 cheetah-run B=256"),
    Case("td3_b256_seed", "TD3 cheetah-run B=256", seeded=True),
    Case("sac_b1024", "SAC humanoid-walk B=1024"),
    Case("sac_b1024_seed", "SAC humanoid-walk B=1024", seeded=True),
    Case("sac_b1024_tuned", "SAC humanoid-walk B=1024", tune_alpha=True),
    Case("tqc_b256", "TQC walker-walk B=256 5x25"),
    Case("tqc_b256_seed", "TQC walker-walk B=256 5x25", seeded=True),
]


@pytest.fixture(scope="module")
def bench_mod():
    import bench
    return bench


def _config(bench_mod, case):
    cls_name, S, A, B, extras, _gflop, _mbytes = bench_mod.BASELINE_CONFIGS[case.bench_name]
    extras = dict(extras, tune_alpha=True) if case.tune_alpha else dict(extras)
    return cls_name, S, A, B, extras


@pytest.fixture(scope="module")
def replays(bench_mod):
    """get(S, A, dones): the benchmark's replay for (S, A) — one resident per dimension pair — with `dones` all zero
    (as make_replay leaves them) or with the seeded 2 % mask written in place."""
    cache = {}

    def get(S, A, dones):
        if (S, A) not in cache:
            dev = t.device("cuda", 0)
            buf = bench_mod.make_replay(dev, seed=0, S=S, A=A)
            g = t.Generator(device=dev).manual_seed(4242 + S * 100 + A)
            shape = buf._tensors["dones"].shape
            mask = (t.rand(shape, device=dev, generator=g) < DONE_FRAC).to(t.float32)
            cache[(S, A)] = (buf, mask)
        buf, mask = cache[(S, A)]
        if dones:
            buf._tensors["dones"].copy_(mask)
        else:
            buf._tensors["dones"].zero_()
        return buf

    yield get
    cache.clear()


def _assert_bench_form(algo, cls_name, prec, B):
    """The form this learner takes at B is the one the benchmark times: the fields that name it, as the table has them
    (the table is measured at S = 24 / 17; SAC humanoid must take the S = 24 row's rt2 all the same)."""
    row = next(r for r in TABLE["rows"] if r["algo"] == cls_name and r["precision"] == prec and r["variant"] == "plain")
    table = dict(zip(TABLE["fields"], row["forms"][str(B)]))
    for f, v in FORM_EXPECT[cls_name].items():
        v = v[prec] if isinstance(v, dict) else v
        assert table[f] == v, (cls_name, prec, B, f, table[f], v)
    got = algo.debug_form(B)
    want = {f: table[f] for f in FORM_EXPECT[cls_name]}
    assert {f: got[f] for f in want} == want, f"{cls_name} {prec} B={B}: form {got}, the benchmark's {want}"


BITWISE = [(c, p, v) for c in CASES for p in ("f32", "x2", "bf16") for v in ("bench", "bench+dones")]


@pytest.mark.parametrize("case,prec,variant", BITWISE, ids=[f"{c.id}-{p}-{v}" for c, p, v in BITWISE])
def test_step_n_equals_sample_then_update_bitwise(case, prec, variant, bench_mod, replays):
    """step_n's in-kernel row gathers (chain staging, prefetch rows, riders) against sample() + update() per update —
    k_replay_gather's rows, the same device noise: every arena, both optimizers' moments, the temperature and the
    counters bit-identical after each call."""
    cls_name, S, A, B, extras = _config(bench_mod, case)
    buf = replays(S, A, variant == "bench+dones")
    dev = t.device("cuda", 0)
    fused, loop = (bench_mod._make_algo(cls_name, S, A, B, extras, dev, prec) for _ in range(2))
    if case.seeded:
        fused.set_seed(*SET_SEED)
        loop.set_seed(*SET_SEED)
    _assert_bench_form(fused.learner, cls_name, prec, B)
    n_done = 0
    for seed, K in CALLS:
        fused.learner.step_n(buf.handle, K, B, seed=seed)
        buf.seed = seed
        for _ in range(K):
            buf._sample_counter = loop.update_step
            batch = buf.sample(B)
            n_done += int(batch[3].sum().item())
            loop.update(*batch)
        t.cuda.synchronize()
        fused.learner.check()
        loop.learner.check()
        a, b = fused.state_dict(), loop.state_dict()
        for k in ("actor", "actor_m", "actor_v", "critic", "critic_m", "critic_v"):
            assert t.equal(a[k], b[k]), (k, (a[k] - b[k]).abs().max().item())
        for i, (x, y) in enumerate(zip(a["targets"], b["targets"])):
            assert t.equal(x, y), (f"targets[{i}]", (x - y).abs().max().item())
        assert ("log_alpha" in a) == (cls_name == "TQC" or case.tune_alpha)
        if "log_alpha" in a:
            for i, (x, y) in enumerate(zip(a["log_alpha"], b["log_alpha"])):
                assert t.equal(x, y), (f"log_alpha[{i}]", x.item(), y.item())
        assert a["counters"] == b["counters"], (a["counters"], b["counters"])
    assert fused.update_step == loop.update_step == N_UPDATES
    # (the done rows reach the gathers: about 2 % of the 33 B sampled rows on the bench+dones replay, none on the bench one)
    assert (n_done > 0) == (variant == "bench+dones"), n_done
    print(f"{case.id} [{prec}] {variant}: {n_done} done rows of {N_UPDATES * B}")
    if cls_name == "SAC":
        assert fused.alpha == loop.alpha


# ---------------------------------------------------------------------------------------- against the CPU oracle
TOL = 2e-5                  # outputs, alpha / log_alpha (tests/test_gpu_algos.py)
X2_MOMENT_TOL = 5e-3        # Adam moments of the x2 learner: tests/test_gpu_x2.py MOMENT_TOL (one row's ReLU flip)
# Adam moments of tuned-alpha SAC: the one-row ReLU-flip value of tests/test_gpu_x2.py (MOMENT_TOL), not
# test_gpu_algos.py's 1e-3.  Measured: sac_b1024_tuned [f32] after20.m_actor.2 at 3.5e-3, every deviating element in row
# 129 of the actor's second weight matrix (one hidden unit: one minibatch row's pre-activation at rounding distance from
# zero); that tensor's parameters agree to 3.3e-5.
TUNED_MOMENT_TOL = 5e-3
# Measured one-unit ReLU flips of the x2 learner against the float64 oracle: (case, mode) -> (checkpoint, net, tensor,
# unit).  Every deviating element of the tensor, its Adam moments and nothing else lies in that unit's row of the weight
# matrix and its bias entry (one minibatch row whose pre-activation of that unit is within rounding of zero falls the other way); the
# parameter gate does not hold for that row (td3: 1.04e-4, q2's second layer, unit 47; tqc: 2.8e-4, critic 2's second
# layer, unit 262) while every other tensor and output does.  Such a case is reported as an expected failure, after
# everything else in it has been checked; the test fails if the deviation reaches any other row.
KNOWN_FLIPS = {("td3_b256", "x2"): ("after33", "critic", 8, 47), ("tqc_b256_seed", "x2"): ("after20", "critic", 18, 262)}
CHECKPOINTS = (20, 33)      # after the first call and after the second
WINDOW = 4                  # updates the oracle runs up to each checkpoint, from the learner's own state
MISS = 10.0                 # a wrongly wired oracle twin must be at least this many output gates away
PROBE_B = 256


def _nets(cls_name, S, A):
    """Fixture weights, the dimensions of tests/scenarios.py."""
    if cls_name == "DDPG":
        return fx.make_net(101, fx.actor_dims(S, A)), fx.make_net(102, fx.critic_dims(S, A))
    if cls_name == "TD3":
        return (fx.make_net(201, fx.actor_dims(S, A)), fx.make_net(202, fx.critic_dims(S, A)),
                fx.make_net(203, fx.critic_dims(S, A)))
    if cls_name == "SAC":
        return (fx.make_net(301, fx.actor_dims(S, A, gaussian=True)), fx.make_net(302, fx.critic_dims(S, A)),
                fx.make_net(303, fx.critic_dims(S, A)))
    return (fx.make_net(401, fx.actor_dims(S, A, gaussian=True)),
            [fx.make_net(402 + n, fx.critic_dims(S, A, out=25, hidden=(512, 512, 512))) for n in range(5)])


def _hip(cls_name, S, A, nets, prec, B, tune_alpha):
    kw = dict(precision=prec, max_batch=B)
    if cls_name == "DDPG":
        return ha.HipDDPG(S, A, *nets, **kw)
    if cls_name == "TD3":
        return ha.HipTD3(S, A, *nets, **kw)
    if cls_name == "SAC":
        return ha.HipSAC(S, A, *nets, tune_alpha, **kw)
    return ha.HipTQC(S, A, *nets, **kw)


def _f64(x):
    return [_f64(y) for y in x] if isinstance(x, (list, tuple)) else x.to(t.float64)


def _oracle(cls_name, S, A, nets, tune_alpha):
    """The oracle in float64.  (In float32 it is one more fp32 implementation with its own summation order: on the
    bench+dones rows of SAC humanoid its policy output is 7e-5 from its own float64 run after the first update, where
    this learner is 3e-7 from it.)"""
    nets = _f64(nets)
    if cls_name == "DDPG":
        return sc.OracleDDPG(S, A, *nets)
    if cls_name == "TD3":
        return sc.OracleTD3(S, A, *nets)
    if cls_name == "SAC":
        return sc.OracleSAC(S, A, *nets, tune_alpha)
    return sc.OracleTQC(S, A, *nets)


PARAM_NAMES = {"DDPG": ("actor", "critic", "actor_target", "critic_target"),
               "TD3": ("actor", "critic", "actor_target", "critic_target"),
               "SAC": ("actor", "critic", "critic_target"), "TQC": ("actor", "critic", "critic_target")}


def _params(ad, cls_name, name):
    """One network's parameters (both critics / all five in one list, parameters() order) as CPU tensors."""
    if isinstance(ad, (ha.HipDDPG, ha.HipTD3, ha.HipSAC, ha.HipTQC)):
        return ha.cpu_params(getattr(ad.algo, name))
    o = ad.o
    if cls_name == "TQC":
        return o.actor if name == "actor" else [x for c in (o.critics if name == "critic" else o.critics_target) for x in c]
    return getattr(o, name)


def _probe(S, A):
    """A fixed batch the networks are evaluated on, and the eps of the policy's draw."""
    s, a, *_ = fx.make_batch(999, PROBE_B, S, A)
    return s, a, fx.make_noise(998, (PROBE_B, A))


def _outputs(ad, cls_name, probe, tune_alpha):
    s, a, eps = probe
    out = {}
    if cls_name == "DDPG":
        out["q"], out["q_target"], out["pi"] = ad.q(s, a), ad.q_target_pi(s), ad.pi(s)
    elif cls_name == "TD3":
        out["q1"], out["q2"], out["tq1"], out["tq2"] = ad.q(s, a, 0), ad.q(s, a, 1), ad.q(s, a, 0, True), ad.q(s, a, 1, True)
        out["pi"], out["pi_target"] = ad.pi(s), ad.pi(s, target=True)
    elif cls_name == "SAC":
        out["q1"], out["q2"], out["tq1"], out["tq2"] = ad.q(s, a, 0), ad.q(s, a, 1), ad.q(s, a, 0, True), ad.q(s, a, 1, True)
        out["pi"], out["logp"] = ad.pi_logp(s, eps)
        if tune_alpha:
            out["alpha"] = ad.alpha
    else:
        out["z"], out["tz"] = ad.z(s, a), ad.z(s, a, True)
        out["pi"], out["logp"] = ad.pi_logp(s, eps)
        out["log_alpha"] = ad.log_alpha
    return {k: np.asarray(v.detach().cpu().numpy() if isinstance(v, t.Tensor) else v, np.float64) for k, v in out.items()}


def _snapshot(ad, cls_name, tag, probe, tune_alpha, full=True):
    """What is compared at one checkpoint: the probe outputs (keys `<tag>.out.*`), and with ``full`` every parameter,
    target and Adam-moment tensor (keys the gates of scenarios.compare recognise: `<tag>.<net>.<i>`, `<tag>.m_<net>.<i>`)."""
    snap = {f"{tag}.out.{k}": v for k, v in _outputs(ad, cls_name, probe, tune_alpha).items()}
    if full:
        for name in PARAM_NAMES[cls_name]:
            for i, x in enumerate(_params(ad, cls_name, name)):
                snap[f"{tag}.{name}.{i}"] = x.detach().cpu().numpy().copy()     # (the oracle's tensors change in place)
        for w in ("critic", "actor"):
            m, v = ad.adam(w)
            for i, (mi, vi) in enumerate(zip(m, v)):
                snap[f"{tag}.m_{w}.{i}"] = mi.detach().cpu().numpy().copy()
                snap[f"{tag}.v_{w}.{i}"] = vi.detach().cpu().numpy().copy()
    return snap


def _oracle_counters(ora):
    o = ora.o
    alpha_steps = o.opt_alpha.step_count if hasattr(o, "opt_alpha") else 0
    return [getattr(o, "update_step", o.opt_critic.step_count), o.opt_critic.step_count, o.opt_actor.step_count,
            alpha_steps]


def _anchor(ora, hip, cls_name):
    """Puts a learner's whole state — parameters, targets, both optimizers' moments and step counts, the temperature and
    its Adam state, the update counter — into the oracle, which then continues from there."""
    o, sd = ora.o, hip.algo.learner.state_dict()
    with t.no_grad():
        for name in PARAM_NAMES[cls_name]:
            for dst, src in zip(_params(ora, cls_name, name), _params(hip, cls_name, name), strict=True):
                dst.copy_(src)
    for w, opt in (("critic", o.opt_critic), ("actor", o.opt_actor)):
        m, v = hip.adam(w)
        opt.m, opt.v = _f64(m), _f64(v)
    n_upd, o.opt_critic.step_count, o.opt_actor.step_count, n_alpha = sd["counters"]
    if hasattr(o, "update_step"):
        o.update_step = n_upd
    if "log_alpha" in sd:
        la, lm, lv = (x.to(t.float64) for x in sd["log_alpha"])
        o.log_alpha = la.reshape(()).clone()
        o.opt_alpha.step_count = n_alpha
        o.opt_alpha.m, o.opt_alpha.v = [lm.reshape(1).clone()], [lv.reshape(1).clone()]
        if cls_name == "SAC":
            o.alpha = float(o.log_alpha.exp())


def _run_window(cls_name, S, A, nets, tune_alpha, rows, noise, probe, first, last, anchor, wiring="as built",
                zero_d=False):
    """The oracle over minibatches first .. last - 1 from ``anchor``'s state (a learner standing at update ``first``);
    returns the snapshot after update ``last`` and the counters.  ``noise[j][u]``: the learner's stream-j draw at
    counter u.  ``wiring``: "as built" (stream 1 -> next-state / smoothing draw, stream 2 -> actor-step draw, counter u at
    update u), "swapped streams" or "counter + 1"; ``zero_d``: every sampled `d` replaced by 0."""
    ora = _oracle(cls_name, S, A, nets, tune_alpha)
    _anchor(ora, anchor, cls_name)
    for u in range(first, last):
        s, a, r, d, s2 = rows[u]
        if zero_d:
            d = t.zeros_like(d)
        if cls_name == "DDPG":
            ora.update(s, a, r, d, s2)
        elif cls_name == "TD3":
            ora.update(s, a, r, d, s2, noise[1][u + 1 if wiring == "counter + 1" else u])
        else:
            e1, e2 = noise[1][u], noise[2][u]
            if wiring == "swapped streams":
                e1, e2 = e2, e1
            ora.update(s, a, r, d, s2, e1, e2)
    full = wiring == "as built" and not zero_d
    return _snapshot(ora, cls_name, f"after{last}", probe, tune_alpha, full=full), _oracle_counters(ora)


def _wrong_wirings(cls_name):
    noisy = {"TD3": [dict(wiring="counter + 1")], "SAC": [dict(wiring="swapped streams")],
             "TQC": [dict(wiring="swapped streams")]}.get(cls_name, [])
    return noisy + [dict(zero_d=True)]


def _twin_name(w):
    return "d = 0" if w.get("zero_d") else w["wiring"]


def _device_noise(learner, B, A):
    """The learner's own N(0, 1) draws, stream 1 and 2, counters 0 .. 33 (oprl_debug_noise: the Philox key of its seed
    and rank), as float64 CPU tensors [34, B, A]."""
    from oprl_amd import _capi
    noise = {}
    for j in (1, 2):
        out = t.empty((N_UPDATES + 1, B, A), dtype=t.float32, device="cuda")
        for u in range(N_UPDATES + 1):
            _capi.check(learner.lib.oprl_debug_noise(learner.handle, j, u, B, A, _capi.ptr(out[u]),
                                                     _capi.current_stream()), "oprl_debug_noise")
        t.cuda.synchronize()
        noise[j] = out.cpu().to(t.float64)
    return noise


def _group(k):
    kind = k.split(".")[1]
    if kind == "out":
        return "out"
    if kind.startswith(("m_", "v_")):
        return "moments"
    return "targets" if kind.endswith("_target") else "params"


ORACLE = [(c, p) for c in CASES for p in ("f32", "x2")]


@pytest.mark.parametrize("case,prec", ORACLE, ids=[f"{c.id}-{p}" for c, p in ORACLE])
def test_step_n_against_the_oracle(case, prec, bench_mod, replays):
    """The benchmark's two step_n calls over the bench+dones replay against the float64 oracle fed the sampler's rows
    (seed of the call, counter u) and the learner's own exported noise.  A twin learner walks the same updates with
    sample() + update() — bit-identical to step_n (the test above; checked again here at update 33) — and hands its
    state at update 20 - WINDOW and 33 - WINDOW to the oracle, which runs the last WINDOW updates of each call.  After
    update 20 and after update 33: every parameter, target and Adam-moment tensor, a probe batch's outputs, the
    temperature and the counters within the suite's gates; and every wrongly wired oracle twin (streams 1 and 2
    swapped, the counter one ahead, every `d` zeroed) at least MISS output gates away."""
    cls_name, S, A, B, extras = _config(bench_mod, case)
    buf = replays(S, A, True)
    nets = _nets(cls_name, S, A)
    hip, loop = (_hip(cls_name, S, A, nets, prec, B, case.tune_alpha) for _ in range(2))
    if case.seeded:
        hip.algo.set_seed(*SET_SEED)
        loop.algo.set_seed(*SET_SEED)
    L = hip.algo.learner
    _assert_bench_form(L, cls_name, prec, B)
    noise = _device_noise(L, B, A)
    probe = _probe(S, A)
    probe64 = tuple(x.to(t.float64) for x in probe)
    (s1, k1), (s2, k2) = CALLS
    batches = []
    for u in range(N_UPDATES):
        buf.seed = s1 if u < k1 else s2
        buf._sample_counter = u
        batches.append(buf.sample(B))
    rows = [[x.cpu().to(t.float64) for x in b] for b in batches]
    n_done = {end: int(sum(float(rows[u][3].sum()) for u in range(end - WINDOW, end))) for end in CHECKPOINTS}
    assert all(n > 0 for n in n_done.values()), f"no done rows in an oracle window: {n_done}"

    want, counters, twins = {}, {}, {}
    for u in range(N_UPDATES):
        if u + WINDOW in CHECKPOINTS:
            t.cuda.synchronize()
            args = (cls_name, S, A, nets, case.tune_alpha, rows, noise, probe64, u, u + WINDOW, loop)
            snap, counters[u + WINDOW] = _run_window(*args)
            want.update(snap)
            for w in _wrong_wirings(cls_name):
                twins.setdefault(_twin_name(w), []).append(_run_window(*args, **w)[0])
        loop.algo.update(*batches[u])

    got = {}
    for (seed, K), tag in zip(CALLS, CHECKPOINTS):
        L.step_n(buf.handle, K, B, seed=seed)
        t.cuda.synchronize()
        L.check()
        got.update(_snapshot(hip, cls_name, f"after{tag}", probe, case.tune_alpha))
        assert L.state_dict()["counters"] == counters[tag], (tag, L.state_dict()["counters"], counters[tag])
    a, b = L.state_dict(), loop.algo.learner.state_dict()
    for k in ("actor", "critic", "actor_m", "actor_v", "critic_m", "critic_v"):
        assert t.equal(a[k], b[k]), k

    worst = {}
    for k, w in want.items():
        g = (k.split(".")[0], _group(k))
        worst[g] = max(worst.get(g, ("", 0.0)), (k, sc.rel_dev(got[k], w)), key=lambda x: x[1])
    for g in sorted(worst):
        print(f"\n{case.id} [{prec}] {g[0]} {g[1]}: worst {worst[g][1]:.2e} ({worst[g][0]})", end="")
    flipped = None
    if (case.id, prec) in KNOWN_FLIPS:
        tag, net, i, unit = KNOWN_FLIPS[(case.id, prec)]
        # (the unit's row of the weight matrix and its bias entry, with their Adam moments)
        keys = [f"{tag}.{kind}{net}.{j}" for j in (i, i + 1) for kind in ("", "m_", "v_")]
        off_unit = np.ones(want[keys[0]].shape[0], bool)
        off_unit[unit] = False
        for k in keys:
            w = want[k]
            assert sc.rel_dev(got[k][off_unit], w[off_unit]) * np.abs(w[off_unit]).max() <= 1e-5 * np.abs(w).max(), k
        flipped = sc.rel_dev(got[keys[0]], want[keys[0]])
        for k in keys:
            got[k] = got[k].copy()
            got[k][unit] = want[k][unit]
    moment_tol = X2_MOMENT_TOL if prec == "x2" else (TUNED_MOMENT_TOL if case.tune_alpha else None)
    sc.compare(got, want, TOL, param_tol=sc.PARAM_TOL, moment_tol=moment_tol)

    # the comparison tells the wirings apart: the learner is far from every wrongly wired twin, at both checkpoints
    print(f"\n{case.id} [{prec}] done rows in the oracle windows: {n_done}", end="")
    for name, snaps in twins.items():
        for tag, twin in zip(CHECKPOINTS, snaps):
            dev = max(sc.rel_dev(got[k], v) for k, v in twin.items())
            print(f"\n{case.id} [{prec}] oracle twin '{name}' after {tag}: learner {dev:.2e} away "
                  f"({dev / TOL:.0f} output gates)", end="")
            assert dev >= MISS * TOL, f"after {tag} the learner is within {dev:.1e} of the oracle twin '{name}'"
    print()
    if flipped is not None and flipped > sc.PARAM_TOL:
        pytest.xfail(f"one-unit ReLU flip {KNOWN_FLIPS[(case.id, prec)]}: {flipped:.2e} in that row alone")


def test_every_benchmarked_config_is_covered(bench_mod):
    """The cases above name every configuration bench.py times (a configuration added there is a red test here)."""
    assert {c.bench_name for c in CASES} == set(bench_mod.BASELINE_CONFIGS)
