"""The oracles that share their update bodies, on the CPU in float64: every knob of every one of them is
connected, and the classes that are one update under different constructors agree bit for bit.

A knob that nothing reads leaves the oracle's state bit-identical, so the criterion for "connected" is inequality and needs
no tolerance: two updates at B = 16 on small nets, with done rows, non-unit weights and an actor step (G = 2, TD3's
policy_freq = 2 takes its actor step at the first update)."""
from __future__ import annotations

import numpy as np
import pytest
import torch as t

from oracle import fixtures as fx
from oracle import oprl_oracle as orc
from tests import cql_oracle as co
from tests import droq_oracle as do
from tests.calql_oracle import CalQLOracle
from tests.d4pg_oracle import D4PGOracle
from tests.iql_oracle import IQLOracle
from tests.ln_oracle import LNOracle
from tests.per_train_oracle import WeightedOracle, WeightedREDQOracle
from tests.redq_oracle import REDQOracle
from tests.soft_oracle import SoftOracle
from tests.td3bc_oracle import TD3BCOracle

S, A, H = 5, 2, 8                   # the nets: MLP(. -> 8 -> 8 -> .); DroQ's mask is 256 columns wide, so its critics are too
N, M, G = 4, 2, 2                   # REDQ: two target critics of four, an actor step at the second update
NA = 3                              # CQL: sampled actions per kind


def nets(n_critics=N, hidden=H):
    return (fx.make_net(1, [S, H, H, 2 * A]), fx.make_net(2, [S, H, H, A]),
            [fx.make_net(10 + i, [S + A, hidden, hidden, 1]) for i in range(n_critics)])


def ln_params(n, width=H):
    gen = t.Generator().manual_seed(77)
    ln = t.zeros(n, 2, 2, width)
    ln[:, :, 0] = 1.0 + 0.1 * t.randn(n, 2, width, generator=gen)
    ln[:, :, 1] = 0.1 * t.randn(n, 2, width, generator=gen)
    return ln


def subset(u):
    return [u % N, (u + 1) % N]     # (another pair at u + 1)


def batches(B=16, n=2, unit_weights=False):
    """n x (s, a, r, d, s2, w, e1, e2, eps, uni) in float64: every fifth row done, weights in [0.2, 1]; eps and uni are
    CQL's draws."""
    out = []
    for k in range(n):
        g = t.Generator().manual_seed(300 + k)
        rnd = lambda *shape: t.randn(*shape, generator=g, dtype=t.float64)      # noqa: E731
        d = t.zeros(B, 1, dtype=t.float64)
        d[::5] = 1.0
        w = 0.2 + 0.8 * t.rand(B, 1, generator=g, dtype=t.float64)      # (drawn in both cases: the rows stay the same)
        if unit_weights:
            w = t.ones_like(w)
        out.append((rnd(B, S), rnd(B, A).tanh(), rnd(B, 1), d, rnd(B, S), w, rnd(B, A), rnd(B, A), rnd(B, 2 * NA, A),
                    t.rand(B, NA, A, generator=g, dtype=t.float64) * 2 - 1))
    return out


def state(o) -> dict:
    """Every tensor an oracle holds: nets, targets, LN parameters, moments, the temperature, ``last``."""
    out = {}

    def walk(key, v):
        if isinstance(v, t.Tensor):
            out[key] = v.detach()
        elif isinstance(v, orc.Adam):
            walk(key + ".m", v.m), walk(key + ".v", v.v)
        elif isinstance(v, (list, tuple)):
            for i, x in enumerate(v):
                walk(f"{key}.{i}", x)
        elif isinstance(v, dict):
            for k, x in v.items():
                walk(f"{key}.{k}", x)
    for k, v in vars(o).items():
        if not k.startswith("_"):
            walk(k, v)
    return out


def differ(a: dict, b: dict) -> list[str]:
    assert a.keys() == b.keys()
    return [k for k in a if not t.equal(a[k], b[k])]


def same_on(a: dict, b: dict, keys) -> None:
    keys = list(keys)
    assert keys
    off = [k for k in keys if not t.equal(a[k], b[k])]
    assert not off, f"not bit-identical: {off[:6]}"


# ---- one (build, feed) per family: build(**knobs) gives the oracle, feed(o, batch) one update ---------------------------------
def _soft(x):
    return *x[:5], x[6], x[7]


def build_redq(**kn):
    actor, _, critics = nets()
    return REDQOracle(S, A, actor, critics, critics, subset, M, G, tau=0.5, **kn)


def build_ln(**kn):
    actor, _, critics = nets()
    return LNOracle("redq", S, A, actor, critics, critics, ln_params(N), ln_params(N), subset=subset, n_min=M, utd_ratio=G, **kn)


def build_droq(**kn):
    actor, _, critics = nets(2, 256)
    ln = ln_params(2, 256)
    return do.DroQOracle("redq", S, A, actor, critics, critics, ln, ln, subset=lambda u: [0, 1], n_min=2, utd_ratio=G, rate=0.1, **kn)


def build_wredq(**kn):
    actor, _, critics = nets()
    return WeightedREDQOracle(S, A, actor, critics, critics, subset, M, G, **kn)


def build_weighted(algo):
    def build(**kn):
        actor, dactor, critics = nets(1 if algo == "ddpg" else 2)
        return WeightedOracle(algo, S, A, actor if algo == "sac" else dactor, critics, **kn)
    return build


def build_td3bc(**kn):
    _, dactor, critics = nets(2)
    return TD3BCOracle(S, A, dactor, *critics, **kn)


def build_iql(**kn):
    _, dactor, critics = nets(2)
    # (adv_clip = 1: exp(beta u) reaches the clip on these rows, so that no_clip has something to drop)
    return IQLOracle(S, A, dactor, *critics, fx.make_net(3, [S, H, H, 1]), adv_clip=1.0, **kn)


def build_cql(**kn):
    actor, _, critics = nets(2)
    return co.CQLOracle(S, A, actor, *critics, n_actions=NA, tune_alpha=True, **kn)


def build_d4pg(**kn):
    _, dactor, _ = nets(1)
    return D4PGOracle(S, A, dactor, fx.make_net(4, [S + A, H, H, 11]), 11, -3.0, 3.0, **kn)


FAMILIES = {
    "redq": (build_redq, lambda o, x: o.update(*_soft(x))),
    "ln": (build_ln, lambda o, x: o.update(*_soft(x))),
    "droq": (build_droq, lambda o, x: o.update(*_soft(x))),
    "wredq": (build_wredq, lambda o, x: o.update(*x[:8])),
    "wsac": (build_weighted("sac"), lambda o, x: o.update(*x[:8])),
    "wtd3": (build_weighted("td3"), lambda o, x: o.update(*x[:8])),
    "wddpg": (build_weighted("ddpg"), lambda o, x: o.update(*x[:8])),
    "td3bc": (build_td3bc, lambda o, x: o.update(*x[:5], x[6])),
    "iql": (build_iql, lambda o, x: o.update(*x[:5])),
    "cql": (build_cql, lambda o, x: o.update(*_soft(x), x[8], x[9])),
    "d4pg": (build_d4pg, lambda o, x: o.update(*x[:5])),
}
WEIGHT_KNOBS = ("ignore_weights", "weight_actor", "normalise_by_sum")
KNOBS = ([("redq", k) for k in ("subset_shift", "use_mean", "polyak_on_actor_steps")]
         + [(f, k) for f in ("wredq", "wsac", "wtd3", "wddpg") for k in WEIGHT_KNOBS]
         + [("ln", k) for k in ("no_ln", "freeze_ln", "no_ln_polyak")]
         + [("droq", k) for k in do.KNOBS]
         + [("td3bc", k) for k in ("no_bc", "no_lambda")]
         + [("iql", k) for k in ("sym", "late", "no_clip")]
         + [("cql", k) for k in ("no_logd", "at_next", "scale_bw")]
         + [("d4pg", k) for k in ("no_done", "skip_polyak")])


def run(family, B=16, unit_weights=False, **kn):
    build, feed = FAMILIES[family]
    o = build(**kn)
    for x in batches(B, unit_weights=unit_weights):
        feed(o, x)
    return o


_plain: dict = {}


def plain(family, B=16):
    """The state after two updates of the oracle without any knob, computed once per family and batch size."""
    if (family, B) not in _plain:
        _plain[family, B] = state(run(family, B))
    return _plain[family, B]


@pytest.mark.parametrize("family,knob", KNOBS, ids=[f"{f}-{k}" for f, k in KNOBS])
def test_every_knob_moves_the_state(family, knob):
    # local_rows takes the row's index modulo 16, which is the index itself for B = 16: only rows 16 .. of a second slice
    # can tell, so this one knob runs at B = 32
    B = 32 if knob == "local_rows" else 16
    o = run(family, B, **{knob: True})
    assert o.update_step == 2
    moved = differ(plain(family, B), state(o))
    assert moved, f"{family}: {knob} is not connected: two updates end bit-identical"
    if family in ("redq", "ln", "droq", "wredq", "wsac"):
        assert "last.actor_loss" in state(o), "no actor step occurred"


def test_no_scale_shows_in_the_rows_layer_norm_does_not_cancel():
    """LayerNorm cancels a common factor of its input up to eps / var, so ``no_scale`` moves the state of
    the test above only through eps.  What it moves in full: the kept pre-activations (zd = z scale) and rstd (1 / scale)."""
    scale = do.drop_scale(0.1)
    _, _, critics = nets(1, 256)
    x = batches()[0]
    keep = do.drop_mask(do.noise_key(7, 0, do.DROP_STREAM), do.drop_stream(0, 1, 0), 16, 0.1)
    rows, rows1 = {}, {}
    sa = t.cat([x[0], x[1]], 1)
    p, ln = [v.double() for v in critics[0]], ln_params(1, 256)[0].double()
    do.drop_mlp(p, ln, sa, keep, scale, rows=rows)
    do.drop_mlp(p, ln, sa, keep, 1.0, rows=rows1)
    assert 0 < int(keep[0].sum()) < keep[0].size
    assert t.equal(rows["zd"][0], rows1["zd"][0] * scale) and not t.equal(rows["zd"][0], rows1["zd"][0])
    ratio = rows["rstd"][0] / rows1["rstd"][0]
    assert float((ratio * scale - 1).abs().max()) < 1e-3 and float((ratio - 1).abs().min()) > 0.05


# ---- the classes that are one update under different constructors -------------------------------------------------------------
def test_redq_is_the_ln_class_without_ln_bit_for_bit():
    a, b = plain("redq"), state(run("ln", no_ln=True, tau=0.5))
    # (the LN class keeps its gamma / beta and their slot, the last of the critic optimiser, with zero moments)
    slot = f"opt_critic.m.{len(nets()[2]) * 6}"
    assert slot in b and slot not in a and not b[slot].any()
    same_on(a, b, a.keys())


def test_unit_weights_are_redq_bit_for_bit():
    actor, _, critics = nets()
    o = REDQOracle(S, A, actor, critics, critics, subset, M, G)
    for x in batches():
        o.update(*_soft(x))
    a, b = state(o), state(run("wredq", unit_weights=True))
    same_on(a, b, a.keys())
    assert "last.td_abs" in b


def test_unit_weights_sac_is_the_shared_class_as_sac_bit_for_bit():
    actor, _, critics = nets(2)
    o = SoftOracle("sac", S, A, actor, critics, critics, lr_alpha=1e-3, alpha_init=0.2)
    for x in batches():
        o.update(*_soft(x))
    a, b = state(o), state(run("wsac", unit_weights=True))
    same_on(a, b, a.keys())


def test_calql_has_no_update_body_beyond_its_returns():
    """Cal-QL with returns-to-go below every Q bounds nothing and is CQL bit for bit; with them above, it is not."""
    actor, _, critics = nets(2)
    lo, hi = (CalQLOracle(S, A, actor, *critics, n_actions=NA, tune_alpha=True) for _ in range(2))
    for x in batches():
        lo.update(*_soft(x), x[8], x[9], np.full(16, -1e6))
        hi.update(*_soft(x), x[8], x[9], np.full(16, 1e6))
    same = {k: v for k, v in plain("cql").items() if k in state(lo)}
    same_on(same, state(lo), same.keys())
    assert differ(state(lo), state(hi))
