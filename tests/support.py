"""The shared parts of the mode, sampler and host tests: one reviewed helper per job, each as strict as the
strictest of the per-file copies it replaced.  What differed between the copies is a parameter; the defaults check the
union.  A plain module, not a conftest: it imports without a GPU and without a built library, so _capi.load(), .cuda()
and the buffer and algorithm classes are reached inside the functions.  A test file keeps its make / step and the
per-mode tail of its got_and_want, and imports the rest from here."""
from __future__ import annotations

import ctypes as C
from pathlib import Path

import numpy as np
import torch as t

ROOT = Path(__file__).resolve().parents[1]
INVALID, STATE = -1, -3             # OPRL_ERR_INVALID, OPRL_ERR_STATE
ABI = 4                             # the one place the tests spell the ABI version out
STATE_KEYS = ("actor", "actor_m", "actor_v", "critic", "critic_m", "critic_v")      # the arenas and their Adam moments


# ---- 1. state equality -----------------------------------------------------------------------------------------------------
def _settled_state(algo):
    if t.cuda.is_available():
        t.cuda.synchronize()
    algo.learner.check()
    return algo.state_dict()


def _same(p, q):
    if t.is_tensor(p) or t.is_tensor(q):
        return t.is_tensor(p) and t.is_tensor(q) and t.equal(p, q)
    return p == q


def _gap(p, q):
    """What the failure message shows: the largest absolute difference, or the two values when there is no such thing."""
    if t.is_tensor(p) and t.is_tensor(q) and p.shape == q.shape:
        return (p.double() - q.double()).abs().max().item()
    return (p, q)


def assert_same_state(a, b, keys=STATE_KEYS, targets=None, counters=True, extra=(), what=""):
    """Two learners hold the same state, bit for bit.  Both are synchronised and check()ed first.  ``keys + extra`` name
    the state_dict entries compared (tensors bitwise, scalars such as value_step by ==; a key missing on either side
    fails); ``targets`` is None for every target list, of equal count on both sides, or a tuple of indices; log_alpha is
    on both sides or on neither, and then equal entry by entry."""
    x, y = _settled_state(a), _settled_state(b)
    if counters:
        assert x["counters"] == y["counters"], (what, "counters", x["counters"], y["counters"])
    for k in (*keys, *extra):
        assert k in x and k in y, (what, k, "missing on one side")
        assert _same(x[k], y[k]), (what, k, _gap(x[k], y[k]))
    if targets is None:
        assert len(x["targets"]) == len(y["targets"]), (what, "targets", len(x["targets"]), len(y["targets"]))
        targets = range(len(x["targets"]))
    for i in targets:
        assert _same(x["targets"][i], y["targets"][i]), (what, f"targets[{i}]", _gap(x["targets"][i], y["targets"][i]))
    assert ("log_alpha" in x) == ("log_alpha" in y), (what, "log_alpha on one side only")
    if "log_alpha" in x:
        assert len(x["log_alpha"]) == len(y["log_alpha"]), (what, "log_alpha")
        for i, (p, q) in enumerate(zip(x["log_alpha"], y["log_alpha"])):
            assert _same(p, q), (what, f"log_alpha[{i}]", _gap(p, q))


# ---- 2. refusals -----------------------------------------------------------------------------------------------------------
def refused(rc, status, word=None, min_len=1):
    """The call just made returned ``status`` and left a message of at least ``min_len`` bytes that holds ``word``;
    returns the message."""
    from oprl_amd import _capi
    msg = _capi.load().oprl_last_error()
    assert rc == status, (rc, status, msg)
    assert len(msg) >= min_len, (min_len, msg)
    if word is not None:
        assert word in msg, (word, msg)
    return msg


def counters(algo, *more):
    """[update count, Adam step counts ...] of a learner, then the learner attributes named in ``more``."""
    t.cuda.synchronize()
    return algo.learner.state_dict()["counters"] + [getattr(algo.learner, k) for k in more]


# ---- 3. parity plumbing ----------------------------------------------------------------------------------------------------
def run_pair(algo, oracles, data, step, to_oracle=None):
    """Every item of ``data`` through ``step(algo, item)`` and through each oracle's update(*item) (``to_oracle`` maps the
    item first); then the learner is synchronised and check()ed."""
    for x in data:
        step(algo, x)
        f = x if to_oracle is None else to_oracle(x)
        for o in oracles:
            o.update(*f)
    t.cuda.synchronize()
    algo.learner.check()


def to_double(x):
    return [v.double() for v in x]


def pair_nets(got, want, name, module, ref):
    """u.<name>.<layer>: a module's parameters against the oracle's list."""
    from tests.hip_adapters import cpu_params
    for l, (x, y) in enumerate(zip(cpu_params(module), ref)):
        got[f"u.{name}.{l}"], want[f"u.{name}.{l}"] = x, y


def pair_adam(got, want, algo, which, opt):
    """u.m_<which>.<layer> and u.v_<which>.<layer>: one optimizer's moments against the oracle's."""
    from tests.hip_adapters import hip_adam
    m, v = hip_adam(algo, which)
    for l in range(len(m)):
        got[f"u.m_{which}.{l}"], want[f"u.m_{which}.{l}"] = m[l], opt.m[l]
        got[f"u.v_{which}.{l}"], want[f"u.v_{which}.{l}"] = v[l], opt.v[l]


def pair_q_y(got, want, algo, B, q, y):
    """u.q and u.y: the rows of the last critic step against the oracle's."""
    gq, gy = algo.learner.debug_q_y(B)
    got["u.q"], want["u.q"] = gq.cpu(), q.reshape(-1)
    got["u.y"], want["u.y"] = gy.cpu(), y.reshape(-1)


def as_np(dct):
    return {k: np.asarray(v.detach().cpu().double().numpy()) for k, v in dct.items()}


def worst_ratio(got, want, out_tol, params_only=False):
    """(max over keys of deviation / the key's gate, that key): parameter, target and moment keys at the parameter gate,
    every other key at ``out_tol`` — or left out with ``params_only``."""
    from tests import scenarios as sc
    worst = (0.0, "")
    for k, v in want.items():
        if sc._is_param_key(k):
            lim = sc.PARAM_TOL
        elif params_only:
            continue
        else:
            lim = out_tol
        worst = max(worst, (sc.rel_dev(got[k], v) / lim, k))
    return worst


# ---- 4. replays ------------------------------------------------------------------------------------------------------------
def fill_random(buf, keys=None, gen_seed=1000):
    """Every row of the named storage tensors random normal, the never-written ones too; ``keys`` fixes the order of the
    draws (None: the buffer's own order)."""
    gen = t.Generator(device="cuda").manual_seed(gen_seed)
    for k in (buf._tensors if keys is None else keys):
        v = buf._tensors[k]
        v.copy_(t.randn(v.shape, device="cuda", generator=gen))
    return buf


def set_table(buf, lens):
    """Write the episode table directly (the storage already holds data)."""
    lens = [int(x) for x in lens]
    buf.ep_lens = lens + [0] * (buf._max_episodes - len(lens))
    buf.episodes_counter = len(lens)
    buf._number_transitions = sum(lens)
    buf._lens_dirty = True


def storage(buf):
    return [getattr(buf, k).cpu().numpy() for k in ("states", "actions", "rewards", "dones")]


def live_lens(buf):
    return buf.ep_lens[:buf.episodes_counter]


def random_dones(buf, E, L, seed=6, share=0.1):
    buf._tensors["dones"].copy_(t.as_tensor((np.random.RandomState(seed).rand(E, L, 1) < share).astype(np.float32)))


def random_replay(env_or_dims, nstep=None, gamma=0.99, E=40, L=30, seed=7, cls=None):
    """E episodes of random length with 10 % done rows, every row random normal; n-step mode (``nstep`` = n) or plain."""
    from oprl_amd.buffers.episodic_buffer import EpisodicReplayBuffer
    from oprl_amd.buffers.nstep_buffer import NStepEpisodicReplayBuffer
    from oracle import fixtures as fx
    S, A = fx.ENVS[env_or_dims] if isinstance(env_or_dims, str) else env_or_dims
    kw = dict(buffer_size_transitions=E * L, state_dim=S, action_dim=A, max_episode_lenth=L, device="cuda", seed=seed)
    if nstep:
        buf = (cls or NStepEpisodicReplayBuffer)(n_step=nstep, gamma=gamma, **kw).create()
    else:
        buf = (cls or EpisodicReplayBuffer)(**kw).create()
    fill_random(buf, gen_seed=1000)
    random_dones(buf, E, L, seed=6)
    set_table(buf, np.random.RandomState(4).randint(1, L + 1, size=E))
    return buf


def fill_full_episodes(buf, E, L, done_share=0.02, gen_seed=4321):
    """E episodes of the full length L: normal states, actions uniform in [-1, 1), rewards uniform in [0, 1) and a share of
    done rows, all from one device generator, which is returned for the caller's further draws."""
    dev, S, A = buf._tensors["states"].device, buf.state_dim, buf.action_dim
    g = t.Generator(device=dev).manual_seed(gen_seed)
    buf._tensors["states"].copy_(t.randn((E, L + 1, S), device=dev, generator=g))
    buf._tensors["actions"].copy_(t.rand((E, L, A), device=dev, generator=g) * 2 - 1)
    buf._tensors["rewards"].copy_(t.rand((E, L, 1), device=dev, generator=g))
    buf._tensors["dones"].copy_((t.rand((E, L, 1), device=dev, generator=g) < done_share).float())
    buf.ep_lens = [L] * E
    buf.episodes_counter = E
    buf._number_transitions = E * L
    buf._lens_dirty = True
    return g


def twin_replays(mode_buf, plain_buf, E, L):
    """A mode buffer and a plain one, both already filled from the same seed, given the same 10 % dones and the same
    table of random lengths: [mode, plain] over identical storage."""
    lens = np.random.RandomState(4).randint(1, L + 1, size=E)
    bufs = [mode_buf, plain_buf]
    for buf in bufs:
        random_dones(buf, E, L, seed=6)
        set_table(buf, lens)
    assert all(t.equal(bufs[0]._tensors[k], bufs[1]._tensors[k]) for k in bufs[0]._tensors)
    return bufs


def make_algo(name, prec, S, A, **kw):
    """A learner of the sampler tests: the same call gives the same initial parameters."""
    from oprl_amd.algos.ddpg import DDPG
    from oprl_amd.algos.iql import IQL
    from oprl_amd.algos.sac import SAC
    from oprl_amd.algos.td3 import TD3
    from oprl_amd.algos.tqc import TQC
    from oprl_amd.logging import NullLogger
    cls = dict(ddpg=DDPG, td3=TD3, sac=SAC, tqc=TQC, iql=IQL)[name]
    if name != "ddpg":
        kw["log_every"] = 10 ** 9
    t.manual_seed(0)
    return cls(logger=NullLogger("/tmp/oprl_amd_test"), state_dim=S, action_dim=A, device="cuda", precision=prec, **kw).create()


def loop_updates(algo, buf, K, seed, B):
    """What step_n(K) stands for: K sample() + update() pairs at the learner's own counters."""
    buf.seed = seed
    for _ in range(K):
        buf._sample_counter = algo.update_step
        algo.update(*buf.sample(B))


# ---- 5. the repeated test bodies -------------------------------------------------------------------------------------------
def _sample_then_update(loop, buf, B):
    batch = buf.sample(B)
    loop.update(*batch)
    return batch


def check_step_n_equals_loop(make_pair, buf, B, K=3, seeds=(3, 5), one=_sample_then_update, **same_state_kw):
    """step_n(K) against K rounds of ``one(loop, buf, B)`` (sample() + update() by default) at the same counters, from the
    same start, for each seed in turn: the same state after each.  Returns (fused, loop, rows with done != 0 seen)."""
    fused, loop = make_pair()
    loop.load_state_dict(fused.state_dict())
    n_done = 0
    for seed in seeds:
        fused.learner.step_n(buf.handle, K, B, seed=seed)
        buf.seed = seed
        for _ in range(K):
            buf._sample_counter = loop.update_step
            batch = one(loop, buf, B)
            n_done += int((batch[3] != 0).sum().item())
        assert_same_state(fused, loop, what=f"seed {seed}", **same_state_kw)
    assert fused.update_step == K * len(seeds)
    return fused, loop, n_done


def check_resume(make, step, data, split, before_load=None, **same_state_kw):
    """A checkpoint taken after data[:split], loaded into a fresh learner, gives the same state after data[split:];
    ``before_load(fresh, checkpoint)`` runs on the fresh learner first.  Returns (a, b, the checkpoint)."""
    a = make()
    for x in data[:split]:
        step(a, x)
    sd = a.state_dict()
    b = make()
    if before_load is not None:
        before_load(b, sd)
    b.load_state_dict(sd)
    for x in data[split:]:
        step(a, x)
        step(b, x)
    assert a.update_step == len(data)
    assert_same_state(a, b, **same_state_kw)
    return a, b, sd


# ---- 6. host tests ---------------------------------------------------------------------------------------------------------
def assert_abi_bound(entries, mode_name=None):
    """The ABI version in the bindings, the library and the header; each entry point bound, returning int, declared in the
    header and (``entries`` a dict) with that many arguments; a mode is no algorithm of its own; the hyper-parameter
    struct still ends in v_min, v_max.  Returns (lib, header text)."""
    from oprl_amd import _capi
    assert _capi.OPRL_ABI_VERSION == ABI
    if mode_name is not None:
        assert mode_name not in _capi.ALGO and len(_capi.ALGO) == 6
    lib = _capi.load()
    assert lib.oprl_abi_version() == ABI
    header = (ROOT / "include" / "oprl_amd.h").read_text()
    assert f"#define OPRL_ABI_VERSION {ABI}" in header
    arity = entries if isinstance(entries, dict) else dict.fromkeys(entries)
    for name, n_args in arity.items():
        assert name in _capi.SIGNATURES and hasattr(lib, name), name
        res, args = _capi.SIGNATURES[name]
        assert res is C.c_int, name
        assert f"int {name}(" in header, name
        if n_args is not None:
            decl = header.split(f"int {name}(", 1)[1].split(");", 1)[0]
            assert len(args) == n_args and decl.count(",") + 1 == n_args, (name, len(args), n_args, decl)
    assert [f[0] for f in _capi.OprlHparams._fields_][-2:] == ["v_min", "v_max"]
    return lib, header


def assert_source_built(stem, header=True):
    from oprl_amd import build
    assert f"{stem}.hip" in build.SOURCES
    assert (build.CSRC / f"{stem}.hip").exists()
    if header:
        assert (build.CSRC / f"{stem}.h").exists()


def cpu_buffer(cls, **kw):
    """A small replay of the class on the host (not create()d): 350 transitions in episodes of 50."""
    args = dict(buffer_size_transitions=350, max_episode_lenth=50)
    args.update(kw)
    return cls(**args)


def small_nets(S=5, A=3, gaussian=False, value=False):
    """Fixture nets of width 16 for an oracle on the CPU: actor, two critics and, with ``value``, V."""
    from oracle import fixtures as fx
    nets = [fx.make_net(11, [S, 16, 16, 2 * A if gaussian else A]), fx.make_net(12, [S + A, 16, 16, 1]),
            fx.make_net(13, [S + A, 16, 16, 1])]
    if value:
        nets.append(fx.make_net(14, [S, 16, 16, 1]))
    return nets


def assert_class_refuses(cls, gpu_module, kw, msg, monkeypatch):
    """ValueError at construction, and again from create() for fields set afterwards — before require_gpu is asked."""
    import pytest
    from oprl_amd.logging import NullLogger
    monkeypatch.setattr(gpu_module, "require_gpu", lambda device: pytest.fail("the GPU was asked for"))
    with pytest.raises(ValueError, match=msg):
        cls(logger=NullLogger(), state_dim=4, action_dim=2, **kw)
    algo = cls(logger=NullLogger(), state_dim=4, action_dim=2)
    for k, v in kw.items():
        setattr(algo, k, v)
    with pytest.raises(ValueError, match=msg):
        algo.create()
