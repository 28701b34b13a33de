"""Common base of the four algorithms + the binding between the torch-owned
parameter arenas and the HIP learner handle.

Reference: /root/reference/src/oprl/algos/base_algorithm.py:7-15 (guard +
``get_policy_state_dict``).  Everything below ``HipLearner`` is new: it replaces
autograd + torch.optim.Adam + the per-tensor Polyak loops of the reference's
``update()`` bodies with one call into liboprl_amd.so."""
from __future__ import annotations

import ctypes as C
from abc import ABC
from typing import Any, Sequence

import numpy as np
import torch as t
import torch.nn as nn

from oprl_amd import _capi
from oprl_amd.algos.nn_models import MLP, flatten_module_, is_flat


class OffPolicyAlgorithm(ABC):
    _created: bool = False
    updates_per_request = 1      # updates update_from_buffer runs per update asked of it (REDQ: its update-to-data ratio)

    def check_created(self) -> None:
        if not self._created:
            raise RuntimeError(
                f"Algorithm {type(self).__name__} has not been created with `create()`."
            )

    def get_policy_state_dict(self) -> dict[str, Any]:
        return self.actor.state_dict()

    @property
    def update_step(self) -> int:
        return self.learner.update_count if self._created else 0

    def _log_update(self, step: int) -> None:
        """Scalar logging at the algorithm's cadence (the only host sync of an update)."""

    def _dispatch_update(self, state, action, reward, done, next_state, weights, noise0, noise1) -> None:
        """One logged update, weighted when ``weights`` ([B] or [B, 1], a prioritized batch's) are given: the rows' |TD|
        is then left in ``last_td_abs`` (device tensor)."""
        step = self.update_step
        if weights is not None:
            self.last_td_abs = self.learner.update_weighted(state, action, reward, done, next_state, weights,
                                                            noise0=noise0, noise1=noise1)
        else:
            self.learner.update(state, action, reward, done, next_state, noise0=noise0, noise1=noise1)
        self._log_update(step)

    def update_from_buffer(self, replay_buffer, batch_size: int, act_next=None, n_updates: int = 1) -> None:
        """``update(*replay_buffer.sample(batch_size))`` as ONE C call (oprl_learner_step_n with
        K = 1): the slice kernels gather their own rows from the HBM replay with the sampler's
        Philox draw, so the per-step host work is one ctypes call instead of a gather launch, five
        output allocations and the update's argument checks.  A buffer without a device handle
        (or a gradient-exporting data-parallel learner) takes the two-call path.

        ``act_next``: the observation the NEXT environment step starts from (the trainer has it before the update,
        base_trainer.py:38-74).  The actor's forward for it rides behind the update in the same call
        (oprl_learner_step_act) and the next ``actor.explore(act_next)`` — with this very array — only collects the
        row: one host wait per environment step instead of update-sync, act-launch, act-sync.

        A 2-D ``act_next`` [N, S] (the next observations of N environments, trainers/vec_trainer.py) rides as ROWS
        behind K = ``n_updates`` updates — one oprl_learner_step_act_rows call — and the next
        ``actor.explore_rows(act_next)`` collects them.  ``n_updates`` > 1 without ``act_next``: one ``step_n(K)``.

        A ``prioritized`` algorithm over a prioritized buffer: one ``step_n_prio`` call instead (draw by priority,
        weighted update, new priorities); ``act_next`` is accepted but rides nowhere, ``explore`` runs its own forward.

        Everywhere above K is ``n_updates x updates_per_request``."""
        refuse_prioritized(self, replay_buffer)
        check_nstep_gamma(self, replay_buffer)
        K = int(n_updates)
        if K < 1:
            raise ValueError(f"n_updates={n_updates!r}: at least one update")
        K *= self.updates_per_request
        if trains_prioritized(self, replay_buffer):
            step = self.update_step
            step_prioritized(self, replay_buffer, K, batch_size)
            self._log_updates(step, K)
            return
        handle = getattr(replay_buffer, "handle", None)
        if handle is None or self.learner.export_grads:
            for _ in range(K):
                self.update(*replay_buffer.sample(batch_size))
            return
        step = self.update_step
        seed = int(getattr(replay_buffer, "seed", 0))
        mlp = self._actor_mlp() if act_next is not None else None
        if mlp is not None and np.ndim(act_next) == 2:
            self.learner.step_act_rows(handle, K, int(batch_size), seed, act_next)
            mlp.set_pending_rows(act_next, self.learner)
        elif mlp is not None:
            if K > 1:
                self.learner.step_n(handle, K - 1, int(batch_size), seed=seed)
            self.learner.step_act(handle, int(batch_size), seed, act_next)
            mlp.set_pending(act_next, self.learner)
        else:
            self.learner.step_n(handle, K, int(batch_size), seed=seed)
        self._log_updates(step, K)

    def _log_updates(self, step: int, K: int) -> None:
        """``_log_update`` for the updates ``step .. step + K - 1`` of one call: at most one of them logs (the scalars
        on the device are the last update's)."""
        if K == 1:
            self._log_update(step)
            return
        every = int(getattr(self, "log_every", 0) or 0)
        if every <= 0:
            return
        first = -(-step // every) * every       # the first multiple of log_every at or after `step`
        if first < step + K:
            self._log_update(first)

    def _actor_mlp(self):
        """The actor's MLP when it is one the learner's policy kernel can run (the policy classes of nn_models.py)."""
        actor = getattr(self, "actor", None)
        mlp = getattr(actor, "mlp", None) or getattr(actor, "net", None)
        return mlp if (mlp is not None and hasattr(mlp, "set_pending") and mlp.on_gpu()) else None

    def debug_form(self, batch_size: int) -> dict[str, int]:
        """Which launch form this algorithm's learner takes for `batch_size` (HipLearner.debug_form)."""
        return self.learner.debug_form(batch_size)

    def set_seed(self, seed: int, rank: int = 0) -> None:
        """Key the learner's device-side noise streams with the run seed (and data-parallel rank)."""
        self.learner.set_seed(seed, rank)

    # full learner state (parameters, targets, optimiser moments, counters): exact resume
    def state_dict(self) -> dict[str, Any]:
        return self.learner.state_dict()

    def load_state_dict(self, sd: dict[str, Any]) -> None:
        self.learner.load_state_dict(sd)


def refuse_prioritized(algo, replay_buffer) -> None:
    """A prioritized buffer (buffers/prioritized_buffer.py) trains only an algorithm created with ``prioritized=True``
    (DDPG, TD3, SAC, REDQ), whose critic loss applies the importance weights; any other algorithm refuses it rather
    than sample it without them."""
    if getattr(replay_buffer, "prioritized", False) and not getattr(algo, "prioritized", False):
        raise ValueError(f"{type(algo).__name__} does not apply importance weights: it cannot train from a prioritized "
                         "replay buffer (use EpisodicReplayBuffer, or create the algorithm with prioritized=True)")


def check_prioritized_config(algo) -> None:
    """``prioritized=True`` runs the exact-fp32 generic launch sequence on one GPU: called by
    ``create()`` before anything touches the GPU."""
    if not getattr(algo, "prioritized", False):
        return
    if algo.precision != "f32":
        raise ValueError(f"{type(algo).__name__}(prioritized=True) needs precision='f32', not {algo.precision!r}")
    if algo.export_grads:
        raise ValueError(f"{type(algo).__name__}(prioritized=True) does not export gradients (no data-parallel "
                         "prioritized training)")


def check_layer_norm_config(algo) -> None:
    """``layer_norm=True`` puts LayerNorm into the critics of SAC and REDQ on the exact-fp32 generic launch sequence of one
    GPU: called by ``create()`` before anything touches the GPU.  ``dropout`` (DroQ's
    Linear -> Dropout -> LayerNorm -> ReLU, section 26) runs inside the LN kernels: a rate in [0, 1), and none without them."""
    name = type(algo).__name__
    rate = getattr(algo, "dropout", 0.0)
    if not 0.0 <= rate < 1.0:        # (NaN fails both)
        raise ValueError(f"{name}(dropout={rate!r}): the rate must lie in [0, 1)")
    if not getattr(algo, "layer_norm", False):
        if rate > 0.0:
            raise ValueError(f"{name}(dropout={rate!r}) needs layer_norm=True: dropout runs inside the LN kernels, in front of "
                             "the normalisation (the DroQ block)")
        return
    if algo.prioritized:
        raise ValueError(f"{name}(layer_norm=True, prioritized=True): the LN kernels take no importance weights "
                         "(prioritized replay with LayerNorm critics is not built)")
    if algo.export_grads:
        raise ValueError(f"{name}(layer_norm=True) does not export gradients (no data-parallel LayerNorm critics)")
    if algo.precision != "f32":
        raise ValueError(f"{name}(layer_norm=True) needs precision='f32', got {algo.precision!r}: the LN kernels run exact fp32")


def check_mode_config(algo, name: str, f32_only: str, uniform_only: str | None = None) -> None:
    """What the learner refuses of an algorithm that runs as a mode of another's learner, or on the generic launch
    sequence alone, said before anything touches the GPU: a precision other than f32 (``f32_only`` says what needs it),
    gradient export and, where ``uniform_only`` says why, prioritized replay."""
    if algo.precision != "f32":
        if algo.precision not in _capi.PRECISION:
            raise ValueError(f"precision={algo.precision!r}: expected one of {sorted(_capi.PRECISION)}")
        raise ValueError(f"{name}: precision={algo.precision!r} unsupported (f32 only: {f32_only})")
    if algo.export_grads:
        raise ValueError(f"{name}: export_grads (data-parallel learners) unsupported")
    if uniform_only is not None and algo.prioritized:
        raise ValueError(f"{name}(prioritized=True): prioritized replay through {name} is not built ({uniform_only})")


class Temperature:
    """``alpha`` of the algorithms with an entropy temperature (SAC, REDQ and what derives from them)."""

    @property
    def alpha(self) -> float:
        if self.log_alpha is not None:
            return float(self.log_alpha.exp().item())
        return self.alpha_init


def trains_prioritized(algo, replay_buffer) -> bool:
    """A prioritized algorithm over a prioritized buffer with its tree on the device: the weighted path.  (A prioritized
    algorithm over a plain buffer trains uniformly through the plain path.)"""
    return (getattr(algo, "prioritized", False) and getattr(replay_buffer, "prioritized", False)
            and getattr(replay_buffer, "handle", None) is not None)


def step_prioritized(algo, replay_buffer, K: int, batch_size: int) -> None:
    """K times: draw by priority at counter u = the update count, one weighted update, new priorities from its |TD| —
    one C call (oprl_learner_step_n_prio), nothing waited for."""
    algo.learner.step_n_prio(replay_buffer.handle, int(K), int(batch_size), seed=int(replay_buffer.seed),
                             beta0=float(replay_buffer.beta0), beta_steps=float(replay_buffer.beta_steps))


def check_nstep_gamma(algo, replay_buffer) -> None:
    """An n-step buffer (buffers/nstep_buffer.py) folds gamma^(m-1) into the done flag it writes and the learner
    multiplies by its own gamma: the two discounts must be the same number."""
    if getattr(replay_buffer, "n_step", 1) > 1 and replay_buffer.gamma != algo.gamma:
        raise ValueError(f"the replay buffer samples {replay_buffer.n_step}-step returns with gamma={replay_buffer.gamma!r} "
                         f"but {type(algo).__name__} discounts with gamma={algo.gamma!r}: build the buffer with the "
                         "algorithm's gamma")


IQL_STATE_KEYS = ("value", "value_m", "value_v", "value_step")
LN_STATE_KEYS = ("critic_ln", "critic_ln_target", "critic_ln_m", "critic_ln_v")
DROPOUT_STATE_KEY = "critic_dropout"     # the rate, only while the dropout mode is on (the masks follow the update count)


def _rows_f32(obs) -> np.ndarray:
    """Observation rows as one contiguous float32 [N, S] host array."""
    x = np.ascontiguousarray(obs, dtype=np.float32)
    if x.ndim != 2:
        raise ValueError(f"observation rows must be a 2-D array [N, S], got shape {x.shape}")
    return x


def require_gpu(device: str) -> t.device:
    dev = t.device(device)
    if dev.type != "cuda":
        raise RuntimeError(
            f"device={device!r}: the oprl_amd learner runs only on an MI355X (device='cuda'); "
            "it has no CPU path")
    if not t.cuda.is_available():
        raise RuntimeError("no GPU visible to torch; the oprl_amd learner has no CPU path")
    _capi.load()
    return dev if dev.index is not None else t.device("cuda", t.cuda.current_device())


def _fill_net(dst: _capi.OprlNet, mlp: MLP, target: MLP | None, arena: t.Tensor, m: t.Tensor, v: t.Tensor,
              g: t.Tensor | None = None) -> None:
    """The descriptor of ``mlp``, whose parameters lie inside ``arena``; ``m``, ``v`` and ``g`` (Adam's moments, the
    exported gradient) are laid out like the arena."""
    o = mlp.theta_ptr() - arena.data_ptr()
    dst.n_layers = len(mlp.dims) - 1
    for i, x in enumerate(mlp.dims):
        dst.dims[i] = x
    dst.theta = mlp.theta_ptr()
    dst.theta_target = target.theta_ptr() if target is not None else None
    dst.pack = mlp.pack_tensor().data_ptr()
    dst.pack_target = target.pack_tensor().data_ptr() if target is not None else None
    dst.adam_m = m.data_ptr() + o
    dst.adam_v = v.data_ptr() + o
    dst.grad = (g.data_ptr() + o) if g is not None else None


class HipLearner:
    """Owns the C handle.  ``actor_mlp`` / ``critic_mlps`` are the trainable MLPs,
    ``*_targets`` their target twins (or None); each group (actor, all critics)
    must already be flat so one Adam-state arena per group lines up with it."""

    def __init__(self, algo: str, state_dim: int, action_dim: int, device: t.device,
                 actor_group: nn.Module, actor_mlp: MLP, actor_target_mlp: MLP | None,
                 critic_group: nn.Module, critic_mlps: Sequence[MLP],
                 critic_target_group: nn.Module, critic_target_mlps: Sequence[MLP],
                 hp: dict, max_batch: int, export_grads: bool = False,
                 log_alpha: t.Tensor | None = None, actor_target_group: nn.Module | None = None,
                 no_fuse: bool = False, precision: str = "f32"):
        self.lib = _capi.load()
        self.device = device
        self.S, self.A = state_dim, action_dim
        self.max_batch = int(max_batch)
        self.export_grads = bool(export_grads)
        if actor_target_mlp is not None and actor_target_group is None:
            actor_target_group = actor_target_mlp
        self._groups = [actor_group, critic_group, critic_target_group]
        self._actor_target_group = actor_target_group
        for g in [*self._groups, actor_target_group]:
            if g is not None and not is_flat(g):
                flatten_module_(g)
        self.actor_arena = actor_group._oprl_arena
        self.critic_arena = critic_group._oprl_arena
        self.actor_m = t.zeros_like(self.actor_arena)
        self.actor_v = t.zeros_like(self.actor_arena)
        self.critic_m = t.zeros_like(self.critic_arena)
        self.critic_v = t.zeros_like(self.critic_arena)
        self.actor_grad = t.zeros_like(self.actor_arena) if export_grads else None
        self.critic_grad = t.zeros_like(self.critic_arena) if export_grads else None
        self.log_alpha = log_alpha
        self.log_alpha_m = t.zeros((), dtype=t.float64, device=device) if log_alpha is not None else None
        self.log_alpha_v = t.zeros((), dtype=t.float64, device=device) if log_alpha is not None else None
        self.log_alpha_grad = (t.zeros((), dtype=t.float64, device=device)
                               if (log_alpha is not None and export_grads) else None)

        cfg = _capi.OprlLearnerConfig()
        cfg.abi_version = _capi.OPRL_ABI_VERSION
        cfg.algo = _capi.ALGO[algo]
        if precision not in _capi.PRECISION:
            raise ValueError(f"precision={precision!r}: expected one of {sorted(_capi.PRECISION)}")
        cfg.precision = _capi.PRECISION[precision]
        self.precision = precision
        cfg.state_dim, cfg.action_dim = state_dim, action_dim
        cfg.max_batch = self.max_batch
        cfg.n_critics = len(critic_mlps)
        cfg.export_grads = int(export_grads)
        cfg.no_fuse = int(no_fuse)

        _fill_net(cfg.actor, actor_mlp, actor_target_mlp, self.actor_arena, self.actor_m, self.actor_v, self.actor_grad)
        for j, (c, ct) in enumerate(zip(critic_mlps, critic_target_mlps)):
            _fill_net(cfg.critics[j], c, ct, self.critic_arena, self.critic_m, self.critic_v, self.critic_grad)
        if log_alpha is not None:
            cfg.log_alpha = log_alpha.data_ptr()
            cfg.log_alpha_m = self.log_alpha_m.data_ptr()
            cfg.log_alpha_v = self.log_alpha_v.data_ptr()
            if self.log_alpha_grad is not None:
                cfg.log_alpha_grad = self.log_alpha_grad.data_ptr()
        for k, v in hp.items():
            setattr(cfg.hp, k, v)
        self._cfg = cfg
        self.algo_name = algo
        self.policy_freq = int(hp.get("policy_freq", 1))
        self._mlps = (actor_mlp, actor_target_mlp, list(critic_mlps), list(critic_target_mlps))
        self._value_mlp = None         # the value net of the implicit-Q-learning mode (set_iql) ...
        self._iql_on = False           # ... and whether the mode is on (the net and its moments are kept while it is off)
        self._ln = None                # the critics' LayerNorm holder (set_layernorm), or None
        self._dropout = 0.0            # the critics' dropout rate (set_dropout); 0: off
        self._ptrs = self._snapshot_ptrs()
        h = C.c_void_p()
        with _capi.on_device(device):
            _capi.check(self.lib.oprl_learner_create(C.byref(cfg), C.byref(h)), "oprl_learner_create")
        self.handle = h
        self._all_mlps = [m for m in [actor_mlp, actor_target_mlp, *critic_mlps, *critic_target_mlps]
                          if m is not None]
        for m in self._all_mlps:       # oprl_learner_create built every pack from the masters
            m.mark_packed()
        self._versions = self._snapshot_versions()

    def target_arenas(self):
        """Flat target-network arenas (critic targets, then the actor target if any)."""
        out = [self._groups[2]._oprl_arena]
        if self._actor_target_group is not None:
            out.append(self._actor_target_group._oprl_arena)
        return out

    # check_bound() runs on every update(): walking the module trees (``module.parameters()``) cost more
    # host time than the four kernel launches, so the Parameter objects are looked up once.  They stay
    # valid across ``module.to()`` / ``load_state_dict`` (which change ``.data`` / the version in place).
    def _param_cache(self):
        c = getattr(self, "_pcache", None)
        if c is None:
            a, at, cs, cts = self._mlps
            mlps = [a, *([at] if at is not None else []), *cs, *cts, *([self._value_mlp] if self._value_mlp is not None else [])]
            first = [next(m.parameters()) for m in mlps]
            every = [p for m in mlps for p in m.parameters()]
            c = self._pcache = (first, every)
        return c

    def _snapshot_ptrs(self):
        # (the LayerNorm holder's four tensors too: the library keeps their raw pointers, set_layernorm)
        ln = () if self._ln is None else tuple(x.data_ptr() for x in self._ln.tensors())
        return tuple(p.data_ptr() for p in self._param_cache()[0]) + ln

    def _snapshot_versions(self):
        return tuple(p._version for p in self._param_cache()[1])

    def sync_params(self) -> None:
        """Rebuild the fragment-order packs from the master parameters.  Called
        automatically when torch reports an in-place change (load_state_dict,
        ``param.copy_``); call it yourself after writing through ``.data``."""
        with _capi.on_device(self.device):
            _capi.check(self.lib.oprl_learner_sync_params(self.handle, _capi.current_stream()),
                        "oprl_learner_sync_params")
        for m in self._all_mlps:
            m.mark_packed()
        self._versions = self._snapshot_versions()

    # ---- checkpoint / exact resume (the reference saves only the policy,
    # base_trainer.py:113-120) ---------------------------------------------------------------
    def state_dict(self) -> dict[str, Any]:
        """Everything a bit-exact resume needs: parameter / target / Adam arenas, the
        temperature and its Adam state, and the learner's counters."""
        cnt = (C.c_int64 * 4)()
        _capi.check(self.lib.oprl_learner_get_counters(self.handle, cnt), "oprl_learner_get_counters")
        t.cuda.synchronize(self.device)
        sd: dict[str, Any] = {
            "algo": self.algo_name,
            "counters": [int(x) for x in cnt],
            "actor": self.actor_arena.detach().cpu().clone(),
            "actor_m": self.actor_m.cpu().clone(), "actor_v": self.actor_v.cpu().clone(),
            "critic": self.critic_arena.detach().cpu().clone(),
            "critic_m": self.critic_m.cpu().clone(), "critic_v": self.critic_v.cpu().clone(),
            "targets": [a.detach().cpu().clone() for a in self.target_arenas()],
        }
        if self.log_alpha is not None:
            sd["log_alpha"] = [x.detach().cpu().clone() for x in (self.log_alpha, self.log_alpha_m, self.log_alpha_v)]
        if self._iql_on:      # the implicit-Q-learning mode: V, its moments and its Adam step count
            n = C.c_int64()
            _capi.check(self.lib.oprl_learner_get_iql_step(self.handle, C.byref(n)), "oprl_learner_get_iql_step")
            sd.update(value=self.value_arena.detach().cpu().clone(), value_m=self.value_m.cpu().clone(),
                      value_v=self.value_v.cpu().clone(), value_step=int(n.value))
        if self._ln is not None:      # LayerNorm critics: the parameters, their target copy and both Adam moments
            sd.update({k: x.detach().cpu().clone() for k, x in zip(LN_STATE_KEYS, self._ln.tensors())})
        if getattr(self, "_dropout", 0.0) > 0.0:
            sd[DROPOUT_STATE_KEY] = float(self._dropout)
        return sd

    def load_state_dict(self, sd: dict[str, Any]) -> None:
        if sd.get("algo") != self.algo_name:
            raise ValueError(f"checkpoint is for {sd.get('algo')!r}, this learner is {self.algo_name!r}")
        pairs = [(self.actor_arena, sd["actor"]), (self.actor_m, sd["actor_m"]), (self.actor_v, sd["actor_v"]),
                 (self.critic_arena, sd["critic"]), (self.critic_m, sd["critic_m"]), (self.critic_v, sd["critic_v"]),
                 *zip(self.target_arenas(), sd["targets"])]
        if self.log_alpha is not None:
            pairs += list(zip((self.log_alpha, self.log_alpha_m, self.log_alpha_v), sd["log_alpha"]))
        if self._iql_on:
            missing = [k for k in IQL_STATE_KEYS if k not in sd]
            if missing:
                raise ValueError(f"checkpoint has no {', '.join(missing)}: this learner's implicit-Q-learning mode is on "
                                 "and resumes its value net, both Adam moments and its step count with the rest")
            pairs += [(self.value_arena, sd["value"]), (self.value_m, sd["value_m"]), (self.value_v, sd["value_v"])]
        have_ln = [k for k in LN_STATE_KEYS if k in sd]
        if self._ln is None and have_ln:
            raise ValueError(f"checkpoint carries {', '.join(have_ln)} but this learner's critics have no layer normalisation "
                             "(layer_norm=False)")
        if self._ln is not None:
            missing = [k for k in LN_STATE_KEYS if k not in sd]
            if missing:
                raise ValueError(f"checkpoint has no {', '.join(missing)}: this learner's critics carry layer normalisation "
                                 "(layer_norm=True) and resume its parameters, target copy and Adam moments with the rest")
            pairs += [(x, sd[k]) for k, x in zip(LN_STATE_KEYS, self._ln.tensors())]
        rate = getattr(self, "_dropout", 0.0)
        if (DROPOUT_STATE_KEY in sd) != (rate > 0.0):
            raise ValueError(f"checkpoint carries {DROPOUT_STATE_KEY}={sd[DROPOUT_STATE_KEY]!r} but this learner's critics have no dropout "
                             "(dropout=0)" if rate == 0.0 else
                             f"checkpoint has no {DROPOUT_STATE_KEY}: this learner's critics drop at rate {rate!r} (dropout > 0)")
        if rate > 0.0 and float(np.float32(sd[DROPOUT_STATE_KEY])) != float(np.float32(rate)):
            raise ValueError(f"checkpoint's {DROPOUT_STATE_KEY}={sd[DROPOUT_STATE_KEY]!r} is not this learner's rate {rate!r}: "
                             "the masks of the updates to come would differ")
        for dst, src in pairs:
            if dst.shape != src.shape:
                raise ValueError(f"checkpoint tensor shape {tuple(src.shape)} != {tuple(dst.shape)}")
        with t.no_grad():
            for dst, src in pairs:
                dst.copy_(src.to(dst.device))
        cnt = (C.c_int64 * 4)(*[int(x) for x in sd["counters"]])
        _capi.check(self.lib.oprl_learner_set_counters(self.handle, cnt), "oprl_learner_set_counters")
        if self._iql_on:
            _capi.check(self.lib.oprl_learner_set_iql_step(self.handle, int(sd["value_step"])), "oprl_learner_set_iql_step")
        self.sync_params()      # the fragment-order packs are derived state

    def check_bound(self) -> None:
        """The kernels hold raw pointers into the arenas: refuse to run if a
        module was moved/re-allocated behind our back (e.g. ``actor.to(...)``)."""
        if self._snapshot_ptrs() != self._ptrs:
            raise RuntimeError("a network's parameters were re-allocated after create(); "
                               "the HIP learner is bound to the original arenas")
        if self._snapshot_versions() != self._versions or any(m._pack_key is None for m in self._all_mlps):
            self.sync_params()

    def close(self) -> None:
        if getattr(self, "handle", None):
            self.lib.oprl_learner_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------ update
    def _prep(self, state, action, reward, done, next_state):
        dev = self.device
        B = state.shape[0]

        def f(x, cols):
            # fast path: a resident, contiguous fp32 batch (what the replay's sample() returns)
            if (isinstance(x, t.Tensor) and x.dtype == t.float32 and x.device == dev and x.is_contiguous()
                    and x.numel() == B * cols):
                return x
            x = t.as_tensor(x).to(device=dev, dtype=t.float32).reshape(B, cols)
            return x.contiguous()

        return B, f(state, self.S), f(action, self.A), f(reward, 1), f(done, 1), f(next_state, self.S)

    def _noise(self, x, B):
        """An injected normal draw as the kernels read it: float32 [B, A] on the device (``None``: Philox)."""
        return None if x is None else x.to(device=self.device, dtype=t.float32).reshape(B, self.A).contiguous()

    def _per_row(self, x, B, noun: str) -> t.Tensor:
        """One number per row of the batch (``noun``: weights, returns), [B] or [B, 1], as float32 [B] on the device."""
        x = t.as_tensor(x).to(device=self.device, dtype=t.float32).reshape(-1).contiguous()
        if x.numel() != B:
            raise ValueError(f"{x.numel()} {noun} for a batch of {B}")
        return x

    def update(self, state, action, reward, done, next_state, noise0=None, noise1=None) -> None:
        self.check_bound()
        B, s, a, r, d, s2 = self._prep(state, action, reward, done, next_state)
        n0, n1 = self._noise(noise0, B), self._noise(noise1, B)
        with _capi.on_device(self.device):
            _capi.check(self.lib.oprl_learner_update(
                self.handle, _capi.ptr(s), _capi.ptr(a), _capi.ptr(r), _capi.ptr(d), _capi.ptr(s2), B,
                _capi.ptr(n0), _capi.ptr(n1), _capi.current_stream()), "oprl_learner_update")

    def update_weighted(self, state, action, reward, done, next_state, weights, noise0=None, noise1=None) -> t.Tensor:
        """One update whose critic loss carries the importance weights ``weights`` ([B] or [B, 1]); returns the rows'
        |TD| (mean over the critics) as a device tensor [B] (oprl_learner_update_weighted)."""
        self.check_bound()
        B, s, a, r, d, s2 = self._prep(state, action, reward, done, next_state)
        w = self._per_row(weights, B, "weights")
        n0, n1 = self._noise(noise0, B), self._noise(noise1, B)
        td = t.empty(B, dtype=t.float32, device=self.device)
        with _capi.on_device(self.device):
            _capi.check(self.lib.oprl_learner_update_weighted(
                self.handle, _capi.ptr(s), _capi.ptr(a), _capi.ptr(r), _capi.ptr(d), _capi.ptr(s2), _capi.ptr(w), B,
                _capi.ptr(n0), _capi.ptr(n1), _capi.ptr(td), _capi.current_stream()), "oprl_learner_update_weighted")
        return td

    def update_phase(self, phase, state, action, reward, done, next_state, noise0=None, noise1=None):
        self.check_bound()
        B, s, a, r, d, s2 = self._prep(state, action, reward, done, next_state)
        n0, n1 = self._noise(noise0, B), self._noise(noise1, B)
        with _capi.on_device(self.device):
            _capi.check(self.lib.oprl_learner_update_phase(
                self.handle, phase, _capi.ptr(s), _capi.ptr(a), _capi.ptr(r), _capi.ptr(d), _capi.ptr(s2),
                B, _capi.ptr(n0), _capi.ptr(n1), _capi.current_stream()), "oprl_learner_update_phase")

    def apply(self, phase: int, grad_scale: float) -> None:
        with _capi.on_device(self.device):
            _capi.check(self.lib.oprl_learner_apply(self.handle, phase, float(grad_scale),
                                                    _capi.current_stream()), "oprl_learner_apply")

    def step_n(self, replay_handle, K: int, B: int, seed: int) -> None:
        self.check_bound()
        with _capi.on_device(self.device):
            _capi.check(self.lib.oprl_learner_step_n(self.handle, replay_handle, K, B, seed,
                                                     _capi.current_stream()), "oprl_learner_step_n")

    def step_n_prio(self, replay_handle, K: int, B: int, seed: int, beta0: float, beta_steps: float) -> None:
        """K prioritized sample + weighted update + priority update rounds over a replay with a sum tree
        (oprl_learner_step_n_prio)."""
        self.check_bound()
        with _capi.on_device(self.device):
            _capi.check(self.lib.oprl_learner_step_n_prio(self.handle, replay_handle, K, B, seed, float(beta0),
                                                          float(beta_steps), _capi.current_stream()),
                        "oprl_learner_step_n_prio")

    def step_act(self, replay_handle, B: int, seed: int, obs) -> None:
        """One sample()+update() and, enqueued behind it, the actor's forward of ``obs`` with the updated weights
        (oprl_learner_step_act): nothing is waited for; ``act_wait`` collects the row."""
        self.check_bound()
        x = np.ascontiguousarray(obs, dtype=np.float32).reshape(-1)
        with _capi.on_device(self.device):
            _capi.check(self.lib.oprl_learner_step_act(self.handle, replay_handle, B, seed, x.ctypes.data_as(C.c_void_p),
                                                       _capi.current_stream()), "oprl_learner_step_act")

    def act_wait(self, n_out: int, timeout_us: int = 5_000_000):
        out = np.empty(n_out, dtype=np.float32)
        _capi.check(self.lib.oprl_learner_act_wait(self.handle, out.ctypes.data_as(C.c_void_p), n_out, timeout_us),
                    "oprl_learner_act_wait")
        return out

    def act_rows(self, obs) -> None:
        """Enqueue the actor's forward of the rows ``obs[N, S]`` (oprl_learner_act_rows): nothing is waited for;
        ``act_rows_wait`` collects them."""
        self.check_bound()
        x = _rows_f32(obs)
        with _capi.on_device(self.device):
            _capi.check(self.lib.oprl_learner_act_rows(self.handle, x.ctypes.data_as(C.c_void_p), x.shape[0],
                                                       _capi.current_stream()), "oprl_learner_act_rows")

    def step_act_rows(self, replay_handle, K: int, B: int, seed: int, obs) -> None:
        """K sample()+update() iterations and, enqueued behind them, the actor's forward of the rows ``obs[N, S]`` with
        the weights they leave (oprl_learner_step_act_rows)."""
        self.check_bound()
        x = _rows_f32(obs)
        with _capi.on_device(self.device):
            _capi.check(self.lib.oprl_learner_step_act_rows(self.handle, replay_handle, K, B, seed,
                                                            x.ctypes.data_as(C.c_void_p), x.shape[0],
                                                            _capi.current_stream()), "oprl_learner_step_act_rows")

    def act_rows_wait(self, n_rows: int, n_out: int, timeout_us: int = 5_000_000):
        out = np.empty((n_rows, n_out), dtype=np.float32)
        _capi.check(self.lib.oprl_learner_act_rows_wait(self.handle, out.ctypes.data_as(C.c_void_p), n_rows, n_out,
                                                        timeout_us), "oprl_learner_act_rows_wait")
        return out

    def check(self) -> None:
        """Raise if a kernel of this learner reported an expired cross-workgroup wait (include/oprl_amd.h,
        "Device-side failures").  Every update / step_n / read_scalars call checks too."""
        _capi.check(self.lib.oprl_learner_check(self.handle), "oprl_learner_check")

    def clear_error(self) -> None:
        _capi.check(self.lib.oprl_learner_clear_error(self.handle), "oprl_learner_clear_error")

    DEBUG_FORM_FIELDS = ("fused", "lean", "form", "updates_per_chain_launch", "wide", "nc", "twin_split", "p2_pair", "arith",
                         "xcd_local", "shared_chip", "dp_inline_form", "rt2")

    def debug_form(self, batch_size: int) -> dict[str, int]:
        """Which launch form this learner takes for `batch_size` (include/oprl_amd.h, oprl_learner_debug_form): the
        decision tests/golden/launch_forms.json pins, under that table's field names."""
        out = (C.c_int32 * len(self.DEBUG_FORM_FIELDS))()
        _capi.check(self.lib.oprl_learner_debug_form(self.handle, int(batch_size), out), "oprl_learner_debug_form")
        return dict(zip(self.DEBUG_FORM_FIELDS, (int(x) for x in out)))

    def set_cluster(self, nc: int) -> None:
        """CUs per 16-row slice in the fused kernels (include/oprl_amd.h): 8 = the default (clusters of four, of
        eight where the kernels have them: a learner that has the GPU to itself), 4 = clusters of four only
        (learners that share a GPU with more than two others), 2 / 1 = least CU time per update."""
        _capi.check(self.lib.oprl_learner_set_cluster(self.handle, int(nc)), "oprl_learner_set_cluster")

    def set_seed(self, seed: int, rank: int = 0) -> None:
        self.seed = int(seed)
        _capi.check(self.lib.oprl_learner_set_seed(self.handle, int(seed) & (2 ** 64 - 1), int(rank)),
                    "oprl_learner_set_seed")

    def _read(self, fn_name: str, n: int, keys, *size) -> dict[str, float]:
        """``keys`` over the first floats of the ``n`` that the library's ``fn_name`` writes (``size``: its count
        argument, where it takes one)."""
        buf = (C.c_float * n)()
        with _capi.on_device(self.device):
            _capi.check(getattr(self.lib, fn_name)(self.handle, buf, *size, _capi.current_stream()), fn_name)
        return dict(zip(keys, (float(x) for x in buf)))

    def read_scalars(self) -> dict[str, float]:
        return self._read("oprl_learner_read_scalars", 10, ("critic_loss", "actor_loss", "q_mean", "q_target_mean", "alpha",
                          "update_step", "q1_mean", "log_pi_mean", "gauss_actor_loss", "alpha_loss"), 10)

    def set_bc(self, alpha: float) -> None:
        """The behaviour-cloning mode of a TD3 learner's actor step (oprl_learner_set_bc; TD3+BC):
        ``alpha > 0`` turns it on, ``0`` turns it off."""
        with _capi.on_device(self.device):
            _capi.check(self.lib.oprl_learner_set_bc(self.handle, float(alpha)), "oprl_learner_set_bc")

    def read_bc(self) -> dict[str, float]:
        """lambda, mean |Q1(s, pi(s))| and the mean squared pi(s) - a of the last actor step with the mode on
        (oprl_learner_read_bc)."""
        return self._read("oprl_learner_read_bc", 4, ("bc_lambda", "q_abs_mean", "bc_mse"))

    def set_cql(self, cql_alpha: float, n_actions: int) -> None:
        """The conservative-Q-learning mode of a SAC learner's critic step (oprl_learner_set_cql; CQL, DESIGN.md section
        19): ``n_actions`` in 1 .. 16 turns it on, ``0`` turns it off.  A refused call leaves the learner as it was."""
        with _capi.on_device(self.device):
            _capi.check(self.lib.oprl_learner_set_cql(self.handle, float(cql_alpha), int(n_actions)), "oprl_learner_set_cql")

    def read_cql(self) -> dict[str, float]:
        """Of the last update with the mode on, per critic: the mean of logsumexp - Q(s, a), the mean Q on the uniform
        actions and on the actions drawn from pi(.|s); and the penalty term of the loss (oprl_learner_read_cql)."""
        return self._read("oprl_learner_read_cql", 8, ("gap1", "gap2", "q_rand1", "q_rand2", "q_pi1", "q_pi2", "penalty",
                                                       "bound_rate"))

    def set_cql_noise(self, eps: t.Tensor | None, uni: t.Tensor | None) -> None:
        """Test hook (oprl_learner_set_cql_noise): device arrays standing in for the mode's normal draws [B, 2N, A] and
        uniform actions [B, N, A], read by every later update until replaced; ``None``: Philox.  The learner keeps them alive."""
        prep = lambda x: None if x is None else x.to(device=self.device, dtype=t.float32).contiguous()     # noqa: E731
        self._cql_noise = (prep(eps), prep(uni))
        _capi.check(self.lib.oprl_learner_set_cql_noise(self.handle, _capi.ptr(self._cql_noise[0]), _capi.ptr(self._cql_noise[1])),
                    "oprl_learner_set_cql_noise")

    def set_layernorm(self, holder) -> None:
        """Layer normalisation in the critics of a SAC / REDQ learner (oprl_learner_set_layernorm):
        ``holder`` is the ``CriticLayerNorm`` whose four device tensors [n_critics, 2, 2, 256] the library reads and steps
        in place.  Once, before the first update; a refused call leaves the learner as it was.  The four tensors must stay
        where they are (write into them in place): ``check_bound`` refuses to run once one of them was replaced or moved."""
        d = _capi.OprlLayerNorm()
        d.theta, d.theta_target, d.adam_m, d.adam_v = (x.data_ptr() for x in holder.tensors())
        d.eps = float(holder.eps)
        with _capi.on_device(self.device):
            _capi.check(self.lib.oprl_learner_set_layernorm(self.handle, C.byref(d)), "oprl_learner_set_layernorm")
        self._ln = holder
        self._ptrs = self._snapshot_ptrs()      # the holder's tensors join the pointers check_bound() watches

    def set_dropout(self, rate: float) -> None:
        """Dropout in front of the critics' layer normalisation (oprl_learner_set_dropout; DroQ), in
        every pass that evaluates a critic, from Philox masks addressed by the update count: nothing is stored and
        ``state_dict()`` carries the rate alone (``critic_dropout``).  After ``set_layernorm``, once, before the first
        update; rate 0, or one below 2^-32, leaves the mode off; a refused call leaves the learner as it was."""
        with _capi.on_device(self.device):
            _capi.check(self.lib.oprl_learner_set_dropout(self.handle, float(rate)), "oprl_learner_set_dropout")
        self._dropout = float(rate) if int(float(np.float32(rate)) * 2.0 ** 32) > 0 else 0.0

    def set_calql(self, on: bool) -> None:
        """The calibrated form of the CQL mode (oprl_learner_set_calql; Cal-QL): the penalty's
        policy entries are bounded below by the rows' returns-to-go, which ``update_calql`` takes and ``step_n``
        computes.  Needs ``set_cql`` first; a refused call leaves the learner as it was."""
        with _capi.on_device(self.device):
            _capi.check(self.lib.oprl_learner_set_calql(self.handle, int(bool(on))), "oprl_learner_set_calql")

    def update_calql(self, state, action, reward, done, next_state, returns, noise0=None, noise1=None) -> None:
        """One update with the rows' returns-to-go ``returns`` ([B] or [B, 1]; oprl_learner_update_calql)."""
        self.check_bound()
        B, s, a, r, d, s2 = self._prep(state, action, reward, done, next_state)
        g = self._per_row(returns, B, "returns")
        n0, n1 = self._noise(noise0, B), self._noise(noise1, B)
        with _capi.on_device(self.device):
            _capi.check(self.lib.oprl_learner_update_calql(
                self.handle, _capi.ptr(s), _capi.ptr(a), _capi.ptr(r), _capi.ptr(d), _capi.ptr(s2), _capi.ptr(g), B,
                _capi.ptr(n0), _capi.ptr(n1), _capi.current_stream()), "oprl_learner_update_calql")

    def set_iql(self, value_mlp: MLP | None, expectile: float = 0.7, beta: float = 3.0, adv_clip: float = 100.0,
                lr_value: float = 3e-4) -> None:
        """The implicit-Q-learning mode of a TD3 learner (oprl_learner_set_iql): ``value_mlp`` is
        the flat value net V(s), dims [S, ..., 1], for which this learner keeps the Adam moments; ``None`` turns the mode
        off (the net, its moments and its step count are kept: the same net turns it on again where it stopped).  A refused
        call leaves the learner as it was."""
        if value_mlp is None:
            with _capi.on_device(self.device):
                _capi.check(self.lib.oprl_learner_set_iql(self.handle, None, 0.0, 0.0, 0.0, 0.0), "oprl_learner_set_iql")
            self._iql_on = False
            return
        if not is_flat(value_mlp):
            flatten_module_(value_mlp)
        arena = value_mlp._oprl_arena
        same = value_mlp is self._value_mlp
        m = self.value_m if same else t.zeros_like(arena)
        v = self.value_v if same else t.zeros_like(arena)
        desc = _capi.OprlNet()
        _fill_net(desc, value_mlp, None, arena, m, v)
        with _capi.on_device(self.device):
            _capi.check(self.lib.oprl_learner_set_iql(self.handle, C.byref(desc), float(expectile), float(beta),
                                                      float(adv_clip), float(lr_value)), "oprl_learner_set_iql")
        if not same:
            self._all_mlps = [x for x in self._all_mlps if x is not self._value_mlp] + [value_mlp]
        self._value_mlp, self.value_arena, self.value_m, self.value_v = value_mlp, arena, m, v
        self._iql_on = True
        self._pcache = None            # V's parameters join the ones check_bound() watches
        self._ptrs = self._snapshot_ptrs()
        self.sync_params()      # V's pack is derived state like the others

    def read_iql(self) -> dict[str, float]:
        """Of the last update with the mode on: the V loss, mean V(s), mean advantage u, mean weight w, the share of rows
        at the clip and the weighted cloning loss (oprl_learner_read_iql)."""
        return self._read("oprl_learner_read_iql", 8, ("v_loss", "v_mean", "adv_mean", "w_mean", "clip_frac", "actor_loss"))

    @property
    def value_step(self) -> int:
        n = C.c_int64()
        _capi.check(self.lib.oprl_learner_get_iql_step(self.handle, C.byref(n)), "oprl_learner_get_iql_step")
        return int(n.value)

    @property
    def update_count(self) -> int:
        n = C.c_int64()
        _capi.check(self.lib.oprl_learner_update_count(self.handle, C.byref(n)))
        return int(n.value)

    def debug_q_y(self, B: int) -> tuple[t.Tensor, t.Tensor]:
        """Per-row Q(s,a) and TD target of the last critic step (critic 0)."""
        q, y = C.c_void_p(), C.c_void_p()
        _capi.check(self.lib.oprl_learner_debug_ptrs(self.handle, C.byref(q), C.byref(y)))
        out = []
        for p in (q, y):
            buf = t.empty(B, dtype=t.float32, device=self.device)
            t.cuda.synchronize(self.device)
            C.cdll.LoadLibrary("libamdhip64.so").hipMemcpy(
                C.c_void_p(buf.data_ptr()), p, C.c_size_t(4 * B), C.c_int(3))
            out.append(buf)
        return out[0], out[1]
