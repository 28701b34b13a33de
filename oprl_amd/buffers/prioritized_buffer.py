"""Prioritized experience replay (Schaul et al., ICLR 2016, proportional variant) over the HBM episodic replay.

The priorities live in a sum tree in HBM next to the storage (``oprl_replay_prio_*``, csrc/replay_prio.hip,
DESIGN.md §11): one leaf per slot (e, t), kept in step with the episode table by every flush, sampled by a stratified
descent and updated from |TD errors| on the device, with no host round trip.  ``sample`` returns the 5-tuple of
``ReplayBufferProtocol`` and keeps the batch's slots (``e·L + t``, int32) and importance weights in ``last_slots`` /
``last_weights`` (device tensors); ``update_priorities(slots, td_abs)`` writes new priorities.

DDPG, TD3, SAC and REDQ created with ``prioritized=True`` train from it: their ``update(..., weights=last_weights)``
applies the importance weights in the critic loss and leaves |TD| in ``last_td_abs`` for ``update_priorities``;
``update_from_buffer`` does the three steps in one C call (``oprl_learner_step_n_prio``, counter = the learner's update
count, ``beta(u)`` from this buffer's ``beta0`` / ``beta_steps``).  Any other algorithm (TQC included) and the trainer
refuse a prioritized buffer instead of sampling it without the weights."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import torch as t

from oprl_amd import _capi
from oprl_amd.buffers.episodic_buffer import EpisodicReplayBuffer

FANOUT = 256     # children per node of the sum tree (csrc/replay_internal.h kPrioFan)


def tree_layout(n_leaves: int) -> tuple[list[int], list[int]]:
    """(nodes per level, offsets of the levels) of the sum tree over ``n_leaves`` slots, leaves first: level k + 1 has
    one node per FANOUT nodes of level k, every level is padded with zeros to a multiple of FANOUT, the last level holds
    the root alone.  ``offsets[-1]`` is the tree's size in floats."""
    counts, offs, c = [], [0], int(n_leaves)
    while True:
        counts.append(c)
        offs.append(offs[-1] + -(-c // FANOUT) * FANOUT)
        if c == 1 and len(counts) >= 2:
            return counts, offs
        c = -(-c // FANOUT)


@dataclass
class PrioritizedEpisodicReplayBuffer(EpisodicReplayBuffer):
    alpha: float = 0.6          # priority = (|delta| + eps)^alpha
    beta0: float = 0.4          # importance-weight exponent at counter 0, annealed to 1 over beta_steps
    beta_steps: float = 1e6
    eps: float = 1e-6

    prioritized = True          # (a class attribute, not a field: what learners and the trainer test for)

    def create(self) -> "PrioritizedEpisodicReplayBuffer":
        if not self.alpha >= 0:
            raise ValueError(f"alpha={self.alpha}: must be >= 0")
        if not 0 <= self.beta0 <= 1:
            raise ValueError(f"beta0={self.beta0}: must lie in [0, 1]")
        if not self.eps > 0:
            raise ValueError(f"eps={self.eps}: must be > 0")
        if not self.beta_steps > 0:
            raise ValueError(f"beta_steps={self.beta_steps}: must be > 0")
        super().create()
        self.last_slots = self.last_weights = None
        if self._handle is not None:
            self._enable()
        return self

    def _enable(self) -> None:
        with _capi.on_device(self._dev):
            _capi.check(self._lib.oprl_replay_prio_enable(self._handle, float(self.alpha), float(self.eps),
                                                          _capi.current_stream()), "oprl_replay_prio_enable")

    def beta(self, u: int) -> float:
        """The importance-weight exponent for counter u: min(1, beta0 + (1 - beta0) * u / beta_steps), in double."""
        return min(1.0, self.beta0 + (1.0 - self.beta0) * u / self.beta_steps)

    def _gpu(self, what: str) -> None:
        self.check_created()
        if self._handle is None:
            raise RuntimeError(f"{what} runs on the MI355X sum tree; create the buffer with device='cuda' "
                               "(there is no CPU sampler)")

    def sample(self, batch_size: int, beta: float | None = None):
        """B transitions drawn in proportion to priority (stratified over B segments of the total), as
        ``(state, action, reward, done, next_state)``; the slots and importance weights go to ``last_slots`` /
        ``last_weights``.  The Philox counter is the buffer's sample count, and ``beta`` defaults to ``beta(it)``."""
        self._gpu("sample()")
        if self._number_transitions <= 0:
            raise ValueError("cannot sample from an empty replay buffer")
        self._sync_lens()
        B, dev = int(batch_size), self._dev
        out_s, out_a, out_r, out_d, out_s2 = self._empty_rows(B)
        slots = t.empty(B, dtype=t.int32, device=dev)
        w = t.empty(B, dtype=t.float32, device=dev)
        b = self.beta(self._sample_counter) if beta is None else float(beta)
        with _capi.on_device(dev):
            _capi.check(self._lib.oprl_replay_prio_sample(
                self._handle, B, self.seed, self._sample_counter, b, _capi.ptr(out_s), _capi.ptr(out_a),
                _capi.ptr(out_r), _capi.ptr(out_d), _capi.ptr(out_s2), _capi.ptr(slots), _capi.ptr(w),
                _capi.current_stream()), "oprl_replay_prio_sample")
        self._sample_counter += 1
        self.last_slots, self.last_weights = slots, w
        return out_s, out_a, out_r, out_d, out_s2

    def update_priorities(self, slots, td_abs) -> None:
        """New priorities (max(td_abs, 0) + eps)^alpha for ``slots`` (as ``last_slots``); a slot listed twice takes
        the later row."""
        self._gpu("update_priorities()")
        sl = t.as_tensor(slots).to(device=self._dev, dtype=t.int32).reshape(-1).contiguous()
        td = t.as_tensor(td_abs).to(device=self._dev, dtype=t.float32).reshape(-1).contiguous()
        if sl.numel() != td.numel():
            raise ValueError(f"{sl.numel()} slots but {td.numel()} TD errors")
        self._sync_lens()
        with _capi.on_device(self._dev):
            _capi.check(self._lib.oprl_replay_prio_update(self._handle, sl.numel(), _capi.ptr(sl), _capi.ptr(td),
                                                          _capi.current_stream()), "oprl_replay_prio_update")

    def tree(self) -> tuple[t.Tensor, float]:
        """The whole sum tree as the device holds it (every level, leaves first: ``tree_layout``) and p_max.
        Synchronises the current stream."""
        self._gpu("tree()")
        self._sync_lens()
        n, pm = C.c_int64(), C.c_float()
        with _capi.on_device(self._dev):
            _capi.check(self._lib.oprl_replay_prio_read(self._handle, None, 0, C.byref(n), None,
                                                        _capi.current_stream()), "oprl_replay_prio_read")
            out = t.empty(n.value, dtype=t.float32, device=self._dev)
            _capi.check(self._lib.oprl_replay_prio_read(self._handle, _capi.ptr(out), n.value, None, C.byref(pm),
                                                        _capi.current_stream()), "oprl_replay_prio_read")
        return out, float(pm.value)

    def priorities(self) -> t.Tensor:
        """The leaves as [E, L]: the priority of slot (e, t), 0 where the slot is not live."""
        E, L = self._max_episodes, self.max_episode_lenth
        return self.tree()[0][:E * L].view(E, L)

    def state_dict(self) -> dict:
        sd = super().state_dict()
        sd["prio"] = {"alpha": self.alpha, "beta0": self.beta0, "beta_steps": self.beta_steps, "eps": self.eps}
        if self._handle is not None:
            tree, pm = self.tree()
            E, L = self._max_episodes, self.max_episode_lenth
            sd["prio"].update(leaves=tree[:E * L].cpu().clone(), p_max=pm)
        return sd

    def load_state_dict(self, sd: dict) -> None:
        super().load_state_dict(sd)
        p = sd["prio"]
        self.alpha, self.beta0, self.beta_steps, self.eps = p["alpha"], p["beta0"], p["beta_steps"], p["eps"]
        if self._handle is not None:
            self._sync_lens()
            self._enable()
            if "leaves" in p:
                leaves = p["leaves"].to(device=self._dev, dtype=t.float32).contiguous()
                with _capi.on_device(self._dev):
                    _capi.check(self._lib.oprl_replay_prio_load(self._handle, _capi.ptr(leaves), float(p["p_max"]),
                                                                _capi.current_stream()), "oprl_replay_prio_load")
