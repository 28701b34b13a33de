"""N-step returns out of the HBM episodic replay.

``sample`` draws slots (e, t) exactly as ``EpisodicReplayBuffer.sample`` does and returns, per row, with m = the steps
taken (at most ``n_step``, never past the episode's stored steps, none after the first step whose done is not 0):

    reward     = sum_{k<m} gamma^k r_{t+k}
    done       = 1 - gamma^(m-1) (1 - d_{t+m-1})        (d_t verbatim when m = 1)
    next_state = s_{t+m}

Every learner's TD target has the form ``r + gamma (1 - d) q'(s')`` with ``d`` read as a float, so these rows make it
``R + gamma^m (1 - d_last) q'(s_{t+m})``, the n-step target, in every algorithm, arithmetic mode and launch form —
provided the learner's gamma is this buffer's: ``update_from_buffer``, the trainer and ``step_n`` refuse a mismatch.
The gather is one HIP kernel (``oprl_replay_sample_nstep``, csrc/replay_nstep.hip); the mode is host state on the C
handle (``oprl_replay_set_nstep``), which is also how ``learner.step_n(buffer.handle, ...)`` finds it.

SAC / TQC / REDQ get the usual n-step target without entropy terms for the intermediate steps.  Not combined with
prioritized replay.  On ``device='cpu'`` this is a host container like its base: ``sample`` raises."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy.typing as npt
import torch as t

from oprl_amd import _capi
from oprl_amd.buffers.episodic_buffer import EpisodicReplayBuffer

MAX_N_STEP = 16      # csrc/replay_internal.h kNstepMax: one lane per (sample, step)


@dataclass
class NStepEpisodicReplayBuffer(EpisodicReplayBuffer):
    n_step: int = 3

    def _validate(self) -> None:
        if isinstance(self.n_step, bool) or int(self.n_step) != self.n_step or not 1 <= self.n_step <= MAX_N_STEP:
            raise ValueError(f"n_step={self.n_step!r}: must be an integer in [1, {MAX_N_STEP}]")
        if not 0 < self.gamma <= 1:
            raise ValueError(f"gamma={self.gamma!r}: must lie in (0, 1]")

    def create(self) -> "NStepEpisodicReplayBuffer":
        self._validate()
        super().create()
        self._set_nstep()
        return self

    def _set_nstep(self) -> None:
        if self._handle is not None:
            _capi.check(self._lib.oprl_replay_set_nstep(self._handle, int(self.n_step), float(self.gamma)),
                        "oprl_replay_set_nstep")

    def sample(self, batch_size: int, inds: t.Tensor | npt.NDArray | None = None, return_indices: bool = False,
               return_steps: bool = False):
        """``(state, action, R, done', state_{t+m})`` for uniformly drawn slots; ``inds`` and ``return_indices`` as in
        the base class (the (episode, step) pairs are those of the FIRST step); ``return_steps`` appends m (int32[B])."""
        out = [x for x in self._sample("oprl_replay_sample_nstep", batch_size, inds, return_indices, bool(return_steps))
               if x is not None]
        return out[0] if len(out) == 1 else tuple(out)

    def state_dict(self) -> dict:
        sd = super().state_dict()
        sd["n_step"] = int(self.n_step)
        sd["gamma"] = float(self.gamma)
        return sd

    def load_state_dict(self, sd: dict) -> None:
        super().load_state_dict(sd)
        self.n_step = int(sd.get("n_step", self.n_step))
        self.gamma = float(sd.get("gamma", self.gamma))
        self._validate()
        self._set_nstep()      # the mode is host state on the handle
