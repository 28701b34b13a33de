"""Hindsight experience replay out of the HBM episodic replay (Andrychowicz et al., NeurIPS 2017).

A flat state row carries the achieved goal at ``[achieved_offset, achieved_offset + goal_dim)`` and the desired goal at
``[desired_offset, desired_offset + goal_dim)``.  ``sample`` draws slots (e, t) exactly as
``EpisodicReplayBuffer.sample`` does and relabels a share ``her_ratio`` of the rows that have a later, always-written
row in their episode: the desired goal of ``state`` and ``next_state`` becomes the goal achieved at a later step t'
(``strategy='future'``: uniform over the rest of the episode; ``'final'``: its last such step) and the reward is
recomputed from the distance between what ``next_state`` achieved and that goal,

    sparse:  0 if dist^2 <= threshold^2 else -1          dense:  -dist

Actions and done flags are the stored ones.  Every learner trains on these rows unchanged, in every arithmetic mode and
launch form.  The gather is one HIP kernel (``oprl_replay_sample_her``, csrc/replay_her.hip); the mode is host state on
the C handle (``oprl_replay_set_her``), which is also how ``learner.step_n(buffer.handle, ...)`` finds it.

Not combined with n-step returns or prioritized replay.  On ``device='cpu'`` this is a host container like its base:
``sample`` raises."""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy.typing as npt
import torch as t

from oprl_amd import _capi
from oprl_amd.buffers.episodic_buffer import EpisodicReplayBuffer

MAX_GOAL_DIM = 16      # csrc/replay_internal.h kHerMaxGoal: one lane per (sample, goal element)
STRATEGIES = {"future": 0, "final": 1}
REWARDS = {"sparse": 0, "dense": 1}


def _is_int(x) -> bool:
    return not isinstance(x, bool) and isinstance(x, (int, float)) and int(x) == x


@dataclass
class HindsightEpisodicReplayBuffer(EpisodicReplayBuffer):
    goal_dim: int = 0
    achieved_offset: int = 0
    desired_offset: int = 0
    her_ratio: float = 0.8          # relabelled share of the eligible rows (k = 4 hindsight goals per stored one)
    strategy: str = "future"
    reward: str = "sparse"
    threshold: float = 0.05

    def _validate(self) -> None:
        G, a, g, S = self.goal_dim, self.achieved_offset, self.desired_offset, self.state_dim
        if not (_is_int(G) and _is_int(a) and _is_int(g)) or not 1 <= G <= MAX_GOAL_DIM:
            raise ValueError(f"goal_dim={G!r}, achieved_offset={a!r}, desired_offset={g!r}: integers, "
                             f"goal_dim in [1, {MAX_GOAL_DIM}]")
        if a < 0 or a + G > S or g < 0 or g + G > S:
            raise ValueError(f"the achieved goal [{a}, {a + G}) and the desired goal [{g}, {g + G}) must lie inside the "
                             f"state row [0, {S})")
        if a < g + G and g < a + G:
            raise ValueError(f"the achieved goal [{a}, {a + G}) and the desired goal [{g}, {g + G}) overlap")
        if not isinstance(self.her_ratio, (int, float)) or not 0 <= self.her_ratio <= 1:      # (nan fails both)
            raise ValueError(f"her_ratio={self.her_ratio!r}: must lie in [0, 1]")
        if not isinstance(self.threshold, (int, float)) or not (self.threshold >= 0 and math.isfinite(self.threshold)):
            raise ValueError(f"threshold={self.threshold!r}: must be finite and >= 0")
        if self.strategy not in STRATEGIES:
            raise ValueError(f"strategy={self.strategy!r}: one of {sorted(STRATEGIES)}")
        if self.reward not in REWARDS:
            raise ValueError(f"reward={self.reward!r}: one of {sorted(REWARDS)}")

    def create(self) -> "HindsightEpisodicReplayBuffer":
        self._validate()          # before the GPU is touched
        super().create()
        self._set_her()
        return self

    def _set_her(self) -> None:
        if self._handle is not None:
            _capi.check(self._lib.oprl_replay_set_her(
                self._handle, int(self.achieved_offset), int(self.desired_offset), int(self.goal_dim),
                float(self.her_ratio), STRATEGIES[self.strategy], REWARDS[self.reward], float(self.threshold)),
                "oprl_replay_set_her")

    def sample(self, batch_size: int, inds: t.Tensor | npt.NDArray | None = None, return_indices: bool = False,
               return_relabel: bool = False):
        """``(state, action, reward, done, next_state)`` for uniformly drawn slots, a share of them relabelled;
        ``inds`` and ``return_indices`` as in the base class; ``return_relabel`` appends t' (int32[B]): the step whose
        next state gave a relabelled row its goal, -1 for a row that is the stored one."""
        out = [x for x in self._sample("oprl_replay_sample_her", batch_size, inds, return_indices, bool(return_relabel))
               if x is not None]
        return out[0] if len(out) == 1 else tuple(out)

    _FIELDS = ("goal_dim", "achieved_offset", "desired_offset", "her_ratio", "strategy", "reward", "threshold")

    def state_dict(self) -> dict:
        sd = super().state_dict()
        sd["her"] = {k: getattr(self, k) for k in self._FIELDS}
        return sd

    def load_state_dict(self, sd: dict) -> None:
        super().load_state_dict(sd)
        for k, v in sd.get("her", {}).items():
            if k in self._FIELDS:
                setattr(self, k, v)
        self._validate()
        self._set_her()          # the mode is host state on the handle
