"""Synthetic goal-conditioned environment: a point mass that has to reach a goal drawn anew every episode.

The sparse-reward, goal-conditioned tasks hindsight experience replay is made for (the Fetch tasks of Andrychowicz et
al. 2017) are CPU simulators outside this build, like the simulators synthetic.py stands in for; this is their cheap
stand-in with the same observation structure, flattened into one row:

    state = [ x (G) | v (G) | achieved goal (G) | desired goal (G) ]        S = 4 G,  A = G

The achieved goal is the position.  The reward is sparse, 0 within ``threshold`` of the goal and -1 elsewhere, computed
by ``sparse_reward`` with the float32 operations, in the order, of the hindsight sampler (csrc/replay_her.hip), so a
stored reward and a recomputed one agree exactly.  It never terminates; episodes are truncated at 50 steps."""
from __future__ import annotations

from typing import Any

import numpy as np
import numpy.typing as npt

from oprl_amd.environment.synthetic import _Box

# task -> goal dimension G
GOAL_TASKS: dict[str, int] = {"goal-reach-2d": 2, "goal-reach-3d": 3}
F = np.float32


def sparse_reward(achieved: npt.NDArray, desired: npt.NDArray, threshold: float) -> float:
    """0 if dist^2 <= threshold^2 else -1; dist^2 summed over the elements in order, every operation one float32
    rounding, the threshold squared in double and rounded once."""
    a, g = np.asarray(achieved, F), np.asarray(desired, F)
    dist2 = F(0)
    for k in range(len(a)):
        d = F(a[k] - g[k])
        dist2 = F(dist2 + F(d * d))
    return 0.0 if dist2 <= F(float(threshold) * float(threshold)) else -1.0


class SyntheticGoalEnv:
    env_family = "synthetic"      # never passes for a simulator: runners and logs can tell

    def __init__(self, name: str, seed: int = 0, episode_length: int = 50, threshold: float = 0.1):
        if name not in GOAL_TASKS:
            raise ValueError(f"unknown env {name!r}; known: {sorted(GOAL_TASKS)}")
        self.name = name
        self.G = G = GOAL_TASKS[name]
        self.S, self.A = 4 * G, G
        self.episode_length = episode_length
        self.threshold = float(threshold)
        self._rng = np.random.RandomState(seed)
        self._t = 0
        self._x = np.zeros(G, F)
        self._v = np.zeros(G, F)
        self._goal = np.zeros(G, F)

    @property
    def goal_layout(self) -> dict[str, Any]:
        """Where the goals sit in a state row, for HindsightEpisodicReplayBuffer."""
        return dict(achieved_offset=2 * self.G, desired_offset=3 * self.G, goal_dim=self.G, threshold=self.threshold)

    @property
    def observation_space(self) -> _Box:
        return _Box((self.S,), -np.inf, np.inf)

    @property
    def action_space(self) -> _Box:
        return _Box((self.A,))

    def _obs(self) -> npt.NDArray:
        return np.concatenate([self._x, self._v, self._x, self._goal]).astype(F)

    def reset(self) -> tuple[npt.NDArray, dict[str, Any]]:
        self._t = 0
        self._x = self._rng.uniform(-1, 1, self.G).astype(F)
        self._v = np.zeros(self.G, F)
        self._goal = self._rng.uniform(-1, 1, self.G).astype(F)
        return self._obs(), {}

    def sample_action(self) -> npt.NDArray:
        return self._rng.uniform(-1, 1, self.A).astype(F)

    def step(self, action: npt.NDArray):
        a = np.clip(np.asarray(action, F).reshape(self.A), -1, 1)
        self._v = (F(0.8) * self._v + F(0.2) * a).astype(F)
        self._x = np.clip(self._x + F(0.25) * self._v, -1.5, 1.5).astype(F)
        self._t += 1
        reward = sparse_reward(self._x, self._goal, self.threshold)
        truncated = self._t >= self.episode_length
        return self._obs(), reward, False, truncated, {}
