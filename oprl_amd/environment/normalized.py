"""An environment whose observations go through a dataset's ``ObsNorm`` (buffers/offline_dataset.py).

A policy pre-trained on a dataset that ``fill_replay`` normalised expects ``(obs - mean) / (std + 1e-3)``.  Wrapped in
``NormalizedObsEnv`` an environment hands the trainer such observations from ``reset`` and ``step``, so the policy acts
on what it was trained on and the rows the trainer stores match the stored dataset rows (trainers/finetune.py,
DESIGN.md §20).  Everything else is the wrapped environment's."""
from __future__ import annotations

from oprl_amd.buffers.offline_dataset import ObsNorm


class NormalizedObsEnv:
    def __init__(self, env, obs_norm: ObsNorm) -> None:
        if obs_norm is None:
            raise ValueError("NormalizedObsEnv: an ObsNorm expected (fill_replay(..., normalize=True) returns one)")
        self.env = env
        self.obs_norm = obs_norm

    def reset(self):
        obs, info = self.env.reset()
        return self.obs_norm(obs), info

    def step(self, action):
        obs, reward, terminated, truncated, info = self.env.step(action)
        return self.obs_norm(obs), reward, terminated, truncated, info

    def __getattr__(self, name):
        # (only what this class does not define: sample_action, the spaces, episode_length, env_family ...)
        if name in ("env", "obs_norm"):
            raise AttributeError(name)
        return getattr(self.env, name)
