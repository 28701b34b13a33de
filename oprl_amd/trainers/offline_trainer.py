"""Training from a fixed dataset: no environment in the loop (TD3+BC, algos/td3_bc.py).

The replay is filled once (buffers/offline_dataset.py ``fill_replay``) and the run is ``num_updates`` updates in calls of
``updates_per_call``: each call is ONE ``algo.update_from_buffer(buffer, batch_size, n_updates=K)``, that is one
``step_n(K)`` — the kernels draw and gather their own rows from the HBM-resident replay, and the host waits for nothing
between calls.  Everything else happens on call boundaries: ``evaluate()`` (the greedy policy on ``make_env_test``
environments, whose observations go through the dataset's ``ObsNorm``, since that is what the policy was trained on),
saving the policy with the ``ObsNorm`` next to the weights, the stdout and logger lines."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Callable

import numpy as np
import torch as t

from oprl_amd.algos.base_algorithm import check_nstep_gamma, refuse_prioritized
from oprl_amd.algos.protocols import AlgorithmProtocol
from oprl_amd.buffers.offline_dataset import ObsNorm
from oprl_amd.buffers.protocols import ReplayBufferProtocol
from oprl_amd.environment.protocols import EnvProtocol
from oprl_amd.logging import LoggerProtocol, create_stdout_logger

logger = create_stdout_logger()


@dataclass
class OfflineTrainer:
    logger: LoggerProtocol
    make_env_test: Callable[[int], EnvProtocol]
    replay_buffer: ReplayBufferProtocol
    algo: AlgorithmProtocol
    obs_norm: ObsNorm | None = None      # what fill_replay returned (None: the observations were stored as they are)
    num_updates: int = int(1e6)
    updates_per_call: int = 1000
    batch_size: int = 256
    eval_interval: int = int(5e3)        # in updates; the periodic work runs on the first call boundary at or after it
    num_eval_episodes: int = 10
    save_policy_every: int = int(100_000)
    stdout_log_every: int = int(1e5)
    seed: int = 0

    def train(self) -> None:
        self.algo.check_created()
        self.replay_buffer.check_created()
        refuse_prioritized(self.algo, self.replay_buffer)
        check_nstep_gamma(self.algo, self.replay_buffer)
        if self.updates_per_call < 1 or self.num_updates < 0:
            raise ValueError(f"updates_per_call={self.updates_per_call}, num_updates={self.num_updates}: need >= 1 and >= 0")
        if len(self.replay_buffer) < 1:
            raise ValueError("the replay buffer is empty: fill_replay(buffer, load_dataset(path)) first")
        done = 0
        while done < self.num_updates:
            K = min(self.updates_per_call, self.num_updates - done)
            self.algo.update_from_buffer(self.replay_buffer, self.batch_size, n_updates=K)
            self._periodic(done, done + K)
            done += K

    @staticmethod
    def _due(every: int, before: int, after: int) -> bool:
        """Did the updates ``before + 1 .. after`` pass a multiple of ``every``?"""
        return every > 0 and after // every > before // every

    def _periodic(self, before: int, after: int) -> None:
        if self._due(self.eval_interval, before, after):
            self.logger.log_scalar("trainer/ep_reward", self.evaluate()["return"], after)
            self.logger.log_scalar("trainer/buffer_transitions", len(self.replay_buffer), after)
        if self._due(self.save_policy_every, before, after):
            self.save_policy(self.logger.log_dir / "weights" / f"{after}.w")
        if self._due(self.stdout_log_every, before, after):
            perc = int(after / max(self.num_updates, 1) * 100)
            logger.info(f"Update {after:8d} ({perc:2d}%)")

    def _obs(self, obs):
        return self.obs_norm(obs) if self.obs_norm is not None else obs

    def evaluate(self) -> dict[str, float]:
        """Mean undiscounted return of the greedy policy over ``num_eval_episodes`` fresh environments."""
        totals = []
        for k in range(self.num_eval_episodes):
            env = self.make_env_test(self.seed + k)
            obs, _ = env.reset()
            ret, over = 0.0, False
            while not over:
                obs, reward, terminated, truncated, _ = env.step(self.algo.actor.exploit(self._obs(obs)))
                ret += reward
                over = bool(terminated or truncated)
            totals.append(ret)
        return {"return": float(np.mean(totals))}

    def save_policy(self, target) -> None:
        """Whole-module pickle of the actor, as trainers/base_trainer.py saves it, and ``<target>.norm.npz`` with the
        observation statistics the policy expects its inputs to have gone through."""
        from pathlib import Path
        target = Path(target)
        target.parent.mkdir(parents=True, exist_ok=True)
        t.save(self.algo.actor, target)
        if self.obs_norm is not None:
            np.savez(target.with_name(target.name + ".norm.npz"), **self.obs_norm.state_dict())
