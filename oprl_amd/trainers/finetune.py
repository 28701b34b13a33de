"""Offline-to-online fine-tuning: what ``configs/td3_bc.py`` / ``iql.py`` / ``cql.py`` do after ``OfflineTrainer.train()``
when ``--finetune-steps N`` is given.

The SAME algorithm object goes on in a ``BaseTrainer`` with ``start_steps=0`` (the pre-trained policy acts from the
second step on; no uniform warm-up), and every batch it trains on comes partly from the dataset and partly from the
fresh experience: the training buffer is a ``PriorDataReplayBuffer`` whose prior is the dataset's buffer.  Where the
dataset was normalised, the training environment and the evaluation environments are wrapped in ``NormalizedObsEnv``:
the policy acts on what it was trained on, and the rows the trainer stores match the stored dataset rows.  The
algorithm's offline mode (TD3+BC's cloning term, IQL's losses, CQL's penalty) stays on."""
from __future__ import annotations

from typing import Callable

from oprl_amd.buffers.offline_dataset import ObsNorm
from oprl_amd.buffers.prior_buffer import PriorDataReplayBuffer
from oprl_amd.environment.normalized import NormalizedObsEnv
from oprl_amd.environment.protocols import EnvProtocol
from oprl_amd.trainers.base_trainer import BaseTrainer


def finetune(algo, prior_buffer, obs_norm: ObsNorm | None, make_env: Callable[[int], EnvProtocol], logger,
             num_steps: int, batch_size: int, prior_share: float = 0.5, seed: int = 0, **trainer_kwargs) -> BaseTrainer:
    """``num_steps`` environment steps of online training on top of what ``algo`` learned from ``prior_buffer``.
    ``obs_norm``: what ``fill_replay`` returned for that buffer (None: the observations were stored as they are).  The
    online replay is sized so that every step of the run fits.  Returns the trainer; its ``replay_buffer`` is the
    ``PriorDataReplayBuffer``."""
    if num_steps < 1:
        raise ValueError(f"finetune: num_steps={num_steps}: at least one environment step")
    if getattr(prior_buffer, "n_step", 1) > 1:
        raise ValueError(f"finetune: the dataset's buffer samples {prior_buffer.n_step}-step returns; batches mixed from "
                         "the dataset and fresh experience are one-step rows")

    def make(s: int):
        env = make_env(s)
        return NormalizedObsEnv(env, obs_norm) if obs_norm is not None else env

    env = make(seed)
    L = int(getattr(env, "episode_length", 1000))
    size = (-(-(num_steps + 1) // L) + 2) * L      # (the loop takes num_steps + 1 steps; one slot stays open behind them)
    buffer = PriorDataReplayBuffer(buffer_size_transitions=size, state_dim=prior_buffer.state_dim,
                                   action_dim=prior_buffer.action_dim, max_episode_lenth=L, device=prior_buffer.device,
                                   seed=int(getattr(prior_buffer, "seed", seed)), prior=prior_buffer,
                                   prior_share=prior_share).create()
    trainer = BaseTrainer(logger=logger, env=env, make_env_test=make, replay_buffer=buffer, algo=algo, num_steps=num_steps,
                          start_steps=0, batch_size=batch_size, seed=seed, **trainer_kwargs)
    trainer.train()
    return trainer
