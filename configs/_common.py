"""Shared body of the single-process training scripts: the factories ``run_training`` wants — environment, algorithm,
replay buffer, logger — built from the command line, importing everything through the ``oprl`` alias package exactly as a
reference config script does.  ``TrainingScript`` is the body of the online scripts (configs/ddpg.py, td3.py, sac.py,
tqc.py, redq.py, d4pg.py), ``OfflineScript`` that of the scripts that train from a fixed dataset (configs/td3_bc.py,
iql.py, cql.py, calql.py): a script is its docstring, its own flags, the algorithm's fields they set and one constructor
call.  No script imports another."""
from __future__ import annotations

import sys
from argparse import Namespace
from dataclasses import dataclass, fields
from pathlib import Path
from typing import Callable

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from oprl.buffers.episodic_buffer import EpisodicReplayBuffer  # noqa: E402
from oprl.buffers.hindsight_buffer import HindsightEpisodicReplayBuffer  # noqa: E402
from oprl.buffers.nstep_buffer import NStepEpisodicReplayBuffer  # noqa: E402
from oprl.buffers.offline_dataset import cut_pieces, fill_replay, load_dataset  # noqa: E402
from oprl.buffers.prior_buffer import PriorDataReplayBuffer  # noqa: E402
from oprl.buffers.prioritized_buffer import PrioritizedEpisodicReplayBuffer  # noqa: E402
from oprl.environment import make_env as build_env  # noqa: E402
from oprl.logging import make_text_logger_func  # noqa: E402
from oprl.parse_args import check_finetune, check_her, check_per, check_prior, parse_args  # noqa: E402
from oprl.runners.config import CommonParameters  # noqa: E402
from oprl.runners.train import run_training, set_seed  # noqa: E402
from oprl.trainers.finetune import finetune  # noqa: E402
from oprl.trainers.offline_trainer import OfflineTrainer  # noqa: E402

TRAIN_STEPS = 100_000
REPLAY_TRANSITIONS = 1_000_000


def dataset_transitions(data) -> int:
    """The size of a replay with exactly the episode slots the dataset's pieces need (fill_replay never wraps)."""
    L = next(f.default for f in fields(EpisodicReplayBuffer) if f.name == "max_episode_lenth")
    pieces, _ = cut_pieces(data, L)
    return (len(pieces) + 1) * L


@dataclass
class TrainingScript:
    """Everything a config script exposes: the four factories, the run configuration, ``run()``."""

    algo_cls: type
    algo_name: str
    estimate_q_every: int
    log_every: int
    extra_flags: tuple = ()                  # the script's own flags, (flag, type, default, help) each (parse_args)
    algo_kwargs: Callable[[Namespace], dict] | None = None   # ... and the algorithm's fields they set
    takes_per: bool = True                   # False: the algorithm applies no importance weights, --per is refused ...
    no_per: str = "its loss takes no importance weights yet"      # ... with this reason

    def __post_init__(self) -> None:
        self.args = parse_args(self.flags())
        self.refuse()
        probe = self.make_env(seed=0)
        self.goal_layout = getattr(probe, "goal_layout", None)
        if self.her and self.goal_layout is None:
            raise ValueError(f"--her: the environment {self.args.env!r} has no goal layout (achieved and desired goal "
                             "inside its state rows); hindsight replay needs a goal-conditioned one, e.g. "
                             "synthetic:goal-reach-2d")
        self.episode_length = int(getattr(probe, "episode_length", 1000))
        self.state_dim = int(probe.observation_space.shape[0])
        self.action_dim = int(probe.action_space.shape[0])
        self.config = CommonParameters(state_dim=self.state_dim, action_dim=self.action_dim, num_steps=TRAIN_STEPS,
                                       eval_every=2500, estimate_q_every=self.estimate_q_every,
                                       log_every=self.log_every, device=self.args.device)
        self.make_logger: Callable = make_text_logger_func(algo=self.algo_name, env=self.args.env)

    def flags(self) -> tuple:
        return self.extra_flags

    def refuse(self) -> None:
        """What the flags rule out, said before an environment is built or a file is opened."""
        self.prior = check_prior(self.args)  # --prior-data: a dataset in every batch, refused with --per, --n-step > 1, --her, --num-envs > 1
        self.per = check_per(self.args)      # --per: prioritized replay and an algorithm that applies its weights
        if self.per and not self.takes_per:
            raise ValueError(f"--per: {self.algo_name} does not train from prioritized replay ({self.no_per})")
        self.her = check_her(self.args)      # --her: hindsight replay, refused with --per and with --n-step > 1

    def make_env(self, seed: int):
        return build_env(self.args.env, seed=seed)

    def make_algo(self, logger):
        return self.algo_cls(logger=logger, state_dim=self.state_dim, action_dim=self.action_dim,
                             device=self.args.device, precision=self.args.precision,
                             **(self.algo_kwargs(self.args) if self.algo_kwargs is not None else {}),
                             **({"prioritized": True} if self.per else {})).create()

    def make_replay_buffer(self):
        kw = dict(buffer_size_transitions=max(self.config.num_steps, REPLAY_TRANSITIONS), state_dim=self.state_dim,
                  action_dim=self.action_dim, device=self.config.device)
        if self.args.n_step > 1:        # n-step returns: the sampler discounts with the ALGORITHM's gamma
            gamma = next(f.default for f in fields(self.algo_cls) if f.name == "gamma")
            return NStepEpisodicReplayBuffer(n_step=self.args.n_step, gamma=gamma, **kw).create()
        if self.her:                    # hindsight goals: the layout and the reward's threshold are the environment's
            return HindsightEpisodicReplayBuffer(her_ratio=self.args.her_ratio, strategy=self.args.her_strategy,
                                                 max_episode_lenth=self.episode_length, **self.goal_layout, **kw).create()
        if self.per:
            return PrioritizedEpisodicReplayBuffer(**kw).create()
        if self.prior:                  # prior data: the dataset as it is (the environment's observations are not normalised)
            return PriorDataReplayBuffer(prior=self.make_prior_buffer(), prior_share=self.args.prior_share, **kw).create()
        return EpisodicReplayBuffer(**kw).create()

    def make_prior_buffer(self):
        """The ``--prior-data`` dataset, as it is, in a replay of its own size (``dataset_transitions``)."""
        data = load_dataset(self.args.prior_data)
        buf = EpisodicReplayBuffer(buffer_size_transitions=dataset_transitions(data), state_dim=self.state_dim,
                                   action_dim=self.action_dim, device=self.config.device).create()
        fill_replay(buf, data, normalize=False)
        return buf

    def run(self) -> None:
        run_training(make_algo=self.make_algo, make_env=self.make_env, make_replay_buffer=self.make_replay_buffer,
                     make_logger=self.make_logger, config=self.config, seeds=self.args.seeds,
                     start_seed=self.args.start_seed, num_envs=self.args.num_envs,
                     open_episodes=self.args.open_episodes)


LAYER_NORM_FLAG = ("--layer-norm", bool, False,
                   "LayerNorm in the critics' hidden layers (Linear -> LayerNorm -> ReLU; RLPD / DroQ): generic launch "
                   "sequence, f32, one learner; not with --per")


DROPOUT_FLAG = ("--dropout", float, 0.0,
                "dropout rate in front of the critics' LayerNorm (Linear -> Dropout -> LayerNorm -> ReLU; DroQ): needs "
                "--layer-norm (configs/droq.py has both on)")


def layer_norm_kwargs(args: Namespace) -> dict:
    kw = dict(layer_norm=bool(args.layer_norm))
    if args.dropout > 0.0:
        kw["dropout"] = float(args.dropout)
    return kw


def droq_kwargs(args: Namespace) -> dict:
    """configs/droq.py: LayerNorm is the recipe's; ``--dropout`` replaces the class's rate only where it is given."""
    return dict(dropout=float(args.dropout)) if args.dropout > 0.0 else {}


@dataclass
class LayerNormScript(TrainingScript):
    """configs/sac.py, configs/redq.py and configs/droq.py: ``--layer-norm`` sets the algorithm's ``layer_norm`` field,
    ``--dropout RATE`` its ``dropout``.  ``recipe``: the algorithm's own defaults have both on (DroQ)."""

    extra_flags: tuple = (LAYER_NORM_FLAG, DROPOUT_FLAG)
    algo_kwargs: Callable[[Namespace], dict] | None = layer_norm_kwargs
    recipe: bool = False

    def refuse(self) -> None:
        super().refuse()
        if not 0.0 <= self.args.dropout < 1.0:
            raise ValueError(f"--dropout {self.args.dropout!r}: the rate must lie in [0, 1)")
        if self.recipe:
            self.args.layer_norm = True
        if not self.args.layer_norm:
            if self.args.dropout > 0.0:
                raise ValueError("--dropout without --layer-norm: dropout runs inside the LayerNorm critics' kernels")
            return
        if self.per:
            raise ValueError("--layer-norm with --per: the LayerNorm critics' kernels take no importance weights")
        if self.args.seeds != 1:
            raise ValueError("--layer-norm with --seeds > 1: LayerNorm critics are built and measured for one learner per "
                             "GPU; one run per invocation (--start_seed picks its seed)")


OFFLINE_FLAGS = (       # of every offline script: --dataset before the script's own flags, the others behind them
    ("--dataset", str, None, "the dataset: an .npz with observations, actions, rewards, terminals [, timeouts, next_observations]"),
    ("--updates", int, 1_000_000, "updates to run"),
    ("--batch", int, 256, "minibatch rows"),
    ("--updates-per-call", int, 1000, "updates per step_n call; evaluation, saving and logging happen between calls"),
    ("--no-normalize", bool, False, "store the observations as they are instead of (x - mean) / (std + 1e-3)"),
    ("--finetune-steps", int, 0, "after the offline updates: that many environment steps of online training, --prior-share of every batch from the dataset (0: none)"),
)


@dataclass
class OfflineScript(TrainingScript):
    """A script that trains from a fixed dataset (``--dataset``; trainers/offline_trainer.py) and may go on online with
    the dataset in every batch (``--finetune-steps``; trainers/finetune.py).  No environment is in its training loop."""

    estimate_q_every: int = 0
    log_every: int = 5000
    takes_per: bool = False
    title: str = ""                          # the algorithm as the refusals name it (default: ``algo_name``)
    no_her: str = ""                         # why --her is refused (default: it trains from a fixed dataset here)

    def flags(self) -> tuple:
        return (OFFLINE_FLAGS[0], *self.extra_flags, *OFFLINE_FLAGS[1:])

    def refuse(self) -> None:
        super().refuse()
        args, title = self.args, self.title or self.algo_name
        if self.her:
            raise ValueError(f"--her: {self.no_her or title + ' trains from a fixed dataset here'}; hindsight replay is "
                             "wired into the online scripts")
        if args.num_envs > 1 or args.open_episodes:
            raise ValueError(f"--num-envs > 1 / --open-episodes: {title} trains from a fixed dataset, no environment is "
                             "stepped during training (evaluation runs its own)")
        if args.seeds != 1:
            raise ValueError("--seeds > 1: one offline run per invocation (--start_seed picks its seed)")
        self.finetune_steps = check_finetune(args)      # --finetune-steps: refused with --n-step > 1

    def make_replay_buffer(self, data):
        kw = dict(buffer_size_transitions=dataset_transitions(data), state_dim=self.state_dim, action_dim=self.action_dim,
                  device=self.config.device)
        if self.args.n_step > 1:        # n-step returns: the sampler discounts with the ALGORITHM's gamma
            gamma = next(f.default for f in fields(self.algo_cls) if f.name == "gamma")
            return NStepEpisodicReplayBuffer(n_step=self.args.n_step, gamma=gamma, **kw).create()
        return EpisodicReplayBuffer(**kw).create()

    def run(self) -> None:
        args, config = self.args, self.config
        if not args.dataset:
            raise ValueError("--dataset PATH is required (tools/make_offline_dataset.py writes one)")
        seed = args.start_seed
        set_seed(seed)
        data = load_dataset(args.dataset)
        buffer = self.make_replay_buffer(data)
        buffer.seed = seed
        norm = fill_replay(buffer, data, normalize=not args.no_normalize)
        logger = self.make_logger(seed)
        algo = self.make_algo(logger)
        algo.set_seed(seed)
        OfflineTrainer(logger=logger, make_env_test=self.make_env, replay_buffer=buffer, algo=algo, obs_norm=norm,
                       num_updates=args.updates, updates_per_call=args.updates_per_call, batch_size=args.batch,
                       eval_interval=config.eval_every * 2, stdout_log_every=config.log_every, seed=seed).train()
        if self.finetune_steps > 0:     # the same algorithm object goes on online, the dataset in every batch
            finetune(algo=algo, prior_buffer=buffer, obs_norm=norm, make_env=self.make_env, logger=logger,
                     num_steps=self.finetune_steps, batch_size=args.batch, prior_share=args.prior_share, seed=seed,
                     eval_interval=config.eval_every, stdout_log_every=config.log_every)
