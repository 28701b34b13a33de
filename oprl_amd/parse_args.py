"""Command line of the config scripts.  The flags and their defaults are the reference's
(src/oprl/parse_args.py) — scripts written against it parse the same way — except ``--device``, which
defaults to the only kind of device this learner runs on."""
from __future__ import annotations

import argparse

# (flag, type, default, help) — shared by both entry points
_SHARED = (
    ("--config", str, None, "path of a config file (accepted for compatibility; the scripts are the config)"),
    ("--env", str, "cartpole-balance", "environment name, e.g. walker-walk"),
    ("--device", str, "cuda", "device of the learner (a ROCm GPU; there is no CPU path)"),
    # extension: the learner's arithmetic mode.  Scripts and algorithm classes alike default to
    # exact fp32 — the reference's arithmetic, no input range.  "x2" is the faster parity mode, opt-in: it has a finite
    # range (|observation|, |hidden activation| < 4094, |w| < 256; leaving it raises from update() / check(), it is never
    # silent) — meant for normalised observations
    # extension: multi-step returns out of the replay sampler (buffers/nstep_buffer.py)
    ("--n-step", int, 1, "n-step returns: the sampler sums up to N discounted rewards and bootstraps N steps on (1..16; 1 = the reference's one-step targets)"),
    ("--precision", str, "f32", "f32 (exact fp32 MFMA, the default) | x2 (fp32 as fp16 hi + lo on the matrix cores: parity mode, |obs| < 4094) | bf16"),
)
_SINGLE = (
    ("--seeds", int, 1, "how many seeds to train, one process each"),
    ("--start_seed", int, 0, "first seed; the others count up from it"),
    # extension: N environments stepped per iteration, their actions from one policy launch (trainers/vec_trainer.py,
    # DESIGN.md section 13); 1 = the reference's loop (trainers/base_trainer.py)
    ("--num-envs", int, 1, "environments stepped per iteration, one policy launch for all (1..256; 1 = the reference's one-environment loop)"),
)
_DISTRIB = (
    ("--seed", int, 0, "random seed of the run"),
    # extension (BASELINE.json config 5): > 1 = that many data-parallel learner processes, one per GPU,
    # fed over shared-memory rings (runners/train_distrib.py::run_dp_training); 1 = the reference's layout
    ("--learners", int, 1, "data-parallel learner processes (one per GPU)"),
    ("--actors", int, 0, "CPU actor processes (0: the script's default)"),
)


def _parser(title: str, extra) -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(description=title)
    for flag, kind, default, text in (*_SHARED, *extra):
        if kind is bool:      # a switch (configs/td3_bc.py --no-normalize)
            parser.add_argument(flag, action="store_true", help=text)
        else:
            parser.add_argument(flag, type=kind, default=default, help=text)
    # extension: prioritized experience replay (buffers/prioritized_buffer.py)
    parser.add_argument("--per", action="store_true",
                        help="prioritized replay: sample by |TD| priority from the sum tree in HBM, importance-weighted "
                             "critic loss (DDPG, TD3, SAC, REDQ; f32, one learner; not with --n-step > 1)")
    return parser


def check_per(args: argparse.Namespace) -> bool:
    """Is ``--per`` given?  Raises ValueError when it comes with ``--n-step > 1``: the replay refuses a sum tree over
    n-step rows, and the scripts say so before anything is built."""
    if not getattr(args, "per", False):
        return False
    if getattr(args, "n_step", 1) > 1:
        raise ValueError(f"--per with --n-step {args.n_step}: n-step TD errors as priorities are not supported "
                         "(the replay refuses a sum tree over n-step rows); give one of the two")
    return True


def parse_args(extra=()) -> argparse.Namespace:
    """Flags of the single-process scripts (configs/ddpg.py ...).  ``extra``: a script's own flags, as (flag, type,
    default, help) tuples (configs/d4pg.py: the atoms of its critic); type ``bool`` makes a switch."""
    parser = _parser("Run training", (*_SINGLE, *extra))
    # extension: one open replay episode per environment (buffers/episodic_buffer.py open_lanes)
    parser.add_argument("--open-episodes", action="store_true",
                        help="with --num-envs N > 1: N open episodes in the replay, every iteration's N transitions "
                             "written at once (next states included) instead of whole episodes when they end")
    # extension: hindsight experience replay (buffers/hindsight_buffer.py)
    parser.add_argument("--her", action="store_true",
                        help="hindsight experience replay: the sampler relabels goals from later steps of the same episode "
                             "and recomputes the sparse reward (goal-conditioned environments, e.g. synthetic:goal-reach-2d; "
                             "not with --per or --n-step > 1)")
    parser.add_argument("--her-ratio", type=float, default=0.8,
                        help="with --her: the relabelled share of the sampled rows that can be relabelled (0.8 = 4 hindsight goals per stored one)")
    parser.add_argument("--her-strategy", type=str, default="future", choices=("future", "final"),
                        help="with --her: goals from a uniformly drawn later step of the episode (future) or from its last one (final)")
    # extension: a fixed dataset in every batch (buffers/prior_buffer.py)
    parser.add_argument("--prior-data", type=str, default=None,
                        help="online training with prior data: an .npz dataset (buffers/offline_dataset.py) that supplies "
                             "--prior-share of every batch (not with --per, --n-step > 1, --her, --num-envs > 1)")
    parser.add_argument("--prior-share", type=float, default=0.5,
                        help="with --prior-data, or --finetune-steps of the offline scripts: the share of every batch that "
                             "comes from the dataset (0.5 = symmetric sampling)")
    return parser.parse_args()


def check_share(args: argparse.Namespace) -> float:
    share = getattr(args, "prior_share", 0.5)
    if not 0 <= share <= 1:      # (nan fails)
        raise ValueError(f"--prior-share {share}: the dataset's share of a batch must lie in [0, 1]")
    return share


def check_prior(args: argparse.Namespace) -> bool:
    """Is ``--prior-data`` given?  Raises ValueError when it comes with ``--per``, ``--n-step > 1`` or ``--her`` (the
    replay refuses those rows on either side of a mixed batch) or with ``--num-envs > 1`` / ``--open-episodes`` (not
    built): the scripts say so before anything is built."""
    if not getattr(args, "prior_data", None):
        return False
    check_share(args)
    for on, flag in ((getattr(args, "per", False), "--per"), (getattr(args, "n_step", 1) > 1, f"--n-step {getattr(args, 'n_step', 1)}"),
                     (getattr(args, "her", False), "--her"), (getattr(args, "num_envs", 1) > 1, f"--num-envs {getattr(args, 'num_envs', 1)}"),
                     (getattr(args, "open_episodes", False), "--open-episodes")):
        if on:
            raise ValueError(f"--prior-data with {flag}: batches mixed from a dataset and fresh experience are plain "
                             "one-step rows collected by one environment; drop one of the two")
    return True


def check_finetune(args: argparse.Namespace) -> int:
    """``--finetune-steps`` of the offline scripts (0: none).  Raises ValueError for a negative count, with
    ``--n-step > 1`` (mixed batches are one-step rows) and with ``--prior-data`` (the dataset is ``--dataset``)."""
    steps = getattr(args, "finetune_steps", 0)
    if getattr(args, "prior_data", None):
        raise ValueError("--prior-data: an offline script's dataset is --dataset; --finetune-steps N continues online "
                         "with that dataset in every batch")
    if steps < 0:
        raise ValueError(f"--finetune-steps {steps}: expected >= 0")
    if steps == 0:
        return 0
    check_share(args)
    if getattr(args, "n_step", 1) > 1:
        raise ValueError(f"--finetune-steps with --n-step {args.n_step}: batches mixed from the dataset and fresh "
                         "experience are one-step rows; drop one of the two")
    return steps


def check_her(args: argparse.Namespace) -> bool:
    """Is ``--her`` given?  Raises ValueError when it comes with ``--per`` or ``--n-step > 1``: the replay refuses both
    combinations, and the scripts say so before anything is built."""
    if not getattr(args, "her", False):
        return False
    if getattr(args, "per", False):
        raise ValueError("--her with --per: hindsight goals over the sum tree are not supported; give one of the two")
    if getattr(args, "n_step", 1) > 1:
        raise ValueError(f"--her with --n-step {args.n_step}: hindsight goals over n-step rows are not supported; give "
                         "one of the two")
    return True


def parse_args_distrib() -> argparse.Namespace:
    """Flags of configs/distrib_ddpg.py."""
    return _parser("Run distrib training", _DISTRIB).parse_args()
