"""Cal-QL on the MI355X learner — offline RL from a fixed dataset that is meant to be fine-tuned online (Nakamoto et al. 2023:
CQL whose penalty bounds the critics' values at the policy's actions below by the dataset's returns-to-go; DESIGN.md section
21); written like configs/cql.py, whose flags it has.  The dataset is an ``.npz`` with the D4RL key names (buffers/offline_dataset.py;
tools/make_offline_dataset.py writes one from a ``synthetic:`` environment — D4RL itself is not available to this build).
``--env`` names the environment the policy is evaluated on.  There is no environment in the training loop, so
``--num-envs > 1`` and ``--open-episodes`` are refused, and so are ``--per`` (a fixed dataset is sampled uniformly) and
``--her`` (relabelled rewards have no stored return).

    python configs/calql.py --dataset data.npz --env synthetic:walker-walk [--cql-alpha 5.0] [--cql-actions 10] [--tune-alpha]
                          [--updates N] [--batch 256] [--updates-per-call K] [--no-normalize] [--n-step N]
                          [--finetune-steps N [--prior-share 0.5]]

``--finetune-steps N``: after the offline updates the same learner goes on for N environment steps online, every batch
drawn partly from the dataset and partly from the fresh experience (trainers/finetune.py; not with ``--n-step > 1``); the
returns-to-go of the fresh rows are those of the episodes as far as they have run.
"""
import sys
from dataclasses import fields
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent))
sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from _common import TrainingScript  # noqa: E402
from oprl.parse_args import check_finetune, parse_args  # noqa: E402
from oprl.algos.calql import CalQL  # noqa: E402

FLAGS = (
    ("--dataset", str, None, "the dataset: an .npz with observations, actions, rewards, terminals [, timeouts, next_observations]"),
    ("--cql-alpha", float, 5.0, "weight of the conservative penalty, >= 0"),
    ("--cql-actions", int, 10, "sampled actions per kind and state (uniform, pi(.|s), pi(.|s')), 1 .. 16"),
    ("--tune-alpha", bool, False, "learn SAC's temperature instead of keeping alpha_init"),
    ("--updates", int, 1_000_000, "updates to run"),
    ("--batch", int, 256, "minibatch rows"),
    ("--updates-per-call", int, 1000, "updates per step_n call; evaluation, saving and logging happen between calls"),
    ("--no-normalize", bool, False, "store the observations as they are instead of (x - mean) / (std + 1e-3)"),
    ("--finetune-steps", int, 0, "after the offline updates: that many environment steps of online training, --prior-share of every batch from the dataset (0: none)"),
)


def hparams_of(args) -> dict:
    return dict(cql_alpha=args.cql_alpha, cql_n_actions=args.cql_actions, tune_alpha=args.tune_alpha, batch_size=args.batch)


def refuse(args) -> int:
    """What this script does not run, said before an environment is built or the dataset is looked at; returns
    ``--finetune-steps``."""
    if args.per:
        raise ValueError("--per: CalQL does not train from prioritized replay (a fixed dataset is sampled uniformly, and "
                         "the penalty takes no importance weights)")
    if args.her:
        raise ValueError("--her: Cal-QL bounds its critics by the stored returns-to-go, and a hindsight replay relabels "
                         "its rewards per sample; hindsight replay is wired into the online scripts")
    if args.num_envs > 1 or args.open_episodes:
        raise ValueError("--num-envs > 1 / --open-episodes: Cal-QL trains from a fixed dataset, no environment is "
                         "stepped during training (evaluation runs its own)")
    if args.seeds != 1:
        raise ValueError("--seeds > 1: one offline run per invocation (--start_seed picks its seed)")
    return check_finetune(args)      # --finetune-steps: refused with --n-step > 1


finetune_steps = refuse(parse_args(FLAGS))
script = TrainingScript(CalQL, "CalQL", estimate_q_every=0, log_every=5000, extra_flags=FLAGS, algo_kwargs=hparams_of,
                        takes_per=False)
# the names a reference-style script defines at module level
make_env, make_algo, make_logger, config = script.make_env, script.make_algo, script.make_logger, script.config


def make_replay_buffer(data):
    """A replay with exactly the episode slots the dataset's pieces need (fill_replay never wraps)."""
    from oprl_amd.buffers.episodic_buffer import EpisodicReplayBuffer
    from oprl_amd.buffers.nstep_buffer import NStepEpisodicReplayBuffer
    from oprl_amd.buffers.offline_dataset import cut_pieces
    L = next(f.default for f in fields(EpisodicReplayBuffer) if f.name == "max_episode_lenth")
    pieces, _ = cut_pieces(data, L)
    kw = dict(buffer_size_transitions=(len(pieces) + 1) * L, state_dim=script.state_dim, action_dim=script.action_dim,
              device=config.device)
    if script.args.n_step > 1:          # n-step returns: the sampler discounts with the ALGORITHM's gamma
        gamma = next(f.default for f in fields(CalQL) if f.name == "gamma")
        return NStepEpisodicReplayBuffer(n_step=script.args.n_step, gamma=gamma, **kw).create()
    return EpisodicReplayBuffer(**kw).create()


def run() -> None:
    from oprl_amd.buffers.offline_dataset import fill_replay, load_dataset
    from oprl_amd.runners.train import set_seed
    from oprl_amd.trainers.offline_trainer import OfflineTrainer
    args = script.args
    if not args.dataset:
        raise ValueError("--dataset PATH is required (tools/make_offline_dataset.py writes one)")
    seed = args.start_seed
    set_seed(seed)
    data = load_dataset(args.dataset)
    buffer = make_replay_buffer(data)
    buffer.seed = seed
    norm = fill_replay(buffer, data, normalize=not args.no_normalize)
    logger = make_logger(seed)
    algo = make_algo(logger)
    algo.set_seed(seed)
    OfflineTrainer(logger=logger, make_env_test=make_env, replay_buffer=buffer, algo=algo, obs_norm=norm,
                   num_updates=args.updates, updates_per_call=args.updates_per_call, batch_size=args.batch,
                   eval_interval=config.eval_every * 2, stdout_log_every=config.log_every, seed=seed).train()
    if finetune_steps > 0:      # the same algorithm object goes on online, the dataset in every batch
        from oprl_amd.trainers.finetune import finetune
        finetune(algo=algo, prior_buffer=buffer, obs_norm=norm, make_env=make_env, logger=logger, num_steps=finetune_steps,
                 batch_size=args.batch, prior_share=args.prior_share, seed=seed, eval_interval=config.eval_every,
                 stdout_log_every=config.log_every)


if __name__ == "__main__":
    run()
