"""IQL on the MI355X learner — offline RL from a fixed dataset (Kostrikov et al. 2021, the deterministic-policy form);
its body is configs/_common.py's ``OfflineScript``.  The dataset is an ``.npz`` with the D4RL key names (buffers/offline_dataset.py;
tools/make_offline_dataset.py writes one from a ``synthetic:`` environment — D4RL itself is not available to this build).
``--env`` names the environment the policy is evaluated on.  There is no environment in the training loop, so
``--num-envs > 1`` and ``--open-episodes`` are refused, and so is ``--per`` (a fixed dataset is sampled uniformly).

    python configs/iql.py --dataset data.npz --env synthetic:walker-walk [--expectile 0.7] [--beta 3.0] [--adv-clip 100]
                          [--updates N] [--batch 256] [--no-normalize] [--n-step N]
                          [--finetune-steps N [--prior-share 0.5]]

``--finetune-steps N``: after the offline updates the same learner goes on for N environment steps online, every batch
drawn partly from the dataset and partly from the fresh experience (trainers/finetune.py; not with ``--n-step > 1``).
"""
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent))
sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from _common import OfflineScript  # noqa: E402
from oprl.algos.iql import IQL  # noqa: E402

FLAGS = (
    ("--expectile", float, 0.7, "tau of the value net's expectile loss, inside (0, 1)"),
    ("--beta", float, 3.0, "inverse temperature of the advantage weights exp(beta (Q - V))"),
    ("--adv-clip", float, 100.0, "clip of the advantage weights"),
)


def hparams_of(args) -> dict:
    return dict(expectile=args.expectile, beta=args.beta, adv_clip=args.adv_clip, batch_size=args.batch)


script = OfflineScript(IQL, "IQL", extra_flags=FLAGS, algo_kwargs=hparams_of)
# the names a reference-style script defines at module level
make_env, make_algo, make_logger, config = script.make_env, script.make_algo, script.make_logger, script.config
make_replay_buffer, run, finetune_steps = script.make_replay_buffer, script.run, script.finetune_steps

if __name__ == "__main__":
    run()
