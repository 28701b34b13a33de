"""CQL on the MI355X learner — offline RL from a fixed dataset (Kumar et al. 2020, CQL(H) with a fixed penalty weight on a
SAC learner); its body is configs/_common.py's ``OfflineScript``.  The dataset is an ``.npz`` with the D4RL key names (buffers/offline_dataset.py;
tools/make_offline_dataset.py writes one from a ``synthetic:`` environment — D4RL itself is not available to this build).
``--env`` names the environment the policy is evaluated on.  There is no environment in the training loop, so
``--num-envs > 1`` and ``--open-episodes`` are refused, and so is ``--per`` (a fixed dataset is sampled uniformly).

    python configs/cql.py --dataset data.npz --env synthetic:walker-walk [--cql-alpha 5.0] [--cql-actions 10] [--tune-alpha]
                          [--updates N] [--batch 256] [--updates-per-call K] [--no-normalize] [--n-step N]
                          [--finetune-steps N [--prior-share 0.5]]

``--finetune-steps N``: after the offline updates the same learner goes on for N environment steps online, every batch
drawn partly from the dataset and partly from the fresh experience (trainers/finetune.py; not with ``--n-step > 1``).
"""
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent))
sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from _common import OfflineScript  # noqa: E402
from oprl.algos.cql import CQL  # noqa: E402

FLAGS = (
    ("--cql-alpha", float, 5.0, "weight of the conservative penalty, >= 0"),
    ("--cql-actions", int, 10, "sampled actions per kind and state (uniform, pi(.|s), pi(.|s')), 1 .. 16"),
    ("--tune-alpha", bool, False, "learn SAC's temperature instead of keeping alpha_init"),
)


def hparams_of(args) -> dict:
    return dict(cql_alpha=args.cql_alpha, cql_n_actions=args.cql_actions, tune_alpha=args.tune_alpha, batch_size=args.batch)


script = OfflineScript(CQL, "CQL", extra_flags=FLAGS, algo_kwargs=hparams_of)
# the names a reference-style script defines at module level
make_env, make_algo, make_logger, config = script.make_env, script.make_algo, script.make_logger, script.config
make_replay_buffer, run, finetune_steps = script.make_replay_buffer, script.run, script.finetune_steps

if __name__ == "__main__":
    run()
