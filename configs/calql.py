"""Cal-QL on the MI355X learner — offline RL from a fixed dataset that is meant to be fine-tuned online (Nakamoto et al. 2023:
CQL whose penalty bounds the critics' values at the policy's actions below by the dataset's returns-to-go; DESIGN.md section
21); its body is configs/_common.py's ``OfflineScript``, its flags are configs/cql.py's (restated here: a script cannot be
imported without running it).  The dataset is an ``.npz`` with the D4RL key names (buffers/offline_dataset.py;
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
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent))
sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from _common import OfflineScript  # noqa: E402
from oprl.algos.calql import CalQL  # noqa: E402

FLAGS = (
    ("--cql-alpha", float, 5.0, "weight of the conservative penalty, >= 0"),
    ("--cql-actions", int, 10, "sampled actions per kind and state (uniform, pi(.|s), pi(.|s')), 1 .. 16"),
    ("--tune-alpha", bool, False, "learn SAC's temperature instead of keeping alpha_init"),
)


def hparams_of(args) -> dict:
    return dict(cql_alpha=args.cql_alpha, cql_n_actions=args.cql_actions, tune_alpha=args.tune_alpha, batch_size=args.batch)


script = OfflineScript(CalQL, "CalQL", extra_flags=FLAGS, algo_kwargs=hparams_of, title="Cal-QL",
                       no_per="a fixed dataset is sampled uniformly, and the penalty takes no importance weights",
                       no_her="Cal-QL bounds its critics by the stored returns-to-go, and a hindsight replay relabels its "
                              "rewards per sample")
# the names a reference-style script defines at module level
make_env, make_algo, make_logger, config = script.make_env, script.make_algo, script.make_logger, script.config
make_replay_buffer, run, finetune_steps = script.make_replay_buffer, script.run, script.finetune_steps

if __name__ == "__main__":
    run()
