"""TD3+BC on the MI355X learner — offline RL from a fixed dataset (Fujimoto & Gu 2021); its body is
configs/_common.py's ``OfflineScript``.  The dataset is an ``.npz`` with the D4RL key names (buffers/offline_dataset.py;
tools/make_offline_dataset.py writes one from a ``synthetic:`` environment — D4RL itself is not available to this
build).  ``--env`` names the environment the policy is evaluated on.  There is no environment in the training loop, so ``--num-envs > 1`` and
``--open-episodes`` are refused, and so is ``--per`` (a fixed dataset is sampled uniformly).

    python configs/td3_bc.py --dataset data.npz --env synthetic:walker-walk [--bc-alpha 2.5] [--updates N] [--batch 256]
                             [--no-normalize] [--n-step N] [--finetune-steps N [--prior-share 0.5]]

``--finetune-steps N``: after the offline updates the same learner goes on for N environment steps online, every batch
drawn partly from the dataset and partly from the fresh experience (trainers/finetune.py; not with ``--n-step > 1``).
"""
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent))
sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from _common import OfflineScript  # noqa: E402
from oprl.algos.td3_bc import TD3BC  # noqa: E402

FLAGS = (
    ("--bc-alpha", float, 2.5, "weight of the Q term against the behaviour-cloning term (the paper's alpha)"),
)


def alpha_of(args) -> dict:
    return dict(bc_alpha=args.bc_alpha, batch_size=args.batch)


script = OfflineScript(TD3BC, "TD3BC", extra_flags=FLAGS, algo_kwargs=alpha_of,
                       no_her="TD3+BC trains from a fixed dataset here")
# the names a reference-style script defines at module level
make_env, make_algo, make_logger, config = script.make_env, script.make_algo, script.make_logger, script.config
make_replay_buffer, run, finetune_steps = script.make_replay_buffer, script.run, script.finetune_steps

if __name__ == "__main__":
    run()
