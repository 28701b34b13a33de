"""D4PG on the MI355X learner — DDPG with a categorical critic (Barth-Maron et al. 2018); its body is configs/_common.py's ``TrainingScript``.
Defaults: 41 atoms from -150 to 150.  ``--n-step 3`` gives the paper's multi-step targets, ``--num-envs N`` its many
actors (``--open-episodes``: one open replay episode per environment); ``--per`` is refused.

    python configs/d4pg.py --env walker-walk --device cuda [--atoms 41 --v-min -150 --v-max 150] [--n-step 3] [--seeds N]
"""
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent))
sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from _common import TrainingScript  # noqa: E402
from oprl.algos.d4pg import D4PG  # noqa: E402

FLAGS = (
    ("--atoms", int, 41, "atoms of the categorical critic (2..48)"),
    ("--v-min", float, -150.0, "the first atom: the smallest discounted return the critic represents"),
    ("--v-max", float, 150.0, "the last atom"),
)


def atoms_of(args) -> dict:
    return dict(n_atoms=args.atoms, v_min=args.v_min, v_max=args.v_max)


# (estimate_q_every = 0: the trainer's Q probe reads a critic's first output, which here is a logit)
script = TrainingScript(D4PG, "D4PG", estimate_q_every=0, log_every=2500, extra_flags=FLAGS, algo_kwargs=atoms_of,
                        takes_per=False)
# the names a reference-style script defines at module level
make_env, make_algo, make_replay_buffer, make_logger, config = (
    script.make_env, script.make_algo, script.make_replay_buffer, script.make_logger, script.config)

if __name__ == "__main__":
    script.run()
