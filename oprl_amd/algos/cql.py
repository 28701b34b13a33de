"""Conservative Q-learning on the MI355X-native learner (Kumar, Zhou, Tucker & Levine, "Conservative Q-Learning for
Offline Reinforcement Learning", NeurIPS 2020), the CQL(H) form with a fixed penalty weight: SAC whose critics also pay

    cql_alpha (1/B) sum_b [ logsumexp_x (Q_j(s_b, x) - logdensity(x)) - Q_j(s_b, a_b) ]

over 3 N sampled actions x per state — N uniform in [-1, 1]^A, N from pi(.|s_b), N from pi(.|s'_b), all evaluated at s_b —
so that values of actions the dataset does not hold are pushed down and the dataset's own are pushed up.  The TD target,
the actor step, the temperature step and Polyak are SAC's.  On the device it is a MODE of a SAC learner
(``HipLearner.set_cql``; csrc/cql_seed.hip): f32, the generic launch sequence (``no_fuse``), one
learner, no prioritized replay.  The critic step runs on ``batch_size (1 + 3 N)`` rows, which ``max_batch`` is sized for.
Not built: the Lagrange form of ``cql_alpha``, the max-target backup, the behaviour-cloning warm-up of the policy, a
deterministic-target variant."""
from __future__ import annotations

import math
from dataclasses import dataclass

from oprl_amd.algos.base_algorithm import check_mode_config
from oprl_amd.algos.sac import SAC

MAX_ACTIONS = 16       # kCqlMaxActions (csrc/cql_seed.h): 3 N <= 48 entries per row


@dataclass
class CQL(SAC):
    cql_alpha: float = 5.0         # the penalty's weight
    cql_n_actions: int = 10        # N: sampled actions per kind and state

    def __post_init__(self) -> None:
        check_config(self)

    def create(self) -> "CQL":
        check_config(self)
        self.no_fuse = True        # the mode exists on the generic launch sequence only
        self.max_batch = max(int(self.max_batch), wide_rows(self.batch_size, self.cql_n_actions))
        super().create()
        self.learner.set_cql(self.cql_alpha, self.cql_n_actions)
        return self

    def _log_update(self, step: int) -> None:
        super()._log_update(step)
        if step % self.log_every == 0:
            q = self.learner.read_cql()
            self.logger.log_scalar("algo/cql_penalty", q["penalty"], step)
            self.logger.log_scalar("algo/cql_q_rand", 0.5 * (q["q_rand1"] + q["q_rand2"]), step)
            self.logger.log_scalar("algo/cql_q_pi", 0.5 * (q["q_pi1"] + q["q_pi2"]), step)

    # (state_dict / load_state_dict: the mode has no state of its own)


def wide_rows(batch_size: int, n_actions: int) -> int:
    """Rows of the critic step: the minibatch's and 3 N sampled actions per state."""
    return int(batch_size) * (1 + 3 * int(n_actions))


def check_config(algo: CQL) -> None:
    """What the learner would refuse, said before anything touches the GPU."""
    check_mode_config(algo, "CQL", "the mode runs the generic launch sequence",
                      "no importance weights in the penalty; a fixed dataset is sampled uniformly")
    if getattr(algo, "layer_norm", False):
        raise ValueError(f"{type(algo).__name__}(layer_norm=True): the conservative penalty's wide critic step has no LayerNorm form")
    try:
        ca = float(algo.cql_alpha)
    except (TypeError, ValueError):
        ca = math.nan
    if not (math.isfinite(ca) and ca >= 0.0):
        raise ValueError(f"CQL: cql_alpha={algo.cql_alpha!r} is not a finite number >= 0")
    n = algo.cql_n_actions
    if isinstance(n, bool) or not isinstance(n, int) or not 1 <= n <= MAX_ACTIONS:
        raise ValueError(f"CQL: cql_n_actions={n!r} is not an integer in 1..{MAX_ACTIONS}")
    if int(algo.batch_size) < 1:
        raise ValueError(f"CQL: batch_size={algo.batch_size!r} < 1")
