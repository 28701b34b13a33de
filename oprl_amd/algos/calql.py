"""Calibrated Q-learning on the MI355X-native learner (Nakamoto, Zhai, Singh, Mark, Ma, Finn, Kumar & Levine, "Cal-QL:
Calibrated Offline RL Pre-Training for Efficient Online Fine-Tuning", NeurIPS 2023): CQL whose penalty sees, at the
actions drawn from the policy, not the critic's value but

    max(Q_j(s_b, x), G_b)

with G_b the discounted return the dataset, or the running experience, achieved from the row's slot.  CQL's critics are
pessimistic far below any real return, so the first online batches of a fine-tuning run pull them up abruptly and the
policy unlearns; values that are never pushed below a return some policy really achieved do not have that cliff.  The
bound passes no gradient, the uniform actions are not bounded, and everything else — the TD target, the actor step, the
temperature step, Polyak — is CQL's, that is SAC's.

On the device it is the calibrated form of the CQL mode (``HipLearner.set_calql``; csrc/cql_seed.hip, DESIGN.md section
21).  The returns-to-go come out of the replay (``EpisodicReplayBuffer.returns_to_go``, csrc/replay_returns.hip):
``update_from_buffer`` reaches ``step_n``, which samples, computes them with this algorithm's ``gamma`` and updates;
``update`` takes them from the caller.  There is no bootstrap at a truncation, so for non-negative rewards the bound is an
underestimate (DESIGN.md section 21 says what that means for negative ones).  Refused like CQL: ``prioritized=True``,
``precision != "f32"``, ``export_grads``; a hindsight buffer has no stored returns and is refused by ``step_n``."""
from __future__ import annotations

from dataclasses import dataclass

import torch as t

from oprl_amd.algos.cql import CQL


@dataclass
class CalQL(CQL):
    def create(self) -> "CalQL":
        super().create()
        self.learner.set_calql(True)
        return self

    def update(
        self,
        state: t.Tensor,
        action: t.Tensor,
        reward: t.Tensor,
        done: t.Tensor,
        next_state: t.Tensor,
        *,
        returns: t.Tensor | None = None,
        noise: tuple[t.Tensor, t.Tensor] | None = None,
        weights: t.Tensor | None = None,
    ) -> None:
        """``returns``: the rows' returns-to-go [B] or [B, 1] (``buffer.returns_to_go(*slots)`` of
        ``buffer.sample(B, return_indices=True)``), required.  ``noise`` as in ``SAC.update``."""
        if returns is None:
            raise ValueError("CalQL.update needs returns=: the rows' returns-to-go (buffer.returns_to_go of the slots "
                             "sample(return_indices=True) gives); update_from_buffer computes them itself")
        if weights is not None:
            raise ValueError("CalQL.update(weights=): prioritized replay through Cal-QL is not built")
        n0, n1 = noise if noise is not None else (None, None)
        step = self.update_step
        self.learner.update_calql(state, action, reward, done, next_state, returns, noise0=n0, noise1=n1)
        self._log_update(step)

    def _log_update(self, step: int) -> None:
        super()._log_update(step)
        if step % self.log_every == 0:
            self.logger.log_scalar("algo/calql_bound_rate", self.learner.read_cql()["bound_rate"], step)
