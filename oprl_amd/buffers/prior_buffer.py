"""Prior data in every batch: an online replay whose batches come partly from a fixed dataset.

``prior`` is a second ``EpisodicReplayBuffer`` — the dataset, written once by ``buffers/offline_dataset.py fill_replay``
— and ``prior_share`` the share of every batch that comes from it.  Of a batch of B rows the first

    n_prior(B) = min(B, max(0, floor(prior_share * B + 0.5)))

are drawn from ``prior`` and the rest from this buffer, each exactly as ``EpisodicReplayBuffer.sample`` draws row i of a
batch of B from that source at the same (seed, counter).  The split is deterministic (Ball et al. 2023, "symmetric
sampling" at 0.5).  Two uses: fine-tuning a policy that ``configs/iql.py`` / ``td3_bc.py`` / ``cql.py`` pre-trained
(trainers/finetune.py), and online training from scratch with a dataset in every batch (``--prior-data``).

Environment steps are written into this buffer only; ``len()`` is its own count, which is what the trainers gate on.
Every learner trains on these rows unchanged.  The gather is one HIP kernel (``oprl_replay_sample_mix``,
csrc/replay_mix.hip); the mode is host state on the C handle (``oprl_replay_set_prior``), which is also how
``learner.step_n(buffer.handle, ...)`` finds it.  The two buffers share state and action dims; their episode slots and
steps per episode are their own.

Not combined with n-step returns, hindsight goals or prioritized replay on either side.  On ``device='cpu'`` this is a
host container like its base: ``sample`` raises."""
from __future__ import annotations

import math
from dataclasses import dataclass, field

import numpy.typing as npt
import torch as t

from oprl_amd import _capi
from oprl_amd.buffers.episodic_buffer import EpisodicReplayBuffer


def n_prior_rows(batch_size: int, share: float) -> int:
    """The prior rows of a batch (csrc/replay_mix.hip prior_rows: the same double arithmetic)."""
    B = int(batch_size)
    return min(B, max(0, int(math.floor(float(share) * B + 0.5))))


def _mode_of(buf) -> str | None:
    """What keeps a buffer from being one side of a mixed batch (None: it is plain)."""
    from oprl_amd.buffers.hindsight_buffer import HindsightEpisodicReplayBuffer
    from oprl_amd.buffers.nstep_buffer import NStepEpisodicReplayBuffer
    from oprl_amd.buffers.prioritized_buffer import PrioritizedEpisodicReplayBuffer
    for cls, what in ((NStepEpisodicReplayBuffer, "samples n-step returns"),
                      (HindsightEpisodicReplayBuffer, "relabels goals in hindsight"),
                      (PrioritizedEpisodicReplayBuffer, "is prioritized"),
                      (PriorDataReplayBuffer, "has a prior of its own")):
        if isinstance(buf, cls):
            return what
    return None


@dataclass
class PriorDataReplayBuffer(EpisodicReplayBuffer):
    prior: EpisodicReplayBuffer | None = field(default=None, repr=False, compare=False)
    prior_share: float = 0.5

    def _validate(self) -> None:
        share = self.prior_share
        if isinstance(share, bool) or not isinstance(share, (int, float)) or not 0 <= share <= 1:      # (nan fails)
            raise ValueError(f"prior_share={share!r}: must lie in [0, 1]")
        p = self.prior
        if p is None:
            return
        if p is self:
            raise ValueError("prior: a buffer cannot be the prior of itself")
        if not isinstance(p, EpisodicReplayBuffer):
            raise ValueError(f"prior: an EpisodicReplayBuffer expected, got {type(p).__name__}")
        what = _mode_of(p)
        if what is not None:
            raise ValueError(f"prior: the {type(p).__name__} {what}; the prior of a mixed batch is a plain "
                             "EpisodicReplayBuffer")
        if (p.state_dim, p.action_dim) != (self.state_dim, self.action_dim):
            raise ValueError(f"prior: its dims ({p.state_dim}, {p.action_dim}) are not this buffer's "
                             f"({self.state_dim}, {self.action_dim})")
        p.check_created()
        if t.device(p.device).type != t.device(self.device).type:
            raise ValueError(f"prior: it lives on {p.device!r}, this buffer on {self.device!r}")

    def create(self) -> "PriorDataReplayBuffer":
        self._validate()          # before the GPU is touched
        super().create()
        self._set_prior()
        return self

    def _set_prior(self) -> None:
        if self._handle is not None:
            p = self.prior._handle if self.prior is not None else None
            _capi.check(self._lib.oprl_replay_set_prior(self._handle, p, float(self.prior_share)),
                        "oprl_replay_set_prior")

    def n_prior(self, batch_size: int) -> int:
        """How many of ``batch_size`` rows come from the prior: rows ``[0, n_prior)`` of every batch."""
        return n_prior_rows(batch_size, self.prior_share) if self.prior is not None else 0

    def _refuse_empty(self, batch_size: int) -> None:
        n = self.n_prior(batch_size)
        if n < batch_size and self._number_transitions <= 0:
            raise ValueError("cannot sample from an empty replay buffer")
        if n > 0 and len(self.prior) <= 0:
            raise ValueError("cannot sample from an empty prior buffer: fill_replay(prior, load_dataset(path)) first")

    @property
    def handle(self):
        """C handle with the episode tables of both buffers up to date (for step_n)."""
        if self.prior is not None:
            self.prior.handle       # (the property syncs the prior's table)
        return super().handle

    def _sync_sources(self) -> None:
        """``returns_to_go``: rows ``[0, n_prior(len(episodes)))`` are slots of the prior (the split is by row index)."""
        if self.prior is not None and self._handle is not None:
            self.prior._sync_lens()
        super()._sync_sources()

    def sample(self, batch_size: int, inds: t.Tensor | npt.NDArray | None = None, return_indices: bool = False,
               return_source: bool = False):
        """``(state, action, reward, done, next_state)``, rows ``[0, n_prior(batch_size))`` from the prior and the rest
        from this buffer.  ``inds[i]`` is a flat index into row i's own source and ``return_indices`` gives the slot
        inside it; ``return_source`` appends int32[B]: 1 for a prior row, 0 for an own row."""
        if self.prior is None:
            rows, pair, _ = self._sample("oprl_replay_sample", batch_size, inds, return_indices)
            src = t.zeros(int(batch_size), dtype=t.int32, device=rows[0].device) if return_source else None
        else:
            if self._handle is not None:
                self.prior._sync_lens()
            rows, pair, src = self._sample("oprl_replay_sample_mix", batch_size, inds, return_indices, bool(return_source))
        out = [x for x in (rows, pair, src) if x is not None]
        return out[0] if len(out) == 1 else tuple(out)

    def state_dict(self) -> dict:
        """The base class's, and the share; the dataset is not stored (it is reloaded from its file)."""
        sd = super().state_dict()
        sd["prior_share"] = float(self.prior_share)
        return sd

    def load_state_dict(self, sd: dict) -> None:
        super().load_state_dict(sd)
        self.prior_share = float(sd.get("prior_share", self.prior_share))
        self._validate()
        self._set_prior()          # the mode is host state on the handle
