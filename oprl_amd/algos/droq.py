"""DroQ on the MI355X-native learner (Dropout Q-functions, Hiraoka et al., ICLR 2022): REDQ (algos/redq.py) with two
critics instead of ten, both in the target's minimum, whose hidden blocks are Linear -> Dropout -> LayerNorm -> ReLU, at
REDQ's update-to-data ratio.  The dropout runs in every pass that evaluates a critic — the target critics on (s', a'), the
critic step on (s, a), the actor phase's critics on (s, pi(s)) — inside the LN slice kernels, from Philox masks addressed by
(update count, pass, critic, batch row, layer, column): DESIGN.md section 26.  Nothing else differs from REDQ; the critic
modules' torch ``forward`` stays the inference form, without dropout."""
from __future__ import annotations

from dataclasses import dataclass

from oprl_amd.algos.redq import REDQ


@dataclass
class DroQ(REDQ):
    n_critics: int = 2
    n_min: int = 2
    utd_ratio: int = 20
    dropout: float = 0.01
    layer_norm: bool = True
