"""Implicit Q-learning on the MI355X-native learner (Kostrikov, Nair & Levine, "Offline Reinforcement Learning with
Implicit Q-Learning", 2021), in its deterministic-policy form: twin critics with targets, a tanh actor and a value net
V(s).  With qt = min_j Qtarget_j(s, a) on the dataset's own action and u = qt - V(s), one update takes

    V:       an Adam step on (1/B) sum_b omega_b u_b^2, omega_b = 1 - expectile where u_b < 0, else expectile;
    critics: TD3's step with the target y = r + (1 - d) gamma V(s')  (V as it was before its step);
    actor:   an Adam step on (1/B) sum_b w_b sum_k (pi(s_b)_k - a_bk)^2, w_b = min(exp(beta u_b), adv_clip) a constant;
    Polyak on the critic targets, every update.

No action outside the dataset is ever evaluated: no target actor, no smoothing noise, no critic on (s, pi).  On the device
it is a MODE of a TD3 learner (``HipLearner.set_iql``; csrc/iql_seed.hip): f32, the generic launch
sequence (``no_fuse``), ``policy_freq = 1``, one learner, no prioritized replay.  Not built: the Gaussian policy, the
cosine learning-rate schedule of the actor, dropout, online fine-tuning."""
from __future__ import annotations

import math
from dataclasses import dataclass, field

from torch import nn

from oprl_amd.algos.base_algorithm import check_mode_config
from oprl_amd.algos.nn_models import MLP, flatten_module_
from oprl_amd.algos.td3 import TD3


@dataclass
class IQL(TD3):
    policy_freq: int = 1           # the actor step and the critics' Polyak step on every update
    expectile: float = 0.7         # tau of the value net's asymmetric squared loss
    beta: float = 3.0              # inverse temperature of the advantage weights
    adv_clip: float = 100.0        # the weights' clip
    lr_value: float = 3e-4

    value: nn.Module = field(init=False)

    def __post_init__(self) -> None:
        check_config(self)

    def create(self) -> "IQL":
        check_config(self)
        self.no_fuse = True        # the mode exists on the generic launch sequence only
        super().create()
        dev = self.learner.device
        self.value = MLP(self.state_dim, 1, (256, 256), nn.ReLU(inplace=True)).to(dev)
        flatten_module_(self.value)
        self.learner.set_iql(self.value, self.expectile, self.beta, self.adv_clip, self.lr_value)
        return self

    def _log_update(self, step: int) -> None:
        super()._log_update(step)
        if step % self.log_every == 0:
            q = self.learner.read_iql()
            self.logger.log_scalar("algo/iql_v_loss", q["v_loss"], step)
            self.logger.log_scalar("algo/iql_adv_mean", q["adv_mean"], step)
            self.logger.log_scalar("algo/iql_w_mean", q["w_mean"], step)
            self.logger.log_scalar("algo/iql_clip_frac", q["clip_frac"], step)

    # (state_dict / load_state_dict: HipLearner's carry V's arena, both moments and V's step count while the mode is on)


def check_config(algo: IQL) -> None:
    """What the learner would refuse, said before anything touches the GPU."""
    check_mode_config(algo, "IQL", "the mode runs the generic launch sequence",
                      "no importance weights in the value and actor steps; a fixed dataset is sampled uniformly")
    if int(algo.policy_freq) != 1:
        raise ValueError(f"IQL: policy_freq={algo.policy_freq!r}; the actor steps on every update (policy_freq=1)")
    tau, beta, clip, lr = (float(x) for x in (algo.expectile, algo.beta, algo.adv_clip, algo.lr_value))
    if not (math.isfinite(tau) and 0.0 < tau < 1.0):
        raise ValueError(f"IQL: expectile={algo.expectile!r} is not a number inside (0, 1)")
    if not (math.isfinite(beta) and beta >= 0.0):
        raise ValueError(f"IQL: beta={algo.beta!r} is not a finite number >= 0")
    if not (math.isfinite(clip) and clip > 0.0):
        raise ValueError(f"IQL: adv_clip={algo.adv_clip!r} is not a finite number above 0")
    if not (math.isfinite(lr) and lr > 0.0):
        raise ValueError(f"IQL: lr_value={algo.lr_value!r} is not a finite number above 0")
