"""DDPG on the MI355X-native learner.

Same dataclass fields, ``create()`` / ``update()`` contract and attributes as
the reference (/root/reference/src/oprl/algos/ddpg.py:16-107); ``update()`` is
one call into liboprl_amd.so — no host sync — instead of autograd + two torch Adam steps + 12 Polyak
tensor ops: ONE launch for the whole update in every arithmetic mode (k_ddpg_chain — through
``learner.step_n`` up to 32 updates per launch)."""
from __future__ import annotations

from dataclasses import dataclass, field

import torch as t
from torch import nn

from oprl_amd.algos.base_algorithm import HipLearner, OffPolicyAlgorithm, check_prioritized_config, require_gpu
from oprl_amd.algos.nn_functions import make_target_
from oprl_amd.algos.nn_models import Critic, DeterministicPolicy, flatten_module_
from oprl_amd.algos.protocols import PolicyProtocol
from oprl_amd.logging import LoggerProtocol


@dataclass
class DDPG(OffPolicyAlgorithm):
    logger: LoggerProtocol
    state_dim: int
    action_dim: int
    expl_noise: float = 0.1
    gamma: float = 0.99
    lr_actor: float = 3e-4
    lr_critic: float = 3e-4
    tau: float = 5e-3
    batch_size: int = 256          # unused, as in the reference (ddpg.py:26)
    max_action: float = 1.
    device: str = "cuda"
    max_batch: int = 4096          # rows the HIP workspace is sized for
    export_grads: bool = False     # data-parallel learner: reduce grads between phases
    no_fuse: bool = False          # force the generic per-net launch sequence (tests / A-B)
    prioritized: bool = False      # train from a PrioritizedEpisodicReplayBuffer: importance-weighted critic loss, |TD| back as priorities (generic launch sequence, f32)
    precision: str = "f32"        # "f32": exact-fp32 MFMA (parity mode, no input range); "x2": fp32 as fp16 hi + lo (parity mode, |obs| < 4094: leaving the range raises); "bf16": bf16 MFMA inputs, fp32 accumulate / master / Adam (include/oprl_amd.h)

    actor: PolicyProtocol = field(init=False)
    actor_target: PolicyProtocol = field(init=False)
    critic: nn.Module = field(init=False)
    critic_target: nn.Module = field(init=False)
    learner: HipLearner = field(init=False, repr=False)
    _created: bool = False

    def create(self) -> "DDPG":
        check_prioritized_config(self)
        dev = require_gpu(self.device)

        def policy():
            return DeterministicPolicy(
                state_dim=self.state_dim, action_dim=self.action_dim, hidden_units=(256, 256),
                hidden_activation=nn.ReLU(inplace=True), expl_noise=self.expl_noise,
                max_action=self.max_action, device=self.device).to(dev)

        self.actor = policy()
        self.actor_target = policy()
        self.critic = Critic(self.state_dim, self.action_dim).to(dev)
        self.critic_target = Critic(self.state_dim, self.action_dim).to(dev)
        for m in (self.actor, self.actor_target, self.critic, self.critic_target):
            flatten_module_(m)
        make_target_(self.actor_target, self.actor)
        make_target_(self.critic_target, self.critic)
        hp = dict(gamma=self.gamma, tau=self.tau, lr_actor=self.lr_actor, lr_critic=self.lr_critic,
                  beta1=0.9, beta2=0.999, adam_eps=1e-8, max_action=self.max_action, policy_freq=1)
        self.learner = HipLearner(
            "ddpg", self.state_dim, self.action_dim, dev,
            actor_group=self.actor, actor_mlp=self.actor.mlp, actor_target_mlp=self.actor_target.mlp,
            actor_target_group=self.actor_target,
            critic_group=self.critic, critic_mlps=[self.critic.q1],
            critic_target_group=self.critic_target, critic_target_mlps=[self.critic_target.q1],
            hp=hp, max_batch=self.max_batch, export_grads=self.export_grads, no_fuse=self.no_fuse or self.prioritized, precision=self.precision)
        self._created = True
        return self

    def update(
        self,
        state: t.Tensor,
        action: t.Tensor,
        reward: t.Tensor,
        done: t.Tensor,
        next_state: t.Tensor,
        weights: t.Tensor | None = None,
    ) -> None:
        """``weights``: importance weights [B] or [B, 1] of a prioritized batch; the rows' |TD| is left in
        ``last_td_abs`` (device tensor)."""
        if weights is not None:
            self.last_td_abs = self.learner.update_weighted(state, action, reward, done, next_state, weights)
            return
        self.learner.update(state, action, reward, done, next_state)
