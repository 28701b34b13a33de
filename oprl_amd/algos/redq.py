"""REDQ on the MI355X-native learner (Randomized Ensembled Double Q-learning, Chen et al., ICLR 2021): SAC's
tanh-Gaussian actor, an ensemble of N scalar critics, a TD target that takes the minimum over M target critics drawn
afresh for every update, and G critic updates per actor step (the update-to-data ratio).

One update u (the learner's update count before it) on a minibatch (s, a, r, d, s'), csrc/learner_generic.hip:
  1. I_u = M distinct critics, drawn on the host (oprl_redq_subset: Philox stream 3, counter u, partial Fisher-Yates);
  2. a', log pi' = pi(s'); y = r + gamma (1 - d) (min_{i in I_u} Qbar_i(s', a') - alpha log pi');
  3. one Adam step over the whole critic arena on sum_i mean_b (Q_i(s, a) - y)^2, then Polyak on all N targets;
  4. only when (u + 1) % G == 0: the actor step on alpha log pi - (1/N) sum_i Q_i(s, pi(s)) and the temperature step.

The actor sees the critics as updated in step 3 of the same update (critic phase, then actor phase, as this project's
SAC does).  The REDQ authors' code takes the policy loss on the critics before their Adam step; DESIGN.md ("REDQ")
records the difference.  F32 only, no gradient export, no fused launch form."""
from __future__ import annotations

import math
from dataclasses import dataclass, field

import torch as t
from torch import nn

from oprl_amd import _capi
from oprl_amd.algos.base_algorithm import HipLearner, OffPolicyAlgorithm, Temperature, check_layer_norm_config, check_prioritized_config, require_gpu
from oprl_amd.algos.nn_functions import make_target_
from oprl_amd.algos.nn_models import MLP, CriticLayerNorm, GaussianActor, _forward_sa, _forward_sa_ln, attach_layer_norm, flatten_module_
from oprl_amd.algos.protocols import PolicyProtocol
from oprl_amd.logging import LoggerProtocol


class EnsembleCritic(nn.Module):
    """N scalar critics MLP(S + A -> 256 -> 256 -> 1), registered as ``qf0`` ... ``qf{N-1}``; forward -> [B, N]."""

    def __init__(self, state_dim: int, action_dim: int, n_nets: int, hidden_units: tuple[int, ...] = (256, 256)) -> None:
        super().__init__()
        self.n_nets = n_nets
        self.nets = []
        for i in range(n_nets):
            net = MLP(state_dim + action_dim, 1, hidden_units, nn.ReLU(inplace=True))
            self.add_module(f"qf{i}", net)
            self.nets.append(net)

    def forward(self, state: t.Tensor, action: t.Tensor) -> t.Tensor:
        ln = self.__dict__.get("_ln")
        if ln is not None:
            return t.cat(tuple(_forward_sa_ln(net, state, action, ln, i) for i, net in enumerate(self.nets)), dim=1)
        return t.cat(tuple(_forward_sa(net, state, action) for net in self.nets), dim=1)


@dataclass
class REDQ(Temperature, OffPolicyAlgorithm):
    logger: LoggerProtocol
    state_dim: int
    action_dim: int
    batch_size: int = 256
    n_critics: int = 10           # N (at most 10: OPRL_MAX_CRITICS)
    n_min: int = 2                # M target critics in the minimum
    utd_ratio: int = 20           # G critic updates per actor step; update_from_buffer runs G updates per call
    tune_alpha: bool = True
    gamma: float = 0.99
    lr_actor: float = 3e-4
    lr_critic: float = 3e-4
    lr_alpha: float = 3e-4
    alpha_init: float = 1.0
    target_update_coef: float = 5e-3
    device: str = "cuda"
    log_every: int = 5000
    max_batch: int = 4096
    export_grads: bool = False    # refused by the learner (no data-parallel REDQ)
    no_fuse: bool = False         # (REDQ has no fused form: no effect)
    prioritized: bool = False      # train from a PrioritizedEpisodicReplayBuffer: importance-weighted critic loss, |TD| back as priorities (generic launch sequence, f32)
    precision: str = "f32"        # f32 only: the learner refuses the others
    dropout: float = 0.0          # Linear -> Dropout -> LayerNorm -> ReLU (DroQ): the rate in [0, 1), needs layer_norm=True
    layer_norm: bool = False      # Linear -> LayerNorm -> ReLU in the critics' hidden layers (RLPD / DroQ)

    actor: PolicyProtocol = field(init=False)
    critic: EnsembleCritic = field(init=False)
    critic_target: EnsembleCritic = field(init=False)
    learner: HipLearner = field(init=False, repr=False)
    _created: bool = False

    def create(self) -> "REDQ":
        check_prioritized_config(self)
        check_layer_norm_config(self)
        dev = require_gpu(self.device)
        if not 1 <= self.n_critics <= _capi.OPRL_MAX_CRITICS:
            raise ValueError(f"REDQ: n_critics={self.n_critics} outside [1, {_capi.OPRL_MAX_CRITICS}]")
        self.actor = GaussianActor(self.state_dim, self.action_dim, (256, 256),
                                   nn.ReLU(inplace=True), device=self.device).to(dev)

        def critic():
            return EnsembleCritic(self.state_dim, self.action_dim, self.n_critics).to(dev)

        self.critic, self.critic_target = critic(), critic().eval()
        for m in (self.actor, self.critic, self.critic_target):
            flatten_module_(m)
        make_target_(self.critic_target, self.critic)
        self.target_entropy = -float(self.action_dim)
        self.log_alpha = None
        if self.tune_alpha:
            self.log_alpha = t.tensor(math.log(self.alpha_init), dtype=t.float64, device=dev)
        hp = dict(gamma=self.gamma, tau=self.target_update_coef, lr_actor=self.lr_actor,
                  lr_critic=self.lr_critic, lr_alpha=self.lr_alpha, beta1=0.9, beta2=0.999,
                  adam_eps=1e-8, alpha_init=self.alpha_init, tune_alpha=int(self.tune_alpha),
                  target_entropy=self.target_entropy, policy_freq=int(self.utd_ratio), n_min=int(self.n_min))
        self.learner = HipLearner(
            "redq", self.state_dim, self.action_dim, dev,
            actor_group=self.actor, actor_mlp=self.actor.net, actor_target_mlp=None,
            critic_group=self.critic, critic_mlps=self.critic.nets,
            critic_target_group=self.critic_target, critic_target_mlps=self.critic_target.nets,
            hp=hp, max_batch=self.max_batch, export_grads=self.export_grads, log_alpha=self.log_alpha,
            no_fuse=self.no_fuse or self.prioritized or self.layer_norm, precision=self.precision)
        if self.layer_norm:
            self.critic_ln = CriticLayerNorm(self.n_critics).to(dev).make_state()
            attach_layer_norm(self.critic, self.critic_ln, False)
            attach_layer_norm(self.critic_target, self.critic_ln, True)
            self.learner.set_layernorm(self.critic_ln)
            if self.dropout > 0.0:
                self.learner.set_dropout(self.dropout)
        self._created = True
        return self

    @property
    def updates_per_request(self) -> int:
        """``update_from_buffer`` runs ``utd_ratio`` updates per update asked of it, K = ``n_updates x utd_ratio`` in
        all: one ``step_n(K)`` call; with ``act_next`` the actor's forward rides behind the last (``step_n(K - 1)`` +
        ``step_act``, the same updates bit for bit), a 2-D ``act_next`` [N, S] as rows behind all K (``step_act_rows``)."""
        return int(self.utd_ratio)

    def update(
        self,
        state: t.Tensor,
        action: t.Tensor,
        reward: t.Tensor,
        done: t.Tensor,
        next_state: t.Tensor,
        *,
        noise: tuple[t.Tensor, t.Tensor] | None = None,
        weights: t.Tensor | None = None,
    ) -> None:
        """ONE update (a critic step; an actor step too when it completes a group of ``utd_ratio``).  ``noise``:
        optional (eps_next [B,A], eps_current [B,A]) standing in for the device draws of streams 1 and 2.
        ``weights``: importance weights [B] or [B, 1] of a prioritized batch (critic loss only); the rows' |TD|, the
        mean over the ensemble, is left in ``last_td_abs`` (device tensor)."""
        n0, n1 = noise if noise is not None else (None, None)
        self._dispatch_update(state, action, reward, done, next_state, weights, n0, n1)

    def _log_update(self, step: int) -> None:
        if step % self.log_every == 0:
            sc = self.learner.read_scalars()
            self.logger.log_scalars({
                "algo/q1": sc["q1_mean"], "algo/q_target": sc["q_target_mean"],
                "algo/abs_q_err": sc["q1_mean"] - sc["q_target_mean"],
                "algo/critic_loss": sc["critic_loss"],
            }, step)
            if self.tune_alpha:
                self.logger.log_scalar("algo/loss_alpha", sc["alpha_loss"], step)
            self.logger.log_scalars({
                "algo/loss_actor": sc["gauss_actor_loss"], "algo/alpha": sc["alpha"],
                "algo/log_pi": sc["log_pi_mean"],
            }, step)
