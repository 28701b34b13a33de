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

import numpy as np
import torch as t
from torch import nn

from oprl_amd import _capi
from oprl_amd.algos.base_algorithm import (HipLearner, OffPolicyAlgorithm, check_nstep_gamma, check_prioritized_config,
                                            refuse_prioritized, require_gpu, step_prioritized, trains_prioritized)
from oprl_amd.algos.nn_functions import disable_gradient
from oprl_amd.algos.nn_models import MLP, GaussianActor, _forward_sa, flatten_module_
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
        return t.cat(tuple(_forward_sa(net, state, action) for net in self.nets), dim=1)


@dataclass
class REDQ(OffPolicyAlgorithm):
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

    actor: PolicyProtocol = field(init=False)
    critic: EnsembleCritic = field(init=False)
    critic_target: EnsembleCritic = field(init=False)
    learner: HipLearner = field(init=False, repr=False)
    _created: bool = False

    def create(self) -> "REDQ":
        check_prioritized_config(self)
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
        self.critic_target._oprl_arena.copy_(self.critic._oprl_arena)
        for m in self.critic_target.modules():
            if hasattr(m, "mark_dirty"):
                m.mark_dirty()
        disable_gradient(self.critic_target)
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
            no_fuse=self.no_fuse or self.prioritized, precision=self.precision)
        self._created = True
        return self

    @property
    def alpha(self) -> float:
        if self.log_alpha is not None:
            return float(self.log_alpha.exp().item())
        return self.alpha_init

    @property
    def update_step(self) -> int:
        return self.learner.update_count if self._created else 0

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
        step = self.update_step
        if weights is not None:
            self.last_td_abs = self.learner.update_weighted(state, action, reward, done, next_state, weights, noise0=n0, noise1=n1)
        else:
            self.learner.update(state, action, reward, done, next_state, noise0=n0, noise1=n1)
        self._log_update(step)

    def update_from_buffer(self, replay_buffer, batch_size: int, act_next=None, n_updates: int = 1) -> None:
        """``utd_ratio`` times ``update(*replay_buffer.sample(batch_size))`` as one ``step_n(K=utd_ratio)`` call.
        ``act_next``: the actor's forward of it rides behind the last update (``step_n(K - 1)`` + ``step_act``, the
        same updates bit for bit).  ``n_updates``: that many environment steps' worth, K = ``n_updates x utd_ratio``;
        a 2-D ``act_next`` [N, S] rides as rows behind all K (one ``step_act_rows`` call)."""
        refuse_prioritized(self, replay_buffer)
        check_nstep_gamma(self, replay_buffer)
        if int(n_updates) < 1:
            raise ValueError(f"n_updates={n_updates!r}: at least one update")
        K = int(n_updates) * int(self.utd_ratio)
        if trains_prioritized(self, replay_buffer):      # (one step_n_prio call; act_next rides nowhere)
            step = self.update_step
            step_prioritized(self, replay_buffer, K, batch_size)
            for u in range(step, step + K):
                if u % self.log_every == 0:
                    self._log_update(u)
                    break
            return
        handle = getattr(replay_buffer, "handle", None)
        if handle is None:
            for _ in range(K):
                self.update(*replay_buffer.sample(batch_size))
            return
        step = self.update_step
        seed = int(getattr(replay_buffer, "seed", 0))
        mlp = self._actor_mlp() if act_next is not None else None
        if mlp is not None and np.ndim(act_next) == 2:
            self.learner.step_act_rows(handle, K, int(batch_size), seed, act_next)
            mlp.set_pending_rows(act_next, self.learner)
        elif mlp is not None:
            if K > 1:
                self.learner.step_n(handle, K - 1, int(batch_size), seed=seed)
            self.learner.step_act(handle, int(batch_size), seed, act_next)
            mlp.set_pending(act_next, self.learner)
        else:
            self.learner.step_n(handle, K, int(batch_size), seed=seed)
        for u in range(step, step + K):
            if u % self.log_every == 0:
                self._log_update(u)
                break

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
