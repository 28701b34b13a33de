"""D4PG on the MI355X-native learner (Barth-Maron et al., ICLR 2018): DDPG's deterministic tanh actor with ONE
categorical critic (Bellemare et al., ICML 2017) whose ``n_atoms`` outputs are logits over the fixed atoms
``z_i = v_min + i (v_max - v_min) / (n_atoms - 1)``.  Multi-step targets come from an n-step replay buffer
(buffers/nstep_buffer.py), many actors from ``--num-envs`` or configs/distrib_ddpg.py's layout.

One update on a minibatch (s, a, r, d, s'), csrc/learner_generic.hip + csrc/learner_modes.hip + csrc/c51_seed.hip:
  1. a' = pi_target(s'), p' = softmax(Z_target(s', a'));
  2. Tz_i = clamp(r + ((1 - d) gamma) z_i, v_min, v_max), projected onto the atoms: the target distribution m;
  3. one Adam step of the critic on (1/B) sum_b -sum_j m_j log softmax(Z(s, a))_j, then Polyak on its target;
  4. the actor step on -(1/B) sum_b Q(s, pi(s)), Q = sum_j z_j p_j, through the critic as step 3 left it, then Polyak.

F32 only, the generic launch sequence only (no fused or chain form), no gradient export, no prioritized replay."""
from __future__ import annotations

from dataclasses import dataclass, field

import torch as t
from torch import nn

from oprl_amd.algos.base_algorithm import HipLearner, OffPolicyAlgorithm, check_mode_config, require_gpu
from oprl_amd.algos.nn_functions import make_target_
from oprl_amd.algos.nn_models import CategoricalCritic, DeterministicPolicy, flatten_module_
from oprl_amd.algos.protocols import PolicyProtocol
from oprl_amd.logging import LoggerProtocol

MAX_ATOMS = 48        # csrc/engine.h kNarrowMax: the widest output the slice kernels carry


@dataclass
class D4PG(OffPolicyAlgorithm):
    logger: LoggerProtocol
    state_dim: int
    action_dim: int
    expl_noise: float = 0.1
    gamma: float = 0.99
    lr_actor: float = 3e-4
    lr_critic: float = 3e-4
    tau: float = 5e-3
    batch_size: int = 256          # unused, as in DDPG
    max_action: float = 1.
    n_atoms: int = 41              # 2 .. 48 (the engine's narrow-output limit)
    v_min: float = -150.0          # the first and the last atom: the range of the discounted return
    v_max: float = 150.0
    device: str = "cuda"
    max_batch: int = 4096          # rows the HIP workspace is sized for
    export_grads: bool = False     # refused by the learner (no data-parallel D4PG)
    no_fuse: bool = False          # (D4PG has no fused form: no effect)
    prioritized: bool = False      # refused: the per-row cross-entropy as priority is a follow-up
    precision: str = "f32"        # f32 only: the learner refuses the others

    actor: PolicyProtocol = field(init=False)
    actor_target: PolicyProtocol = field(init=False)
    critic: nn.Module = field(init=False)
    critic_target: nn.Module = field(init=False)
    learner: HipLearner = field(init=False, repr=False)
    _created: bool = False

    def __post_init__(self) -> None:
        check_config(self)

    def create(self) -> "D4PG":
        check_config(self)
        dev = require_gpu(self.device)

        def policy():
            return DeterministicPolicy(
                state_dim=self.state_dim, action_dim=self.action_dim, hidden_units=(256, 256),
                hidden_activation=nn.ReLU(inplace=True), expl_noise=self.expl_noise,
                max_action=self.max_action, device=self.device).to(dev)

        def critic():
            return CategoricalCritic(self.state_dim, self.action_dim, self.n_atoms, self.v_min, self.v_max).to(dev)

        self.actor, self.actor_target = policy(), policy()
        self.critic, self.critic_target = critic(), critic()
        for m in (self.actor, self.actor_target, self.critic, self.critic_target):
            flatten_module_(m)
        make_target_(self.actor_target, self.actor)
        make_target_(self.critic_target, self.critic)
        hp = dict(gamma=self.gamma, tau=self.tau, lr_actor=self.lr_actor, lr_critic=self.lr_critic,
                  beta1=0.9, beta2=0.999, adam_eps=1e-8, max_action=self.max_action, policy_freq=1,
                  v_min=float(self.v_min), v_max=float(self.v_max))
        self.learner = HipLearner(
            "d4pg", self.state_dim, self.action_dim, dev,
            actor_group=self.actor, actor_mlp=self.actor.mlp, actor_target_mlp=self.actor_target.mlp,
            actor_target_group=self.actor_target,
            critic_group=self.critic, critic_mlps=[self.critic.q1],
            critic_target_group=self.critic_target, critic_target_mlps=[self.critic_target.q1],
            hp=hp, max_batch=self.max_batch, export_grads=self.export_grads, no_fuse=True, precision=self.precision)
        self._created = True
        return self

    def update(self, state: t.Tensor, action: t.Tensor, reward: t.Tensor, done: t.Tensor, next_state: t.Tensor) -> None:
        self.learner.update(state, action, reward, done, next_state)


def check_config(algo: D4PG) -> None:
    """What the learner would refuse, said before anything touches the GPU."""
    if algo.prioritized:
        raise ValueError("D4PG(prioritized=True): D4PG does not train from prioritized replay yet (the follow-up: the "
                         "per-row cross-entropy as priority, importance weights on the categorical loss)")
    if not 2 <= int(algo.n_atoms) <= MAX_ATOMS:
        raise ValueError(f"D4PG: n_atoms={algo.n_atoms} outside 2..{MAX_ATOMS} (the critic's output is one of the "
                         f"engine's narrow outputs, at most {MAX_ATOMS} columns)")
    if not float(algo.v_max) > float(algo.v_min):
        raise ValueError(f"D4PG: v_max={algo.v_max} is not above v_min={algo.v_min}")
    check_mode_config(algo, "D4PG", "the generic launch sequence")
