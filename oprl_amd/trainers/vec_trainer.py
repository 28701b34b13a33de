"""Training loop over N environments at once (extension — the reference's trainer steps one
environment, base_trainer.py:38-74, and its roadmap leaves "Distributed Training Improvements" open).

Per iteration: N actions from ONE policy launch (``actor.explore_rows``; uniform during the first ``start_steps``
environment steps, counted across all environments), one step of every environment, and — once the buffer holds a
batch — ONE ``algo.update_from_buffer(..., act_next=<the N next observations>, n_updates=N)``: N updates for N
environment steps (update-to-data ratio 1, as in the reference's loop) with the next iteration's policy rows riding
behind them in the same C call.

Episodes.  The replay has one open episode, so the transitions of each environment are assembled on the host
(``EpisodeAssembler``) and enter the replay as one ``add_transitions(rows, episode_done=True)`` when that environment's
episode ends — how the learner ranks of the distributed runner take in actor episodes.  Data therefore becomes
visible to the sampler ONE EPISODE LATE: nothing of an environment's running episode can be drawn.

``open_episodes=True`` lifts that: the replay opens one episode per environment
(``replay_buffer.open_lanes(N)``) and every iteration's N transitions go in with ONE ``add_step_rows`` call, next states
included, so the learner trains from the first iteration whose end finds a batch in the buffer."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from oprl_amd.algos.base_algorithm import check_nstep_gamma, refuse_prioritized
from oprl_amd.environment.protocols import EnvProtocol
from oprl_amd.trainers.base_trainer import BaseTrainer


def crossed(prev: int, cur: int, every: int) -> int | None:
    """The largest multiple of ``every`` in (prev, cur], or None when there is none (or ``every`` <= 0): periodic work
    of a loop whose step count moves by N fires when its interval was crossed, at that multiple."""
    if every <= 0 or cur // every <= prev // every:
        return None
    return cur // every * every


class EpisodeAssembler:
    """Host-side open episodes of N environments: float32 records [state (S) | action (A) | reward | done] kept in
    order per environment, handed out as one [n, S + A + 2] block when that environment's episode ends."""

    def __init__(self, n_envs: int) -> None:
        self._open: list[list[np.ndarray]] = [[] for _ in range(n_envs)]

    def pending(self, env: int) -> int:
        """Records of ``env``'s running episode."""
        return len(self._open[env])

    def add(self, env: int, state, action, reward: float, done: bool, episode_over: bool) -> np.ndarray | None:
        """Append one transition to ``env``'s episode; returns the whole episode's records (and starts a new one) when
        ``episode_over``, else None."""
        s = np.asarray(state, dtype=np.float32).reshape(-1)
        a = np.asarray(action, dtype=np.float32).reshape(-1)
        self._open[env].append(np.concatenate([s, a, np.asarray([reward, float(done)], dtype=np.float32)]))
        if not episode_over:
            return None
        rows = np.stack(self._open[env])
        self._open[env] = []
        return rows


@dataclass(kw_only=True)
class VecTrainer(BaseTrainer):
    envs: list[EnvProtocol]
    env: EnvProtocol | None = None      # (BaseTrainer's single environment: unused here, envs[0] when not given)
    open_episodes: bool = False         # one open replay episode per environment instead of the host-side assembler

    def __post_init__(self) -> None:
        if not self.envs:
            raise ValueError("VecTrainer needs at least one environment")
        if self.env is None:
            self.env = self.envs[0]

    def train(self) -> None:
        self.algo.check_created()
        self.replay_buffer.check_created()
        refuse_prioritized(self.algo, self.replay_buffer)
        check_nstep_gamma(self.algo, self.replay_buffer)
        n = len(self.envs)
        obs = np.stack([np.asarray(env.reset()[0], dtype=np.float32) for env in self.envs])
        assembler = EpisodeAssembler(n)
        if self.open_episodes:
            self.replay_buffer.open_lanes(n)
        steps = 0
        while steps < self.num_steps:
            prev = steps
            obs = self._collect_open(prev, obs) if self.open_episodes else self._collect_rows(prev, obs, assembler)
            steps += n
            if len(self.replay_buffer) < self.batch_size:
                continue
            rewards = self._learn_rows(prev, steps, obs)
            self._periodic_rows(prev, steps, rewards)

    def _collect_rows(self, steps: int, obs: np.ndarray, assembler: EpisodeAssembler) -> np.ndarray:
        """One step of every environment; closed episodes into the replay.  Returns the next observations [N, S]."""
        if steps < self.start_steps:
            actions = [env.sample_action() for env in self.envs]
        else:
            actions = self.algo.actor.explore_rows(obs)
        nxt = np.empty_like(obs)
        for i, env in enumerate(self.envs):
            o2, reward, terminated, truncated, _ = env.step(actions[i])
            over = bool(terminated or truncated)
            rows = assembler.add(i, obs[i], actions[i], reward, terminated, over)
            if rows is not None:
                self.replay_buffer.add_transitions(rows, episode_done=True)
                o2, _ = env.reset()
            nxt[i] = o2
        return nxt

    def _collect_open(self, steps: int, obs: np.ndarray) -> np.ndarray:
        """One step of every environment and ONE ``add_step_rows`` for all of them.  s' is the observation the
        environment returned — the terminal or truncation observation where an episode ended; the observations handed
        back are the reset ones there."""
        if steps < self.start_steps:
            actions = [env.sample_action() for env in self.envs]
        else:
            actions = self.algo.actor.explore_rows(obs)
        n = len(self.envs)
        acts = np.stack([np.asarray(a, dtype=np.float32).reshape(-1) for a in actions])
        s2, nxt = np.empty_like(obs), np.empty_like(obs)
        rewards, dones, over = np.empty(n, np.float32), np.empty(n, np.float32), np.zeros(n, bool)
        for i, env in enumerate(self.envs):
            o2, reward, terminated, truncated, _ = env.step(actions[i])
            s2[i], rewards[i], dones[i] = o2, reward, float(terminated)
            over[i] = bool(terminated or truncated)
            if over[i]:
                o2, _ = env.reset()
            nxt[i] = o2
        self.replay_buffer.add_step_rows(obs, acts, rewards, dones, s2, over)
        return nxt

    def _due(self, prev: int, cur: int) -> dict[str, int | None]:
        return {"eval": crossed(prev, cur, self.eval_interval), "policy": crossed(prev, cur, self.save_policy_every),
                "checkpoint": crossed(prev, cur, self.save_checkpoint_every), "stdout": crossed(prev, cur, self.stdout_log_every)}

    def _learn_rows(self, prev: int, steps: int, next_obs: np.ndarray):
        """N updates as one call; the next iteration's policy rows ride behind them when that iteration explores and no
        periodic work of this one uses the actor in between."""
        n = len(self.envs)
        due = self._due(prev, steps)
        if self.fused_sample_update and hasattr(self.algo, "update_from_buffer"):
            quiet = due["eval"] is None and due["policy"] is None and due["checkpoint"] is None
            ride = quiet and hasattr(self.algo, "_actor_mlp") and self.start_steps <= steps < self.num_steps
            self.algo.update_from_buffer(self.replay_buffer, self.batch_size, act_next=next_obs if ride else None, n_updates=n)
        else:
            for _ in range(n * int(getattr(self.algo, "utd_ratio", 1))):
                self.algo.update(*self.replay_buffer.sample(self.batch_size))
        wanted = due["eval"] is not None or due["stdout"] is not None
        return self.replay_buffer.sample(self.batch_size)[2] if wanted else None

    def _periodic_rows(self, prev: int, steps: int, rewards) -> None:
        due = self._due(prev, steps)
        if due["eval"] is not None:
            self._log_evaluation(due["eval"], rewards)
        if due["policy"] is not None:
            self._save_policy(due["policy"])
        if due["checkpoint"] is not None:
            self.save_checkpoint(self.logger.log_dir / "checkpoints" / f"{due['checkpoint']}.ckpt", due["checkpoint"])
        if due["stdout"] is not None:
            self._log_stdout(due["stdout"], rewards)

    def evaluate(self) -> dict[str, float]:
        """``BaseTrainer.evaluate`` with all ``num_eval_episodes`` test environments (the same seeds) stepped in
        lockstep through ``actor.exploit_rows``; finished ones drop out."""
        envs = [self.make_env_test(self.seed + k) for k in range(self.num_eval_episodes)]
        obs = [env.reset()[0] for env in envs]
        totals = [0.0] * len(envs)
        live = list(range(len(envs)))
        while live:
            actions = self.algo.actor.exploit_rows(np.stack([np.asarray(obs[k], dtype=np.float32) for k in live]))
            still = []
            for action, k in zip(actions, live):
                obs[k], reward, terminated, truncated, _ = envs[k].step(action)
                totals[k] += reward
                if not (terminated or truncated):
                    still.append(k)
            live = still
        return {"return": float(np.mean(totals))}
