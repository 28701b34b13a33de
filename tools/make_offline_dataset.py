"""Write an offline dataset (.npz, D4RL key names: buffers/offline_dataset.py) by rolling a ``synthetic:`` environment
with uniform actions, or with a saved policy plus Gaussian noise.

D4RL's files cannot be fetched for this build, and its simulators are not part of it: the synthetic linear-dynamics
environments (environment/synthetic.py) are the only source of data here.  They never terminate, so every episode ends
in a timeout; ``next_observations`` is written, so no row is lost to that.

    python tools/make_offline_dataset.py --env synthetic:walker-walk --episodes 100 --out walker_random.npz
    python tools/make_offline_dataset.py --env synthetic:walker-walk --policy logs/.../weights/100000.w --noise 0.1 \\
                                         [--norm logs/.../weights/100000.w.norm.npz] --out walker_medium.npz
"""
import argparse
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from oprl_amd.environment.make_env import PREFIX, make_env  # noqa: E402


def roll(env, episodes: int, act) -> dict:
    """``episodes`` episodes of ``env`` under ``act(obs) -> action``, as the dataset's arrays."""
    cols = {k: [] for k in ("observations", "actions", "rewards", "terminals", "timeouts", "next_observations")}
    for _ in range(episodes):
        obs, _ = env.reset()
        over = False
        while not over:
            a = np.clip(np.asarray(act(obs), dtype=np.float32), -1, 1)
            nxt, reward, terminated, truncated, _ = env.step(a)
            for k, v in zip(cols, (obs, a, reward, bool(terminated), bool(truncated and not terminated), nxt)):
                cols[k].append(v)
            over = bool(terminated or truncated)
            obs = nxt
    return {"observations": np.asarray(cols["observations"], np.float32), "actions": np.asarray(cols["actions"], np.float32),
            "rewards": np.asarray(cols["rewards"], np.float32), "terminals": np.asarray(cols["terminals"], bool),
            "timeouts": np.asarray(cols["timeouts"], bool),
            "next_observations": np.asarray(cols["next_observations"], np.float32)}


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--env", required=True, help=f"{PREFIX}<task>, e.g. {PREFIX}walker-walk")
    ap.add_argument("--episodes", type=int, default=100)
    ap.add_argument("--out", required=True, help="the .npz to write")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--policy", default=None, help="a saved actor (trainers' weights/<step>.w); default: uniform actions")
    ap.add_argument("--norm", default=None, help="the ObsNorm saved next to an offline policy (<weights>.norm.npz)")
    ap.add_argument("--noise", type=float, default=0.1, help="std of the Gaussian noise added to the policy's actions")
    args = ap.parse_args()
    if not args.env.startswith(PREFIX):
        sys.exit(f"--env {args.env!r}: only the {PREFIX}<task> environments exist in this build")
    env = make_env(args.env, seed=args.seed)
    if args.policy is None:
        act = lambda obs: env.sample_action()      # noqa: E731
    else:
        import torch as t
        actor = t.load(args.policy, weights_only=False)
        rng = np.random.RandomState(args.seed + 1)
        norm = None
        if args.norm is not None:
            from oprl_amd.buffers.offline_dataset import ObsNorm
            with np.load(args.norm) as z:
                norm = ObsNorm(z["mean"], z["std"])

        def act(obs):
            a = np.asarray(actor.exploit(norm(obs) if norm is not None else obs), dtype=np.float32)
            return a + args.noise * rng.standard_normal(a.shape).astype(np.float32)
    data = roll(env, args.episodes, act)
    np.savez_compressed(args.out, **data)
    print(f"{args.out}: {len(data['rewards'])} rows, {args.episodes} episodes, mean reward {data['rewards'].mean():.4f}")


if __name__ == "__main__":
    main()
