#!/usr/bin/env python3
"""Train a SmallReactivePolicy-shaped MLP on the device with evolution strategies (pybullet-gym_amd/es.py:
mirrored sampling, centred ranks, plain SGD) and write it as an npz that tools/enjoy.py and
MLPPolicy.from_npz load.

  python tools/train_es.py InvertedPendulumPyBulletEnv-v0 [--pairs 32] [--envs-per-member 4] [--steps 200]
         [--generations 60] [--sigma 0.1] [--lr 0.2] [--seed 0] [--precision 64] [--hidden 16 8] [--out es_policy.npz]
         [--obs-norm] [--obs-clip 5.0] [--curve curve.json]

--obs-norm trains under running observation normalisation (EvolutionStrategy(obs_norm=True)) and saves the
final normaliser in the npz (obs_mean, obs_inv_std, obs_clip), which MLPPolicy.from_npz picks up; --curve
writes the per-generation centre returns and lengths as JSON.

Per generation it prints the centre's mean first-episode return and length over all envs (one extra
rollout with every member set to the centre; --eval-every N does it every N-th generation only)."""
from __future__ import annotations

import argparse
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("env_id")
    ap.add_argument("--pairs", type=int, default=32, help="mirrored pairs (the population has twice as many members)")
    ap.add_argument("--envs-per-member", type=int, default=4)
    ap.add_argument("--steps", type=int, default=200, help="env steps per rollout")
    ap.add_argument("--generations", type=int, default=60)
    ap.add_argument("--sigma", type=float, default=0.1)
    ap.add_argument("--lr", type=float, default=0.2)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--precision", type=int, choices=(32, 64), default=64)
    ap.add_argument("--hidden", type=int, nargs=2, default=(16, 8), metavar=("H1", "H2"))
    ap.add_argument("--eval-every", type=int, default=1)
    ap.add_argument("--out", default="es_policy.npz")
    ap.add_argument("--obs-norm", action="store_true", help="running observation normalisation")
    ap.add_argument("--obs-clip", type=float, default=5.0)
    ap.add_argument("--curve", default=None, help="write the per-generation centre evaluation here (JSON)")
    args = ap.parse_args()

    import json

    import torch
    import pybulletgym_amd  # noqa: F401
    from pybulletgym_amd.es import EvolutionStrategy
    from pybulletgym_amd.policy import MLPPopulation
    from pybulletgym_amd.vec_env import VecEnv

    n = 2 * args.pairs * args.envs_per_member
    env = VecEnv(args.env_id, n, device="cuda:0", seed=args.seed, autoreset=False, precision=args.precision)
    dims = (env.info.obs_dim, args.hidden[0], args.hidden[1], env.info.action_dim)
    pop = MLPPopulation(dims, args.pairs, env.device)
    es = EvolutionStrategy(env, pop, args.sigma, args.lr, args.steps, seed=args.seed, obs_norm=args.obs_norm,
                           obs_clip=args.obs_clip)
    print(f"{args.env_id} (float{args.precision}): {pop.n_members} members x {args.envs_per_member} envs, MLP {dims}, "
          f"{pop.n_params} parameters, sigma {args.sigma} lr {args.lr}, {args.steps}-step rollouts, "
          f"observation normalisation {'on' if args.obs_norm else 'off'}")
    curve = []

    def report(gen):
        ret, length = es.evaluate()
        curve.append(dict(generation=gen, return_mean=ret.mean().item(), return_min=ret.min().item(),
                          length_mean=length.double().mean().item()))
        print(f"generation {gen:4d}: centre return mean {ret.mean().item():9.2f} min {ret.min().item():9.2f}  "
              f"first-episode length mean {length.double().mean().item():6.1f} of {args.steps}", flush=True)

    report(0)
    for gen in range(1, args.generations + 1):
        es.step()
        if gen % args.eval_every == 0 or gen == args.generations:
            report(gen)
    torch.cuda.synchronize()
    pop.save_npz(args.out, es.theta)
    print(f"wrote {args.out}")
    if args.curve:
        with open(args.curve, "w") as f:
            json.dump(dict(env_id=args.env_id, obs_norm=args.obs_norm, obs_clip=args.obs_clip, pairs=args.pairs,
                           envs_per_member=args.envs_per_member, steps=args.steps, sigma=args.sigma, lr=args.lr,
                           seed=args.seed, precision=args.precision, hidden=list(args.hidden), curve=curve), f, indent=1)
        print(f"wrote {args.curve}")
    pop.close()
    env.close()


if __name__ == "__main__":
    main()
