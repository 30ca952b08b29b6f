#!/usr/bin/env python3
"""Train a SmallReactivePolicy-shaped MLP on the device with PPO (pybullet-gym_amd/ppo.py: Gaussian action noise
inside the actor launch, one-launch GAE, clipped-surrogate updates by torch autograd) and write the mean policy
as an npz that tools/enjoy.py and MLPPolicy.from_npz load.

  python tools/train_ppo.py InvertedPendulumPyBulletEnv-v0 [--envs 256] [--steps 32] [--iterations 40]
         [--lr 3e-3] [--epochs 4] [--minibatches 4] [--gamma 0.99] [--lam 0.95] [--clip 0.2] [--log-std -0.5]
         [--ent-coef 0.0] [--vf-coef 0.5] [--seed 0] [--precision 64] [--hidden 64 64] [--out ppo_policy.npz]
         [--obs-norm] [--obs-clip 5.0] [--eval-envs 256] [--eval-steps 200] [--eval-every 1] [--curve curve.json]
         [--backward hip] [--optimizer hip] [--graph [iteration]] [--permutation device]
         [--lr-schedule linear --schedule-iterations N] [--grad-path mfma] [--truncation bootstrap] [--sharded]
         [--reward-norm] [--reward-clip 10.0] [--vf-clip X] [--target-kl Y]

--obs-norm trains under running observation normalisation (PPO(obs_norm=True)) and saves the final normaliser
in the npz (obs_mean, obs_inv_std, obs_clip); --curve writes the per-iteration evaluation as JSON.  --optimizer hip
(with --backward hip) also runs the advantage normaliser, the gradient clipping and Adam as the library's launches
(pbg_adv_norm, pbg_ppo_opt), and --graph replays the whole update as one captured graph.  --permutation device draws
the minibatch permutations on the device (pbg_perm_fill, a function of the seed that numpy restates), --lr-schedule
linear anneals the learning rate to zero over --schedule-iterations iterations from a device-side iteration count, and
--graph iteration (needs --permutation device) replays a whole iteration, rollout included, as one captured graph.
--grad-path mfma (with --backward hip) takes the gradient from the matrix-core path of pbg_ppo_grad, the one for hidden
layers wider than 64.  --truncation bootstrap (PPO(truncation="bootstrap")) bootstraps the critic's value of the terminal
observation through a TimeLimit truncation instead of treating it as a death; the default, terminal, is the trainer as it was.
--reward-norm (PPO(reward_norm=True)) divides the rewards the critic regresses by a running standard deviation of the
discounted return (ppo.RetStats, pbg_ret_stats) and clips them to +-reward-clip; the printed returns stay in the robot's
units, the curve's vf_loss is then in scaled units and gains rew_scale.
--vf-clip X (PPO(vf_clip=X)) clips the value loss PPO2's way, against the values the batch was collected under; --target-kl Y
(PPO(target_kl=Y), needs --optimizer hip) stops an update on the device once a minibatch's mean(logp_old - logp) exceeds
1.5 Y; the curve gains updates (minibatch steps applied) and kl.

--sharded trains data-parallel (ppo.ShardedPPO: --envs is the global count; --backward, --optimizer and --permutation
default to hip, hip and device, any other choice is refused by ShardedPPO, and it takes no --graph): one process per
rank, started with RANK, WORLD_SIZE, MASTER_ADDR and MASTER_PORT in the environment (the env:// convention, e.g. by torchrun); "nccl" with one device per rank when the
machine has as many GPUs as ranks, else gloo with every rank on cuda:0.  Every rank holds the one-process trainer's
bits; rank 0 prints and writes the npz.

Per evaluated iteration it prints the noise-free mean policy's mean first-episode return and length over
--eval-envs envs of a separate batch without auto-reset."""
from __future__ import annotations

import argparse
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("env_id")
    ap.add_argument("--envs", type=int, default=256, help="training envs (even)")
    ap.add_argument("--steps", type=int, default=32, help="env steps per iteration's rollout")
    ap.add_argument("--iterations", type=int, default=40)
    ap.add_argument("--lr", type=float, default=3e-3)
    ap.add_argument("--epochs", type=int, default=4)
    ap.add_argument("--minibatches", type=int, default=4)
    ap.add_argument("--gamma", type=float, default=0.99)
    ap.add_argument("--lam", type=float, default=0.95)
    ap.add_argument("--clip", type=float, default=0.2)
    ap.add_argument("--log-std", type=float, default=-0.5, help="initial log standard deviation of the actions")
    ap.add_argument("--ent-coef", type=float, default=0.0)
    ap.add_argument("--vf-coef", type=float, default=0.5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--precision", type=int, choices=(32, 64), default=64)
    ap.add_argument("--hidden", type=int, nargs=2, default=(64, 64), metavar=("H1", "H2"))
    ap.add_argument("--eval-envs", type=int, default=256)
    ap.add_argument("--eval-steps", type=int, default=200)
    ap.add_argument("--eval-every", type=int, default=1)
    ap.add_argument("--out", default="ppo_policy.npz")
    ap.add_argument("--obs-norm", action="store_true", help="running observation normalisation")
    ap.add_argument("--obs-clip", type=float, default=5.0)
    ap.add_argument("--backward", choices=("torch", "hip"), default=None,
                    help="the update's gradient: torch autograd, or the HIP backward pass (pbg_ppo_grad)")
    ap.add_argument("--optimizer", choices=("torch", "hip"), default=None,
                    help="gradient clipping and Adam: torch, or the HIP step (pbg_ppo_opt; needs --backward hip)")
    def graph_arg(s):
        if s != "iteration":
            raise argparse.ArgumentTypeError("--graph takes no value (the update as one graph) or 'iteration'")
        return s

    ap.add_argument("--graph", nargs="?", const=True, default=False, type=graph_arg,
                    help="capture the update as one graph (needs --optimizer hip); --graph iteration: the whole "
                         "iteration (needs --permutation device)")
    ap.add_argument("--permutation", choices=("torch", "device"), default=None,
                    help="the minibatch permutations: torch.randperm, or pbg_perm_fill (needs --optimizer hip)")
    ap.add_argument("--lr-schedule", choices=("linear",), default=None,
                    help="anneal the learning rate on the device (needs --optimizer hip and --schedule-iterations)")
    ap.add_argument("--schedule-iterations", type=int, default=None, help="iterations over which lr reaches zero")
    ap.add_argument("--grad-path", choices=("fma", "mfma"), default="fma",
                    help="the path of pbg_ppo_grad: vector FMA, or the matrix cores for wide networks (needs --backward hip)")
    ap.add_argument("--truncation", choices=("terminal", "bootstrap"), default="terminal",
                    help="a TimeLimit truncation in the advantages: a death, or bootstrapped through with V(terminal obs)")
    ap.add_argument("--reward-norm", action="store_true",
                    help="scale the rewards by a running std of the discounted return (pbg_ret_stats)")
    ap.add_argument("--reward-clip", type=float, default=10.0, help="the scaled rewards' clip")
    ap.add_argument("--vf-clip", type=float, default=None, help="clip the value loss within this range of the batch's values")
    ap.add_argument("--target-kl", type=float, default=None,
                    help="stop an update on the device once mean(logp_old - logp) exceeds 1.5 times this (needs --optimizer hip)")
    ap.add_argument("--curve", default=None, help="write the per-iteration evaluation here (JSON)")
    ap.add_argument("--sharded", action="store_true",
                    help="data-parallel over the ranks of RANK / WORLD_SIZE / MASTER_ADDR / MASTER_PORT (ShardedPPO)")
    args = ap.parse_args()

    import json

    import torch
    import pybulletgym_amd  # noqa: F401
    from pybulletgym_amd.ppo import PPO
    from pybulletgym_amd.vec_env import VecEnv

    rank, device, say = 0, "cuda:0", print
    if not args.sharded:   # the defaults
        args.backward, args.optimizer = args.backward or "torch", args.optimizer or "torch"
        args.permutation = args.permutation or "torch"
    if args.sharded:
        import torch.distributed as dist
        from pybulletgym_amd.distributed import ShardedVecEnv
        from pybulletgym_amd.ppo import ShardedPPO
        if args.graph:
            ap.error("--sharded takes no --graph")
        # what ShardedPPO needs where nothing was asked for; an explicit other choice reaches it and is refused by name
        args.backward, args.optimizer = args.backward or "hip", args.optimizer or "hip"
        args.permutation = args.permutation or "device"
        rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
        one_each = torch.cuda.device_count() >= world
        device = f"cuda:{rank}" if one_each else "cuda:0"
        if one_each:
            torch.cuda.set_device(rank)
        dist.init_process_group("nccl" if one_each else "gloo", init_method="env://", rank=rank, world_size=world)
        if rank != 0:
            say = lambda *a, **k: None  # noqa: E731
        env = ShardedVecEnv(args.env_id, args.envs, rank, world, device, seed=args.seed, autoreset=True, precision=args.precision)
        trainer = lambda e, **kw: ShardedPPO(e, graph=False, **kw)  # noqa: E731
    else:
        env = VecEnv(args.env_id, args.envs, device=device, seed=args.seed, autoreset=True, precision=args.precision)
        trainer = lambda e, **kw: PPO(e, graph=args.graph, **kw)  # noqa: E731
    test = VecEnv(args.env_id, args.eval_envs, device=device, seed=args.seed + 1, autoreset=False, precision=args.precision)
    ppo = trainer(env, hidden=args.hidden, steps=args.steps, seed=args.seed, gamma=args.gamma, lam=args.lam, clip=args.clip,
              lr=args.lr, epochs=args.epochs, minibatches=args.minibatches, vf_coef=args.vf_coef, ent_coef=args.ent_coef,
              log_std=args.log_std, obs_norm=args.obs_norm, obs_clip=args.obs_clip, backward=args.backward,
              optimizer=args.optimizer, permutation=args.permutation, lr_schedule=args.lr_schedule,
              schedule_iterations=args.schedule_iterations, grad_path=args.grad_path, truncation=args.truncation,
              reward_norm=args.reward_norm, reward_clip=args.reward_clip, vf_clip=args.vf_clip, target_kl=args.target_kl)
    say(f"{args.env_id} (float{args.precision}): {args.envs} envs x {args.steps} steps per iteration, actor MLP "
          f"{ppo.actor_dims}, lr {args.lr}, {args.epochs} epochs x {args.minibatches} minibatches, observation "
          f"normalisation {'on' if args.obs_norm else 'off'}, backward pass {args.backward}, optimizer "
          f"{args.optimizer}{' (one graph per iteration)' if args.graph == 'iteration' else ' (one graph)' if args.graph else ''}, "
          f"permutation {args.permutation}, lr schedule {args.lr_schedule}, gradient path {args.grad_path}, truncation "
          f"{args.truncation}, reward normalisation {'on' if args.reward_norm else 'off'}, vf_clip {args.vf_clip}, target_kl "
          f"{args.target_kl}" +
        (f", {ppo.world} ranks" if args.sharded else ""))
    curve = []
    stats = {}   # the last iterate()'s: the last minibatch's losses

    def report(it):
        ret, length = ppo.evaluate(test, args.eval_steps)
        curve.append(dict(iteration=it, return_mean=ret.mean().item(), return_min=ret.min().item(),
                          length_mean=length.double().mean().item(), std_mean=ppo.log_std.data.exp().mean().item(),
                          vf_loss=float(stats["vf"]) if "vf" in stats else None,
                          grad_norm=float(stats["grad_norm"]) if "grad_norm" in stats else None,
                          rew_scale=float(stats["rew_scale"]) if "rew_scale" in stats else None,
                          kl=float(stats["kl"]) if "kl" in stats else None,
                          updates=int(stats["updates"]) if "updates" in stats else None))
        say(f"iteration {it:4d}: mean policy return mean {ret.mean().item():9.2f} min {ret.min().item():9.2f}  "
              f"first-episode length mean {length.double().mean().item():6.1f} of {args.eval_steps}  "
              f"action std {curve[-1]['std_mean']:.3f}", flush=True)

    report(0)
    for it in range(1, args.iterations + 1):
        stats = ppo.iterate()
        if it % args.eval_every == 0 or it == args.iterations:
            report(it)
    torch.cuda.synchronize()
    if rank == 0:
        ppo.save_npz(args.out)
        print(f"wrote {args.out}")
    if args.curve and rank == 0:
        with open(args.curve, "w") as f:
            json.dump(dict(vars(args), curve=curve), f, indent=1)
        print(f"wrote {args.curve}")
    ppo.close()
    test.close()
    (env.env if args.sharded else env).close()
    if args.sharded:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
