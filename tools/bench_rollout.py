#!/usr/bin/env python3
"""Closed-loop rollout benchmark: what the policy costs beside the step.

Four legs per workload (float64 Ant at 16,384 envs, float64 Humanoid at 4,096), each a HIP graph
of K = 20 closed-loop steps on an env of its own, timed in one process with bench.py's protocol
(pre-roll, warm-up, five windows bracketed by device events), the legs alternated A/B/C/C2 per window:

  A  the torch chain of tests/policies.py Policy.torch_act (three matmuls, bias adds, ReLUs) plus
     VecEnv.step: the closed loop as it could be written before the policy kernel existed
  B  VecEnv.rollout (pbg_rollout: the actor kernel + the step, 2 launches per step + 1 per call)
  C  the bare step on pre-generated random actions (bench.py's workload)
  C2 the bare step replaying, step for step, the actions B's policy computes (recorded beforehand
     by an identical env through rollout(trajectory=True)), so its envs go through exactly B's
     states; each replay's 20 action batches are copied into the graph's staging buffer inside the
     timed region (one device copy per 20 steps)

B - C2 is the actor's (and the bookkeeping's) cost inside the loop on the same states; B - C also
carries whatever the step costs more on policy-driven poses than on random-action ones.  Writes every
window, the medians and the differences to --out.

Leg A imports tests/policies.py (Policy.torch_act and the fixture table): this tool depends on the
tests directory staying where it is.

  python tools/bench_rollout.py [--out profiles/rollout_closed_loop.json] [--only ant|humanoid]
  python tools/bench_rollout.py --actor-only     # a few actor launches alone, for a kernel trace
"""
from __future__ import annotations

import os
import sys

from benchlib import REPO, capture, device_windows, finish, parser, summary

sys.path.insert(0, os.path.join(REPO, "tests"))

WORKLOADS = {"ant": ("AntPyBulletEnv-v0", 16384), "humanoid": ("HumanoidPyBulletEnv-v0", 4096)}
K = 20  # steps per graph


def run_workload(name, args):
    import torch
    import policies
    import pybulletgym_amd  # noqa: F401
    from pybulletgym_amd.policy import MLPPolicy
    from pybulletgym_amd.vec_env import VecEnv, sample_actions

    env_id, n = WORKLOADS[name]
    dev = torch.device("cuda:0")
    tp = policies.Policy(env_id)
    pi = MLPPolicy(*tp.w, device=dev)
    LEGS = ("A", "B", "C", "C2")
    envs = {leg: VecEnv(env_id, n, device=dev, seed=0, autoreset=True, precision=64) for leg in LEGS}
    for e in envs.values():
        e.reset()
    na = envs["C"].info.action_dim
    acts = sample_actions(na, n, args.preroll + args.warmup + K, seed=0x5EED, device=dev)

    def leg_a():
        for _ in range(K):
            envs["A"].step(tp.torch_act(envs["A"].obs))

    def leg_b():
        envs["B"].rollout(pi, K)

    c_t0 = args.preroll + args.warmup

    def leg_c():
        for j in range(K):
            envs["C"].step(acts[c_t0 + j])

    # pre-roll + warm-up, untimed: closed-loop for A and B (the episodes age under the policy), the
    # random batches for C
    pre = (args.preroll + args.warmup + K - 1) // K
    # C2's actions: every 20-step chunk B will ever run (pre-roll, the warm replay, the timed replays),
    # recorded by an env identical to B's
    chunks = pre + 1 + args.windows * args.replays
    rec = VecEnv(env_id, n, device=dev, seed=0, autoreset=True, precision=64)
    rec.reset()
    acts_rec = torch.empty((chunks, K, n, na), dtype=torch.float32, device=dev)
    for c in range(chunks):
        acts_rec[c].copy_(rec.rollout(pi, K, trajectory=True).act_traj)
    rec.close()
    stage = torch.empty((K, n, na), dtype=torch.float32, device=dev)
    c2_chunk = 0

    def leg_c2():
        for j in range(K):
            envs["C2"].step(stage[j])

    def run_c2(g=None):
        nonlocal c2_chunk
        stage.copy_(acts_rec[c2_chunk])
        c2_chunk += 1
        leg_c2() if g is None else g.replay()

    for _ in range(pre):
        leg_a()
        leg_b()
        run_c2()
    for i in range(args.preroll + args.warmup):
        envs["C"].step(acts[i])
    torch.cuda.synchronize(dev)
    graphs = {"A": capture(leg_a, dev), "B": capture(leg_b, dev), "C": capture(leg_c, dev),
              "C2": capture(leg_c2, dev)}
    replay = {leg: (lambda: run_c2(graphs["C2"])) if leg == "C2" else graphs[leg].replay for leg in LEGS}
    s = summary(device_windows(dev, replay, args.windows, args.replays, warmup=1, per=K))  # us per step
    windows, med = s["windows"], s["median"]
    out = {"env_id": env_id, "n_envs": n, "precision": 64, "steps_per_graph": K, "replays_per_window": args.replays,
           "unit": "us per env-batch step", "windows": windows, "median": med, "min": s["min"], "max": s["max"],
           "B_minus_C_us": med["B"] - med["C"], "A_minus_C_us": med["A"] - med["C"],
           "B_minus_C2_us": med["B"] - med["C2"], "A_minus_C2_us": med["A"] - med["C2"],
           "C2_minus_C_us": med["C2"] - med["C"],
           # C2 replayed B's actions from the same start: its envs must be where B's are, bit for bit
           "C2_final_obs_equals_B": bool(torch.equal(envs["C2"].obs, envs["B"].obs)),
           "B_slowest_faster_than_A_fastest": max(windows["B"]) < min(windows["A"]),
           "launches_per_step": {"B": 2 + 1.0 / K, "C": 1, "C2": 1 + 1.0 / K},
           "mean_episode_length_B": float((envs["B"]._ro_acc["done_length"].sum() /
                                           envs["B"]._ro_acc["done_episodes"].sum().clamp(min=1)).item())}
    for e in envs.values():
        e.close()
    pi.close()
    return out


def actor_only(args):
    """A few launches of the actor alone at both workloads' shapes (run under a kernel trace)."""
    import torch
    import policies
    import pybulletgym_amd  # noqa: F401
    from pybulletgym_amd.policy import MLPPolicy
    for name, (env_id, n) in WORKLOADS.items():
        if args.only not in (None, name):
            continue
        tp = policies.Policy(env_id)
        pi = MLPPolicy(*tp.w, device="cuda:0")
        obs = torch.randn((n, pi.obs_dim), device="cuda:0")
        out = torch.empty((n, pi.act_dim), device="cuda:0")
        for _ in range(50):
            pi.act(obs, out=out)
            tp.torch_act(obs)
        torch.cuda.synchronize()
        pi.close()
    print("actor-only done")


def main():
    ap = parser("rollout_closed_loop.json", warmup=20)
    ap.add_argument("--only", choices=sorted(WORKLOADS), default=None)
    ap.add_argument("--preroll", type=int, default=200)
    ap.add_argument("--replays", type=int, default=10, help="graph replays (of 20 steps) per timed window")
    ap.add_argument("--actor-only", action="store_true")
    args = ap.parse_args()
    if args.actor_only:
        return actor_only(args)
    res = {"workloads": {name: run_workload(name, args) for name in WORKLOADS if args.only in (None, name)}}
    res["done"] = all(w["B_slowest_faster_than_A_fastest"] for w in res["workloads"].values())
    for name, w in res["workloads"].items():
        print(f"{name}: A {w['median']['A']:.1f} us  B {w['median']['B']:.1f} us  C {w['median']['C']:.1f} us  "
              f"C2 {w['median']['C2']:.1f} us  B-C {w['B_minus_C_us']:.1f} us  B-C2 {w['B_minus_C2_us']:.1f} us  "
              f"A-C2 {w['A_minus_C2_us']:.1f} us  C2==B states: {w['C2_final_obs_equals_B']}  "
              f"B max {w['max']['B']:.1f} < A min {w['min']['A']:.1f}: {w['B_slowest_faster_than_A_fastest']}")
    finish(res, args.out, res["done"])


if __name__ == "__main__":
    main()
