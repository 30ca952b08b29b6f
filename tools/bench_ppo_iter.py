#!/usr/bin/env python3
"""The device-side permutation against torch.randperm, and one whole PPO.iterate() with the update's graph, with the
device's permutations and as one captured iteration.  tools/bench_ppo_opt.py's protocol: warm-up,
five windows bracketed by a synchronise, the legs alternated per window, medians with [min, max].

  perm      Permutation.fill (pbg_perm_fill: the fill and the counter's launch) beside torch.randperm into a given
            buffer, 4 permutations per call, B = 8,192 (the pendulum trainer's batch) and B = 524,288
  iterate   the pendulum trainer (256 envs x 32 steps, 4 epochs x 4 minibatches, backward="hip", optimizer="hip"):
              hip_opt_graph    graph=True                          (the parent commit's fastest leg)
              device_perm      graph=True, permutation="device"
              iteration_graph  graph="iteration", permutation="device"

A library is loaded once per process, so every round is three child processes: the hip_opt_graph leg alone with --lib
PATH (another build of libpbg_amd.so, the parent commit's), the same leg alone with this tree's library, and this tree's
two new legs alternated per window; --rounds rounds, the windows of all rounds pooled.

  python tools/bench_ppo_iter.py [--lib PARENT_LIB] [--rounds 2] [--out profiles/ppo_iter.json]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

PERM_SHAPES = ((8192, 4), (524288, 4))
HP = dict(hidden=(64, 64), steps=32, lr=3e-3, epochs=4, minibatches=4, log_std=-0.5)
LEGS = {"hip_opt_graph": dict(graph=True), "device_perm": dict(graph=True, permutation="device"),
        "iteration_graph": dict(graph="iteration", permutation="device")}


def summary(w):
    return {"windows": w, "median": {k: statistics.median(v) for k, v in w.items()}, "min": {k: min(v) for k, v in w.items()},
            "max": {k: max(v) for k, v in w.items()}}


def bench_perm(args, dev):
    import torch
    from pybulletgym_amd.ppo import Permutation
    res = {}
    for B, n in PERM_SHAPES:
        perm = Permutation(0, dev)
        gen = torch.Generator(device=dev)
        gen.manual_seed(0)
        out = torch.zeros((n, B), dtype=torch.int64, device=dev)

        def randperm():
            for j in range(n):
                torch.randperm(B, device=dev, generator=gen, out=out[j])

        legs = {"pbg_perm_fill": lambda: perm.fill(B, n, out=out), "torch_randperm": randperm}
        for _ in range(args.warmup):
            for f in legs.values():
                f()
        w = {leg: [] for leg in legs}
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        stream = torch.cuda.current_stream(dev)
        for _ in range(args.windows):
            for leg, f in legs.items():
                torch.cuda.synchronize(dev)
                e0.record(stream)
                for _ in range(args.calls):
                    f()
                e1.record(stream)
                torch.cuda.synchronize(dev)
                w[leg].append(e0.elapsed_time(e1) * 1e3 / args.calls)
        perm.close()
        res[f"{B}x{n}"] = dict(summary(w), rows=B, permutations=n, unit=f"us per {n} permutations", calls_per_window=args.calls)
    return res


def bench_iterate(args, dev, legs):
    import torch
    from pybulletgym_amd.ppo import PPO
    from pybulletgym_amd.vec_env import VecEnv
    tr = {}
    for leg in legs:
        env = VecEnv("InvertedPendulumPyBulletEnv-v0", 256, device=dev, seed=0, autoreset=True, precision=64)
        tr[leg] = (env, PPO(env, seed=0, backward="hip", optimizer="hip", **HP, **LEGS[leg]))
        for _ in range(3):
            tr[leg][1].iterate()
    w = {leg: [] for leg in tr}
    for _ in range(args.windows):
        for leg, (_, ppo) in tr.items():
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            for _ in range(args.iterations):
                ppo.iterate()
            torch.cuda.synchronize(dev)
            w[leg].append((time.perf_counter() - t0) * 1e3 / args.iterations)
    finite = {leg: bool(torch.isfinite(ppo.actor_theta.data).all()) for leg, (_, ppo) in tr.items()}
    for env, ppo in tr.values():
        ppo.close()
        env.close()
    return w, finite


def child(args):
    """One process, one library: its legs' windows as one JSON line."""
    import torch
    import pybulletgym_amd  # noqa: F401
    from pybulletgym_amd import _native
    if args.lib:
        _native.LIB_PATH = os.path.abspath(args.lib)
    dev = torch.device("cuda:0")
    legs = args.child.split(",")
    out = {}
    if "perm" in legs:
        legs.remove("perm")
        out["perm"] = bench_perm(args, dev)
    out["iterate"], out["finite"] = bench_iterate(args, dev, legs)
    print(json.dumps(out))


def run_child(args, legs, lib=None):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", ",".join(legs), "--warmup", str(args.warmup), "--windows",
           str(args.windows), "--calls", str(args.calls), "--iterations", str(args.iterations)]
    if lib:
        cmd += ["--lib", lib]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if p.returncode:
        raise RuntimeError(f"{' '.join(cmd)} failed ({p.returncode}):\n{p.stderr[-3000:]}")
    return json.loads(p.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "ppo_iter.json"))
    ap.add_argument("--lib", default=None, help="another build of libpbg_amd.so (the parent commit's, to alternate with)")
    ap.add_argument("--rounds", type=int, default=2, help="child processes per library")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20, help="permutation calls per timed window")
    ap.add_argument("--iterations", type=int, default=5, help="PPO.iterate() calls per timed window")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    w, res = {}, {}
    for r in range(args.rounds):
        if args.lib:
            got = run_child(args, ["hip_opt_graph"], args.lib)
            w.setdefault("parent_hip_opt_graph", []).extend(got["iterate"]["hip_opt_graph"])
        for legs in (["hip_opt_graph"], (["perm"] if r == 0 else []) + ["device_perm", "iteration_graph"]):
            got = run_child(args, legs)
            if "perm" in got:
                res["perm"] = got["perm"]
            for leg, v in got["iterate"].items():
                w.setdefault(leg, []).extend(v)
            assert all(got["finite"].values()), got["finite"]
    res["iterate"] = it = dict(summary(w), trainer=dict(HP, env_id="InvertedPendulumPyBulletEnv-v0", envs=256, backward="hip",
                                                        optimizer="hip"),
                               unit="ms per PPO.iterate()", iterations_per_window=args.iterations, rounds=args.rounds,
                               parent_library=args.lib)
    ref = "parent_hip_opt_graph" if args.lib else "hip_opt_graph"
    it["iteration_graph_median_not_above_the_reference_maximum"] = it["median"]["iteration_graph"] <= it["max"][ref]
    it["iteration_graph_minus_reference_median_ms"] = it["median"]["iteration_graph"] - it["median"][ref]
    for k, r in res["perm"].items():
        print(f"perm {k}: us median [min, max]  " + "  ".join(
            f"{leg} {r['median'][leg]:.1f} [{r['min'][leg]:.1f}, {r['max'][leg]:.1f}]" for leg in r["median"]), flush=True)
    print("PPO.iterate() ms median [min, max]  " + "  ".join(
        f"{k} {it['median'][k]:.3f} [{it['min'][k]:.3f}, {it['max'][k]:.3f}]" for k in it["median"]) +
        f"  iteration_graph median <= {ref} maximum: {it['iteration_graph_median_not_above_the_reference_maximum']}")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({"done": True, "out": args.out}))


if __name__ == "__main__":
    main()
