#!/usr/bin/env python3
"""The device-side permutation against torch.randperm, and one whole PPO.iterate() with the update's graph, with the
device's permutations and as one captured iteration.  tools/benchlib.py's protocol.

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

import json

from benchlib import ENV_ID, ENVS, HP, device_windows, finish, parser, pendulum_windows, run_child, summary, use_library

PERM_SHAPES = ((8192, 4), (524288, 4))
LEGS = {"hip_opt_graph": dict(graph=True), "device_perm": dict(graph=True, permutation="device"),
        "iteration_graph": dict(graph="iteration", permutation="device")}


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
        w = device_windows(dev, legs, args.windows, args.calls, warmup=args.warmup)
        perm.close()
        res[f"{B}x{n}"] = dict(summary(w), rows=B, permutations=n, unit=f"us per {n} permutations", calls_per_window=args.calls)
    return res


def child(args):
    """One process, one library: its legs' windows as one JSON line."""
    import torch
    use_library(args.lib)
    dev = torch.device("cuda:0")
    legs = args.child.split(",")
    out = {}
    if "perm" in legs:
        legs.remove("perm")
        out["perm"] = bench_perm(args, dev)
    out["iterate"], out["finite"] = pendulum_windows(dev, {leg: LEGS[leg] for leg in legs}, args.windows, args.iterations,
                                                     base=dict(backward="hip", optimizer="hip"))
    print(json.dumps(out))


def main():
    args = parser("ppo_iter.json", calls=20, calls_help="permutation calls per timed window",
                  iterations_help="PPO.iterate() calls per timed window", rounds=2).parse_args()
    if args.child:
        return child(args)
    w, res = {}, {}
    for r in range(args.rounds):
        if args.lib:
            got = run_child(__file__, "hip_opt_graph", args, args.lib)
            w.setdefault("parent_hip_opt_graph", []).extend(got["iterate"]["hip_opt_graph"])
        for legs in (["hip_opt_graph"], (["perm"] if r == 0 else []) + ["device_perm", "iteration_graph"]):
            got = run_child(__file__, ",".join(legs), args)
            if "perm" in got:
                res["perm"] = got["perm"]
            for leg, v in got["iterate"].items():
                w.setdefault(leg, []).extend(v)
            assert all(got["finite"].values()), got["finite"]
    res["iterate"] = it = dict(summary(w), trainer=dict(HP, env_id=ENV_ID, envs=ENVS, backward="hip", optimizer="hip"),
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
    finish(res, args.out)


if __name__ == "__main__":
    main()
