#!/usr/bin/env python3
"""What bootstrapping through TimeLimit truncations costs.  tools/bench_ppo_iter.py's protocol:
warm-up, five windows bracketed by a synchronise, the legs alternated per window, medians with [min, max].

  iterate   one PPO.iterate() of the pendulum trainer of profiles/ppo_iter.json (256 envs x 32 steps, 4 epochs x 4
            minibatches, backward="hip", optimizer="hip", permutation="device", graph="iteration"):
              terminal    truncation="terminal", the default: with --lib also under the parent commit's library
              bootstrap   truncation="bootstrap", alternated per window with a second terminal trainer
  where     pbg_population_act_where alone at Ant's critic (28, 128, 64, 1) over 32 x 16,384 rows under four flag
            patterns (none, 0.1 % random, one whole step, all), beside pbg_population_act on as many dense rows as
            the pattern flags

A library is loaded once per process, so every round is three child processes: the terminal leg alone with --lib PATH
(another build of libpbg_amd.so, the parent commit's), the same leg alone with this tree's library, and this tree's
terminal and bootstrap legs alternated per window; --rounds rounds, the windows of all rounds pooled.

  python tools/bench_ppo_trunc.py [--lib PARENT_LIB] [--rounds 3] [--out profiles/ppo_trunc.json]
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

HP = dict(hidden=(64, 64), steps=32, lr=3e-3, epochs=4, minibatches=4, log_std=-0.5)
LEGS = {"terminal": {}, "terminal_beside": {}, "bootstrap": dict(truncation="bootstrap")}
WHERE_DIMS, WHERE_T, WHERE_N = (28, 128, 64, 1), 32, 16384


def summary(w):
    return {"windows": w, "median": {k: statistics.median(v) for k, v in w.items()}, "min": {k: min(v) for k, v in w.items()},
            "max": {k: max(v) for k, v in w.items()}}


def bench_iterate(args, dev, legs):
    import torch
    from pybulletgym_amd.ppo import PPO
    from pybulletgym_amd.vec_env import VecEnv
    tr = {}
    for leg in legs:
        env = VecEnv("InvertedPendulumPyBulletEnv-v0", 256, device=dev, seed=0, autoreset=True, precision=64)
        tr[leg] = (env, PPO(env, seed=0, backward="hip", optimizer="hip", permutation="device", graph="iteration", **HP,
                            **LEGS[leg]))
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


def bench_where(args, dev):
    """us per launch: act_where under each pattern, and act on the pattern's count of dense rows."""
    import numpy as np
    import torch
    from pybulletgym_amd.policy import MLPPopulation
    T, n, dims = WHERE_T, WHERE_N, WHERE_DIMS
    pop = MLPPopulation(dims, 1, dev)
    pop.set_all(pop.init_theta(0))
    r = np.random.default_rng(0)
    obs = torch.from_numpy(r.standard_normal((T, n, dims[0])).astype(np.float32)).to(dev)
    out = torch.zeros((T, n, dims[3]), dtype=torch.float32, device=dev)
    patterns = {"none": np.zeros((T, n), np.uint8), "random_0.1_percent": (r.random((T, n)) < 1e-3).astype(np.uint8),
                "one_step": np.zeros((T, n), np.uint8), "all": np.ones((T, n), np.uint8)}
    patterns["one_step"][T // 2] = 1
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    stream = torch.cuda.current_stream(dev)
    res = {}
    for name, f in patterns.items():
        flags = torch.from_numpy(f).to(dev)
        rows = int(f.sum())
        tiles = int(f.reshape(T, n // 16, 16).any(axis=2).sum())
        dense = rows + rows % 2
        legs = {"act_where": lambda: pop.act_where(flags, obs, out=out)}
        if dense:
            x, y = obs.view(T * n, -1)[:dense], out.view(T * n, -1)[:dense]
            legs["act_dense_rows"] = lambda: pop.act(x, out=y)
        for _ in range(args.warmup):
            for g in legs.values():
                g()
        w = {leg: [] for leg in legs}
        for _ in range(args.windows):
            for leg, g in legs.items():
                torch.cuda.synchronize(dev)
                e0.record(stream)
                for _ in range(args.calls):
                    g()
                e1.record(stream)
                torch.cuda.synchronize(dev)
                w[leg].append(e0.elapsed_time(e1) * 1e3 / args.calls)
        res[name] = dict(summary(w), flagged_rows=rows, tiles_with_a_flag=tiles, tiles=T * n // 16, unit="us per launch",
                         calls_per_window=args.calls)
    pop.close()
    return res


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
    if "where" in legs:
        legs.remove("where")
        out["where"] = bench_where(args, dev)
    if legs:
        out["iterate"], out["finite"] = bench_iterate(args, dev, legs)
    print(json.dumps(out))


def run_child(args, legs, lib=None):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", ",".join(legs), "--warmup", str(args.warmup), "--windows",
           str(args.windows), "--calls", str(args.calls), "--iterations", str(args.iterations)]
    if lib:
        cmd += ["--lib", lib]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if p.returncode:
        raise RuntimeError(f"{' '.join(cmd)} failed ({p.returncode}):\n{p.stderr[-3000:]}")
    return json.loads(p.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "ppo_trunc.json"))
    ap.add_argument("--lib", default=None, help="another build of libpbg_amd.so (the parent commit's, to alternate with)")
    ap.add_argument("--rounds", type=int, default=3, help="child processes per library")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20, help="actor launches per timed window")
    ap.add_argument("--iterations", type=int, default=5, help="PPO.iterate() calls per timed window")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    w, per_round, res = {}, [], {}
    for r in range(args.rounds):
        this_round = {}
        if args.lib:
            got = run_child(args, ["terminal"], args.lib)
            this_round["parent_terminal"] = got["iterate"]["terminal"]
        for legs in (["terminal"], ["terminal_beside", "bootstrap"]):
            got = run_child(args, legs)
            assert all(got["finite"].values()), got["finite"]
            this_round.update(got["iterate"])
        for leg, v in this_round.items():
            w.setdefault(leg, []).extend(v)
        per_round.append({leg: dict(median=statistics.median(v), min=min(v), max=max(v)) for leg, v in this_round.items()})
    res["where"] = run_child(args, ["where"])["where"]
    res["iterate"] = it = dict(summary(w), per_round=per_round,
                               trainer=dict(HP, env_id="InvertedPendulumPyBulletEnv-v0", envs=256, backward="hip", optimizer="hip",
                                            permutation="device", graph="iteration"),
                               unit="ms per PPO.iterate()", iterations_per_window=args.iterations, rounds=args.rounds,
                               parent_library=args.lib)
    if args.lib:
        it["terminal_median_not_above_the_parent_maximum"] = it["median"]["terminal"] <= it["max"]["parent_terminal"]
        it["terminal_minus_parent_median_ms"] = it["median"]["terminal"] - it["median"]["parent_terminal"]
    it["bootstrap_minus_terminal_beside_median_ms"] = it["median"]["bootstrap"] - it["median"]["terminal_beside"]
    for k, r in res["where"].items():
        ratio = r["median"]["act_where"] / r["median"]["act_dense_rows"] if "act_dense_rows" in r["median"] else None
        r["act_where_over_act_dense_rows"] = ratio
        print(f"where {k} ({r['flagged_rows']} rows in {r['tiles_with_a_flag']} of {r['tiles']} tiles): us median [min, max]  " +
              "  ".join(f"{leg} {r['median'][leg]:.1f} [{r['min'][leg]:.1f}, {r['max'][leg]:.1f}]" for leg in r["median"]) +
              (f"  ratio {ratio:.3f}" if ratio else ""), flush=True)
    print("PPO.iterate() ms median [min, max]  " + "  ".join(
        f"{k} {it['median'][k]:.3f} [{it['min'][k]:.3f}, {it['max'][k]:.3f}]" for k in it["median"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({"done": True, "out": args.out}))


if __name__ == "__main__":
    main()
