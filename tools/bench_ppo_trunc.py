#!/usr/bin/env python3
"""What bootstrapping through TimeLimit truncations costs.  tools/benchlib.py's protocol.

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

import json
import statistics

from benchlib import ENV_ID, ENVS, HP, device_windows, finish, parser, pendulum_windows, run_child, summary, use_library

BASE = dict(backward="hip", optimizer="hip", permutation="device", graph="iteration")
LEGS = {"terminal": {}, "terminal_beside": {}, "bootstrap": dict(truncation="bootstrap")}
WHERE_DIMS, WHERE_T, WHERE_N = (28, 128, 64, 1), 32, 16384


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
        w = device_windows(dev, legs, args.windows, args.calls, warmup=args.warmup)
        res[name] = dict(summary(w), flagged_rows=rows, tiles_with_a_flag=tiles, tiles=T * n // 16, unit="us per launch",
                         calls_per_window=args.calls)
    pop.close()
    return res


def child(args):
    """One process, one library: its legs' windows as one JSON line."""
    import torch
    use_library(args.lib)
    dev = torch.device("cuda:0")
    legs = args.child.split(",")
    out = {}
    if "where" in legs:
        legs.remove("where")
        out["where"] = bench_where(args, dev)
    if legs:
        out["iterate"], out["finite"] = pendulum_windows(dev, {leg: LEGS[leg] for leg in legs}, args.windows, args.iterations,
                                                         base=BASE)
    print(json.dumps(out))


def main():
    args = parser("ppo_trunc.json", calls=20, calls_help="actor launches per timed window",
                  iterations_help="PPO.iterate() calls per timed window", rounds=3).parse_args()
    if args.child:
        return child(args)
    w, per_round, res = {}, [], {}
    for r in range(args.rounds):
        this_round = {}
        if args.lib:
            got = run_child(__file__, "terminal", args, args.lib, timeout=300)
            this_round["parent_terminal"] = got["iterate"]["terminal"]
        for legs in (["terminal"], ["terminal_beside", "bootstrap"]):
            got = run_child(__file__, ",".join(legs), args, timeout=300)
            assert all(got["finite"].values()), got["finite"]
            this_round.update(got["iterate"])
        for leg, v in this_round.items():
            w.setdefault(leg, []).extend(v)
        per_round.append({leg: dict(median=statistics.median(v), min=min(v), max=max(v)) for leg, v in this_round.items()})
    res["where"] = run_child(__file__, "where", args, timeout=300)["where"]
    res["iterate"] = it = dict(summary(w), per_round=per_round,
                               trainer=dict(HP, env_id=ENV_ID, envs=ENVS, **BASE),
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
    finish(res, args.out)


if __name__ == "__main__":
    main()
