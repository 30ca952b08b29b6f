#!/usr/bin/env python3
"""What value clipping and the KL gate cost, and that with both off nothing got slower.
tools/benchlib.py's protocol; a round is one child process per library, the parent's first.

  grad      PPOGrad.run (two launches) on both paths at the pendulum trainer's shape, (5, 64, 64, 1) x 2,048 rows of
            8,192, and at Ant's, (28, 128, 64, 8) x 131,072 rows:
              plain       no option, the struct's first version: with --lib also under the parent commit's library
              value_old   with value_old / vf_clip = 0.2 (one more float per row)
              gate_open   with an open gate (one more word per workgroup)
  minibatch one minibatch of the trainer with target_kl at the pendulum shape, its six launches (adv_norm, tiles, reduce,
            gate, two of the optimiser): with the gate open (kl_limit never reached) and after a stop (six launches that
            return at entry); and the gate's launch alone
  iterate   one PPO.iterate() of the pendulum trainer of profiles/ppo_iter.json (256 envs x 32 steps, 4 epochs x 4
            minibatches, backward="hip", optimizer="hip", permutation="device", graph="iteration"):
              plain       no option: with --lib also under the parent commit's library
              both        vf_clip=0.2, target_kl=0.02

  python tools/bench_ppo_klstop.py [--lib PARENT_LIB] [--rounds 3] [--out profiles/ppo_vclip_klstop.json]
"""
from __future__ import annotations

import json
import statistics

from benchlib import ENV_ID, ENVS, HP, device_windows, finish, parser, pendulum_windows, run_child, summary, use_library

BASE = dict(backward="hip", optimizer="hip", permutation="device", graph="iteration")
ITER_LEGS = {"plain": {}, "plain_beside": {}, "both": dict(vf_clip=0.2, target_kl=0.02)}
SHAPES = {"pendulum": ((5, 64, 64, 1), 8192, 2048), "ant": ((28, 128, 64, 8), 131072, 131072)}


def batch_of(torch, np, dev, dims, B, Bm):
    r = np.random.default_rng(0)
    o, h1, h2, A = dims
    f = lambda *s: torch.from_numpy(r.standard_normal(s).astype(np.float32)).to(dev)  # noqa: E731
    Da, Dc = o * h1 + h1 + h1 * h2 + h2 + h2 * A + A, o * h1 + h1 + h1 * h2 + h2 + h2 + 1
    params = [0.1 * f(Da), 0.1 * f(Dc), -0.5 + 0.0 * f(A)]
    data = [f(B, o), f(B, A), -1.0 + 0.1 * f(B), f(B), f(B)]   # obs, act, logp_old, adv, ret
    idx = torch.from_numpy(r.permutation(B)[:Bm].astype(np.int64)).to(dev)
    return params, data, idx, f(B)


def bench_grad(args, dev, options):
    import numpy as np
    import torch
    from pybulletgym_amd.ppo import KLGate, PPOGrad
    res = {}
    for shape, (dims, B, Bm) in SHAPES.items():
        params, data, idx, value_old = batch_of(torch, np, dev, dims, B, Bm)
        an = torch.tensor([0.0, 1.0], dtype=torch.float32, device=dev)
        for path in ("fma", "mfma"):
            g = PPOGrad(dims, Bm, dev, path=path)
            out = dict(zip(("grad_actor", "grad_critic", "grad_log_std", "stats"), g._outputs(None, None, None, None)))
            kw = dict(idx=idx, adv_norm=an, **out)
            legs = {"plain": lambda: g.run(*params, *data, **kw)}
            if options:
                gate = KLGate(dev)
                legs["value_old"] = lambda: g.run(*params, *data, value_old=value_old, vf_clip=0.2, **kw)
                legs["gate_open"] = lambda: g.run(*params, *data, gate=gate.gate, **kw)
            w = device_windows(dev, legs, args.windows, args.calls if shape == "pendulum" else max(2, args.calls // 10),
                               warmup=args.warmup)
            assert bool(torch.isfinite(out["grad_actor"]).all())
            res[f"{shape}_{path}"] = w
            g.close()
    return res


def bench_minibatch(args, dev):
    import numpy as np
    import torch
    from pybulletgym_amd.ppo import AdamClip, KLGate, PPOGrad, adv_norm
    dims, B, Bm = SHAPES["pendulum"]
    params, data, idx, value_old = batch_of(torch, np, dev, dims, B, Bm)
    res = {}
    for path in ("fma", "mfma"):
        g, opt = PPOGrad(dims, Bm, dev, path=path), AdamClip([p.numel() for p in params], dev)
        grads = [torch.zeros_like(p) for p in params]
        stats, an = torch.zeros(4, dtype=torch.float64, device=dev), torch.zeros(2, dtype=torch.float32, device=dev)
        info = torch.zeros(2, dtype=torch.float64, device=dev)
        gates = {"open": KLGate(dev), "stopped": KLGate(dev)}
        gates["stopped"].check(torch.ones(4, dtype=torch.float64, device=dev), 0.0)   # 1 > 0: shut
        work = [p.clone() for p in params]

        def minibatch(gate, limit):
            adv_norm(data[3], idx, out=an)
            g.run(*work, *data, idx=idx, adv_norm=an, grad_actor=grads[0], grad_critic=grads[1], grad_log_std=grads[2],
                  stats=stats, value_old=value_old, vf_clip=0.2, gate=gate.gate)
            gate.check(stats, limit)
            opt.step(work, grads, 0.0, (0.9, 0.999), 1e-5, 0.5, info=info, gate=gate.gate)   # lr 0: the weights stay

        legs = {"six_launches_open": lambda: minibatch(gates["open"], 1e30),
                "six_launches_stopped": lambda: minibatch(gates["stopped"], 1e30),
                "gate_launch": lambda: gates["open"].check(stats, 1e30)}
        res[path] = device_windows(dev, legs, args.windows, args.calls, warmup=args.warmup)
        assert gates["stopped"].state.cpu().tolist()[0] == 1 and gates["open"].state.cpu().tolist()[0] == 0
        g.close()
        opt.close()
    return res


def bench_iterate(args, dev, legs):
    updates = {leg: [] for leg in legs}

    def after(leg, ppo):   # what the window's last iterate() reported as stats["updates"]
        if ppo.kl_gate is not None:
            updates[leg].append(int(ppo.kl_gate.state[1]))

    w, finite = pendulum_windows(dev, {leg: ITER_LEGS[leg] for leg in legs}, args.windows, args.iterations, base=BASE, after=after)
    return w, finite, {k: v for k, v in updates.items() if v}


def child(args):
    """One process, one library: its legs' windows as one JSON line."""
    import torch
    use_library(args.lib)
    dev = torch.device("cuda:0")
    out = {}
    if args.child == "plain":
        out["grad"] = bench_grad(args, dev, options=False)
        out["iterate"], out["finite"], _ = bench_iterate(args, dev, ["plain"])
    else:
        out["grad"] = bench_grad(args, dev, options=True)
        out["minibatch"] = bench_minibatch(args, dev)
        out["iterate"], out["finite"], out["updates"] = bench_iterate(args, dev, ["plain_beside", "both"])
    print(json.dumps(out))


def pool(into, got, rename=lambda k: k):
    for group, legs in got.items():
        for leg, v in legs.items():
            into.setdefault(group, {}).setdefault(rename(leg), []).extend(v)


def main():
    args = parser("ppo_vclip_klstop.json", calls=40, calls_help="calls per timed window at the pendulum shape (a tenth at Ant's)",
                  iterations_help="PPO.iterate() calls per timed window", rounds=3).parse_args()
    if args.child:
        return child(args)
    grad, mb, it, updates, rounds = {}, {}, {}, [], []
    for r in range(args.rounds):
        this = {}
        if args.lib:
            got = run_child(__file__, "plain", args, args.lib, timeout=400)
            pool(grad, got["grad"], lambda k: "parent_" + k)
            pool(it, {"iterate": got["iterate"]}, lambda k: "parent_" + k)
            this["parent"] = {k: statistics.median(v["plain"]) for k, v in got["grad"].items()}
            this["parent"]["iterate"] = statistics.median(got["iterate"]["plain"])
        got = run_child(__file__, "plain", args, timeout=400)
        assert all(got["finite"].values()), got["finite"]
        pool(grad, got["grad"])
        pool(it, {"iterate": got["iterate"]})
        this["this_tree"] = {k: statistics.median(v["plain"]) for k, v in got["grad"].items()}
        this["this_tree"]["iterate"] = statistics.median(got["iterate"]["plain"])
        got = run_child(__file__, "options", args, timeout=400)
        assert all(got["finite"].values()), got["finite"]
        pool(grad, got["grad"], lambda k: k if k != "plain" else "plain_beside")
        pool(mb, got["minibatch"])
        pool(it, {"iterate": got["iterate"]})
        updates.extend(got["updates"].get("both", []))
        rounds.append(this)
    res = dict(protocol=f"{args.rounds} rounds; a round is one process per library (the parent's first), {args.windows} windows per "
                        f"leg and process, legs alternated per window, {args.warmup} warm-up calls; medians over all windows",
               parent_library=args.lib, per_round_medians=rounds,
               grad={k: dict(summary(v), unit="us per PPOGrad.run (two launches)", shape=SHAPES[k.split("_")[0]][0],
                             rows=SHAPES[k.split("_")[0]][2]) for k, v in grad.items()},
               minibatch={k: dict(summary(v), unit="us", shape=SHAPES["pendulum"][0], rows=SHAPES["pendulum"][2])
                          for k, v in mb.items()},
               iterate=dict(summary(it["iterate"]), unit="ms per PPO.iterate()", updates_of_both_per_window_end=updates,
                            trainer=dict(HP, env_id=ENV_ID, envs=ENVS, **BASE)))
    if args.lib:
        # each median of this tree against the parent's median and the parent's own round-to-round spread
        verdict = {}
        for name, s in list(res["grad"].items()) + [("iterate", res["iterate"])]:
            p = [r["parent"][name] for r in rounds]
            mine, theirs, spread = s["median"]["plain"], s["median"]["parent_plain"], max(p) - min(p)
            verdict[name] = dict(this_tree_median=mine, parent_median=theirs, parent_round_spread=spread,
                                 within_the_parents_spread=abs(mine - theirs) <= spread or mine <= theirs)
        res["options_off_vs_parent"] = verdict
    for k, s in res["grad"].items():
        print(f"grad {k} us median [min, max]  " + "  ".join(f"{leg} {s['median'][leg]:.1f} [{s['min'][leg]:.1f}, {s['max'][leg]:.1f}]"
                                                             for leg in s["median"]), flush=True)
    for k, s in res["minibatch"].items():
        print(f"minibatch {k} us median [min, max]  " + "  ".join(
            f"{leg} {s['median'][leg]:.1f} [{s['min'][leg]:.1f}, {s['max'][leg]:.1f}]" for leg in s["median"]), flush=True)
    s = res["iterate"]
    print("PPO.iterate() ms median [min, max]  " + "  ".join(
        f"{k} {s['median'][k]:.3f} [{s['min'][k]:.3f}, {s['max'][k]:.3f}]" for k in s["median"]) + f"  updates {updates}", flush=True)
    if args.lib:
        print(json.dumps(res["options_off_vs_parent"], indent=1))
    finish(res, args.out)


if __name__ == "__main__":
    main()
