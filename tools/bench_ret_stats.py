#!/usr/bin/env python3
"""What reward scaling by a running std of the discounted return costs.  tools/benchlib.py's
protocol.

  launches  pbg_ret_stats_walk, _finalize and _apply alone and as one round, at Ant's 32 x 16,384 and at the pendulum
            trainer's 32 x 256, beside a torch restatement of the same round (a Python loop over t with float64
            tensors, then var, rsqrt and clamp; no read-back either): us per call, device events.  Each leg twice:
            launched from Python call by call ("eager", which at these sizes times the host's enqueue), and as one
            captured graph of --calls calls replayed ("graph", the device's time)
  iterate   one PPO.iterate() of the pendulum trainer of profiles/ppo_iter.json (256 envs x 32 steps, 4 epochs x 4
            minibatches, backward="hip", optimizer="hip", permutation="device", graph="iteration") with reward_norm off
            and on, and a second trainer with it off (what two trainers of one process differ by), alternated per
            window in one process: ms per iterate()

  python tools/bench_ret_stats.py [--out profiles/ret_stats.json]
"""
from __future__ import annotations

from benchlib import ENV_ID, ENVS, HP, device_windows, finish, parser, pendulum_windows, summary, warm_up

BASE = dict(backward="hip", optimizer="hip", permutation="device", graph="iteration")
SHAPES = {"ant_32x16384": (32, 16384), "pendulum_32x256": (32, 256)}
GAMMA, CLIP, FLOOR = 0.99, 10.0, 1e-2


def torch_round(rew, done, carry, tot, out):
    """The round in torch kernels: the same scan, sums and scale (another order of the sums), nothing read back."""
    import torch
    T = rew.shape[0]
    R = carry
    cnt = torch.zeros_like(carry)
    s1, s2 = torch.zeros_like(carry), torch.zeros_like(carry)
    zero = torch.zeros_like(carry)
    for t in range(T):
        R = GAMMA * R + rew[t].double()
        fin = torch.isfinite(R)
        cnt += fin
        s1 += torch.where(fin, R, zero)
        s2 += torch.where(fin, R * R, zero)
        R = torch.where(~fin | (done[t] != 0), zero, R)
    carry.copy_(R)
    tot[0] += cnt.sum()
    tot[1] += s1.sum()
    tot[2] += s2.sum()
    m = tot[1] / tot[0]
    var = torch.clamp(tot[2] / tot[0] - m * m, min=FLOOR)
    scale = (1.0 / torch.sqrt(var)).float()
    torch.clamp(rew * scale, -CLIP, CLIP, out=out)


def bench_launches(args, dev):
    import numpy as np
    import torch
    from pybulletgym_amd.ppo import RetStats
    res = {}
    for name, (T, n) in SHAPES.items():
        r = np.random.default_rng(0)
        rew = torch.from_numpy((2.0 * r.standard_normal((T, n))).astype(np.float32)).to(dev)
        done = torch.from_numpy((r.random((T, n)) < 0.01).astype(np.uint8)).to(dev)
        out, out_t = torch.zeros_like(rew), torch.zeros_like(rew)
        obj = RetStats(n, GAMMA, dev)
        carry, tot = torch.zeros(n, dtype=torch.float64, device=dev), torch.zeros(3, dtype=torch.float64, device=dev)

        def round_():
            obj.update(rew, done)
            obj.finalize(var_floor=FLOOR)
            obj.apply(rew, out=out, clip=CLIP)

        legs = {"walk": lambda: obj.update(rew, done), "finalize": lambda: obj.finalize(var_floor=FLOOR),
                "apply": lambda: obj.apply(rew, out=out, clip=CLIP), "round": round_,
                "torch_round": lambda: torch_round(rew, done, carry, tot, out_t)}
        warm_up(legs, args.warmup)
        graphs = {}
        for leg, g in legs.items():   # --calls calls of the leg as one graph: no host work between its kernels
            torch.cuda.synchronize(dev)
            graphs[leg] = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graphs[leg]):
                for _ in range(args.calls):
                    g()
            graphs[leg].replay()
        # each leg's eager window, then its graph's, before the next leg's
        both = {(leg, how): f for leg, g in legs.items() for how, f in (("eager", g), ("graph", graphs[leg].replay))}
        both = device_windows(dev, both, args.windows, args.calls, once=[k for k in both if k[1] == "graph"])
        w, wg = ({leg: both[leg, how] for leg in legs} for how in ("eager", "graph"))
        # the two rounds agree to rounding (the sums' order differs): both scales, for the record
        obj.reset()
        carry.zero_()
        tot.zero_()
        round_()
        torch_round(rew, done, carry, tot, out_t)
        m = tot[1] / tot[0]
        res[name] = dict(summary(wg), eager=summary(w), T=T, n=n, calls_per_window=args.calls,
                         unit="us per call in a replayed graph of calls_per_window calls (eager: call by call from Python)",
                         bytes_read_by_walk=T * n * 5, bytes_moved_by_apply=T * n * 8,
                         scale=float(obj.scale.item()), torch_scale=float((1.0 / torch.sqrt(tot[2] / tot[0] - m * m)).item()),
                         max_abs_difference_of_the_scaled_rewards=float((out - out_t).abs().max().item()))
        res[name]["torch_round_over_round"] = res[name]["median"]["torch_round"] / res[name]["median"]["round"]
        obj.close()
    return res


def bench_iterate(args, dev):
    # a second trainer without the option: what two trainers of one process differ by
    legs = {"reward_norm_off": {}, "reward_norm_on": dict(reward_norm=True), "reward_norm_off_second": {}}
    w, finite = pendulum_windows(dev, legs, args.windows, args.iterations, base=BASE)
    assert all(finite.values()), finite
    it = dict(summary(w), trainer=dict(HP, env_id=ENV_ID, envs=ENVS, **BASE),
              unit="ms per PPO.iterate()", iterations_per_window=args.iterations,
              note="reward_norm_on also copies rew_scale out after every iterate(): one launch outside the graph")
    it["on_minus_off_median_ms"] = it["median"]["reward_norm_on"] - it["median"]["reward_norm_off"]
    return it


def main():
    args = parser("ret_stats.json", calls=20, calls_help="calls per timed window of a launch leg",
                  iterations_help="PPO.iterate() calls per timed window").parse_args()
    import torch
    import pybulletgym_amd  # noqa: F401
    dev = torch.device("cuda:0")
    res = dict(launches=bench_launches(args, dev), iterate=bench_iterate(args, dev))
    for name, r in res["launches"].items():
        print(f"{name}: us median [min, max]  " +
              "  ".join(f"{leg} {r['median'][leg]:.1f} [{r['min'][leg]:.1f}, {r['max'][leg]:.1f}] (eager "
                        f"{r['eager']['median'][leg]:.1f})" for leg in r["median"]) +
              f"  torch / hip {r['torch_round_over_round']:.1f}", flush=True)
    it = res["iterate"]
    print("PPO.iterate() ms median [min, max]  " + "  ".join(
        f"{k} {it['median'][k]:.3f} [{it['min'][k]:.3f}, {it['max'][k]:.3f}]" for k in it["median"]), flush=True)
    finish(res, args.out)


if __name__ == "__main__":
    main()
