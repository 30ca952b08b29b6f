#!/usr/bin/env python3
"""The PPO gradient as parts and the data-parallel trainer.  tools/bench_ppo_update.py's shapes
and tools/benchlib.py's protocol (section 11's).

  grad      at the five shapes and on both paths: PPOGrad.run alone in a process ("run"); with --lib PATH (another
            build of libpbg_amd.so, the parent commit's) the parent's PPOGrad.run, likewise alone in a process
            ("parent_run"); and in a third process PPOGrad.run ("run_beside_parts") alternated per window with
            run_part(0, G) + reduce ("parts"), the same two launches with the partials in the caller's buffer.  The
            parent's library has no parts, so its run can only be timed alone; this tree's run is compared with it
            under the same conditions, and what the alternation with a second [G, Dtot] buffer costs run is reported
            beside it.  A library is loaded once per process, so every round is these child processes in turn, the
            parent's first (the legs of two libraries alternate per process, not per window); --rounds rounds.  "run" is compared with "parent_run"
            inside each round -- its median against the parent's window maximum of that round -- and the windows of
            all rounds are pooled for the medians reported.  Per shape and path also G, Dtot and the bytes one minibatch all-gathers,
            G (4 Dtot + 32).
  iterate   the pendulum trainer (256 envs x 32 steps, 4 epochs x 4 minibatches, backward="hip", optimizer="hip",
            permutation="device"): PPO.iterate() in one process beside ShardedPPO.iterate() in two ranks that share
            cuda:0 and exchange through gloo, i.e. through host memory: what the machinery costs when the link is the
            host, not a multi-GPU time (one GPU cannot give one, and the partial gather over RCCL is unmeasured).

  python tools/bench_ppo_sharded.py [--lib PARENT_LIB] [--rounds 2] [--out profiles/ppo_sharded.json]
"""
from __future__ import annotations

import json
import math
import os
import socket
import statistics
import subprocess

from bench_ppo_update import CLIP, ENT_COEF, SHAPES, VF_COEF
from benchlib import (ENV_ID, ENVS, HP, child_cmd, device_windows, finish, last_json, parser, pendulum_windows, run_child,
                      summary, use_library, wall_windows, warm_up)

BASE = dict(backward="hip", optimizer="hip", permutation="device")


def bench_grad(args, dev, parts):
    """Per shape and path the windows of "run" (and "parts" when the library has them), in us per minibatch gradient."""
    import torch
    from pybulletgym_amd.policy import MLPPopulation
    from pybulletgym_amd.ppo import PPOGrad, mlp_forward
    res = {}
    for name in args.shapes:
        dims, B, Bm = SHAPES[name]
        gen = torch.Generator(device=dev)
        gen.manual_seed(0)
        rnd = lambda *s: torch.randn(s, device=dev, generator=gen)  # noqa: E731
        cd = dims[:3] + (1,)
        pa, pc = MLPPopulation(dims, 1, dev), MLPPopulation(cd, 1, dev)
        theta_a, theta_c = pa.init_theta(0), pc.init_theta(1)
        pa.close()
        pc.close()
        log_std = torch.full((dims[3],), -0.5, device=dev)
        obs = rnd(B, dims[0])
        mu, eps = mlp_forward(theta_a, dims, obs), rnd(B, dims[3])
        act = (mu + math.exp(-0.5) * eps).contiguous()
        logp_old = (-0.5 * (eps * eps).sum(1) + 0.5 * dims[3] - 0.5 * dims[3] * math.log(2.0 * math.pi) + 0.15 * rnd(B)).contiguous()
        ret = (mlp_forward(theta_c, cd, obs).squeeze(1) + rnd(B)).contiguous()
        adv = rnd(B)
        idx = torch.randperm(B, device=dev, generator=gen)[:Bm].contiguous()
        a_mb = adv[idx]
        adv_norm = torch.stack((a_mb.mean(), 1.0 / (a_mb.std() + 1e-8)))
        pos = (theta_a, theta_c, log_std, obs, act, logp_old, adv, ret)
        kw = dict(idx=idx, adv_norm=adv_norm, clip_eps=CLIP, vf_coef=VF_COEF, ent_coef=ENT_COEF)
        for path in ("fma", "mfma"):
            g = PPOGrad(dims, Bm, dev, path=path)
            out = dict(grad_actor=torch.zeros(g.Da, device=dev), grad_critic=torch.zeros(g.Dc, device=dev),
                       grad_log_std=torch.zeros(dims[3], device=dev), stats=torch.zeros(4, dtype=torch.float64, device=dev))
            legs = {"run": lambda: g.run(*pos, **out, **kw)}
            rec = {"dims": dims, "minibatch_rows": Bm}
            if parts:
                G, dtot = g.geometry(Bm)
                part = torch.zeros((G, dtot), device=dev)
                part_stats = torch.zeros((G, 4), dtype=torch.float64, device=dev)

                def by_parts():
                    g.run_part(*pos, 0, G, part, part_stats, **kw)
                    g.reduce(*pos, G, part, part_stats, **out, **kw)

                legs["parts"] = by_parts
                rec.update(G=G, Dtot=dtot, bytes_all_gathered_per_minibatch=G * (4 * dtot + 32), launches={"run": 2, "parts": 2})
            warm_up(legs, args.warmup)
            if parts:   # the last leg was "parts": its bits are run's
                got = [t.clone() for t in out.values()]
                legs["run"]()
                torch.cuda.synchronize(dev)
                rec["parts_equal_run_bitwise"] = all(torch.equal(a.view(torch.uint8), b.view(torch.uint8))
                                                     for a, b in zip(got, out.values()))
            rec["windows"] = device_windows(dev, legs, args.windows, args.calls)
            g.close()
            res[f"{name}/{path}"] = rec
    return res


def child(args):
    """One process, one library: its legs' windows as one JSON line."""
    import torch
    use_library(args.lib)
    dev = torch.device("cuda:0")
    if args.child == "grad_run":   # PPOGrad.run alone: what the parent's library can do, under the same conditions
        out = bench_grad(args, dev, False)
    elif args.child == "grad":
        out = bench_grad(args, dev, True)
    elif args.child == "one":
        out = pendulum_windows(dev, {"one_process": BASE}, args.windows, args.iterations)[0]
    else:   # a rank of the two: RANK, WORLD_SIZE, MASTER_ADDR and MASTER_PORT are in the environment
        import torch.distributed as dist
        from pybulletgym_amd.distributed import ShardedVecEnv
        from pybulletgym_amd.ppo import ShardedPPO
        rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
        dist.init_process_group("gloo", init_method="env://", rank=rank, world_size=world)
        shard = ShardedVecEnv(ENV_ID, ENVS, rank, world, dev, seed=0, autoreset=True, precision=64)
        ppo = ShardedPPO(shard, seed=0, **HP)
        for _ in range(3):
            ppo.iterate()
        out = wall_windows(lambda: torch.cuda.synchronize(dev), {f"two_ranks_gloo_rank{rank}": ppo.iterate}, args.windows,
                           args.iterations)
        dist.barrier()
        ppo.close()
        shard.env.close()
        dist.destroy_process_group()
    print(json.dumps(out))


def run_ranks(args, world=2):
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = child_cmd(__file__, "rank", args)
    procs = [subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                              env=dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port)))
             for r in range(world)]
    out, texts = {}, []
    try:
        for p in procs:
            texts.append(p.communicate(timeout=600))
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    for p, (so, se) in zip(procs, texts):
        out.update(last_json(cmd, p.returncode, so, se))
    return out


def main():
    ap = parser("ppo_sharded.json", calls=20, calls_help="gradient calls per timed window",
                iterations_help="iterate() calls per timed window", rounds=2)
    ap.add_argument("--shapes", nargs="*", default=list(SHAPES))
    ap.add_argument("--skip-iterate", action="store_true", help="the gradient legs only")
    args = ap.parse_args()
    if args.child:
        return child(args)
    grad, it = {}, {}
    for _ in range(args.rounds):
        # like with like: the parent's library and this tree's each run PPOGrad.run alone in a process of their own;
        # a third process alternates run and parts per window on this tree ("run_beside_parts", "parts")
        for what, lib, names in ([("grad_run", args.lib, {"run": "parent_run"})] if args.lib else []) + \
                [("grad_run", None, {"run": "run"}), ("grad", None, {"run": "run_beside_parts", "parts": "parts"})]:
            for key, rec in run_child(__file__, what, args, lib).items():
                g = grad.setdefault(key, {"windows": {}, "windows_per_round": {}})
                for leg, v in rec.pop("windows").items():
                    g["windows"].setdefault(names[leg], []).extend(v)
                    g["windows_per_round"].setdefault(names[leg], []).append(v)
                if what == "grad":
                    g.update(rec)
        if not args.skip_iterate:
            for k, v in list(run_child(__file__, "one", args).items()) + list(run_ranks(args).items()):
                it.setdefault(k, []).extend(v)
    res = {"unit": "us per minibatch gradient", "calls_per_window": args.calls, "rounds": args.rounds,
           "parent_library": "another build of libpbg_amd.so, given with --lib" if args.lib else None, "grad": {}}
    for key, g in grad.items():
        r = res["grad"][key] = dict(g, **summary(g["windows"]))
        r["parts_minus_run_beside_parts_median_us"] = r["median"]["parts"] - r["median"]["run_beside_parts"]
        r["run_beside_parts_minus_run_median_us"] = r["median"]["run_beside_parts"] - r["median"]["run"]
        if args.lib:
            # a round is one process per library, the parent's first: the comparison is made inside each round, so that
            # what differs between two processes of one library does not widen the margin; the pooled figure beside it
            pr = g["windows_per_round"]
            r["run_median_minus_parent_maximum_us_per_round"] = [statistics.median(a) - max(b) for a, b in zip(pr["run"], pr["parent_run"])]
            r["run_median_not_above_parent_window_maximum"] = all(d <= 0.0 for d in r["run_median_minus_parent_maximum_us_per_round"])
            r["run_median_not_above_parent_window_maximum_pooled"] = r["median"]["run"] <= r["max"]["parent_run"]
        print(f"{key} x {r['minibatch_rows']}: us median [min, max]  " + "  ".join(
            f"{k} {r['median'][k]:.1f} [{r['min'][k]:.1f}, {r['max'][k]:.1f}]" for k in r["median"]) +
            f"  G {r['G']} gathered {r['bytes_all_gathered_per_minibatch'] / 1e6:.2f} MB" +
            (f"  run median <= parent maximum in every round: {r['run_median_not_above_parent_window_maximum']} "
             f"({', '.join(f'{d:+.1f}' for d in r['run_median_minus_parent_maximum_us_per_round'])} us; pooled "
             f"{r['run_median_not_above_parent_window_maximum_pooled']})" if args.lib else ""), flush=True)
    if it:
        res["iterate"] = r = dict(summary(it), trainer=dict(HP, env_id=ENV_ID, envs=ENVS, **BASE),
                                  unit="ms per iterate()", iterations_per_window=args.iterations,
                                  note="two ranks on one device over gloo: host-staged collectives, not representative of xGMI; "
                                       "no multi-GPU time can be measured on one GPU")
        print("iterate() ms median [min, max]  " + "  ".join(
            f"{k} {r['median'][k]:.2f} [{r['min'][k]:.2f}, {r['max'][k]:.2f}]" for k in r["median"]))
    finish(res, args.out)


if __name__ == "__main__":
    main()
