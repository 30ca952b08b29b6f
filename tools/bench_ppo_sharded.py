#!/usr/bin/env python3
"""The PPO gradient as parts and the data-parallel trainer.  tools/bench_ppo_update.py's shapes
and section 11's protocol: warm-up, five windows bracketed by device events (iterate: a host clock around a
synchronise), the legs alternated per window, medians with [min, max].

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

import argparse
import json
import math
import os
import socket
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

from bench_ppo_update import CLIP, ENT_COEF, SHAPES, VF_COEF  # noqa: E402

HP = dict(hidden=(64, 64), steps=32, lr=3e-3, epochs=4, minibatches=4, log_std=-0.5)
ENV_ID, ENVS = "InvertedPendulumPyBulletEnv-v0", 256


def summary(w):
    return {"windows": w, "median": {k: statistics.median(v) for k, v in w.items()}, "min": {k: min(v) for k, v in w.items()},
            "max": {k: max(v) for k, v in w.items()}}


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
            for _ in range(args.warmup):
                for f in legs.values():
                    f()
            if parts:   # the last leg was "parts": its bits are run's
                got = [t.clone() for t in out.values()]
                legs["run"]()
                torch.cuda.synchronize(dev)
                rec["parts_equal_run_bitwise"] = all(torch.equal(a.view(torch.uint8), b.view(torch.uint8))
                                                     for a, b in zip(got, out.values()))
            stream = torch.cuda.current_stream(dev)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            w = {leg: [] for leg in legs}
            for _ in range(args.windows):
                for leg, f in legs.items():
                    torch.cuda.synchronize(dev)
                    e0.record(stream)
                    for _ in range(args.calls):
                        f()
                    e1.record(stream)
                    torch.cuda.synchronize(dev)
                    w[leg].append(e0.elapsed_time(e1) * 1e3 / args.calls)
            g.close()
            rec["windows"] = w
            res[f"{name}/{path}"] = rec
    return res


def time_iterate(args, ppo, dev):
    import torch
    for _ in range(3):
        ppo.iterate()
    w = []
    for _ in range(args.windows):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(args.iterations):
            ppo.iterate()
        torch.cuda.synchronize(dev)
        w.append((time.perf_counter() - t0) * 1e3 / args.iterations)
    return w


def child(args):
    """One process, one library: its legs' windows as one JSON line."""
    import torch
    import pybulletgym_amd  # noqa: F401
    from pybulletgym_amd import _native
    if args.lib:
        _native.LIB_PATH = os.path.abspath(args.lib)
    dev = torch.device("cuda:0")
    if args.child == "grad_run":   # PPOGrad.run alone: what the parent's library can do, under the same conditions
        out = bench_grad(args, dev, False)
    elif args.child == "grad":
        out = bench_grad(args, dev, True)
    elif args.child == "one":
        from pybulletgym_amd.ppo import PPO
        from pybulletgym_amd.vec_env import VecEnv
        env = VecEnv(ENV_ID, ENVS, device=dev, seed=0, autoreset=True, precision=64)
        ppo = PPO(env, seed=0, backward="hip", optimizer="hip", permutation="device", **HP)
        out = {"one_process": time_iterate(args, ppo, dev)}
        ppo.close()
        env.close()
    else:   # a rank of the two: RANK, WORLD_SIZE, MASTER_ADDR and MASTER_PORT are in the environment
        import torch.distributed as dist
        from pybulletgym_amd.distributed import ShardedVecEnv
        from pybulletgym_amd.ppo import ShardedPPO
        rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
        dist.init_process_group("gloo", init_method="env://", rank=rank, world_size=world)
        shard = ShardedVecEnv(ENV_ID, ENVS, rank, world, dev, seed=0, autoreset=True, precision=64)
        ppo = ShardedPPO(shard, seed=0, **HP)
        out = {f"two_ranks_gloo_rank{rank}": time_iterate(args, ppo, dev)}
        dist.barrier()
        ppo.close()
        shard.env.close()
        dist.destroy_process_group()
    print(json.dumps(out))


def child_cmd(args, what, lib=None):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", what, "--warmup", str(args.warmup), "--windows", str(args.windows),
           "--calls", str(args.calls), "--iterations", str(args.iterations), "--shapes"] + list(args.shapes)
    return cmd + (["--lib", lib] if lib else [])


def last_json(p, cmd):
    if p.returncode:
        raise RuntimeError(f"{' '.join(cmd)} failed ({p.returncode}):\n{p.stderr[-3000:]}")
    return json.loads(p.stdout.strip().splitlines()[-1])


def run_child(args, what, lib=None):
    cmd = child_cmd(args, what, lib)
    return last_json(subprocess.run(cmd, capture_output=True, text=True, timeout=600), cmd)


def run_ranks(args, world=2):
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = child_cmd(args, "rank")
    procs = [subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                              env=dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port)))
             for r in range(world)]
    out = {}
    try:
        for p in procs:
            so, se = p.communicate(timeout=600)
            p.stdout_text, p.stderr_text = so, se
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    for p in procs:
        if p.returncode:
            raise RuntimeError(f"a rank failed ({p.returncode}):\n{p.stderr_text[-3000:]}")
        out.update(json.loads(p.stdout_text.strip().splitlines()[-1]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "ppo_sharded.json"))
    ap.add_argument("--lib", default=None, help="another build of libpbg_amd.so (the parent commit's, to alternate with)")
    ap.add_argument("--rounds", type=int, default=2, help="child processes per library")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20, help="gradient calls per timed window")
    ap.add_argument("--iterations", type=int, default=5, help="iterate() calls per timed window")
    ap.add_argument("--shapes", nargs="*", default=list(SHAPES))
    ap.add_argument("--skip-iterate", action="store_true", help="the gradient legs only")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    grad, it = {}, {}
    for _ in range(args.rounds):
        # like with like: the parent's library and this tree's each run PPOGrad.run alone in a process of their own;
        # a third process alternates run and parts per window on this tree ("run_beside_parts", "parts")
        for what, lib, names in ([("grad_run", args.lib, {"run": "parent_run"})] if args.lib else []) + \
                [("grad_run", None, {"run": "run"}), ("grad", None, {"run": "run_beside_parts", "parts": "parts"})]:
            for key, rec in run_child(args, what, lib).items():
                g = grad.setdefault(key, {"windows": {}, "windows_per_round": {}})
                for leg, v in rec.pop("windows").items():
                    g["windows"].setdefault(names[leg], []).extend(v)
                    g["windows_per_round"].setdefault(names[leg], []).append(v)
                if what == "grad":
                    g.update(rec)
        if not args.skip_iterate:
            for k, v in list(run_child(args, "one").items()) + list(run_ranks(args).items()):
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
        res["iterate"] = r = dict(summary(it), trainer=dict(HP, env_id=ENV_ID, envs=ENVS, backward="hip", optimizer="hip",
                                                            permutation="device"),
                                  unit="ms per iterate()", iterations_per_window=args.iterations,
                                  note="two ranks on one device over gloo: host-staged collectives, not representative of xGMI; "
                                       "no multi-GPU time can be measured on one GPU")
        print("iterate() ms median [min, max]  " + "  ".join(
            f"{k} {r['median'][k]:.2f} [{r['min'][k]:.2f}, {r['max'][k]:.2f}]" for k in r["median"]))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({"done": True, "out": args.out}))


if __name__ == "__main__":
    main()
