#!/usr/bin/env python3
"""Population rollout benchmark: what per-member weights cost beside the shared-weight actor.

Float64 Ant at 16,384 envs; each leg a HIP graph of K = 20 closed-loop steps on an env of its own, timed
in one process with tools/bench_rollout.py's protocol (pre-roll, warm replay, five windows bracketed by
device events, the legs alternated per window):

  A  VecEnv.rollout(MLPPolicy): one weight set for every env (pbg_rollout, the baseline)
  B  VecEnv.rollout(MLPPopulation) at 1,024 members x 16 envs (pbg_rollout_population)
  C  the same at 4,096 members x 4 envs: a quarter-filled 16-env tile per member

Every member holds the pretrained Ant weights the baseline runs, so the three legs compute the same
actions from the same states (asserted on the final observations) and differ only in where the actor
reads its weights from: one 49 KB set through L2, or one set per member from HBM.

Also measured: a device-to-device copy's bandwidth on the same box (the yardstick for the actor's weight
stream) and the once-per-generation work outside the rollout (perturb + fitness + ranks + grad + update,
one HIP graph) at 512 pairs.

With --obs-norm the rollout legs are A and B, each of them again with a normaliser applied (`_norm`) and
again with a normaliser applied and observation statistics collected (`_norm_stats`, an ObsStats attached
to the actor), written to profiles/obs_norm_rollout.json.  The normaliser is the identity (mean 0, inv_std
1, a clip no observation reaches): the same three float32 operations per loaded element as any other, and
all six legs stay in the same state bit for bit (asserted on the final observations).

With --action-noise the rollout legs are A and B, each of them again with an ActionNoise of std zero attached
(`_noise`: the sampling actor's whole work, the same states), and pbg_gae at T = 200 is set against the torch
loop it replaces; written to profiles/action_noise_rollout.json.  --lib runs the legs a library has against
another build of libpbg_amd.so (the parent commit's, alternated with this tree's in one session).

  python tools/bench_population.py [--out profiles/population_rollout.json]
  python tools/bench_population.py --obs-norm [--out profiles/obs_norm_rollout.json]
  python tools/bench_population.py --action-noise [--lib PATH] [--out profiles/action_noise_rollout.json]
  python tools/bench_population.py --actor-only [--members 1024]   # actor launches alone, for a kernel trace
"""
from __future__ import annotations

import os
import statistics
import sys

from benchlib import REPO, capture, device_windows, finish, parser, summary, use_library

sys.path.insert(0, os.path.join(REPO, "tests"))

ENV_ID, N = "AntPyBulletEnv-v0", 16384
K = 20  # steps per graph
LEGS = {"A": None, "B": 1024, "C": 4096}  # members (None: the shared-weight policy)


def actors(dev, members):
    """The pretrained Ant policy as an MLPPolicy and as populations whose members all hold its weights."""
    import torch
    import policies
    from pybulletgym_amd.policy import MLPPolicy, MLPPopulation, pack_theta
    ws = policies.Policy(ENV_ID).w
    dims = (ws[0].shape[0], ws[0].shape[1], ws[2].shape[1], ws[4].shape[1])
    theta = torch.from_numpy(pack_theta(ws)).to(dev)
    out = {}
    for leg, m in members.items():
        if m is None:
            out[leg] = MLPPolicy(*ws, device=dev)
        else:
            out[leg] = MLPPopulation(dims, m // 2, dev)
            out[leg].set_all(theta)
    return out, dims, theta


def replay_windows(args, dev, graphs):
    """us per step of the K-step graphs, after one warm replay of each."""
    return device_windows(dev, {leg: g.replay for leg, g in graphs.items()}, args.windows, args.replays, warmup=1, per=K)


def bench_rollout(args, dev):
    import torch
    from pybulletgym_amd.vec_env import VecEnv
    pis, dims, _ = actors(dev, LEGS)
    envs = {leg: VecEnv(ENV_ID, N, device=dev, seed=0, autoreset=True, precision=64) for leg in LEGS}
    for e in envs.values():
        e.reset()
    pre = (args.preroll + args.warmup + K - 1) // K
    for _ in range(pre):
        for leg in LEGS:
            envs[leg].rollout(pis[leg], K)
    torch.cuda.synchronize(dev)
    graphs = {leg: capture(lambda leg=leg: envs[leg].rollout(pis[leg], K), dev) for leg in LEGS}
    w = replay_windows(args, dev, graphs)
    out = summary(w)
    med = out["median"]
    D = pis["B"].n_params
    out.update({"env_id": ENV_ID, "n_envs": N, "precision": 64, "steps_per_graph": K, "replays_per_window": args.replays,
                "unit": "us per env-batch step", "members": LEGS, "mlp_dims": dims, "params_per_member": D,
                "B_minus_A_us": med["B"] - med["A"], "C_minus_A_us": med["C"] - med["A"],
                # every member holds A's weights: the three envs must be in the same state, bit for bit
                "final_obs_equal": bool(torch.equal(envs["A"].obs, envs["B"].obs) and
                                        torch.equal(envs["A"].obs, envs["C"].obs)),
                "actor_weight_bytes_per_step": {leg: (1 if m is None else m * ((N // m + 15) // 16)) * D * 4
                                                for leg, m in LEGS.items()}})
    for e in envs.values():
        e.close()
    for p in pis.values():
        p.close()
    return out


NORM_LEGS = {"A": (None, ""), "B": (1024, ""), "A_norm": (None, "norm"), "B_norm": (1024, "norm"),
             "A_norm_stats": (None, "norm+stats"), "B_norm_stats": (1024, "norm+stats")}


def bench_obs_norm(args, dev):
    """Legs A and B of bench_rollout, each plain, with a normaliser, and with a normaliser and statistics."""
    import torch
    from pybulletgym_amd.policy import ObsStats
    from pybulletgym_amd.vec_env import VecEnv
    pis, dims, _ = actors(dev, {leg: m for leg, (m, _) in NORM_LEGS.items()})
    mean, inv_std = torch.zeros(dims[0], device=dev), torch.ones(dims[0], device=dev)
    stats = {}
    for leg, (m, mode) in NORM_LEGS.items():
        if "norm" in mode:
            pis[leg].set_obs_norm(mean, inv_std, clip=1e30)
        if "stats" in mode:
            stats[leg] = ObsStats(dims[0], N, group=None if m is None else N // m, device=dev)
            pis[leg].attach_obs_stats(stats[leg])
    envs = {leg: VecEnv(ENV_ID, N, device=dev, seed=0, autoreset=True, precision=64) for leg in NORM_LEGS}
    for e in envs.values():
        e.reset()
    pre = (args.preroll + args.warmup + K - 1) // K
    for _ in range(pre):
        for leg in NORM_LEGS:
            envs[leg].rollout(pis[leg], K)
    torch.cuda.synchronize(dev)
    graphs = {leg: capture(lambda leg=leg: envs[leg].rollout(pis[leg], K), dev) for leg in NORM_LEGS}
    w = replay_windows(args, dev, graphs)
    out = summary(w)
    med = out["median"]
    counted = {}
    for leg, st in stats.items():
        st.finalize()
        counted[leg] = float(st.totals[0]) - 1e-2
    out.update({"env_id": ENV_ID, "n_envs": N, "precision": 64, "steps_per_graph": K, "replays_per_window": args.replays,
                "unit": "us per env-batch step", "legs": {leg: {"members": m, "mode": mode or "plain"}
                                                          for leg, (m, mode) in NORM_LEGS.items()},
                "mlp_dims": dims, "normaliser": "identity (mean 0, inv_std 1, clip 1e30)",
                "delta_us": {leg: med[leg] - med[leg[0]] for leg in NORM_LEGS if leg not in ("A", "B")},
                "parent_leg_spread_us": {leg: out["max"][leg] - out["min"][leg] for leg in ("A", "B")},
                "observations_counted": counted,
                "final_obs_equal": bool(all(torch.equal(envs["A"].obs, envs[leg].obs) for leg in NORM_LEGS))})
    for e in envs.values():
        e.close()
    for p in pis.values():
        p.attach_obs_stats(None)
        p.close()
    for st in stats.values():
        st.close()
    return out


NOISE_LEGS = {"A": (None, False), "B": (1024, False), "A_noise": (None, True), "B_noise": (1024, True)}


def bench_action_noise(args, dev):
    """Legs A and B of bench_rollout, each plain and with an ActionNoise attached.  The noise's std is zero (a
    fresh object's): every sampled action is mu + 0 eps = mu through the same Philox block, Box-Muller pair,
    LDS round trip, barrier and float64 multiply-add as under any other std, and all four legs stay in the same
    state bit for bit (asserted on the final observations).  A library without the action noise (--lib, a
    build of the parent commit) runs the plain legs only."""
    import torch
    from pybulletgym_amd import _native
    from pybulletgym_amd.policy import ActionNoise
    from pybulletgym_amd.vec_env import VecEnv
    has = hasattr(_native.lib(), "pbg_action_noise_create")
    legs = {leg: v for leg, v in NOISE_LEGS.items() if has or not v[1]}
    pis, dims, _ = actors(dev, {leg: m for leg, (m, _) in legs.items()})
    noises = {}
    for leg, (m, sample) in legs.items():
        if sample:
            noises[leg] = ActionNoise(dims[3], 0, dev)
            pis[leg].attach_action_noise(noises[leg])
    envs = {leg: VecEnv(ENV_ID, N, device=dev, seed=0, autoreset=True, precision=64) for leg in legs}
    for e in envs.values():
        e.reset()
    pre = (args.preroll + args.warmup + K - 1) // K
    for _ in range(pre):
        for leg in legs:
            envs[leg].rollout(pis[leg], K)
    torch.cuda.synchronize(dev)
    graphs = {leg: capture(lambda leg=leg: envs[leg].rollout(pis[leg], K), dev) for leg in legs}
    w = replay_windows(args, dev, graphs)
    out = summary(w)
    med = out["median"]
    out.update({"env_id": ENV_ID, "n_envs": N, "precision": 64, "steps_per_graph": K, "replays_per_window": args.replays,
                "unit": "us per env-batch step", "library": os.path.relpath(_native.LIB_PATH, REPO),
                "legs": {leg: {"members": m, "mode": "sampling" if s else "plain"} for leg, (m, s) in legs.items()},
                "mlp_dims": dims, "std": "zero (mu + 0 eps: the same operations, the same states)",
                "delta_us": {leg: med[leg] - med[leg[0]] for leg in legs if legs[leg][1]},
                "plain_leg_spread_us": {leg: out["max"][leg] - out["min"][leg] for leg in ("A", "B")},
                "steps_sampled": {leg: z.counter for leg, z in noises.items()},
                "final_obs_equal": bool(all(torch.equal(envs["A"].obs, envs[leg].obs) for leg in legs))})
    for e in envs.values():
        e.close()
    for leg, p in pis.items():
        if leg in noises:
            p.attach_action_noise(None)
        p.close()
    for z in noises.values():
        z.close()
    return out


def gae_torch_loop(rew, done, value, gamma, lam):
    """The chain of small torch kernels pbg_gae replaces: T steps of about six launches each."""
    import torch
    T = rew.shape[0]
    adv, ret = torch.empty_like(rew), torch.empty_like(rew)
    A = torch.zeros_like(value[0], dtype=torch.float64)
    for t in range(T - 1, -1, -1):
        nd = 1.0 - done[t].double()
        v = value[t].double()
        delta = rew[t].double() + gamma * value[t + 1].double() * nd - v
        A = delta + gamma * lam * nd * A
        adv[t] = A.float()
        ret[t] = (A + v).float()
    return adv, ret


def bench_gae(args, dev, T=200):
    """pbg_gae at T = 200, n = 16,384 beside the torch loop it replaces (eager launches, as a learner would run it)."""
    import torch
    from pybulletgym_amd.ppo import gae
    g = torch.Generator(device=dev)
    g.manual_seed(0)
    rew = torch.randn((T, N), device=dev, generator=g)
    value = torch.randn((T + 1, N), device=dev, generator=g)
    done = (torch.rand((T, N), device=dev, generator=g) < 0.01).to(torch.uint8)
    adv, ret = torch.empty_like(rew), torch.empty_like(rew)
    runs = {"pbg_gae": lambda: gae(rew, done, value, 0.99, 0.95, adv=adv, ret=ret),
            "torch_loop": lambda: gae_torch_loop(rew, done, value, 0.99, 0.95)}
    for f in runs.values():
        f()
    ta, tr = runs["torch_loop"]()
    runs["pbg_gae"]()
    err = max(float((ta - adv).abs().max()), float((tr - ret).abs().max()))
    w = device_windows(dev, runs, args.windows, 5)
    out = summary(w)
    out.update({"T": T, "n": N, "unit": "us per call", "max_abs_difference_from_the_torch_loop": err,
                "bytes_touched": T * N * (4 + 1 + 4 + 4 + 4) + N * 4,
                "speedup_median": out["median"]["torch_loop"] / out["median"]["pbg_gae"]})
    return out


def bench_copy(args, dev):
    """Device-to-device copy of 1 GiB: bytes read plus bytes written over the time."""
    import torch
    n = 1 << 28
    a = torch.empty(n, dtype=torch.float32, device=dev).normal_()
    b = torch.empty_like(a)
    for _ in range(3):
        b.copy_(a)
    w = device_windows(dev, {"copy": lambda: b.copy_(a)}, args.windows, 10)["copy"]
    gbs = [2 * 4 * n / (us * 1e-6) / 1e9 for us in w]
    return {"bytes_each_way": 4 * n, "us": w, "GB_per_s_read_plus_write": {"median": statistics.median(gbs),
                                                                           "min": min(gbs), "max": max(gbs)}}


def bench_generation(args, dev):
    """perturb + fitness + centred ranks + grad + the centre's update at 512 pairs x 16 envs, one graph."""
    import torch
    from pybulletgym_amd.es import EvolutionStrategy
    from pybulletgym_amd.vec_env import VecEnv
    pis, dims, theta = actors(dev, {"B": 1024})
    pop = pis["B"]
    env = VecEnv(ENV_ID, N, device=dev, seed=0, autoreset=True, precision=64)
    env.reset()
    es = EvolutionStrategy(env, pop, sigma=0.02, lr=0.01, steps=K, seed=0)
    es.theta.copy_(theta)
    res = env.rollout(pop, K, fresh=True)

    def generation():
        pop.perturb(es.theta, es.sigma, es.seed, 0)
        es.update(res, 0)

    generation()
    torch.cuda.synchronize(dev)
    g = capture(generation, dev)
    w = device_windows(dev, {"generation": g.replay}, args.windows, 20, warmup=1)["generation"]
    out = {"n_pairs": pop.n_pairs, "params": pop.n_params, "unit": "us per generation (without the rollout)", "us": w,
           "median": statistics.median(w), "min": min(w), "max": max(w)}
    env.close()
    pop.close()
    return out


def actor_only(args, dev):
    """Launches of the actor alone at n = 16,384 (run under a kernel trace): actor_kernel with one member
    (the shared-weight policy) and at --members."""
    import torch
    pis, dims, _ = actors(dev, {"A": None, "P": args.members})
    obs = torch.randn((N, dims[0]), device=dev)
    out = torch.empty((N, dims[3]), device=dev)
    for _ in range(50):
        pis["A"].act(obs, out=out)
        pis["P"].act(obs, out=out)
    torch.cuda.synchronize(dev)
    print(f"actor-only done: actor_kernel with one member x {N} and at {args.members} members x {N // args.members}")


def main():
    ap = parser(None, warmup=20)   # --out: profiles/population_rollout.json, obs_norm_rollout.json, action_noise_rollout.json
    ap.add_argument("--obs-norm", action="store_true", help="the observation-normalisation legs only")
    ap.add_argument("--action-noise", action="store_true", help="the action-noise legs and pbg_gae only")
    ap.add_argument("--lib", default=None, help="another build of libpbg_amd.so (the parent commit's, to alternate with)")
    ap.add_argument("--preroll", type=int, default=200)
    ap.add_argument("--replays", type=int, default=10, help="graph replays (of 20 steps) per timed window")
    ap.add_argument("--actor-only", action="store_true")
    ap.add_argument("--members", type=int, default=1024)
    args = ap.parse_args()
    import torch
    use_library(args.lib)
    dev = torch.device("cuda:0")
    if args.actor_only:
        return actor_only(args, dev)
    if args.out is None:
        name = "action_noise_rollout.json" if args.action_noise else \
            "obs_norm_rollout.json" if args.obs_norm else "population_rollout.json"
        args.out = os.path.join(REPO, "profiles", name)
    if args.action_noise:
        from pybulletgym_amd import _native
        res = {"rollout": bench_action_noise(args, dev)}
        if hasattr(_native.lib(), "pbg_gae"):
            res["gae"] = bench_gae(args, dev)
        r = res["rollout"]
        print("rollout us/step median [min, max]: " + "  ".join(
            f"{leg} {r['median'][leg]:.1f} [{r['min'][leg]:.1f}, {r['max'][leg]:.1f}]" for leg in r["median"]) +
            f"  same states: {r['final_obs_equal']}")
        if "gae" in res:
            g = res["gae"]
            print("gae us/call median [min, max]: " + "  ".join(
                f"{k} {g['median'][k]:.1f} [{g['min'][k]:.1f}, {g['max'][k]:.1f}]" for k in g["median"]))
        return finish(res, args.out, bool(r["final_obs_equal"]))
    if args.obs_norm:
        res = {"rollout": bench_obs_norm(args, dev)}
        r = res["rollout"]
        print("rollout us/step median [min, max]: " + "  ".join(
            f"{leg} {r['median'][leg]:.1f} [{r['min'][leg]:.1f}, {r['max'][leg]:.1f}]" for leg in NORM_LEGS) +
            f"  same states: {r['final_obs_equal']}")
        return finish(res, args.out, bool(r["final_obs_equal"]))
    res = {"rollout": bench_rollout(args, dev), "copy": bench_copy(args, dev), "generation": bench_generation(args, dev)}
    bw = res["copy"]["GB_per_s_read_plus_write"]["median"]
    res["actor_weight_stream_at_copy_bandwidth_us"] = {
        leg: b / (bw * 1e9) * 1e6 for leg, b in res["rollout"]["actor_weight_bytes_per_step"].items()}
    r = res["rollout"]
    print("rollout us/step median [min, max]: " + "  ".join(
        f"{leg} {r['median'][leg]:.1f} [{r['min'][leg]:.1f}, {r['max'][leg]:.1f}]" for leg in LEGS) +
        f"  B-A {r['B_minus_A_us']:.1f}  C-A {r['C_minus_A_us']:.1f}  same states: {r['final_obs_equal']}")
    print(f"copy {bw:.0f} GB/s (read + write)  generation {res['generation']['median']:.1f} us")
    finish(res, args.out, bool(r["final_obs_equal"]))


if __name__ == "__main__":
    main()
