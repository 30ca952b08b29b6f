#!/usr/bin/env python3
"""The PPO update's gradient: torch autograd beside pbg_ppo_grad (DESIGN.md sections 14 and 17).

Three legs compute one minibatch's gradient from the same data, eager launches as the trainer issues them:

  torch     the body of PPO.update from the gather to loss.backward() (ppo.py's torch path)
  hip       PPOGrad.run: the tile kernel and the reduction (plus the two torch reductions that form adv_norm)
  hip_mfma  the same with PPOGrad(path="mfma"), the matrix-core path

at five shapes: the pendulum trainer's (5, 64, 64, 1) with 2,048 rows of 8,192, Ant's (28, 64, 64, 8) with
131,072 rows of 524,288, (44, 256, 256, 17) with 16,384 rows of 65,536, and the two reference networks, Ant's
(28, 128, 64, 8) with 131,072 rows of 524,288 and Humanoid's (44, 256, 128, 17) with 16,384 rows of 65,536.  Then
(unless --skip-iterate) one whole PPO.iterate() of the
pendulum trainer (256 envs x 32 steps, 4 epochs x 4 minibatches) in both modes.  tools/benchlib.py's protocol (section
11's).  The FLOP count is the algorithm's: per row and network 2 K H for each layer's
forward, 2 K H for its weight gradient and 2 K H for the input gradient of layers two and three.

  python tools/bench_ppo_update.py [--out profiles/ppo_grad_mfma.json] [--shapes wide ant_ref ...] [--skip-iterate]

profiles/ppo_grad.json is the record of the two-leg version of this tool (section 14) and is not rewritten.
"""
from __future__ import annotations

import math

from benchlib import ENV_ID, ENVS, HP, device_windows, finish, parser, pendulum_windows, summary, warm_up

SHAPES = {"pendulum": ((5, 64, 64, 1), 8192, 2048), "ant": ((28, 64, 64, 8), 524288, 131072),
          "wide": ((44, 256, 256, 17), 65536, 16384), "ant_ref": ((28, 128, 64, 8), 524288, 131072),
          "humanoid_ref": ((44, 256, 128, 17), 65536, 16384)}
PEAK_FP32_TF = 157.0
CLIP, VF_COEF, ENT_COEF = 0.2, 0.5, 0.0


def flops_per_row(dims):
    o, h1, h2, a = dims
    total = 0
    for out in (a, 1):
        layers = (o * h1, h1 * h2, h2 * out)
        total += 2 * sum(layers) * 2 + 2 * (layers[1] + layers[2])
    return total


def torch_gradient(theta_a, theta_c, log_std, dims, obs, act, logp_old, adv, ret, idx):
    """ppo.py's torch path for one minibatch."""
    import torch
    from pybulletgym_amd.ppo import mlp_forward
    A = dims[3]
    a_mb = adv[idx]
    a_mb = (a_mb - a_mb.mean()) / (a_mb.std() + 1e-8)
    mu = mlp_forward(theta_a, dims, obs[idx], None)
    v = mlp_forward(theta_c, dims[:3] + (1,), obs[idx], None).squeeze(1)
    z = (act[idx] - mu) * torch.exp(-log_std)
    logp = -0.5 * (z * z).sum(1) - log_std.sum() - 0.5 * A * math.log(2.0 * math.pi)
    ratio = torch.exp(logp - logp_old[idx])
    pg = -torch.min(ratio * a_mb, torch.clamp(ratio, 1.0 - CLIP, 1.0 + CLIP) * a_mb).mean()
    vf = 0.5 * ((v - ret[idx]) ** 2).mean()
    entropy = log_std.sum() + 0.5 * A * (1.0 + math.log(2.0 * math.pi))
    loss = pg + VF_COEF * vf - ENT_COEF * entropy
    for p in (theta_a, theta_c, log_std):
        p.grad = None
    loss.backward()


def bench_shape(name, dims, B, Bm, args, dev):
    import torch
    from pybulletgym_amd.policy import MLPPopulation
    from pybulletgym_amd.ppo import PPOGrad, mlp_forward
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    rnd = lambda *s: torch.randn(s, device=dev, generator=gen)  # noqa: E731
    cd = dims[:3] + (1,)
    pa, pc = MLPPopulation(dims, 1, dev), MLPPopulation(cd, 1, dev)
    theta_a, theta_c = torch.nn.Parameter(pa.init_theta(0)), torch.nn.Parameter(pc.init_theta(1))
    pa.close()
    pc.close()
    log_std = torch.nn.Parameter(torch.full((dims[3],), -0.5, device=dev))
    obs = rnd(B, dims[0])
    with torch.no_grad():
        mu = mlp_forward(theta_a, dims, obs)
        eps = rnd(B, dims[3])
        act = (mu + math.exp(-0.5) * eps).contiguous()
        logp_old = (-0.5 * (eps * eps).sum(1) + 0.5 * dims[3] - 0.5 * dims[3] * math.log(2.0 * math.pi) + 0.15 * rnd(B)).contiguous()
        ret = (mlp_forward(theta_c, cd, obs).squeeze(1) + rnd(B)).contiguous()
    adv = rnd(B)
    idx = torch.randperm(B, device=dev, generator=gen)[:Bm].contiguous()
    g, gm = PPOGrad(dims, Bm, dev), PPOGrad(dims, Bm, dev, path="mfma")
    ga, gc, gl = torch.zeros_like(theta_a.data), torch.zeros_like(theta_c.data), torch.zeros_like(log_std.data)
    stats = torch.zeros(4, dtype=torch.float64, device=dev)

    def hip(obj=g):
        a_mb = adv[idx]
        adv_norm = torch.stack((a_mb.mean(), 1.0 / (a_mb.std() + 1e-8)))
        obj.run(theta_a.data, theta_c.data, log_std.data, obs, act, logp_old, adv, ret, idx=idx, adv_norm=adv_norm, clip_eps=CLIP,
                vf_coef=VF_COEF, ent_coef=ENT_COEF, grad_actor=ga, grad_critic=gc, grad_log_std=gl, stats=stats)

    legs = {"torch": lambda: torch_gradient(theta_a, theta_c, log_std, dims, obs, act, logp_old, adv, ret, idx), "hip": hip,
            "hip_mfma": lambda: hip(gm)}
    rel = lambda: max(float((x - p.grad).abs().max() / p.grad.abs().max())  # noqa: E731
                      for x, p in ((ga, theta_a), (gc, theta_c), (gl, log_std)))
    warm_up(legs, args.warmup)
    # ga, gc, gl hold the last leg's result: the matrix-core path's; then the FMA path's once more
    torch.cuda.synchronize(dev)
    diff_mfma = rel()
    hip()
    torch.cuda.synchronize(dev)
    diff = rel()
    s = summary(device_windows(dev, legs, args.windows, args.calls))
    g.close()
    gm.close()
    w, med = s["windows"], s["median"]
    fl = flops_per_row(dims) * Bm
    return {"dims": dims, "batch_rows": B, "minibatch_rows": Bm, "unit": "us per minibatch gradient", "windows": w, "median": med,
            "min": s["min"], "max": s["max"],
            "torch_over_hip": med["torch"] / med["hip"], "torch_over_hip_mfma": med["torch"] / med["hip_mfma"],
            "hip_over_hip_mfma": med["hip"] / med["hip_mfma"],
            "hip_mfma_median_below_hip_window_minimum": med["hip_mfma"] < min(w["hip"]), "flops_per_minibatch": fl,
            "achieved_TFLOPs": {k: fl / (us * 1e-6) / 1e12 for k, us in med.items()},
            "share_of_fp32_peak": {k: fl / (us * 1e-6) / 1e12 / PEAK_FP32_TF for k, us in med.items()},
            "max_relative_difference_of_the_gradients": diff,
            "max_relative_difference_of_the_gradients_mfma": diff_mfma, "calls_per_window": args.calls}


def bench_iterate(args, dev):
    modes = {"torch": dict(backward="torch"), "hip": dict(backward="hip"), "hip_mfma": dict(backward="hip", grad_path="mfma")}
    s = summary(pendulum_windows(dev, modes, args.windows, args.iterations)[0])
    return {"trainer": dict(HP, env_id=ENV_ID, envs=ENVS), "unit": "ms per PPO.iterate()", "windows": s["windows"],
            "median": s["median"], "min": s["min"], "max": s["max"],
            "torch_over_hip": s["median"]["torch"] / s["median"]["hip"], "iterations_per_window": args.iterations}


def main():
    ap = parser("ppo_grad_mfma.json", calls=20, calls_help="gradient calls per timed window",
                iterations_help="PPO.iterate() calls per timed window")
    ap.add_argument("--shapes", nargs="*", default=list(SHAPES))
    ap.add_argument("--skip-iterate", action="store_true", help="the gradient legs only")
    args = ap.parse_args()
    import torch
    import pybulletgym_amd  # noqa: F401
    dev = torch.device("cuda:0")
    res = {"peak_fp32_TFLOPs": PEAK_FP32_TF, "shapes": {}}
    for name in args.shapes:
        res["shapes"][name] = r = bench_shape(name, *SHAPES[name], args, dev)
        print(f"{name} {r['dims']} x {r['minibatch_rows']}: us median [min, max]  " + "  ".join(
            f"{k} {r['median'][k]:.1f} [{r['min'][k]:.1f}, {r['max'][k]:.1f}] ({r['achieved_TFLOPs'][k]:.2f} TF)"
            for k in r["median"]) + f"  torch / hip {r['torch_over_hip']:.2f}  torch / hip_mfma {r['torch_over_hip_mfma']:.2f}  "
            f"grad diff {r['max_relative_difference_of_the_gradients']:.1e} (mfma {r['max_relative_difference_of_the_gradients_mfma']:.1e})",
            flush=True)
    if not args.skip_iterate:
        res["iterate"] = r = bench_iterate(args, dev)
        print("PPO.iterate() ms median [min, max]  " + "  ".join(
            f"{k} {r['median'][k]:.2f} [{r['min'][k]:.2f}, {r['max'][k]:.2f}]" for k in r["median"]) +
            f"  torch / hip {r['torch_over_hip']:.2f}")
    finish(res, args.out)


if __name__ == "__main__":
    main()
