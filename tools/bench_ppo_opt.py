#!/usr/bin/env python3
"""One whole PPO minibatch step (advantage normaliser + gradient + clip + Adam): torch beside the library's launches
(DESIGN.md section 15).  tools/bench_ppo_update.py's protocol and shapes.

Legs of one minibatch step from the same data, eager launches as the trainer issues them:

  torch       torch autograd, clip_grad_norm_, torch.optim.Adam               (PPO(backward="torch"))
  hip_grad    the torch reductions behind adv_norm, PPOGrad.run, clip_grad_norm_, Adam   (backward="hip")
  hip         adv_norm, PPOGrad.run, AdamClip.step: five launches             (backward="hip", optimizer="hip")
  adv_norm    pbg_adv_norm alone
  opt_step    pbg_ppo_opt_step alone (bytes/s: 7 floats read or written per element)

Then one whole PPO.iterate() of the pendulum trainer (256 envs x 32 steps, 4 epochs x 4 minibatches), all with
backward="hip": optimizer="torch", optimizer="hip", and optimizer="hip" with graph=True.  tools/benchlib.py's protocol.

  python tools/bench_ppo_opt.py [--out profiles/ppo_opt.json]
"""
from __future__ import annotations

import math

import bench_ppo_update as base
from benchlib import ENV_ID, ENVS, HP, device_windows, finish, parser, pendulum_windows, summary

LR, EPS, MAX_GRAD_NORM = 1e-5, 1e-5, 0.5   # a small lr: hundreds of timed steps on one minibatch stay finite


def bench_shape(name, dims, B, Bm, args, dev):
    import torch
    from pybulletgym_amd.policy import MLPPopulation
    from pybulletgym_amd.ppo import AdamClip, PPOGrad, adv_norm, mlp_forward
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    rnd = lambda *s: torch.randn(s, device=dev, generator=gen)  # noqa: E731
    cd = dims[:3] + (1,)
    pa, pc = MLPPopulation(dims, 1, dev), MLPPopulation(cd, 1, dev)
    ta0, tc0 = pa.init_theta(0), pc.init_theta(1)
    pa.close()
    pc.close()
    obs = rnd(B, dims[0])
    mu = mlp_forward(ta0, dims, obs)
    eps = rnd(B, dims[3])
    act = (mu + math.exp(-0.5) * eps).contiguous()
    logp_old = (-0.5 * (eps * eps).sum(1) + 0.5 * dims[3] - 0.5 * dims[3] * math.log(2.0 * math.pi) + 0.15 * rnd(B)).contiguous()
    ret = (mlp_forward(tc0, cd, obs).squeeze(1) + rnd(B)).contiguous()
    adv = rnd(B)
    idx = torch.randperm(B, device=dev, generator=gen)[:Bm].contiguous()

    def params():
        ps = [torch.nn.Parameter(ta0.clone()), torch.nn.Parameter(tc0.clone()),
              torch.nn.Parameter(torch.full((dims[3],), -0.5, device=dev))]
        return ps, torch.optim.Adam(ps, lr=LR, eps=EPS)

    stats = torch.zeros(4, dtype=torch.float64, device=dev)
    g = PPOGrad(dims, Bm, dev)

    p_t, opt_t = params()

    def torch_leg():
        base.torch_gradient(*p_t, dims, obs, act, logp_old, adv, ret, idx)
        torch.nn.utils.clip_grad_norm_(p_t, MAX_GRAD_NORM)
        opt_t.step()

    p_g, opt_g = params()
    for p in p_g:
        p.grad = torch.zeros_like(p.data)

    def hip_grad_leg():
        a_mb = adv[idx]
        an = torch.stack((a_mb.mean(), 1.0 / (a_mb.std() + 1e-8)))
        g.run(p_g[0].data, p_g[1].data, p_g[2].data, obs, act, logp_old, adv, ret, idx=idx, adv_norm=an, clip_eps=base.CLIP,
              vf_coef=base.VF_COEF, ent_coef=base.ENT_COEF, grad_actor=p_g[0].grad, grad_critic=p_g[1].grad,
              grad_log_std=p_g[2].grad, stats=stats)
        torch.nn.utils.clip_grad_norm_(p_g, MAX_GRAD_NORM)
        opt_g.step()

    p_h = [p.data for p in params()[0]]
    g_h = [torch.zeros_like(p) for p in p_h]
    adam = AdamClip([p.numel() for p in p_h], dev)
    pair = torch.zeros(2, device=dev)
    info = torch.zeros(2, dtype=torch.float64, device=dev)

    def hip_leg():
        adv_norm(adv, idx, out=pair)
        g.run(p_h[0], p_h[1], p_h[2], obs, act, logp_old, adv, ret, idx=idx, adv_norm=pair, clip_eps=base.CLIP,
              vf_coef=base.VF_COEF, ent_coef=base.ENT_COEF, grad_actor=g_h[0], grad_critic=g_h[1], grad_log_std=g_h[2], stats=stats)
        adam.step(p_h, g_h, LR, (0.9, 0.999), EPS, MAX_GRAD_NORM, info=info)

    # the optimiser alone, on its own parameters and a fixed gradient
    p_o = [p.data for p in params()[0]]
    g_o = [0.01 * torch.randn(p.shape, device=dev, generator=gen) for p in p_o]
    adam_o = AdamClip([p.numel() for p in p_o], dev)
    legs = {"torch": torch_leg, "hip_grad": hip_grad_leg, "hip": hip_leg, "adv_norm": lambda: adv_norm(adv, idx, out=pair),
            "opt_step": lambda: adam_o.step(p_o, g_o, LR, (0.9, 0.999), EPS, MAX_GRAD_NORM)}
    w = device_windows(dev, legs, args.windows, args.calls, warmup=args.warmup)
    finite = all(bool(torch.isfinite(p).all()) for p in p_h + [q.data for q in p_t + p_g])
    for o in (g, adam, adam_o):
        o.close()
    n = sum(p.numel() for p in p_o)
    r = dict(summary(w), dims=dims, batch_rows=B, minibatch_rows=Bm, unit="us per minibatch step", calls_per_window=args.calls,
             optimiser_elements=n, parameters_finite=finite)
    r["opt_step_GB_per_s"] = 7 * 4 * n / (r["median"]["opt_step"] * 1e-6) / 1e9
    r["hip_grad_over_hip"] = r["median"]["hip_grad"] / r["median"]["hip"]
    return r


def bench_iterate(args, dev):
    modes = {"torch_opt": dict(optimizer="torch"), "hip_opt": dict(optimizer="hip"), "hip_opt_graph": dict(optimizer="hip", graph=True)}
    w, _ = pendulum_windows(dev, modes, args.windows, args.iterations, base=dict(backward="hip"))
    r = dict(summary(w), trainer=dict(HP, env_id=ENV_ID, envs=ENVS, backward="hip"),
             unit="ms per PPO.iterate()", iterations_per_window=args.iterations)
    r["median_below_the_torch_optimiser_window_minimum"] = {k: r["median"][k] < r["min"]["torch_opt"]
                                                            for k in ("hip_opt", "hip_opt_graph")}
    return r


def main():
    ap = parser("ppo_opt.json", calls=20, calls_help="minibatch steps per timed window",
                iterations_help="PPO.iterate() calls per timed window")
    ap.add_argument("--shapes", nargs="*", default=list(base.SHAPES))
    args = ap.parse_args()
    import torch
    import pybulletgym_amd  # noqa: F401
    dev = torch.device("cuda:0")
    res = {"shapes": {}}
    fmt = lambda r, k: f"{k} {r['median'][k]:.1f} [{r['min'][k]:.1f}, {r['max'][k]:.1f}]"  # noqa: E731
    for name in args.shapes:
        res["shapes"][name] = r = bench_shape(name, *base.SHAPES[name], args, dev)
        print(f"{name} {r['dims']} x {r['minibatch_rows']}: us median [min, max]  " + "  ".join(fmt(r, k) for k in r["median"]) +
              f"  opt_step {r['opt_step_GB_per_s']:.1f} GB/s over {r['optimiser_elements']} elements  finite {r['parameters_finite']}",
              flush=True)
    res["iterate"] = r = bench_iterate(args, dev)
    print("PPO.iterate() ms median [min, max]  " + "  ".join(
        f"{k} {r['median'][k]:.2f} [{r['min'][k]:.2f}, {r['max'][k]:.2f}]" for k in r["median"]) +
        f"  below the torch optimiser's minimum: {r['median_below_the_torch_optimiser_window_minimum']}")
    finish(res, args.out)


if __name__ == "__main__":
    main()
