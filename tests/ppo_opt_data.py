"""What the optimiser-step tests share (tests/test_ppoopt_host.py, tests/test_ppoopt_gpu.py): numpy restatements of
pbg_adv_norm and of one pbg_ppo_opt step in the arithmetic order include/pbg.h "PPO optimiser step" states (float64
numpy operations are IEEE and never fused, so the restatement is bit-exact), seeded cases, the torch reference
(``torch.optim.Adam`` + ``clip_grad_norm_``) and the bound on the parameters' movement."""
import numpy as np
import torch

AN_LANES, OB, MAX_WG = 1024, 256, 64   # pbg_adv_norm's workgroup; the optimiser's workgroup and workgroups per block
LR, BETAS, EPS = 3e-3, (0.9, 0.999), 1e-5   # the trainer's Adam

ADV_ROWS = (2, 17, 1023, 1024, 1025)   # around the one-workgroup stride
# (Bm, value) of constant advantages: the unshifted sums S2 - S1 * mean leave a residue at the last three (scales of
# 10,032, 6,399 and 9.99e7 instead of 1e8)
CONSTANT = ((2, 0.0), (17, 1.5), (1025, -0.1), (1025, 3.0e4), (1537, 6836.862), (5000, -13077.53), (3000, 4.2e-4))


def sizes_of(dims):
    """(Da, Dc, A) of an actor / critic pair: the flat layout's counts."""
    o, h1, h2, a = dims
    trunk = o * h1 + h1 + h1 * h2 + h2
    return (trunk + h2 * a + a, trunk + h2 + 1, a)


# the trainer's three blocks at (44,65,129,17): recomputed from the layout
SIZES = ((1,), (8, 6, 1), (255, 256, 257), sizes_of((44, 65, 129, 17)))
SIZES_GPU = SIZES + (sizes_of((256, 256, 256, 64)),)   # ~280 thousand elements: several strides per lane, a ragged tail


def tree(x):
    """pbg.h's tree over the last axis (a power of two): for s = N/2 .. 1: x[l] += x[l + s], l < s."""
    x = np.array(x, dtype=np.float64)
    s = x.shape[-1] // 2
    while s >= 1:
        x[..., :s] += x[..., s:2 * s]
        s //= 2
    return x[..., 0]


def adv_norm_ref(adv, idx=None):
    """(shift, scale) float32 [2]."""
    a = (adv if idx is None else adv[idx]).astype(np.float64)
    Bm = a.shape[0]
    K = -(-Bm // AN_LANES)
    c0 = a[0]
    rows = np.zeros(K * AN_LANES)    # the zeros past Bm add nothing: a lane sum is never -0.0
    rows[:Bm] = a - c0               # the sums are of the advantages less the first one
    rows = rows.reshape(K, AN_LANES)
    s1, s2 = np.zeros(AN_LANES), np.zeros(AN_LANES)
    for k in range(K):
        s1 += rows[k]
        s2 += rows[k] * rows[k]
    S1, S2 = tree(s1), tree(s2)
    ms = S1 / np.float64(Bm)
    var = (S2 - S1 * ms) / np.float64(Bm - 1)
    var = np.float64(0.0) if var < 0.0 else var
    return np.array([c0 + ms, 1.0 / (np.sqrt(var) + 1e-8)]).astype(np.float32)


def block_wgs(n):
    groups = -(-n // 4)
    return min(-(-groups // OB), MAX_WG)


def partials_ref(g):
    """The workgroups' float64 sums of squares of one block, launch 1's geometry."""
    n = g.shape[0]
    G = block_wgs(n)
    S = G * OB
    groups = -(-n // 4)
    K = -(-groups // S)
    sq = np.zeros(K * S * 4)
    g64 = g.astype(np.float64)
    sq[:n] = g64 * g64
    sq = sq.reshape(K, G, OB, 4)
    acc = np.zeros((G, OB))
    for k in range(K):
        for j in range(4):
            acc += sq[k, :, :, j]
    return tree(acc)


def new_state(sizes):
    return dict(m=[np.zeros(s, np.float32) for s in sizes], v=[np.zeros(s, np.float32) for s in sizes], t=0, b1t=1.0, b2t=1.0)


def opt_step_ref(state, params, grads, lr=LR, betas=BETAS, eps=EPS, max_grad_norm=0.0):
    """One step in place on ``params`` and ``state``; returns (norm, coef)."""
    b1, b2 = np.float64(betas[0]), np.float64(betas[1])
    state["t"] += 1
    state["b1t"] = np.float64(state["b1t"]) * b1
    state["b2t"] = np.float64(state["b2t"]) * b2
    sumsq = np.float64(0.0)
    for g in grads:
        for p in partials_ref(g):
            sumsq = sumsq + p
    norm = np.sqrt(sumsq)
    coef = np.float64(1.0)
    if max_grad_norm > 0.0:
        c = np.float64(max_grad_norm) / (norm + 1e-6)
        coef = np.float64(1.0) if c > 1.0 else c
    omb1, omb2 = 1.0 - b1, 1.0 - b2
    c1 = np.float64(lr) / (1.0 - state["b1t"])
    c2 = np.sqrt(1.0 - state["b2t"])
    for p, g, m, v in zip(params, grads, state["m"], state["v"]):
        gd = g.astype(np.float64) * coef
        md = b1 * m.astype(np.float64) + omb1 * gd
        vd = b2 * v.astype(np.float64) + omb2 * (gd * gd)
        p[:] = (p.astype(np.float64) - c1 * (md / (np.sqrt(vd) / c2 + np.float64(eps)))).astype(np.float32)
        m[:] = md.astype(np.float32)
        v[:] = vd.astype(np.float32)
    return float(norm), float(coef)


# per step, the gradient's expected global norm: with max_grad_norm = 0.5 the clip is active on steps 1, 3, 4
GRAD_NORMS = (0.1, 3.0, 0.2, 5.0, 1.0)


def params0(sizes, seed=0):
    rng = np.random.default_rng(1000 + seed)
    return [rng.standard_normal(s).astype(np.float32) for s in sizes]


def grads_of(sizes, step, seed=0, zero_block=None):
    """The step's gradients: normals scaled to a global norm of about GRAD_NORMS[step]; block ``zero_block`` all zero."""
    rng = np.random.default_rng(seed * 100 + step)
    n = sum(s for b, s in enumerate(sizes) if b != zero_block)
    scale = GRAD_NORMS[step % len(GRAD_NORMS)] / np.sqrt(n)
    return [np.zeros(s, np.float32) if b == zero_block else (scale * rng.standard_normal(s)).astype(np.float32)
            for b, s in enumerate(sizes)]


def torch_steps(sizes, steps, dtype, max_grad_norm, seed=0):
    """The parameters after ``steps`` steps of torch.optim.Adam + clip_grad_norm_ at ``dtype`` on the CPU."""
    ps = [torch.nn.Parameter(torch.from_numpy(p).to(dtype)) for p in params0(sizes, seed)]
    opt = torch.optim.Adam(ps, lr=LR, betas=BETAS, eps=EPS)
    for s in range(steps):
        for p, g in zip(ps, grads_of(sizes, s, seed)):
            p.grad = torch.from_numpy(g).to(dtype)
        if max_grad_norm:
            torch.nn.utils.clip_grad_norm_(ps, max_grad_norm)
        opt.step()
    return [p.detach().numpy().astype(np.float64) for p in ps]


def movement_err(p, p64, p0):
    """max |dp - dp64| / max |dp64|, d: the movement since step 0."""
    d, d64 = p.astype(np.float64) - p0.astype(np.float64), p64 - p0.astype(np.float64)
    return float(np.abs(d - d64).max() / np.abs(d64).max())


def check_movement(got, sizes, steps, max_grad_norm, what, seed=0):
    """Section 14's rule on the movement: per block err <= max(4 err(torch float32), 1e-5); returns the worst
    err / err_torch32."""
    p0 = params0(sizes, seed)
    p64 = torch_steps(sizes, steps, torch.float64, max_grad_norm, seed)
    p32 = torch_steps(sizes, steps, torch.float32, max_grad_norm, seed)
    worst = 0.0
    for b, (g, r64, r32, z) in enumerate(zip(got, p64, p32, p0)):
        e, e32 = movement_err(g, r64, z), movement_err(r32.astype(np.float32), r64, z)
        print(f"{what} block {b}: err {e:.3e} torch32 {e32:.3e}")
        assert e <= max(4.0 * e32, 1e-5), (what, b, e, e32)
        worst = max(worst, e / e32 if e32 > 0 else 0.0)
    return worst
