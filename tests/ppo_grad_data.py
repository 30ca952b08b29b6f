"""What the PPO-gradient tests share (tests/test_ppograd_host.py, tests/test_ppograd_gpu.py): seeded cases, the
torch autograd reference over the expression PPO.update differentiates (float64: the truth; float32: the
yardstick), and the bound of include/pbg.h "PPO gradient"'s tests.

The gradient is discontinuous at the clip edges and at ReLU zeros, so the generator redraws every row of the
batch whose float64 ratio lies within 1e-3 of 1 +- c or that has a hidden pre-activation (either network) with
|pre| < 1e-5, and asserts three things about every case: at most 2 % of the batch's rows were redrawn, no such
row is left, and the clipped fraction (|ratio - 1| > c, over the batch: a minibatch of one row cannot have a
fraction) is between 5 % and 50 %, so both branches of the surrogate run."""
import functools
import math

import numpy as np
import torch

CLIP_EPS, VF_COEF = 0.2, 0.5
BLOCKS = ("w1", "b1", "w2", "b2", "w3", "b3")

# (dims, B, Bm, seed): the issue's shapes.  (44, 65, 129, 17) crosses `layer`'s 64 and 128 thresholds; the last is
# the widest MLP the library admits.
# Each seed is the smallest whose batch meets the generator's three conditions with and without a normaliser (2 % of
# a batch of 24 rows is no row at all, so a seed that needs one redraw is passed over).
#
# The last four reach paths of the device kernel the others leave out.  The widest MLP on a ragged tile: with 5 rows
# the float64 forward's second half-tile pass does not run, with 13 it is partial.  (5, 129, 16, 1) at 8,209 rows: a
# hidden layer above 128 columns (one column group) whose workgroups 0 and 1 own a second tile, so the weight gradient
# accumulates onto the workgroup's partial in memory.  The widest MLP at 1,921 rows: WIDEST_TILES tiles for the
# WIDEST_WGS workgroups its workspace cap allows, so again workgroups 0 and 1 own two tiles.
CASES = (((3, 1, 1, 1), 24, 1, 1), ((3, 1, 1, 1), 24, 17, 0), ((5, 16, 8, 1), 40, 33, 0), ((28, 64, 64, 8), 300, 257, 0),
         ((44, 65, 129, 17), 64, 48, 1), ((256, 256, 256, 64), 24, 16, 3),
         ((256, 256, 256, 64), 24, 5, 1), ((256, 256, 256, 64), 24, 13, 0), ((5, 129, 16, 1), 8300, 8209, 0),
         ((256, 256, 256, 64), 2000, 1921, 0))
# pbg_ppo_grad_create's geometry for (256, 256, 256, 64): Dtot = Da + Dc + A = 148,032 + 131,841 + 64 = 279,937 floats
# and four doubles of statistics per workgroup, 1,119,780 bytes; the 128 MiB workspace cap admits 119 of them
WIDEST_WGS = (128 << 20) // (4 * 279937 + 4 * 8)
WIDEST_TILES = -(-1921 // 16)
OPTIONS = [(norm, an, ent) for norm in (False, True) for an in (False, True) for ent in (0.0, 0.01)]


def param_count(dims):
    o, h1, h2, a = dims
    return o * h1 + h1 + h1 * h2 + h2 + h2 * a + a


def critic_dims(dims):
    return dims[:3] + (1,)


def split(dims, flat):
    """The flat vector -> {block: array}, include/pbg.h's layout."""
    o, h1, h2, a = dims
    out, at = {}, 0
    for name, shape in zip(BLOCKS, ((o, h1), (h1,), (h1, h2), (h2,), (h2, a), (a,))):
        cnt = int(np.prod(shape))
        out[name] = flat[at:at + cnt].reshape(shape)
        at += cnt
    assert at == flat.shape[0]
    return out


def forward(theta, dims, x, obs_norm=None):
    """PPO.update's MLP (ppo.mlp_forward) on torch tensors, also returning the hidden pre-activations."""
    o, h1, h2, a = dims
    if obs_norm is not None:
        mean, inv_std, clip = obs_norm
        x = torch.clamp((x - mean) * inv_std, -clip, clip)
    at, pres = 0, []
    for k, h, relu in ((o, h1, True), (h1, h2, True), (h2, a, False)):
        w = theta[at:at + k * h].view(k, h)
        b = theta[at + k * h:at + k * h + h]
        at += k * h + h
        x = x @ w + b
        if relu:
            pres.append(x)
            x = torch.relu(x)
    return x, pres


def _theta(r, dims):
    o, h1, h2, a = dims
    parts = []
    for k, h in ((o, h1), (h1, h2), (h2, a)):
        parts.append((r.standard_normal((k, h)) / math.sqrt(k)).astype(np.float32).ravel())
        parts.append((0.1 * r.standard_normal(h)).astype(np.float32))
    return np.concatenate(parts)


@functools.lru_cache(maxsize=None)
def case(dims, B, Bm, seed, norm):
    """A dict of numpy arrays (read-only: the tests share it)."""
    r = np.random.default_rng([seed, B, Bm, int(norm), *dims])
    o, A = dims[0], dims[3]
    c = dict(dims=dims, B=B, Bm=Bm)
    c["theta_actor"], c["theta_critic"] = _theta(r, dims), _theta(r, critic_dims(dims))
    c["log_std"] = r.uniform(-1.0, 0.0, A).astype(np.float32)
    c["mean"] = (0.3 * r.standard_normal(o)).astype(np.float32) if norm else None
    c["inv_std"] = r.uniform(0.5, 2.0, o).astype(np.float32) if norm else None
    c["clip"] = 1.5
    obs, act = np.zeros((B, o), np.float32), np.zeros((B, A), np.float32)
    logp_old, ret = np.zeros(B, np.float32), np.zeros(B, np.float32)
    t64 = lambda a: torch.from_numpy(a).double()  # noqa: E731
    obs_norm = (t64(c["mean"]), t64(c["inv_std"]), c["clip"]) if norm else None
    todo, redrawn = np.ones(B, bool), 0
    for attempt in range(50):
        n = int(todo.sum())
        if attempt:
            redrawn += n
        obs[todo] = r.standard_normal((n, o)).astype(np.float32)
        with torch.no_grad():
            mu, pa = forward(t64(c["theta_actor"]), dims, t64(obs), obs_norm)
            v, pc = forward(t64(c["theta_critic"]), critic_dims(dims), t64(obs), obs_norm)
        sig = np.exp(c["log_std"].astype(np.float64))
        act[todo] = (mu.numpy()[todo] + sig * r.standard_normal((n, A))).astype(np.float32)
        z = (act.astype(np.float64) - mu.numpy()) / sig
        logp = -0.5 * (z * z).sum(1) - c["log_std"].astype(np.float64).sum() - 0.5 * A * math.log(2.0 * math.pi)
        logp_old[todo] = (logp[todo] + 0.15 * r.standard_normal(n)).astype(np.float32)
        ret[todo] = (v.numpy()[todo, 0] + r.standard_normal(n)).astype(np.float32)
        ratio = np.exp(logp - logp_old.astype(np.float64))
        pre = torch.cat([p.abs() for p in pa + pc], 1).min(1).values.numpy()
        todo = (np.abs(ratio - (1.0 - CLIP_EPS)) < 1e-3) | (np.abs(ratio - (1.0 + CLIP_EPS)) < 1e-3) | (pre < 1e-5)
        if not todo.any():
            break
    assert not todo.any(), "a row on a discontinuity is left"
    assert redrawn <= 0.02 * B, (redrawn, B)
    clipped = float((np.abs(ratio - 1.0) > CLIP_EPS).mean())
    assert 0.05 <= clipped <= 0.5, clipped
    c["obs"], c["act"], c["logp_old"], c["ret"] = obs, act, logp_old, ret
    c["adv"] = (0.3 + r.standard_normal(B)).astype(np.float32)
    c["idx"] = r.permutation(B)[:Bm].astype(np.int64)
    a = c["adv"][c["idx"]].astype(np.float64)
    # (shift, scale) as the trainer forms them; one row has no standard deviation: a plain scale stands in
    c["adv_norm"] = np.array([a.mean(), 1.0 / (a.std(ddof=1) + 1e-8) if Bm > 1 else 0.7], np.float32)
    for k, a in c.items():
        if isinstance(a, np.ndarray):
            a.flags.writeable = False
    return c


def reference(c, adv_norm, ent_coef, dtype=torch.float64, idx=None, device="cpu"):
    """Torch autograd over PPO.update's expression for the minibatch ``idx`` (default: the case's) in ``dtype``:
    ({"actor": {block: grad}, "critic": {...}, "log_std": grad}, stats [4], logp [Bm], v [Bm]) as float64 numpy."""
    dims, A = c["dims"], c["dims"][3]
    t = lambda a: torch.from_numpy(np.array(a)).to(device=device, dtype=dtype)  # noqa: E731
    idx = torch.from_numpy(np.array(c["idx"] if idx is None else idx)).to(device)
    ta, tc, ls = (t(c[k]).requires_grad_() for k in ("theta_actor", "theta_critic", "log_std"))
    obs_norm = (t(c["mean"]), t(c["inv_std"]), c["clip"]) if c["mean"] is not None else None
    obs, act, logp_old, adv, ret = (t(c[k])[idx] for k in ("obs", "act", "logp_old", "adv", "ret"))
    if adv_norm:
        an = t(c["adv_norm"])
        adv = (adv - an[0]) * an[1]
    mu, _ = forward(ta, dims, obs, obs_norm)
    v = forward(tc, critic_dims(dims), obs, obs_norm)[0].squeeze(1)
    z = (act - mu) * torch.exp(-ls)
    logp = -0.5 * (z * z).sum(1) - ls.sum() - 0.5 * A * math.log(2.0 * math.pi)
    ratio = torch.exp(logp - logp_old)
    pg = -torch.min(ratio * adv, torch.clamp(ratio, 1.0 - CLIP_EPS, 1.0 + CLIP_EPS) * adv).mean()
    vf = 0.5 * ((v - ret) ** 2).mean()
    entropy = ls.sum() + 0.5 * A * (1.0 + math.log(2.0 * math.pi))
    (pg + VF_COEF * vf - ent_coef * entropy).backward()
    n64 = lambda x: x.detach().double().cpu().numpy()  # noqa: E731
    grads = dict(actor=split(dims, n64(ta.grad)), critic=split(critic_dims(dims), n64(tc.grad)), log_std=n64(ls.grad))
    stats = np.array([float(pg.detach()), float(vf.detach()), float(((ratio.detach() - 1.0).abs() > CLIP_EPS).double().mean()),
                      float((logp_old - logp.detach()).mean())])
    return grads, stats, n64(logp), n64(v)


@functools.lru_cache(maxsize=None)
def references(dims, B, Bm, seed, norm, adv_norm, ent_coef):
    """(float64 reference, float32 reference) of a case, computed once."""
    c = case(dims, B, Bm, seed, norm)
    return reference(c, adv_norm, ent_coef, torch.float64), reference(c, adv_norm, ent_coef, torch.float32)


def blocks(dims, grad_actor, grad_critic, grad_log_std):
    """A result's three arrays in `reference`'s form."""
    f = lambda a: np.asarray(a, dtype=np.float64)  # noqa: E731
    return dict(actor=split(dims, f(grad_actor)), critic=split(critic_dims(dims), f(grad_critic)), log_std=f(grad_log_std))


def err(g, g64):
    """max|g - g64| / max|g64|; a block whose true gradient is zero (a dead unit) must be zero."""
    top = float(np.abs(g64).max())
    d = float(np.abs(g - g64).max())
    return d / top if top > 0.0 else (0.0 if d == 0.0 else math.inf)


def flat_blocks(b):
    for net in ("actor", "critic"):
        for name in BLOCKS:
            yield f"{net}.{name}", b[net][name]
    yield "log_std", b["log_std"]


def check_grads(got, ref64, ref32, what=""):
    """The bound: per block err <= max(4 err(torch float32), 1e-5).  Returns the worst err / err32 (for the record;
    blocks under the floor with err32 == 0 do not count) after asserting."""
    worst, report = 0.0, []
    for (name, g), (_, g64), (_, g32) in zip(flat_blocks(got), flat_blocks(ref64), flat_blocks(ref32)):
        assert g.shape == g64.shape, (name, g.shape, g64.shape)
        e, e32 = err(g, g64), err(g32, g64)
        report.append((name, e, e32))
        if e32 > 0.0:
            worst = max(worst, e / e32)
    bad = [(n, e, e32) for n, e, e32 in report if not e <= max(4.0 * e32, 1e-5)]
    assert not bad, (what, bad)
    return worst


def check_stats(stats, logp, want_stats, want_logp, what=""):
    """stats within 1e-5 relative of the float64 values, logp within 1e-5 max(1, |logp|)."""
    stats, logp = np.asarray(stats, np.float64), np.asarray(logp, np.float64)
    assert (np.abs(stats - want_stats) <= 1e-5 * np.abs(want_stats)).all(), (what, stats, want_stats)
    assert (np.abs(logp - want_logp) <= 1e-5 * np.maximum(1.0, np.abs(want_logp))).all(), what
