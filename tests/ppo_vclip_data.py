"""What the value-clipping tests share (tests/test_ppo_vclip_host.py, tests/test_ppo_vclip_gpu.py): the cases of
tests/ppo_grad_data.py with a ``value_old`` column, and the torch autograd reference over the expression PPO.update
differentiates with ``vf_clip`` (float64: the truth; float32: the yardstick).  The bound is ppo_grad_data.check_grads.

``value_old = float32(v64 + 0.3 N(0, 1))`` from a generator of this module's own, ``vf_clip = 0.2``.  The clipped value
loss is discontinuous in its derivative where |v - value_old| = e and where the two squared errors of a clamped row
tie, so the generator redraws ``value_old`` alone for rows within 1e-3 of the first or, clamped, with
|u1 - u2| < 1e-3 max(u1, 1e-6), and asserts of every case: at most 2 % of the batch's rows were redrawn, none is left,
and the clipped term wins in 10 % to 60 % of the batch's rows, so both branches run.  A case takes the smallest of the
generator seeds 0, 1, 2 that meets all three."""
import functools
import math

import numpy as np
import torch

import ppo_grad_data as pd

VF_CLIP = 0.2
# the issue's shapes, ppo_grad_data.CASES' entries (their seeds)
CASES = (((3, 1, 1, 1), 24, 1, 1), ((3, 1, 1, 1), 24, 17, 0), ((5, 16, 8, 1), 40, 33, 0), ((44, 65, 129, 17), 64, 48, 1),
         ((256, 256, 256, 64), 24, 13, 0))
# workgroups 0 and 1 own a second tile (ppo_grad_data.CASES): once per path on the device
TWO_TILES = ((5, 129, 16, 1), 8300, 8209, 0)
OPTIONS = [(norm, an, 0.01) for norm in (False, True) for an in (False, True)]
assert all(c in pd.CASES for c in CASES + (TWO_TILES,))


def _terms(v, vo, ret, e=VF_CLIP):
    """(clamped, u1, u2) per row, float64."""
    dv = v - vo
    vc = vo + np.clip(dv, -e, e)
    return np.abs(dv) > e, (v - ret) ** 2, (vc - ret) ** 2


def _value_old(c, v64, gseed):
    """``value_old`` for generator seed ``gseed``, or the condition it misses."""
    B = c["B"]
    r = np.random.default_rng([gseed, 0x7C11, B, c["Bm"], int(c["mean"] is not None), *c["dims"]])
    ret = c["ret"].astype(np.float64)
    vo = np.zeros(B, np.float32)
    todo, redrawn = np.ones(B, bool), 0
    for attempt in range(50):
        n = int(todo.sum())
        if attempt:
            redrawn += n
        vo[todo] = (v64[todo] + 0.3 * r.standard_normal(n)).astype(np.float32)
        clamped, u1, u2 = _terms(v64, vo.astype(np.float64), ret)
        todo = (np.abs(np.abs(v64 - vo.astype(np.float64)) - VF_CLIP) < 1e-3) | \
            (clamped & (np.abs(u1 - u2) < 1e-3 * np.maximum(u1, 1e-6)))
        if not todo.any():
            break
    if todo.any():
        return None, "a row on a discontinuity is left"
    if redrawn > 0.02 * B:
        return None, f"{redrawn} of {B} rows redrawn"
    share = float((u2 > u1).mean())
    if not 0.10 <= share <= 0.60:
        return None, f"the clipped term wins in {share:.3f} of the rows"
    return vo, share


@functools.lru_cache(maxsize=None)
def case(dims, B, Bm, seed, norm):
    """ppo_grad_data.case plus ``value_old`` and ``vf_clip`` (read-only arrays: the tests share it)."""
    c = dict(pd.case(dims, B, Bm, seed, norm))
    t64 = lambda a: torch.from_numpy(np.array(a)).double()  # noqa: E731
    obs_norm = (t64(c["mean"]), t64(c["inv_std"]), c["clip"]) if norm else None
    with torch.no_grad():
        v64 = pd.forward(t64(c["theta_critic"]), pd.critic_dims(dims), t64(c["obs"]), obs_norm)[0][:, 0].numpy()
    why = []
    for gseed in range(3):
        vo, got = _value_old(c, v64, gseed)
        if vo is not None:
            break
        why.append(got)
    assert vo is not None, (dims, B, Bm, norm, why)
    vo.flags.writeable = False
    c.update(value_old=vo, vf_clip=VF_CLIP, vclip_seed=gseed, vclip_share=got)
    return c


def reference(c, adv_norm, ent_coef, dtype=torch.float64, idx=None, device="cpu"):
    """ppo_grad_data.reference with the value term replaced by the clipped one, 1/2 mean(max(u1, u2))."""
    dims, A = c["dims"], c["dims"][3]
    t = lambda a: torch.from_numpy(np.array(a)).to(device=device, dtype=dtype)  # noqa: E731
    idx = torch.from_numpy(np.array(c["idx"] if idx is None else idx)).to(device)
    ta, tc, ls = (t(c[k]).requires_grad_() for k in ("theta_actor", "theta_critic", "log_std"))
    obs_norm = (t(c["mean"]), t(c["inv_std"]), c["clip"]) if c["mean"] is not None else None
    obs, act, logp_old, adv, ret, vo = (t(c[k])[idx] for k in ("obs", "act", "logp_old", "adv", "ret", "value_old"))
    if adv_norm:
        an = t(c["adv_norm"])
        adv = (adv - an[0]) * an[1]
    mu, _ = pd.forward(ta, dims, obs, obs_norm)
    v = pd.forward(tc, pd.critic_dims(dims), obs, obs_norm)[0].squeeze(1)
    z = (act - mu) * torch.exp(-ls)
    logp = -0.5 * (z * z).sum(1) - ls.sum() - 0.5 * A * math.log(2.0 * math.pi)
    ratio = torch.exp(logp - logp_old)
    pg = -torch.min(ratio * adv, torch.clamp(ratio, 1.0 - pd.CLIP_EPS, 1.0 + pd.CLIP_EPS) * adv).mean()
    vc = vo + torch.clamp(v - vo, -c["vf_clip"], c["vf_clip"])
    vf = 0.5 * torch.maximum((v - ret) ** 2, (vc - ret) ** 2).mean()
    entropy = ls.sum() + 0.5 * A * (1.0 + math.log(2.0 * math.pi))
    (pg + pd.VF_COEF * vf - ent_coef * entropy).backward()
    n64 = lambda x: x.detach().double().cpu().numpy()  # noqa: E731
    grads = dict(actor=pd.split(dims, n64(ta.grad)), critic=pd.split(pd.critic_dims(dims), n64(tc.grad)), log_std=n64(ls.grad))
    stats = np.array([float(pg.detach()), float(vf.detach()), float(((ratio.detach() - 1.0).abs() > pd.CLIP_EPS).double().mean()),
                      float((logp_old - logp.detach()).mean())])
    return grads, stats, n64(logp), n64(v)


@functools.lru_cache(maxsize=None)
def references(dims, B, Bm, seed, norm, adv_norm, ent_coef):
    """(float64 reference, float32 reference) of a case, computed once."""
    c = case(dims, B, Bm, seed, norm)
    return reference(c, adv_norm, ent_coef, torch.float64), reference(c, adv_norm, ent_coef, torch.float32)


def host_run(g, c, adv_norm, ent_coef, clipped=True, **kw):
    """``PPOGrad.run`` of the host twin ``g`` on case ``c``: ((grad_actor, grad_critic, grad_log_std, stats), logp, v)."""
    Bm = c["Bm"]
    logp, v = np.full(Bm, np.nan, np.float32), np.full(Bm, np.nan, np.float32)
    norm = (c["mean"], c["inv_std"], c["clip"]) if c["mean"] is not None else None
    if clipped:
        kw = dict(value_old=c["value_old"], vf_clip=c["vf_clip"], **kw)
    out = g.run(c["theta_actor"], c["theta_critic"], c["log_std"], c["obs"], c["act"], c["logp_old"], c["adv"], c["ret"],
                idx=c["idx"], adv_norm=c["adv_norm"] if adv_norm else None, obs_norm=norm, clip_eps=pd.CLIP_EPS,
                vf_coef=pd.VF_COEF, ent_coef=ent_coef, logp_out=logp, v_out=v, **kw)
    return out, logp, v
