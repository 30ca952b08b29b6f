"""The PPO gradient on the host (include/pbg.h "PPO gradient", pbg_ppo_grad_host, ppo.PPOGrad without a device; no
GPU): against torch float64 autograd over PPO.update's expression under the bound of tests/ppo_grad_data.py, v_out
against a host-only MLPPolicy bit for bit, and the argument checks that come before any HIP call."""
import ctypes

import numpy as np
import pytest

import pybulletgym_amd  # noqa: F401
from pybulletgym_amd import _native
from pybulletgym_amd.policy import MLPPolicy, unpack_theta
from pybulletgym_amd.ppo import PPOGrad

import ppo_grad_data as pd


def run(g, c, adv_norm, ent_coef, idx="case", rows=None, **kw):
    Bm = c["Bm"] if rows is None else rows
    logp, v = np.full(Bm, np.nan, np.float32), np.full(Bm, np.nan, np.float32)
    norm = (c["mean"], c["inv_std"], c["clip"]) if c["mean"] is not None else None
    out = g.run(c["theta_actor"], c["theta_critic"], c["log_std"], c["obs"], c["act"], c["logp_old"], c["adv"], c["ret"],
                idx=c["idx"] if isinstance(idx, str) else idx, rows=rows, adv_norm=c["adv_norm"] if adv_norm else None,
                obs_norm=norm, clip_eps=pd.CLIP_EPS, vf_coef=pd.VF_COEF, ent_coef=ent_coef, logp_out=logp, v_out=v, **kw)
    return out, logp, v


@pytest.mark.parametrize("norm,adv_norm,ent_coef", pd.OPTIONS)
@pytest.mark.parametrize("dims,B,Bm,seed", pd.CASES)
def test_host_gradient_against_float64_autograd(dims, B, Bm, seed, norm, adv_norm, ent_coef):
    c = pd.case(dims, B, Bm, seed, norm)
    (g64, s64, logp64, _), (g32, _, _, _) = pd.references(dims, B, Bm, seed, norm, adv_norm, ent_coef)
    g = PPOGrad(dims, Bm)
    (ga, gc, gl, stats), logp, v = run(g, c, adv_norm, ent_coef)
    assert ga.dtype == gc.dtype == gl.dtype == np.float32 and stats.dtype == np.float64
    worst = pd.check_grads(pd.blocks(dims, ga, gc, gl), g64, g32, (dims, Bm, norm, adv_norm, ent_coef))
    print(f"dims {dims} Bm {Bm} norm {norm} adv_norm {adv_norm} ent {ent_coef}: worst err / err_torch32 {worst:.3f}")
    # the forward is the actor's chain: the critic's value of every gathered row, bit for bit
    ws = unpack_theta(pd.critic_dims(dims), c["theta_critic"])
    critic = MLPPolicy(*ws, device=None, obs_norm=(c["mean"], c["inv_std"], c["clip"]) if norm else None)
    assert np.array_equal(v, critic.act(c["obs"][c["idx"]])[:, 0])
    critic.close()


@pytest.mark.parametrize("norm,adv_norm,ent_coef", pd.OPTIONS)
@pytest.mark.parametrize("dims,B,Bm,seed", pd.CASES)
def test_host_stats_and_logp_against_float64(dims, B, Bm, seed, norm, adv_norm, ent_coef):
    """stats within 1e-5 relative of the float64 values, logp_out within 1e-5 max(1, |logp|).  Three of the stats
    come from the library's float64 forward of the actor: mean(logp_old - logp) is a mean of cancelling terms that
    the float32 forward leaves with three digits at the two wide shapes."""
    c = pd.case(dims, B, Bm, seed, norm)
    (_, s64, logp64, _), _ = pd.references(dims, B, Bm, seed, norm, adv_norm, ent_coef)
    (_, _, _, stats), logp, _ = run(PPOGrad(dims, Bm), c, adv_norm, ent_coef)
    rel = np.abs(stats - s64) / np.maximum(np.abs(s64), 1e-300)
    print(f"dims {dims} Bm {Bm} norm {norm} adv_norm {adv_norm}: stats rel err {rel}, logp err "
          f"{(np.abs(logp - logp64) / np.maximum(1.0, np.abs(logp64))).max():.2e}")
    pd.check_stats(stats, logp, s64, logp64, (dims, Bm, norm, adv_norm))


@pytest.mark.parametrize("dims,B,Bm,seed", pd.CASES)
def test_idx_null_is_an_explicit_arange(dims, B, Bm, seed):
    c = pd.case(dims, B, Bm, seed, True)
    g = PPOGrad(dims, Bm)
    a, logp_a, v_a = run(g, c, True, 0.01, idx=None, rows=Bm)
    b, logp_b, v_b = run(g, c, True, 0.01, idx=np.arange(Bm, dtype=np.int64))
    for x, y in zip(a + (logp_a, v_a), b + (logp_b, v_b)):
        assert x.tobytes() == y.tobytes()
    assert np.isfinite(a[0]).all() and np.isfinite(a[3]).all()


def test_outputs_are_written_in_place():
    dims, B, Bm, seed = pd.CASES[2]
    c = pd.case(dims, B, Bm, seed, False)
    g = PPOGrad(dims, Bm)
    bufs = dict(grad_actor=np.full(g.Da, np.nan, np.float32), grad_critic=np.full(g.Dc, np.nan, np.float32),
                grad_log_std=np.full(dims[3], np.nan, np.float32), stats=np.full(4, np.nan))
    out, _, _ = run(g, c, False, 0.0, **bufs)
    fresh, _, _ = run(g, c, False, 0.0)
    for o, f, k in zip(out, fresh, bufs):
        assert o is bufs[k] and np.array_equal(o, f)


def _io(c, **over):
    """A valid pbg_ppo_grad_io_t of case `c` and what keeps its arrays alive."""
    dims = c["dims"]
    keep = dict(ga=np.zeros(pd.param_count(dims), np.float32), gc=np.zeros(pd.param_count(pd.critic_dims(dims)), np.float32),
                gl=np.zeros(dims[3], np.float32), st=np.zeros(4))
    p = lambda a: a.ctypes.data  # noqa: E731
    kw = dict(batch_rows=c["B"], mb_rows=c["Bm"], theta_actor=p(c["theta_actor"]), theta_critic=p(c["theta_critic"]),
              log_std=p(c["log_std"]), clip=0.0, clip_eps=0.2, vf_coef=0.5, ent_coef=0.0, obs=p(c["obs"]), act=p(c["act"]),
              logp_old=p(c["logp_old"]), adv=p(c["adv"]), ret=p(c["ret"]), idx=p(c["idx"]), grad_actor=p(keep["ga"]),
              grad_critic=p(keep["gc"]), grad_log_std=p(keep["gl"]), stats=p(keep["st"]))
    kw.update(over)
    return _native.PPOGradIO(**kw), keep


def test_argument_errors_before_any_hip_call():
    L = _native.lib()
    dims, B, Bm, seed = pd.CASES[2]
    c = pd.case(dims, B, Bm, seed, True)
    io, keep = _io(c)
    assert L.pbg_ppo_grad_host(*dims, ctypes.byref(io)) == 0 and keep["ga"].any()
    # the struct's version
    for size in (ctypes.sizeof(io) - 4, ctypes.sizeof(io) + 4, ctypes.sizeof(io) - 2, 0):
        bad, _ = _io(c)
        bad.struct_size = size
        assert L.pbg_ppo_grad_host(*dims, ctypes.byref(bad)) == -1, size
        assert b"struct_size" in L.pbg_last_error()
    assert L.pbg_ppo_grad_host(*dims, None) == -1
    # dims out of pbg_policy_create's ranges
    for bad_dims in ((0, 16, 8, 1), (5, 257, 8, 1), (5, 16, 0, 1), (5, 16, 8, 65), (5, 16, 8, 0)):
        assert L.pbg_ppo_grad_host(*bad_dims, ctypes.byref(io)) == -1, bad_dims
    # rows, required pointers, the normaliser's pair, clip_eps, indices
    mean = np.zeros(dims[0], np.float32)
    for over in (dict(mb_rows=0), dict(mb_rows=-1), dict(batch_rows=0), dict(idx=None, mb_rows=B + 1),
                 dict(mean=mean.ctypes.data), dict(inv_std=mean.ctypes.data),
                 dict(mean=mean.ctypes.data, inv_std=mean.ctypes.data, clip=0.0), dict(clip_eps=-0.1),
                 dict(clip_eps=float("nan")), dict(batch_rows=int(c["idx"].max()))) + \
            tuple({k: None} for k in ("theta_actor", "theta_critic", "log_std", "obs", "act", "logp_old", "adv", "ret",
                                      "grad_actor", "grad_critic", "grad_log_std", "stats")):
        bad, keep = _io(c, **over)
        assert L.pbg_ppo_grad_host(*dims, ctypes.byref(bad)) == -1, over
        assert not keep["ga"].any() and not keep["st"].any(), over
    neg = c["idx"].copy()
    neg[3] = -1
    bad, _ = _io(c, idx=neg.ctypes.data)
    assert L.pbg_ppo_grad_host(*dims, ctypes.byref(bad)) == -1
    # the device entries refuse these before they touch HIP
    h = ctypes.c_void_p(1)
    for args in ((0, 0, 16, 8, 1, 64), (0, 5, 16, 8, 65, 64), (0, 5, 16, 8, 1, 0), (-1, 5, 16, 8, 1, 64)):
        assert L.pbg_ppo_grad_create(*args, ctypes.byref(h)) == -1, args
        assert h.value is None
        h = ctypes.c_void_p(1)
    assert L.pbg_ppo_grad_create(0, 5, 16, 8, 1, 64, None) == -1
    assert L.pbg_ppo_grad_run(None, ctypes.byref(io), None) == -1
    L.pbg_ppo_grad_destroy(None)


def test_wrapper_strictness():
    dims, B, Bm, seed = pd.CASES[2]
    c = dict(pd.case(dims, B, Bm, seed, True))
    g = PPOGrad(dims, Bm)
    with pytest.raises(_native.PbgError):   # Bm > max_rows
        run(PPOGrad(dims, Bm - 1), c, True, 0.0)
    for key, bad in (("obs", c["obs"].astype(np.float64)), ("obs", c["obs"][:, :4]), ("obs", c["obs"][:, 0]),
                     ("act", c["act"][:-1]), ("logp_old", c["logp_old"][:, None]), ("adv", c["adv"][::2]),
                     ("ret", c["ret"].astype(np.float64)), ("idx", c["idx"].astype(np.int32)),
                     ("theta_actor", c["theta_actor"][:-1]), ("theta_critic", c["theta_critic"][:-1]),
                     ("log_std", c["log_std"].astype(np.float64)), ("adv_norm", c["adv_norm"][:1]),
                     ("mean", c["mean"][:-1]), ("inv_std", None), ("obs", c["obs"].tolist())):
        with pytest.raises(_native.PbgError):
            run(g, {**c, key: bad}, True, 0.0)
    for kw in (dict(grad_actor=np.zeros(g.Da)), dict(stats=np.zeros(4, np.float32)), dict(grad_log_std=np.zeros(2, np.float32))):
        with pytest.raises(_native.PbgError):
            run(g, c, True, 0.0, **kw)
    for bad_dims, rows in (((5, 16, 8), 4), ((5, 16, 8, 65), 4), ((0, 16, 8, 1), 4), ((5, 16, 8, 1), 0)):
        with pytest.raises(_native.PbgError):
            PPOGrad(bad_dims, rows)


def test_the_symbols_are_exported():
    assert set(_native.PPO_GRAD_EXPORTED) <= set(_native.EXPORTED)
    for f in _native.PPO_GRAD_EXPORTED:
        assert hasattr(_native.lib(), f), f
