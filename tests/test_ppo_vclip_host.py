"""Value clipping in the PPO gradient on the host (include/pbg.h "Value clipping and the KL gate", pbg_ppo_grad_host with
value_old; no GPU): against torch float64 autograd over PPO.update's expression with vf_clip under the bound of
tests/ppo_grad_data.py, what the option leaves alone when it is off or never binds, and the argument and struct-size
checks that come before any work."""
import ctypes

import numpy as np
import pytest

import pybulletgym_amd  # noqa: F401
from pybulletgym_amd import _native
from pybulletgym_amd.ppo import PPOGrad

import ppo_grad_data as pd
import ppo_vclip_data as vd


@pytest.mark.parametrize("norm,adv_norm,ent_coef", vd.OPTIONS)
@pytest.mark.parametrize("dims,B,Bm,seed", vd.CASES)
def test_host_gradient_with_value_old_against_float64_autograd(dims, B, Bm, seed, norm, adv_norm, ent_coef):
    c = vd.case(dims, B, Bm, seed, norm)
    (g64, s64, logp64, _), (g32, _, _, _) = vd.references(dims, B, Bm, seed, norm, adv_norm, ent_coef)
    (ga, gc, gl, stats), logp, v = vd.host_run(PPOGrad(dims, Bm), c, adv_norm, ent_coef)
    what = (dims, Bm, norm, adv_norm, ent_coef)
    worst = pd.check_grads(pd.blocks(dims, ga, gc, gl), g64, g32, what)
    print(f"dims {dims} Bm {Bm} norm {norm} adv_norm {adv_norm}: generator seed {c['vclip_seed']}, the clipped term wins in "
          f"{c['vclip_share']:.3f} of the batch, worst err / err_torch32 {worst:.3f}, stats {stats} (float64 {s64})")
    pd.check_stats(stats, logp, s64, logp64, what)
    # the option touches the critic's loss alone: v_out and logp_out are those of a run without it
    _, logp0, v0 = vd.host_run(PPOGrad(dims, Bm), c, adv_norm, ent_coef, clipped=False)
    assert np.array_equal(v, v0) and np.array_equal(logp, logp0)


def test_the_clipped_gradient_differs_from_the_plain_one():
    """Both branches run (ppo_vclip_data asserts the share over the batch): the critic's gradient and the value loss
    move, the actor's gradient, log_std's and the other three stats keep their bits."""
    dims, B, Bm, seed = vd.CASES[2]
    c = vd.case(dims, B, Bm, seed, True)
    (ga, gc, gl, st), _, _ = vd.host_run(PPOGrad(dims, Bm), c, True, 0.01)
    (pa, pc, pl, ps), _, _ = vd.host_run(PPOGrad(dims, Bm), c, True, 0.01, clipped=False)
    assert np.array_equal(ga, pa) and np.array_equal(gl, pl) and np.array_equal(st[[0, 2, 3]], ps[[0, 2, 3]])
    assert not np.array_equal(gc, pc) and st[1] > ps[1]   # the mean of a maximum


def _io(c, IO=_native.PPOGradIO2, **over):
    """A valid pbg_ppo_grad_io_t of case `c` (of struct version `IO`) and what keeps its arrays alive."""
    dims = c["dims"]
    keep = dict(ga=np.full(pd.param_count(dims), np.nan, np.float32),
                gc=np.full(pd.param_count(pd.critic_dims(dims)), np.nan, np.float32), gl=np.full(dims[3], np.nan, np.float32),
                st=np.full(4, np.nan), logp=np.full(c["Bm"], np.nan, np.float32), v=np.full(c["Bm"], np.nan, np.float32))
    p = lambda a: a.ctypes.data  # noqa: E731
    kw = dict(batch_rows=c["B"], mb_rows=c["Bm"], theta_actor=p(c["theta_actor"]), theta_critic=p(c["theta_critic"]),
              log_std=p(c["log_std"]), mean=p(c["mean"]), inv_std=p(c["inv_std"]), clip=c["clip"], clip_eps=0.2, vf_coef=0.5,
              ent_coef=0.01, obs=p(c["obs"]), act=p(c["act"]), logp_old=p(c["logp_old"]), adv=p(c["adv"]), ret=p(c["ret"]),
              idx=p(c["idx"]), adv_norm=p(c["adv_norm"]), grad_actor=p(keep["ga"]), grad_critic=p(keep["gc"]),
              grad_log_std=p(keep["gl"]), stats=p(keep["st"]), logp_out=p(keep["logp"]), v_out=p(keep["v"]))
    kw.update(over)
    return IO(**kw), keep


def _same(a, b):
    return all(a[k].tobytes() == b[k].tobytes() for k in a)


def test_value_old_none_is_the_first_version_struct():
    """The new struct with value_old and gate NULL against the struct that ends with v_out: array_equal outputs,
    the bits of stats[1] included."""
    L = _native.lib()
    assert ctypes.sizeof(_native.PPOGradIO) == 176 and ctypes.sizeof(_native.PPOGradIO2) == 200
    for dims, B, Bm, seed in vd.CASES:
        c = vd.case(dims, B, Bm, seed, True)
        old, keep_old = _io(c, _native.PPOGradIO)
        new, keep_new = _io(c, _native.PPOGradIO2)
        assert old.struct_size == 176 and new.struct_size == 200
        assert L.pbg_ppo_grad_host(*dims, ctypes.byref(old)) == 0 and L.pbg_ppo_grad_host(*dims, ctypes.byref(new)) == 0
        assert np.isfinite(keep_old["ga"]).all() and np.isfinite(keep_old["st"]).all()
        assert _same(keep_old, keep_new), (dims, Bm)


def test_a_clip_that_never_binds_is_no_clipping():
    """vf_clip = 1e30: no row is clamped, max(u1, u1) = u1, and every output has the bits of a run without value_old."""
    L = _native.lib()
    for dims, B, Bm, seed in vd.CASES:
        c = vd.case(dims, B, Bm, seed, True)
        plain, keep_plain = _io(c)
        huge, keep_huge = _io(c, value_old=c["value_old"].ctypes.data, vf_clip=1e30)
        assert L.pbg_ppo_grad_host(*dims, ctypes.byref(plain)) == 0 and L.pbg_ppo_grad_host(*dims, ctypes.byref(huge)) == 0
        assert _same(keep_plain, keep_huge), (dims, Bm)


def test_argument_errors_before_any_work():
    L = _native.lib()
    dims, B, Bm, seed = vd.CASES[2]
    c = vd.case(dims, B, Bm, seed, True)
    vo = c["value_old"].ctypes.data
    io, keep = _io(c, value_old=vo, vf_clip=0.2)
    assert L.pbg_ppo_grad_host(*dims, ctypes.byref(io)) == 0 and np.isfinite(keep["ga"]).all()
    for bad_clip in (0.0, -0.2, float("nan")):
        bad, keep = _io(c, value_old=vo, vf_clip=bad_clip)
        assert L.pbg_ppo_grad_host(*dims, ctypes.byref(bad)) == -1, bad_clip
        assert b"vf_clip" in L.pbg_last_error()
        assert all(np.isnan(a).all() for a in keep.values()), bad_clip
    # vf_clip is not looked at without value_old
    ok, _ = _io(c, vf_clip=-1.0)
    assert L.pbg_ppo_grad_host(*dims, ctypes.byref(ok)) == 0
    # the struct's versions: exactly 176 and 200
    for size, want in ((176, 0), (200, 0), (176 + 4, -1), (200 - 4, -1), (200 + 4, -1), (176 - 4, -1), (188, -1)):
        probe, keep = _io(c)
        # the struct followed by readable zero bytes: a size past its end is refused by its value
        buf = (ctypes.c_char * (ctypes.sizeof(probe) + 16))()
        ctypes.memmove(buf, ctypes.byref(probe), ctypes.sizeof(probe))
        ctypes.cast(buf, ctypes.POINTER(ctypes.c_uint32))[0] = size
        assert L.pbg_ppo_grad_host(*dims, ctypes.cast(buf, ctypes.POINTER(_native.PPOGradIO))) == want, size
        if want:
            assert b"struct_size" in L.pbg_last_error() and np.isnan(keep["ga"]).all()


def test_wrapper_strictness():
    dims, B, Bm, seed = vd.CASES[2]
    c = vd.case(dims, B, Bm, seed, True)
    g = PPOGrad(dims, Bm)
    vo = c["value_old"]
    for kw in (dict(value_old=vo), dict(vf_clip=0.2), dict(value_old=vo.astype(np.float64), vf_clip=0.2),
               dict(value_old=vo[:-1], vf_clip=0.2), dict(value_old=vo[:, None], vf_clip=0.2),
               dict(value_old=np.concatenate((vo, vo))[::2], vf_clip=0.2), dict(value_old=vo.tolist(), vf_clip=0.2),
               dict(value_old=vo, vf_clip=0.0), dict(value_old=vo, vf_clip=float("nan")),
               dict(gate=np.zeros(2, np.int64)), dict(gate=np.zeros(3, np.int32)), dict(gate=[0, 0])):
        with pytest.raises(_native.PbgError):
            vd.host_run(g, c, True, 0.01, clipped=False, **kw)


def test_the_symbols_are_exported():
    assert set(_native.PPO_GATE_EXPORTED) == {"pbg_ppo_gate_reset", "pbg_ppo_gate", "pbg_ppo_gate_host"}
    assert set(_native.PPO_GATE_EXPORTED) <= set(_native.EXPORTED)
    for f in _native.PPO_GATE_EXPORTED:
        assert hasattr(_native.lib(), f), f
