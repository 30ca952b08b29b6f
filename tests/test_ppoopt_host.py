"""The advantage normaliser and the clip + Adam step on the host (include/pbg.h "PPO optimiser step",
pbg_adv_norm_host, pbg_ppo_opt_host, ppo.adv_norm and ppo.AdamClip without a device; no GPU): bit for bit against the
numpy restatement of tests/ppo_opt_data.py, against torch's Adam + clip_grad_norm_ under section 14's bound, and
the argument checks that come before any HIP call."""
import ctypes

import numpy as np
import pytest

import pybulletgym_amd  # noqa: F401
from pybulletgym_amd import _native
from pybulletgym_amd.ppo import AdamClip, PPOGrad, adv_norm

import ppo_opt_data as od

E_ARG = -1  # PBG_E_ARG


def advantages(B, seed=0):
    rng = np.random.default_rng(seed)
    return (0.3 + 2.0 * rng.standard_normal(B)).astype(np.float32)


@pytest.mark.parametrize("Bm", od.ADV_ROWS)
def test_adv_norm_host_is_the_numpy_restatement(Bm):
    adv = advantages(Bm, Bm)
    out = adv_norm(adv)
    assert out.dtype == np.float32 and np.array_equal(out, od.adv_norm_ref(adv))
    # against numpy's own mean and std (another order): a few float32 ulps
    a = adv.astype(np.float64)
    assert abs(out[0] - a.mean()) <= 1e-6 * max(1.0, abs(a.mean())) and abs(out[1] * (a.std(ddof=1) + 1e-8) - 1.0) <= 1e-6
    # a permutation prefix of a larger batch
    B = 2 * Bm + 5
    big = advantages(B, Bm + 1)
    idx = np.random.default_rng(Bm).permutation(B)[:Bm].astype(np.int64)
    got = adv_norm(big, idx)
    assert np.array_equal(got, od.adv_norm_ref(big, idx))
    assert np.array_equal(got, adv_norm(np.ascontiguousarray(big[idx])))
    assert np.array_equal(adv_norm(big, np.arange(Bm, dtype=np.int64)), od.adv_norm_ref(big[:Bm]))


@pytest.mark.parametrize("Bm,value", od.CONSTANT)
def test_adv_norm_of_constant_advantages(Bm, value):
    """var is exactly 0: the shift is the value, the scale 1e8 and every normalised value 0, also through idx."""
    adv = np.full(Bm, value, np.float32)
    for out in (adv_norm(adv), adv_norm(np.full(2 * Bm, value, np.float32), np.arange(Bm, dtype=np.int64)[::-1].copy())):
        assert np.array_equal(out, od.adv_norm_ref(adv))
        assert out[0] == np.float32(value) and out[1] == np.float32(1e8), out
        assert ((adv - out[0]) * out[1] == 0.0).all()


def test_adv_norm_of_a_small_spread_about_a_large_mean():
    """What the shift by the first advantage buys besides the constant case: a spread of 1e-3 about 6836.862 keeps
    its scale to float32 accuracy (float64 two-pass numpy as truth)."""
    rng = np.random.default_rng(5)
    adv = (6836.862 + 1e-3 * rng.standard_normal(1537)).astype(np.float32)
    out, a = adv_norm(adv), adv.astype(np.float64)
    assert np.array_equal(out, od.adv_norm_ref(adv))
    assert out[0] == np.float32(a.mean()) and abs(out[1] * (a.std(ddof=1) + 1e-8) - 1.0) <= 1e-6


def test_adv_norm_argument_errors():
    L = _native.lib()
    adv, out = advantages(8), np.zeros(2, np.float32)
    idx = np.arange(4, dtype=np.int64)
    a, o, i = adv.ctypes.data, out.ctypes.data, idx.ctypes.data
    assert L.pbg_adv_norm_host(8, 4, a, i, o) == 0
    for args in ((8, 1, a, i, o), (8, 0, a, None, o), (0, 4, a, i, o), (8, 9, a, None, o), (8, 4, None, i, o), (8, 4, a, i, None)):
        assert L.pbg_adv_norm_host(*args) == E_ARG, args
        assert L.pbg_adv_norm(*args, None) == E_ARG, args   # refused before any HIP call
    for bad in (-1, 8):
        idx[2] = bad
        assert L.pbg_adv_norm_host(8, 4, a, i, o) == E_ARG
        with pytest.raises(_native.PbgError):
            adv_norm(adv, idx)
    with pytest.raises(_native.PbgError):
        adv_norm(adv.astype(np.float64))
    with pytest.raises(_native.PbgError):
        adv_norm(adv, np.arange(4, dtype=np.int32))


def run_host(sizes, steps, max_grad_norm, zero_block=None, seed=0):
    """``steps`` steps of AdamClip on the host beside the restatement; asserts bit equality after every step."""
    opt, ref = AdamClip(sizes), od.new_state(sizes)
    p, q = od.params0(sizes, seed), od.params0(sizes, seed)
    coefs, info = [], np.zeros(2)
    for s in range(steps):
        g = od.grads_of(sizes, s, seed, zero_block)
        opt.step(p, g, od.LR, od.BETAS, od.EPS, max_grad_norm, info=info)
        norm, coef = od.opt_step_ref(ref, q, g, max_grad_norm=max_grad_norm)
        m, v, t = opt.state()
        assert int(t[0]) == s + 1 == ref["t"]
        assert info[0] == norm and info[1] == coef, (s, info, norm, coef)
        for b in range(len(sizes)):
            assert np.array_equal(p[b], q[b]) and np.array_equal(m[b], ref["m"][b]) and np.array_equal(v[b], ref["v"][b]), (s, b)
        coefs.append(coef)
    return p, coefs


@pytest.mark.parametrize("max_grad_norm", (0.0, 0.5))
@pytest.mark.parametrize("sizes", od.SIZES)
def test_opt_host_is_the_numpy_restatement(sizes, max_grad_norm):
    g = PPOGrad((44, 65, 129, 17), 1)   # the trainer's three blocks at that pair, from the layout
    assert od.SIZES[3] == (g.Da, g.Dc, 17) == (13649, 11569, 17)
    p, coefs = run_host(sizes, 5, max_grad_norm)
    assert all(np.isfinite(b).all() for b in p)
    if max_grad_norm:   # clipping active on some steps and not on others
        assert any(c < 1.0 for c in coefs) and any(c == 1.0 for c in coefs), coefs
    else:
        assert all(c == 1.0 for c in coefs)


@pytest.mark.parametrize("sizes,zero", (((8, 6, 1), 1), ((255, 256, 257), 0), ((13649, 11569, 17), 2)))
def test_a_block_of_zero_gradients_does_not_move(sizes, zero):
    p, _ = run_host(sizes, 5, 0.5, zero_block=zero)
    p0 = od.params0(sizes)
    assert np.array_equal(p[zero], p0[zero])
    assert all(not np.array_equal(p[b], p0[b]) for b in range(len(sizes)) if b != zero)


def test_reset_starts_over():
    sizes = (8, 6, 1)
    opt = AdamClip(sizes)
    first = od.params0(sizes)
    for s in range(2):
        opt.step(first, od.grads_of(sizes, s), od.LR, od.BETAS, od.EPS, 0.5)
    opt.reset()
    assert int(opt.state()[2][0]) == 0 and not any(m.any() for m in opt.state()[0])
    again = od.params0(sizes)
    for s in range(2):
        opt.step(again, od.grads_of(sizes, s), od.LR, od.BETAS, od.EPS, 0.5)
    assert all(np.array_equal(a, b) for a, b in zip(first, again))


@pytest.mark.parametrize("max_grad_norm", (0.0, 0.5))
@pytest.mark.parametrize("sizes", od.SIZES)
def test_opt_host_against_torch_adam(sizes, max_grad_norm):
    """Five steps against torch.optim.Adam + clip_grad_norm_ on float64 copies: per block the movement's error is at
    most max(4 err(the same torch code in float32), 1e-5)."""
    opt, p = AdamClip(sizes), od.params0(sizes)
    for s in range(5):
        opt.step(p, od.grads_of(sizes, s), od.LR, od.BETAS, od.EPS, max_grad_norm)
    worst = od.check_movement(p, sizes, 5, max_grad_norm, f"sizes {sizes} max_grad_norm {max_grad_norm}")
    print(f"sizes {sizes} max_grad_norm {max_grad_norm}: worst err / err_torch32 {worst:.3f}")


def test_struct_layout_and_versioning():
    IO = _native.PPOOptIO
    ptr, nb = ctypes.sizeof(ctypes.c_void_p), _native.PPO_OPT_MAX_BLOCKS
    assert nb == 8
    want, at = {}, 8   # struct_size, reserved
    for name, size in (("param", nb * ptr), ("grad", nb * ptr), ("lr", 8), ("beta1", 8), ("beta2", 8), ("eps", 8),
                       ("max_grad_norm", 8), ("info", ptr), ("m", nb * ptr), ("v", nb * ptr), ("t", ptr), ("bpow", ptr)):
        want[name] = at
        at += size
    assert IO.struct_size.offset == 0 and IO.reserved.offset == 4
    for name, off in want.items():
        assert getattr(IO, name).offset == off, name
    assert ctypes.sizeof(IO) == at == 328 and at % 4 == 0   # the first version ends with bpow
    sizes = (3, 2)
    csz = (ctypes.c_int64 * 2)(*sizes)
    arrs = {k: [np.zeros(s, np.float32) for s in sizes] for k in ("param", "grad", "m", "v")}
    t, bpow = np.zeros(1, np.uint32), np.ones(2)
    io = IO(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, t=t.ctypes.data, bpow=bpow.ctypes.data,
            **{k: [a.ctypes.data for a in v] for k, v in arrs.items()})
    L = _native.lib()
    assert io.struct_size == 328 and L.pbg_ppo_opt_host(2, csz, ctypes.byref(io)) == 0 and t[0] == 1
    for size in (328 - 4, 328 + 4, 328 - 2, 328 + 2, 0):
        io.struct_size = size
        assert L.pbg_ppo_opt_host(2, csz, ctypes.byref(io)) == E_ARG, size
    assert t[0] == 1
    assert b"struct_size" in L.pbg_last_error()


@pytest.mark.parametrize("bad", (np.nan, np.inf))
@pytest.mark.parametrize("max_grad_norm", (0.0, 0.5))
def test_a_non_finite_gradient_propagates_as_the_header_says(bad, max_grad_norm):
    """One NaN or infinite gradient element in block 1, after one ordinary step (so the moments are not zero)."""
    sizes = (8, 6, 1)
    opt, ref = AdamClip(sizes), od.new_state(sizes)
    p, q = od.params0(sizes), od.params0(sizes)
    info = np.zeros(2)
    for s, poison in ((0, False), (1, True)):
        g = od.grads_of(sizes, s)
        if poison:
            g[1][2] = bad
            before = [a.copy() for a in p]
        opt.step(p, g, od.LR, od.BETAS, od.EPS, max_grad_norm, info=info)
        with np.errstate(invalid="ignore"):
            norm, coef = od.opt_step_ref(ref, q, g, max_grad_norm=max_grad_norm)
        for b in range(3):
            assert np.array_equal(p[b], q[b], equal_nan=True)
    m, v, _ = opt.state()
    hit = np.zeros(6, bool)
    hit[2] = True
    assert (np.isnan(info[0]) if np.isnan(bad) else np.isinf(info[0])) and np.isnan(p[1][2])
    if not max_grad_norm:        # coef 1: only the element whose own gradient is not finite
        assert info[1] == 1.0 and np.isfinite(p[0]).all() and np.isfinite(p[2]).all() and np.isfinite(p[1][~hit]).all()
    elif np.isnan(bad):          # coef NaN: every parameter and both moments of every block
        assert np.isnan(info[1]) and all(np.isnan(a).all() for a in p + m + v)
    else:                        # coef 0: inf * 0 = NaN there; elsewhere gd = 0 and the old moments alone move p
        assert info[1] == 0.0 and np.isfinite(p[0]).all() and np.isfinite(p[2]).all() and np.isfinite(p[1][~hit]).all()
        assert all(not np.array_equal(a, b, equal_nan=True) for a, b in zip(p, before))


def test_opt_argument_errors():
    L = _native.lib()
    sizes = (3, 2)
    csz = (ctypes.c_int64 * 2)(*sizes)
    arrs = {k: [np.zeros(s, np.float32) for s in sizes] for k in ("param", "grad", "m", "v")}
    t, bpow = np.zeros(1, np.uint32), np.ones(2)

    def io(**kw):
        base = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, t=t.ctypes.data, bpow=bpow.ctypes.data,
                    **{k: [a.ctypes.data for a in v] for k, v in arrs.items()})
        base.update(kw)
        return _native.PPOOptIO(**base)

    assert L.pbg_ppo_opt_host(2, csz, ctypes.byref(io())) == 0
    for bad in (dict(beta1=1.0), dict(beta1=-0.1), dict(beta2=1.0), dict(beta2=float("nan")), dict(eps=0.0), dict(eps=-1e-8),
                dict(param=[arrs["param"][0].ctypes.data, None]), dict(grad=[None, arrs["grad"][1].ctypes.data]),
                dict(m=[None, None]), dict(v=[arrs["v"][0].ctypes.data, None]), dict(t=None), dict(bpow=None)):
        assert L.pbg_ppo_opt_host(2, csz, ctypes.byref(io(**bad))) == E_ARG, bad
    assert L.pbg_ppo_opt_host(2, csz, None) == E_ARG
    for n in (0, 9, -1):
        many = (ctypes.c_int64 * 9)(*([1] * 9))
        assert L.pbg_ppo_opt_host(n, many, ctypes.byref(io())) == E_ARG
        h = ctypes.c_void_p()
        assert L.pbg_ppo_opt_create(0, n, many, ctypes.byref(h)) == E_ARG and not h   # before any HIP call
    zero = (ctypes.c_int64 * 2)(3, 0)
    assert L.pbg_ppo_opt_host(2, zero, ctypes.byref(io())) == E_ARG
    h = ctypes.c_void_p()
    assert L.pbg_ppo_opt_create(0, 2, zero, ctypes.byref(h)) == E_ARG and not h
    assert L.pbg_ppo_opt_create(0, 2, None, ctypes.byref(h)) == E_ARG
    assert L.pbg_ppo_opt_create(0, 2, csz, None) == E_ARG
    assert L.pbg_ppo_opt_step(None, ctypes.byref(io()), None) == E_ARG
    assert t[0] == 1
    for bad in ((), (1,) * 9, (3, 0)):
        with pytest.raises(_native.PbgError):
            AdamClip(bad)
    opt = AdamClip(sizes)
    with pytest.raises(_native.PbgError):
        opt.step(arrs["param"][:1], arrs["grad"], 1e-3)
    with pytest.raises(_native.PbgError):
        opt.step(arrs["param"], [a.astype(np.float64) for a in arrs["grad"]], 1e-3)
