"""The KL gate on the host (include/pbg.h "Value clipping and the KL gate": pbg_ppo_gate_host, and the gate that
pbg_ppo_grad_host and pbg_ppo_opt_host obey; ppo.KLGate without a device; no GPU): the gate's arithmetic on hand-made
stats, a stopped gradient and a stopped step leave everything as it is, the optimiser struct's three versions, and the
gated chain of tests/ppo_klgate_data.py against the ungated one cut at the step that trips."""
import ctypes

import numpy as np
import pytest

import pybulletgym_amd  # noqa: F401
from pybulletgym_amd import _native
from pybulletgym_amd.ppo import AdamClip, KLGate, PPOGrad, adv_norm

import ppo_grad_data as pd
import ppo_klgate_data as kd
import ppo_opt_data as od

E_ARG = -1


def test_gate_arithmetic():
    """Below and equal count a step, above stops, a NaN counts a step (the comparison is false), and a stopped gate
    stays as it is whatever comes."""
    g = KLGate()
    assert g.host and g.gate.dtype == np.int32 and g.gate.tolist() == [0, 0]
    st = lambda kl: np.array([0.1, 0.2, 0.3, kl])  # noqa: E731
    for kl, want in ((0.01, [0, 1]), (0.03, [0, 2]), (float("nan"), [0, 3]), (-5.0, [0, 4]), (np.nextafter(0.03, 1.0), [1, 4]),
                     (0.0, [1, 4]), (float("nan"), [1, 4]), (1.0, [1, 4])):
        g.check(st(kl), 0.03)
        assert g.gate.tolist() == want, (kl, g.gate)
    state = g.state
    assert state.tolist() == [1, 4] and state is not g.gate
    g.reset()
    assert g.gate.tolist() == [0, 0]
    g.check(st(float("inf")), 1e300)
    assert g.gate.tolist() == [1, 0]
    L = _native.lib()
    s, w = st(0.0), np.zeros(2, np.int32)
    assert L.pbg_ppo_gate_host(None, 0.0, w.ctypes.data) == E_ARG and L.pbg_ppo_gate_host(s.ctypes.data, 0.0, None) == E_ARG
    # the device entries refuse these before any HIP call
    assert L.pbg_ppo_gate(None, 0.0, w.ctypes.data, None) == E_ARG and L.pbg_ppo_gate(s.ctypes.data, 0.0, None, None) == E_ARG
    assert L.pbg_ppo_gate_reset(None, None) == E_ARG
    for bad in (np.zeros(4, np.float32), np.zeros(3), [0.0] * 4):
        with pytest.raises(_native.PbgError):
            g.check(bad, 0.03)


def _grad_run(g, c, gate, **out):
    return g.run(c["theta_actor"], c["theta_critic"], c["log_std"], c["obs"], c["act"], c["logp_old"], c["adv"], c["ret"],
                 idx=c["idx"], adv_norm=c["adv_norm"], clip_eps=pd.CLIP_EPS, vf_coef=pd.VF_COEF, ent_coef=0.01, gate=gate, **out)


def test_a_stopped_gradient_and_a_stopped_step_write_nothing():
    dims, B, Bm, seed = pd.CASES[2]
    c = pd.case(dims, B, Bm, seed, False)
    g = PPOGrad(dims, Bm)
    nan = lambda n, dt=np.float32: np.full(n, np.nan, dt)  # noqa: E731
    out = dict(grad_actor=nan(g.Da), grad_critic=nan(g.Dc), grad_log_std=nan(dims[3]), stats=nan(4, np.float64),
               logp_out=nan(Bm), v_out=nan(Bm))
    _grad_run(g, c, np.array([1, 7], np.int32), **out)
    assert all(np.isnan(a).all() for a in out.values())
    # an open gate is no gate
    open_ = {k: a.copy() for k, a in out.items()}
    _grad_run(g, c, np.array([0, 7], np.int32), **open_)
    none = {k: a.copy() for k, a in out.items()}
    _grad_run(g, c, None, **none)
    assert all(np.isfinite(a).all() and np.array_equal(a, none[k]) for k, a in open_.items())
    # the arguments are still checked when the gate is shut
    with pytest.raises(_native.PbgError):
        _grad_run(g, dict(c, idx=np.full(Bm, B, np.int64)), np.array([1, 0], np.int32), **out)

    sizes = (8, 6, 1)
    opt, info = AdamClip(sizes), np.full(2, np.nan)
    p = od.params0(sizes)
    opt.step(p, od.grads_of(sizes, 0), od.LR, od.BETAS, od.EPS, 0.5)
    before = ([a.copy() for a in p], *opt.state(), opt._bpow.copy())
    shut = np.array([1, 1], np.int32)
    opt.step(p, od.grads_of(sizes, 1), od.LR, od.BETAS, od.EPS, 0.5, info=info, gate=shut)
    m, v, t = opt.state()
    assert np.isnan(info).all() and shut.tolist() == [1, 1]
    assert int(t[0]) == 1 == int(before[3][0]) and np.array_equal(opt._bpow, before[4])
    for a, b in zip(p + m + v, before[0] + before[1] + before[2]):
        assert np.array_equal(a, b)
    # an open gate: the step of no gate
    q, ref = [a.copy() for a in p], AdamClip(sizes)
    ref._m, ref._v, ref._t, ref._bpow = [a.copy() for a in m], [a.copy() for a in v], t.copy(), opt._bpow.copy()
    opt.step(p, od.grads_of(sizes, 1), od.LR, od.BETAS, od.EPS, 0.5, info=info, gate=np.zeros(2, np.int32))
    ref.step(q, od.grads_of(sizes, 1), od.LR, od.BETAS, od.EPS, 0.5)
    assert np.isfinite(info).all() and int(opt.state()[2][0]) == 2
    assert all(np.array_equal(a, b) for a, b in zip(p + opt.state()[0], q + ref.state()[0]))
    for bad in (np.zeros(2, np.int64), np.zeros(1, np.int32), [0, 0]):
        with pytest.raises(_native.PbgError):
            opt.step(p, od.grads_of(sizes, 1), od.LR, gate=bad)


def test_the_optimiser_structs_three_versions():
    """328 (ends with bpow), 336 (lr_ptr) and 352 (gate and a reserved word) are accepted; 352 +- 4 and the sizes between
    are refused.  The issue asked for 344 as the third size; tests/test_perm_host.py pins 344 = 336 + 8 as refused, so
    the third version carries a reserved word and is 352 bytes, and 344 +- 4 and 344 itself stay refused."""
    assert [ctypes.sizeof(s) for s in (_native.PPOOptIO, _native.PPOOptIO2, _native.PPOOptIO3)] == [328, 336, 352]
    assert _native.PPOOptIO3.gate.offset == 336 and _native.PPOOptIO3.lr_ptr.offset == 328
    sizes = (3, 2)
    csz = (ctypes.c_int64 * 2)(*sizes)
    arrs = {k: [np.zeros(s, np.float32) for s in sizes] for k in ("param", "grad", "m", "v")}
    t, bpow = np.zeros(1, np.uint32), np.ones(2)
    L = _native.lib()
    io = _native.PPOOptIO3(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, t=t.ctypes.data, bpow=bpow.ctypes.data,
                           **{k: [a.ctypes.data for a in v] for k, v in arrs.items()})
    # the struct followed by readable zero bytes: a size past its end is refused by its value
    buf = (ctypes.c_char * (ctypes.sizeof(io) + 16))()
    ctypes.memmove(buf, ctypes.byref(io), ctypes.sizeof(io))
    steps = 0
    for size, want in ((328, 0), (336, 0), (352, 0), (352 - 4, E_ARG), (352 + 4, E_ARG), (332, E_ARG), (344, E_ARG),
                       (344 - 4, E_ARG), (360, E_ARG)):
        ctypes.cast(buf, ctypes.POINTER(ctypes.c_uint32))[0] = size
        assert L.pbg_ppo_opt_host(2, csz, buf) == want, size
        steps += want == 0
        assert t[0] == steps
        if want:
            assert b"struct_size" in L.pbg_last_error()


def chain(c, perm, kl_limit=None):
    """The host chain over the batch `c`: per step ``adv_norm``, ``PPOGrad.run``, with ``kl_limit`` the gate, and
    ``AdamClip.step``.  Returns (per-step stats [K, 4] as they stood after each gradient, per-step snapshots
    (params, m, v, t) after each step, the gate's final words or None)."""
    g, opt = PPOGrad(kd.DIMS, kd.BM), AdamClip(od.sizes_of(kd.DIMS))
    params = [c[k].copy() for k in ("theta_actor", "theta_critic", "log_std")]
    grads = [np.full_like(p, np.nan) for p in params]
    stats, an = np.full(4, np.nan), np.zeros(2, np.float32)
    gate = KLGate() if kl_limit is not None else None
    kw = {} if gate is None else dict(gate=gate.gate)
    if gate is not None:
        gate.gate[:] = (1, 99)   # a reset starts the chain
        gate.reset()
    all_stats, snaps = [], []
    for e in range(kd.EPOCHS):
        for idx in perm[e]:
            adv_norm(c["adv"], idx, out=an)
            g.run(*params, c["obs"], c["act"], c["logp_old"], c["adv"], c["ret"], idx=idx, adv_norm=an, clip_eps=pd.CLIP_EPS,
                  vf_coef=pd.VF_COEF, ent_coef=kd.ENT_COEF, grad_actor=grads[0], grad_critic=grads[1], grad_log_std=grads[2],
                  stats=stats, **kw)
            if gate is not None:
                gate.check(stats, kl_limit)
            opt.step(params, grads, kd.LR, kd.BETAS, kd.EPS, kd.MAX_GRAD_NORM, **kw)
            all_stats.append(stats.copy())
            m, v, t = opt.state()
            snaps.append(([p.copy() for p in params], m, v, int(t[0])))
    return np.array(all_stats), snaps, None if gate is None else gate.state


def test_the_gated_chain_is_the_ungated_one_cut_at_the_step_that_trips():
    c, seed = kd.batch()
    perm = kd.permutations(seed)
    free_stats, free, _ = chain(c, perm)
    kl = free_stats[:, 3]
    assert free[-1][3] == kd.K and np.isfinite(free_stats).all()
    stops = kd.stops(kl)
    print(f"batch seed {seed}; kl per step {kl.tolist()}; records {kd.records(kl)}; stops {stops}")
    start = [c[k] for k in ("theta_actor", "theta_critic", "log_std")]
    for j, limit in stops:
        st, snaps, gate = chain(c, perm, limit)
        assert gate.tolist() == [1, j], (j, gate)
        want = free[j - 1]
        got = snaps[-1]
        assert got[3] == want[3] == j
        for a, b in zip(got[0] + got[1] + got[2], want[0] + want[1] + want[2]):
            assert np.array_equal(a, b), j
        assert not any(np.array_equal(a, b) for a, b in zip(got[0], start))
        # the stats are the tripping step's, from the first stopped step to the last
        assert all(np.array_equal(s, free_stats[j]) for s in st[j:]) and np.array_equal(st[:j], free_stats[:j])
    # a limit nothing reaches: the ungated chain's bits, every step counted
    st, snaps, gate = chain(c, perm, 1e9)
    assert gate.tolist() == [0, kd.K] and np.array_equal(st, free_stats)
    for a, b in zip(snaps[-1][0] + snaps[-1][1] + snaps[-1][2], free[-1][0] + free[-1][1] + free[-1][2]):
        assert np.array_equal(a, b)
