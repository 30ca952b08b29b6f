"""Counter-based permutations, the optimiser's learning rate from memory and the linear schedule on the host
(include/pbg.h "Counter-based permutations and an on-device learning rate": pbg_perm_host, pbg_ppo_opt_host with lr_ptr,
pbg_ppo_lr_linear_host, ppo.Permutation / ppo.lr_linear / ppo.AdamClip without a device; no GPU): bit for bit against
the numpy mirrors of pybulletgym_amd.rng, against the pins of tests/perm_data.py, the uniformity of the construction,
and the argument checks that come before any HIP call."""
import ctypes

import numpy as np
import pytest

import pybulletgym_amd  # noqa: F401
from pybulletgym_amd import _native, rng
from pybulletgym_amd.ppo import AdamClip, Permutation, lr_linear

import perm_data as pd
import ppo_opt_data as od

E_ARG = -1  # PBG_E_ARG


def host_perm(seed, counter, B, n_perms=1):
    out = np.full((n_perms, B), -1, np.int64)
    assert _native.lib().pbg_perm_host(seed, counter, B, n_perms, out.ctypes.data) == 0
    return out


@pytest.mark.parametrize("B", pd.SIZES)
def test_perm_host_is_the_numpy_mirror_and_a_bijection(B):
    for seed in pd.SEEDS:
        for c in pd.COUNTERS:
            got = host_perm(seed, c, B)[0]
            assert np.array_equal(got, rng.permutation(B, seed, c)), (seed, c)
            assert np.array_equal(np.sort(got), np.arange(B)), (seed, c)
            three = host_perm(seed, c, B, 3)   # n_perms = 3 at c: the rows at c, c + 1, c + 2 (the counter wraps)
            for j in range(3):
                assert np.array_equal(three[j], host_perm(seed, (c + j) % 2 ** 32, B)[0]), (seed, c, j)


@pytest.mark.parametrize("seed,counter,B,first,wsum", pd.PINS)
def test_the_pins_of_the_construction(seed, counter, B, first, wsum):
    for p in (host_perm(seed, counter, B)[0], rng.permutation(B, seed, counter)):
        assert tuple(p[:8]) == first
        if wsum is not None:
            assert pd.weighted_sum(p) == wsum


def test_the_round_keys_pin():
    assert tuple(int(k) for k in rng.permutation_keys(pd.SEED, 7)) == pd.KEYS_7


def test_the_host_object_keeps_its_counter_and_wraps():
    p = Permutation(pd.SEED)
    assert p.host and p.counter == 0
    a = p.fill(17, 2)
    assert p.counter == 2 and a.shape == (2, 17) and a.dtype == np.int64
    assert np.array_equal(a[1], rng.permutation(17, pd.SEED, 1))
    p.counter = 2 ** 32 - 1
    b = p.fill(17, 3)
    assert p.counter == 2   # 2^32 - 1, 0, 1
    for j, c in enumerate((2 ** 32 - 1, 0, 1)):
        assert np.array_equal(b[j], rng.permutation(17, pd.SEED, c))
    out = np.zeros((1, 5), np.int64)
    assert p.fill(5, out=out) is out and np.array_equal(out[0], rng.permutation(5, pd.SEED, 2))
    for bad in (dict(B=0), dict(B=5, n_perms=0), dict(B=5, n_perms=65536), dict(B=5, out=np.zeros((1, 5), np.int32)),
                dict(B=5, out=np.zeros((2, 5), np.int64)), dict(B=5, out=np.zeros((5, 2), np.int64).T)):
        with pytest.raises(_native.PbgError):
            p.fill(**bad)
    assert p.counter == 3


@pytest.mark.parametrize("seed", (12345, pd.SEED))
def test_uniformity_of_positions_and_adjacent_pairs(seed):
    """B = 64 over the counters 0 .. 8191: |z| <= 4 for the position-by-value table and for the ordered adjacent pairs
    (perm_data.uniformity_z).  A condition on the construction, not a measurement: the numpy restatement gave 1.07 and
    -1.14 at seed 12345, 1.56 (positions) at the other seed."""
    perms = host_perm(seed, 0, 64, 8192)
    z_pos, z_adj = pd.uniformity_z(perms)
    print(f"seed {seed:#x}: z positions {z_pos:.2f}, adjacent pairs {z_adj:.2f}")
    assert abs(z_pos) <= 4.0 and abs(z_adj) <= 4.0


@pytest.mark.parametrize("N", pd.SCHEDULE_N)
def test_lr_linear_host_is_the_numpy_expression(N):
    for lr0 in pd.SCHEDULE_LR0:
        for it in pd.schedule_its(N):
            got = lr_linear(np.array([it], np.uint32), N, lr0)
            want = np.float64(lr0) * (np.float64(1.0) - np.float64(min(it, N)) / np.float64(N))
            assert got.dtype == np.float64 and got[0].tobytes() == want.tobytes(), (N, lr0, it)
            assert rng.lr_linear(it, N, lr0) == got[0]
    assert lr_linear(np.array([N], np.uint32), N, 3e-4)[0] == 0.0 and lr_linear(np.array([0], np.uint32), N, 3e-4)[0] == 3e-4


def io_of(cls, sizes, params, grads, state, lr, max_grad_norm, **kw):
    ptrs = lambda arrs: [a.ctypes.data for a in arrs]
    return cls(param=ptrs(params), grad=ptrs(grads), m=ptrs(state["m"]), v=ptrs(state["v"]), t=state["t"].ctypes.data,
               bpow=state["bpow"].ctypes.data, lr=lr, beta1=od.BETAS[0], beta2=od.BETAS[1], eps=od.EPS,
               max_grad_norm=max_grad_norm, **kw)


def host_state(sizes):
    return dict(m=[np.zeros(s, np.float32) for s in sizes], v=[np.zeros(s, np.float32) for s in sizes],
                t=np.zeros(1, np.uint32), bpow=np.ones(2))


@pytest.mark.parametrize("sizes", od.SIZES)
@pytest.mark.parametrize("max_grad_norm", (0.0, 0.5))
def test_opt_host_with_lr_ptr_gives_the_bits_of_lr(sizes, max_grad_norm):
    """Five steps with a learning rate that changes every step: read through lr_ptr (``AdamClip.step(lr=array)``), passed
    as the float, and the numpy restatement."""
    a, b, ref = AdamClip(sizes), AdamClip(sizes), od.new_state(sizes)
    pa, pb, pr = od.params0(sizes), od.params0(sizes), od.params0(sizes)
    lr = np.zeros(1)
    for s in range(5):
        lr[0] = od.LR * (1.0 - s / 7.0)
        g = od.grads_of(sizes, s)
        a.step(pa, g, lr, od.BETAS, od.EPS, max_grad_norm)
        b.step(pb, g, float(lr[0]), od.BETAS, od.EPS, max_grad_norm)
        od.opt_step_ref(ref, pr, g, lr=float(lr[0]), max_grad_norm=max_grad_norm)
        for x, y, z in zip(pa, pb, pr):
            assert np.array_equal(x, y) and np.array_equal(x, z), (sizes, s)
    for x, y in zip(a.state()[0] + a.state()[1], b.state()[0] + b.state()[1]):
        assert np.array_equal(x, y)


def test_the_previous_struct_size_is_accepted_and_behaves_as_today():
    """A caller built with the struct that ends with bpow: its size is accepted and lr_ptr is NULL for it, whatever lies
    behind its struct; the sizes in between and beyond are refused."""
    L = _native.lib()
    IO, IO2 = _native.PPOOptIO, _native.PPOOptIO2
    assert ctypes.sizeof(IO2) == ctypes.sizeof(IO) + ctypes.sizeof(ctypes.c_void_p) == 336
    assert IO2.lr_ptr.offset == ctypes.sizeof(IO)
    sizes = (8, 6, 1)
    csz = (ctypes.c_int64 * 3)(*sizes)
    g = od.grads_of(sizes, 0)
    results = []
    other = np.array([123.0])
    for cls, size, kw in ((IO, None, {}), (IO2, None, {}), (IO2, ctypes.sizeof(IO), dict(lr_ptr=other.ctypes.data))):
        p, st = od.params0(sizes), host_state(sizes)
        io = io_of(cls, sizes, p, g, st, od.LR, 0.5, **kw)
        if size is not None:
            io.struct_size = size   # the old size: the library must not read the pointer behind it
        assert L.pbg_ppo_opt_host(3, csz, ctypes.byref(io)) == 0 and st["t"][0] == 1
        results.append(p)
    ref, pr = od.new_state(sizes), od.params0(sizes)
    od.opt_step_ref(ref, pr, g, max_grad_norm=0.5)
    for p in results:
        for x, y in zip(p, pr):
            assert np.array_equal(x, y)
    p, st = od.params0(sizes), host_state(sizes)
    io = io_of(IO2, sizes, p, g, st, od.LR, 0.5)
    for size in (ctypes.sizeof(IO) + 4, ctypes.sizeof(IO2) + 4, ctypes.sizeof(IO) - 4, ctypes.sizeof(IO2) + 8):
        io.struct_size = size
        assert L.pbg_ppo_opt_host(3, csz, ctypes.byref(io)) == E_ARG, size
        assert b"struct_size" in L.pbg_last_error()
    assert st["t"][0] == 0


def test_argument_errors_before_any_hip_call():
    L = _native.lib()
    out = np.zeros((2, 5), np.int64)
    assert L.pbg_perm_host(1, 0, 5, 2, out.ctypes.data) == 0
    for n_rows, n_perms, ptr in ((0, 1, out.ctypes.data), (-3, 1, out.ctypes.data), (5, 0, out.ctypes.data),
                                 (5, -1, out.ctypes.data), (5, 65536, out.ctypes.data), (5, 1, None)):
        assert L.pbg_perm_host(1, 0, n_rows, n_perms, ptr) == E_ARG, (n_rows, n_perms)
        assert b"pbg_perm_host" in L.pbg_last_error()
        assert L.pbg_perm_fill(None, n_rows, n_perms, ptr, None) == E_ARG
    h = ctypes.c_void_p(0x1234)
    assert L.pbg_perm_create(-1, 1, ctypes.byref(h)) == E_ARG and not h.value   # *out is NULL after a failure
    assert L.pbg_perm_create(0, 1, None) == E_ARG
    assert L.pbg_perm_fill(None, 5, 1, out.ctypes.data, None) == E_ARG
    assert L.pbg_perm_set_counter(None, 3, None) == E_ARG
    assert L.pbg_perm_get_counter(None, out.ctypes.data, None) == E_ARG
    L.pbg_perm_destroy(None)
    it, lr = np.zeros(1, np.uint32), np.zeros(1)
    for f, tail in ((L.pbg_ppo_lr_linear_host, ()), (L.pbg_ppo_lr_linear, (None,))):
        assert f(it.ctypes.data, 0, 1e-3, lr.ctypes.data, *tail) == E_ARG
        assert f(None, 5, 1e-3, lr.ctypes.data, *tail) == E_ARG
        assert f(it.ctypes.data, 5, 1e-3, None, *tail) == E_ARG
    with pytest.raises(_native.PbgError):
        lr_linear(it, 0, 1e-3)
    with pytest.raises(_native.PbgError):
        lr_linear(np.zeros(1, np.int64), 5, 1e-3)
    sizes = (3, 2)
    opt = AdamClip(sizes)
    p, g = od.params0(sizes), od.grads_of(sizes, 0)
    for bad in (np.zeros(2), np.zeros(1, np.float32), np.zeros((1, 1))):
        with pytest.raises(_native.PbgError):
            opt.step(p, g, bad)
    with pytest.raises(ValueError):
        rng.permutation(0, 1, 0)


def test_a_build_without_permutations_says_so(monkeypatch):
    real = _native.lib()

    class Old:
        def __getattr__(self, name):
            if name.startswith("pbg_perm") or name.startswith("pbg_ppo_lr"):
                raise AttributeError(name)
            return getattr(real, name)

    monkeypatch.setattr(_native, "_lib", Old())
    with pytest.raises(_native.PbgError, match="a build without counter-based permutations"):
        Permutation(1)
    with pytest.raises(_native.PbgError, match="a build without counter-based permutations"):
        lr_linear(np.zeros(1, np.uint32), 5, 1e-3)
