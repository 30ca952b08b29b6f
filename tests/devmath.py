"""Shared by test_devmath_host.py, test_devmath_gpu.py and test_sincos64.py: the ctypes binding of the
test-only library libpbg_devtest.so (pybullet-gym_amd/csrc/pbg_devtest.hip, `make devtest`), the
argument sets, and the high-precision references (each computed once per process and never modified).

The float64 sin / cos contract (pbg_sincos64.h):  |err| <= 1 ulp(ref) + (|n| + 1) 2^-87,  n = rint(x 2/pi).
"""
import ctypes
import functools
import os

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.path.join(REPO, "pybullet-gym_amd", "libpbg_devtest.so")
N_MAX = 63662  # rint(1e5 2/pi): N_MAX pi/2 = 100,000.036


@functools.lru_cache(maxsize=None)
def lib():
    """A missing library is an error, never a skip: build it with `python __graft_entry__.py` (or
    `make -C pybullet-gym_amd devtest`)."""
    assert os.path.exists(LIB_PATH), f"{LIB_PATH} is missing: run `make -C pybullet-gym_amd devtest`"
    L = ctypes.CDLL(LIB_PATH)
    for name in dir_symbols():
        fn = getattr(L, name)
        fn.restype = None if name.endswith("_host") else ctypes.c_int
    return L


def dir_symbols():
    names = ["sincos32_dev", "sincos32_host", "sincos64_dev", "sincos64_host", "rcp32_dev", "sqrt32_dev", "rsq32_dev",
             "rcp64_dev", "sqrt64_dev", "clamp32_dev", "clamp64_dev", "quad_sum_f32_dev", "quad_sum_f64_dev",
             "quad_sum_i32_dev", "row_pair_swap_f32_dev", "row_pair_swap_u32_dev", "row_pair_swap_f64_dev",
             "box_muller_dev"]
    names += [f"gang_sum{t}_{ty}_dev" for t in (4, 8, 16, 32) for ty in ("f32", "f64", "u32")]
    names += [f"quad_bcast{k}_{ty}_dev" for k in range(4) for ty in ("f32", "f64", "i32")]
    names += [f"quad_bcast_f64_{k}_dev" for k in range(4)]
    return ["pbgdt_" + n for n in names]


def _p(a):
    return ctypes.c_void_p(a.ctypes.data)


def host_sincos(x):
    """(sin, cos) of the host build of sincos_fast(float) / pbg::sincos_reduced64, by x's dtype."""
    x = np.ascontiguousarray(x)
    assert x.dtype in (np.float32, np.float64)
    s, c = np.empty_like(x), np.empty_like(x)
    fn = lib().pbgdt_sincos32_host if x.dtype == np.float32 else lib().pbgdt_sincos64_host
    fn(_p(x), _p(s), _p(c), ctypes.c_long(x.size))
    return s, c


# ------------------------------------------------------------------ float64: directed arguments next to n pi/2
@functools.lru_cache(maxsize=None)
def directed64():
    """x = fl(n pi/2) and both neighbours for every |n| <= 4,096 and every 16th n up to 63,662, with the
    mpmath (50 digits) sin and cos of each as double-doubles (hi + lo).  Returns read-only arrays
    (x, n, sin_hi, sin_lo, cos_hi, cos_lo)."""
    import mpmath
    mp = mpmath.mp.clone()
    mp.dps = 50
    ns = list(range(-4096, 4097))
    far = list(range(4096 + 16, N_MAX + 1, 16))
    if far[-1] != N_MAX:
        far.append(N_MAX)
    ns += far + [-k for k in far]
    half_pi = mp.pi / 2
    xs, nn = [], []
    for n in ns:
        x = np.float64(float(n * half_pi))  # mpmath rounds to nearest
        xs += [np.nextafter(x, -np.inf), x, np.nextafter(x, np.inf)]
        nn += [n, n, n]
    x = np.array(xs, np.float64)
    out = np.empty((4, x.size), np.float64)
    for i, v in enumerate(x):
        m = mp.mpf(float(v))
        for j, r in enumerate((mp.sin(m), mp.cos(m))):
            hi = float(r)
            out[2 * j, i] = hi
            out[2 * j + 1, i] = float(r - mp.mpf(hi))
    arrs = (x, np.array(nn, np.float64), out[0], out[1], out[2], out[3])
    for a in arrs:
        a.setflags(write=False)
    return arrs


def ulp64(ref):
    """The spacing of the doubles at |ref| (the smallest denormal at and below the denormals)."""
    return np.spacing(np.abs(ref))


def err_dd(got, hi, lo):
    """|got - (hi + lo)| in float64: got - hi is exact wherever the error is small enough to matter."""
    return np.abs((got - hi) - lo)


def sincos64_bound(n, ref):
    """The contract: 1 ulp(ref) + (|n| + 1) 2^-87."""
    return ulp64(ref) + (np.abs(n) + 1.0) * 2.0 ** -87


def check_directed64(s, c, label):
    """Assert the contract on directed64() for the (sin, cos) some build returned; returns the worst
    fraction of the bound and the worst error in ulp."""
    x, n, sh, sl, ch, cl = directed64()
    worst, worst_ulp, fails = 0.0, 0.0, []
    for name, got, hi, lo in (("sin", s, sh, sl), ("cos", c, ch, cl)):
        assert np.isfinite(got).all(), (label, name)
        err = err_dd(got, hi, lo)
        frac = err / sincos64_bound(n, hi)
        i = int(np.argmax(frac))
        print(f"{label} {name}: max err / bound = {frac[i]:.4f} at x = {x[i]!r} (n = {int(n[i])}), "
              f"over the bound at {int((frac > 1.0).sum())} of {x.size} arguments, max err = {(err / ulp64(hi)).max():.4g} ulp")
        if frac[i] > 1.0:
            fails.append((label, name, float(x[i]), int(n[i]), float(got[i]), float(hi[i]), float(frac[i])))
        worst, worst_ulp = max(worst, float(frac[i])), max(worst_ulp, float((err / ulp64(hi)).max()))
    assert not fails, fails
    return worst, worst_ulp


# ------------------------------------------------------------------ float32 argument sets
def f32_stride_chunks(chunk=1 << 20, stride=64):
    """Every `stride`-th float bit pattern in [0, 1e5], positive then negative, in chunks."""
    top = int(np.float32(1e5).view(np.uint32))
    for sign in (0, 0x80000000):
        for lo in range(0, top + 1, stride * chunk):
            bits = np.arange(lo, min(top + 1, lo + stride * chunk), stride, dtype=np.uint32) | np.uint32(sign)
            yield bits.view(np.float32)


@functools.lru_cache(maxsize=None)
def f32_directed():
    """The floats nearest to n pi/2 with both neighbours for |n| <= 63,662, then +-0, denormals (smallest,
    largest, one in between, both signs) and the smallest normal."""
    n = np.arange(-N_MAX, N_MAX + 1, dtype=np.float64)
    x = (n * (np.pi / 2)).astype(np.float32)  # fl64(pi/2) n is within 2^-52 relative: the nearest float or its twin
    d = np.concatenate([np.nextafter(x, np.float32(-np.inf)), x, np.nextafter(x, np.float32(np.inf))])
    den = np.array([0x00000001, 0x00000200, 0x007FFFFF, 0x00800000], np.uint32)
    e = np.concatenate([np.zeros(1, np.uint32), den]).view(np.float32)
    out = np.concatenate([d, e, -e]).astype(np.float32)
    out.setflags(write=False)
    return out


F32_NONFINITE = np.array([np.nan, np.inf, -np.inf], np.float32)


def ulp32(ref):
    """2^(floor(log2 |ref|) - 23) for a float64 reference, from 2^-149."""
    _, e = np.frexp(np.abs(ref))
    return np.ldexp(1.0, np.maximum(e - 24, -149))


# ------------------------------------------------------------------ device side (torch tensors)
def dev_call(name, *args):
    """Call pbgdt_<name>_dev on the current stream with torch tensors / python scalars, then synchronise."""
    import torch
    conv = []
    n = None
    for a in args:
        if isinstance(a, torch.Tensor):
            assert a.is_cuda and a.is_contiguous()
            n = a.numel() if n is None else n
            assert a.numel() == n
            conv.append(ctypes.c_void_p(a.data_ptr()))
        else:
            conv.append(a)
    rc = getattr(lib(), f"pbgdt_{name}_dev")(*conv, ctypes.c_long(n), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, (name, rc)
    torch.cuda.synchronize()


def dev_map(name, x, n_out=1, scalars=()):
    """x: numpy array -> n_out numpy arrays of the same dtype and shape, through pbgdt_<name>_dev."""
    import torch
    x = np.ascontiguousarray(x)
    if not x.flags.writeable:  # the shared references are read-only; torch wants a writable source
        x = x.copy()
    assert x.size <= 1 << 20
    tx = torch.from_numpy(x.view(_carrier(x.dtype))).cuda()
    outs = [torch.zeros_like(tx) for _ in range(n_out)]
    dev_call(name, tx, *scalars, *outs)
    res = [o.cpu().numpy().view(x.dtype).reshape(x.shape) for o in outs]
    return res[0] if n_out == 1 else res


def _carrier(dt):
    """torch moves the bits: unsigned words travel as signed ones of the same width."""
    return {np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}.get(np.dtype(dt), dt)
