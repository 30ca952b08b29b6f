"""The step kernels' device math and cross-lane primitives, each alone in a trivial kernel on the GPU
(libpbg_devtest.so: pybullet-gym_amd/csrc/pbg_devtest.hip, built with the product's flags), against plain
high-precision references.  The step kernels are held to the float64 oracle at 1e-9 / 1e-4 relative, about
1e7 ulp; these tests hold what is underneath to its own stated accuracy.

No tolerance here is tuned to the device's output: each is the project's existing contract (pbg_math.h,
pbg_sincos64.h, include/pbg.h "Noise contract"), a bound derived there, or a host measurement against an
independent reference with stated headroom (tests/test_devmath_host.py).  Device figures that a test only
reports are recorded in its docstring and in DESIGN.md section 6.

The lane primitives run as whole 64-lane waves (full EXEC mask: their contract), every lane holding a
distinct random value; a launch is at most 2^20 elements.
"""
import ctypes

import numpy as np
import pytest
import torch

import devmath as dm

pytestmark = pytest.mark.gpu

CHUNK = 1 << 20


def bits(a):
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same_bits(a, b):
    return np.array_equal(bits(np.ascontiguousarray(a)), bits(np.ascontiguousarray(b)))


# ================================================================== sin / cos
def test_sincos32_device_equals_host_bitwise():
    """sincos_fast(float): every multiply-add is a spelled-out fmaf, so the device's bits are the host
    build's on the whole argument set of test_devmath_host.py (every 64th float in [0, 1e5], both signs;
    the floats at n pi/2 with neighbours; +-0, denormals); NaN and +-inf give NaN on both."""
    n = 0
    for x in list(dm.f32_stride_chunks(CHUNK)) + [dm.f32_directed()]:
        s, c = dm.dev_map("sincos32", x, 2)
        hs, hc = dm.host_sincos(x)
        ds, dc = bits(s) != bits(hs), bits(c) != bits(hc)
        assert not ds.any() and not dc.any(), (int(ds.sum()), int(dc.sum()), x[ds | dc][:8], s[ds | dc][:8], hs[ds | dc][:8])
        n += x.size
    s, c = dm.dev_map("sincos32", dm.F32_NONFINITE, 2)
    assert np.isnan(s).all() and np.isnan(c).all()
    print(f"sincos_fast(float): device == host bit for bit on {n} arguments")


def test_sincos64_device_directed():
    """The device build of sincos_fast(double) on fl(n pi/2) and neighbours, against mpmath:
    |err| <= 1 ulp + (|n| + 1) 2^-87, the bound the host builds meet at 0.545.

    This test found a defect: with the reduction contracted (the device build's default) the result reached
    2.44 times the bound (sin at x = 53708.668005771106, n = 34192; 12,642 of the 46,917 arguments over it):
    r = r1 - p and p + bb became fmas of n and pio2_1t, and the tail subtracted the product's rounding error
    twice.  pbg::sincos_reduced64 now keeps its reduction uncontracted.
    Measured on an MI355X with that: 0.5449 of the bound (sin) and 0.5448 (cos), as on the host."""
    x = dm.directed64()[0]
    s, c = dm.dev_map("sincos64", x, 2)
    dm.check_directed64(s, c, "device")


def test_sincos64_device_edge_values():
    """As on the host: +-0 -> (+0, 1), the smallest denormal -> (x, 1), NaN, +-inf and huge finite -> NaN."""
    tiny = 5e-324
    big = np.array([1e171, 1e200, 1e300, np.finfo(np.float64).max])
    e = np.concatenate([[0.0, -0.0, tiny, -tiny, np.nan, np.inf, -np.inf], big, -big])
    s, c = dm.dev_map("sincos64", e, 2)
    assert same_bits(s[:4], np.array([0.0, 0.0, tiny, -tiny])) and same_bits(c[:4], np.ones(4))
    assert np.isnan(s[4:]).all() and np.isnan(c[4:]).all()


@pytest.mark.parametrize("R", [1e-8, 1e-3, 0.7853981633974483, 3.2, 10.0, 1e3, 1e5], ids=str)
def test_sincos64_device_random(R):
    """2^18 uniform arguments in [-R, R] (the ranges of test_sincos64.py up to 1e5) against np.longdouble
    sin / cos (64-bit mantissa): the project's 1.0 ulp plus the reduction's (|n| + 1) 2^-87.
    Reported, not asserted -- measured on an MI355X, per range (1e-8 .. 1e5): maximum error
    0.23 / 0.50 / 0.74 / 0.78 / 0.75 / 0.76 / 1.41 ulp (the last next to a zero, inside the |n| term); share
    of arguments whose sin or cos bits differ from the host build (its polynomials are not contracted)
    0 / 0 / 0.0101 / 0.0105 / 0.0103 / 0.0109 / 0.0109."""
    assert np.finfo(np.longdouble).nmant >= 63, "needs an extended-precision long double"
    rng = np.random.default_rng(int(np.float64(R).view(np.uint64) >> np.uint64(32)))
    x = rng.uniform(-R, R, 1 << 18)
    s, c = dm.dev_map("sincos64", x, 2)
    hs, hc = dm.host_sincos(x)
    xl = x.astype(np.longdouble)
    n = np.rint(x * 0.6366197723675814)
    worst = 0.0
    for got, ref in ((s, np.sin(xl)), (c, np.cos(xl))):
        u = dm.ulp64(ref.astype(np.float64))
        err = np.abs(got.astype(np.longdouble) - ref).astype(np.float64)
        worst = max(worst, float((err / u).max()))
        bad = err > u + (np.abs(n) + 1.0) * 2.0 ** -87
        assert not bad.any(), (R, x[bad][:4], got[bad][:4], (err / u)[bad][:4])
    differ = float(((bits(s) != bits(hs)) | (bits(c) != bits(hc))).mean())
    print(f"sincos_fast(double) device, R = {R:g}: max err {worst:.4f} ulp, bits differ from the host build "
          f"for {differ:.4f} of the arguments")


# ================================================================== reciprocal, sqrt, rsq
def rcp64_arguments():
    """Every exponent in [-1021, 1021] x both signs x 256 mantissas in [1, 2): 1, 1 + 2^-52, 2 - 2^-52 and
    253 random ones (1,046,016 <= 2^20 arguments)."""
    rng = np.random.default_rng(64)
    e = np.arange(-1021, 1022)
    m = 1.0 + rng.integers(0, 1 << 52, (e.size, 2, 256)).astype(np.float64) * 2.0 ** -52
    m[..., 0], m[..., 1], m[..., 2] = 1.0, 1.0 + 2.0 ** -52, 2.0 - 2.0 ** -52
    x = np.ldexp(m, e[:, None, None])
    x[:, 1, :] *= -1.0
    return x.reshape(-1)


def test_fast_rcp64_within_one_ulp():
    """fast_rcp(double) (v_rcp_f64 + two Newton steps) against numpy's IEEE 1.0 / x: pbg_math.h's
    'within 1 ulp of the IEEE quotient', over every exponent the header's domain allows (the largest
    arguments have denormal reciprocals).
    Measured on an MI355X: 0 ulp -- the IEEE quotient's bits on all 1,046,016 arguments."""
    x = rcp64_arguments()
    assert x.size <= CHUNK and np.isfinite(x).all() and (x != 0).all()
    ref = 1.0 / x
    assert np.isfinite(ref).all() and (ref != 0).all()
    got = dm.dev_map("rcp64", x)
    err = np.abs(got - ref) / np.spacing(np.abs(ref))
    i = int(np.argmax(err))
    inexact = float((got != ref).mean())
    print(f"fast_rcp(double): max err {err[i]:.3f} ulp at x = {x[i]!r} (got {got[i]!r}, IEEE {ref[i]!r}); "
          f"differs from the IEEE quotient for {inexact:.4f} of {x.size} arguments; "
          f"worst with a normal result: {err[np.abs(ref) >= 2.0 ** -1022].max():.3f} ulp")
    assert np.isfinite(got).all()
    assert err[i] <= 1.0


def _f32_normals(rng, n, signs):
    b = rng.integers(0x00800000, 0x7F800000, n, dtype=np.uint32)
    b[:4] = [0x00800000, 0x7F7FFFFF, 0x3F800000, 0x3F800001]
    if signs:
        b[n // 2:] |= np.uint32(0x80000000)
    return b.view(np.float32)


@pytest.mark.parametrize("name", ["rcp32", "sqrt32", "rsq32"])
def test_fast_float_wrappers_within_one_ulp(name):
    """v_rcp_f32 / v_sqrt_f32 / v_rsq_f32 behind fast_rcp / fast_sqrt / fast_rsq (float): <= 1 ulp of the
    float64 numpy value over 2^20 normal arguments of every exponent (rcp: both signs).
    Measured on an MI355X: sqrt 0.911 ulp, rsq 0.863 ulp, rcp 0.878 ulp where the reciprocal is a normal float.
    This test found a defect: for |x| > 2^126 the reciprocal is a denormal float and v_rcp_f32 alone returns
    a zero (x = 8.511027e+37: 0.0 for 1.1749e-38); fast_rcp(float) now scales those arguments (pbg_math.h).
    Measured with that: 0.923 ulp over all normal arguments (at x = -8.742248e+37, a denormal reciprocal)."""
    x = _f32_normals(np.random.default_rng(32), CHUNK, name == "rcp32")
    xd = x.astype(np.float64)
    ref = {"rcp32": lambda: 1.0 / xd, "sqrt32": lambda: np.sqrt(xd), "rsq32": lambda: 1.0 / np.sqrt(xd)}[name]()
    got = dm.dev_map(name, x)
    err = np.abs(got.astype(np.float64) - ref) / dm.ulp32(ref)
    i = int(np.argmax(err))
    normal = np.abs(ref) >= 2.0 ** -126
    print(f"fast_{name}: max err {err[i]:.3f} ulp at x = {x[i]!r} (got {got[i]!r}, float64 {ref[i]!r}); "
          f"where the result is a normal float: {err[normal].max():.3f} ulp")
    assert err[i] <= 1.0


def test_fast_rcp32_normal_results():
    """fast_rcp(float) wherever the reciprocal is a normal float (|x| <= 2^126), both signs: <= 1 ulp."""
    x = _f32_normals(np.random.default_rng(33), CHUNK, True)
    x = x[np.abs(x) <= np.float32(2.0 ** 126)]
    ref = 1.0 / x.astype(np.float64)
    assert x.size > 0.9 * CHUNK and (np.abs(ref) >= 2.0 ** -126).all()
    got = dm.dev_map("rcp32", x)
    err = np.abs(got.astype(np.float64) - ref) / dm.ulp32(ref)
    print(f"fast_rcp32, normal results: max err {err.max():.3f} ulp")
    assert err.max() <= 1.0


def test_fast_sqrt64_is_ieee():
    """fast_sqrt(double) is the correctly rounded sqrt: numpy's bits, over every exponent, denormals, 0, inf."""
    rng = np.random.default_rng(65)
    x = rng.integers(0, 0x7FF0000000000000, CHUNK - 8, dtype=np.uint64).view(np.float64)
    x = np.concatenate([x, [0.0, 5e-324, 2.2250738585072014e-308, 1.0, 2.0, 4.0, np.finfo(np.float64).max, np.inf]])
    got = dm.dev_map("sqrt64", x)
    d = bits(got) != bits(np.sqrt(x))
    assert not d.any(), (int(d.sum()), x[d][:4], got[d][:4])


# ================================================================== clampf
CLAMPS = [(-1.0, 1.0), (0.0, 0.0), (-np.inf, np.inf)]


@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("lo,hi", CLAMPS, ids=["unit", "zero", "inf"])
def test_clampf(dt, lo, hi):
    """clampf (float: one v_med3_f32; double: v_max_f64 / v_min_f64) against np.clip, bit for bit, for
    normal inputs of every exponent and sign, +-0 and +-inf.  A denormal input returns itself or a zero of
    its sign (or, clamped to [0, 0], a zero); a NaN input gives NaN or a value inside [lo, hi].
    One input has no portable np.clip: x = -0 in [+0, +0], where numpy's maximum(-0, +0) returns whichever
    operand its SIMD path happens to (-0 on x86); the reference there is IEEE 754-2019's
    minimum(maximum(x, lo), hi) with -0 < +0, i.e. +0 = lo = hi.
    Measured on an MI355X: denormal inputs come back as themselves, float and double, in all three ranges
    (the float32 kernels run with denormals enabled); a NaN input never comes back as NaN: float gives lo or hi
    (by the NaN's sign and kind), double gives lo (fmax drops the NaN)."""
    rng = np.random.default_rng(7)
    fi = np.finfo(dt)
    ut = np.uint32 if dt == np.float32 else np.uint64
    sign = ut(1) << ut(8 * dt().itemsize - 1)
    expo_lo, expo_hi = int(np.array(fi.tiny, dt).view(ut)), int(np.array(np.inf, dt).view(ut))
    b = rng.integers(expo_lo, expo_hi, 1 << 16, dtype=ut)
    b[1::2] |= sign
    near = np.array([-1.0, 1.0, np.nextafter(dt(1), dt(2)), np.nextafter(dt(1), dt(0)), -np.nextafter(dt(1), dt(2)),
                     -np.nextafter(dt(1), dt(0)), 0.0, -0.0, np.inf, -np.inf, fi.tiny, -fi.tiny, fi.max, -fi.max], dt)
    x = np.concatenate([b.view(dt), near])
    arg = (ctypes.c_float if dt == np.float32 else ctypes.c_double)
    name = "clamp32" if dt == np.float32 else "clamp64"
    got = dm.dev_map(name, x, scalars=(arg(lo), arg(hi)))
    ref = np.clip(x, dt(lo), dt(hi))
    if lo == 0.0 and hi == 0.0:
        ref[bits(x) == sign] = dt(0.0)  # x = -0 (docstring)
    d = bits(got) != bits(ref)
    assert not d.any(), (int(d.sum()), x[d][:8], got[d][:8], ref[d][:8])
    # denormals
    den = rng.integers(1, expo_lo, 1024, dtype=ut)
    den[:2] = [1, expo_lo - 1]
    den[1::2] |= sign
    xd = den.view(dt)
    gd = dm.dev_map(name, xd, scalars=(arg(lo), arg(hi)))
    kept = bits(gd) == bits(xd)
    zero = (gd == 0) & (np.signbit(gd) == np.signbit(xd))
    print(f"clampf {dt.__name__} [{lo}, {hi}]: denormal inputs kept {int(kept.sum())}, flushed to a zero of their sign "
          f"{int((zero & ~kept).sum())} of {xd.size}")
    if lo == 0.0 and hi == 0.0:
        assert (gd == 0).all()
    else:
        assert (kept | zero).all(), (xd[~(kept | zero)][:4], gd[~(kept | zero)][:4])
    # NaN: quiet and signalling, both signs, payloads
    nan_bits = np.array([expo_hi | (1 << (fi.nmant - 1)), expo_hi | 1, expo_hi | (1 << (fi.nmant - 1)) | 0x1234], ut)
    xn = np.concatenate([nan_bits, nan_bits | sign]).view(dt)
    assert np.isnan(xn).all()
    gn = dm.dev_map(name, xn, scalars=(arg(lo), arg(hi)))
    print(f"clampf {dt.__name__} [{lo}, {hi}]: NaN inputs give {gn}")
    assert (np.isnan(gn) | ((gn >= lo) & (gn <= hi))).all(), gn


# ================================================================== lane primitives
WAVES = 16
NL = 64 * WAVES
FLOATS = {"f32": np.float32, "f64": np.float64}


def spread(rng, dt, n):
    """Distinct values of mixed sign over 12 decades: sums whose bits depend on the order of addition."""
    x = (rng.standard_normal(n) * 10.0 ** rng.uniform(-6, 6, n)).astype(dt)
    assert np.unique(x).size == n
    return x


def tree_sum(x, T):
    """The helpers' stated order: lanes pairwise, quad halves, quads (row_half_mirror), half rows
    (row_mirror), even row + odd row -- a binary tree over the segment, each sum rounded in x's dtype."""
    v = x.reshape(-1, T)
    while v.shape[1] > 1:
        v = v[:, 0::2] + v[:, 1::2]
    return np.repeat(v[:, 0], T)


def serial_sum(x, T):
    v = x.reshape(-1, T)
    acc = v[:, 0].copy()
    for j in range(1, T):
        acc = acc + v[:, j]
    return np.repeat(acc, T)


def check_sum(name, x, T):
    got = dm.dev_map(name, x)
    ref = tree_sum(x, T)
    d = bits(got) != bits(ref)
    assert not d.any(), (name, int(d.sum()), np.flatnonzero(d)[:8], got[d][:4], ref[d][:4])
    seg = bits(got).reshape(-1, T)
    assert (seg == seg[:, :1]).all()  # identical bits in every lane of a segment
    return got


def check_isolation(name, x, T, dt):
    """A NaN / inf in one lane of one segment: that segment only."""
    base = tree_sum(x, T)
    for k, (lane, poison) in enumerate(((T - 1, np.nan), (0, np.inf), (T // 2, -np.inf))):
        seg = 1 + 2 * k  # a segment with neighbours on both sides
        y = x.copy()
        y[seg * T + lane] = poison
        got = dm.dev_map(name, y).reshape(-1, T)
        want = tree_sum(y, T).reshape(-1, T)
        hit = np.zeros(got.shape[0], bool)
        hit[seg] = True
        assert same_bits(got[~hit], base.reshape(-1, T)[~hit]), (name, poison)
        if np.isnan(poison):
            assert np.isnan(got[hit]).all()
        else:
            assert same_bits(got[hit], want[hit]) and (got[hit] == poison).all()


@pytest.mark.parametrize("ty", ["f32", "f64"])
def test_quad_sum(ty):
    """quad_sum: (x0 + x1) + (x2 + x3) in every lane of the quad, bit for bit."""
    x = spread(np.random.default_rng(4), FLOATS[ty], NL)
    assert (bits(tree_sum(x, 4)) != bits(serial_sum(x, 4))).any()  # the order does show in these inputs
    check_sum(f"quad_sum_{ty}", x, 4)
    check_isolation(f"quad_sum_{ty}", x, 4, FLOATS[ty])


@pytest.mark.parametrize("T", [4, 8, 16, 32])
@pytest.mark.parametrize("ty", ["f32", "f64"])
def test_gang_sum(ty, T):
    """gang_sum<T>: quad pairs, half mirror, row mirror, even row + odd row; identical bits in the segment's
    lanes; a neighbouring segment's lanes never enter."""
    x = spread(np.random.default_rng(100 + T), FLOATS[ty], NL)
    assert (bits(tree_sum(x, T)) != bits(serial_sum(x, T))).any()
    check_sum(f"gang_sum{T}_{ty}", x, T)
    check_isolation(f"gang_sum{T}_{ty}", x, T, FLOATS[ty])


def test_integer_sums_exact_mod_2_32():
    """quad_sum_i and gang_sum_u32<T>: exact mod 2^32 with operands near 2^31 (every partial sum wraps)."""
    rng = np.random.default_rng(31)
    x = (np.uint32(1 << 31) + rng.integers(-(1 << 20), 1 << 20, NL).astype(np.int64)).astype(np.uint32)
    assert np.unique(x).size == NL
    with np.errstate(over="ignore"):
        got = dm.dev_map("quad_sum_i32", x.view(np.int32)).view(np.uint32)
        assert np.array_equal(got, tree_sum(x, 4))
        assert np.array_equal(got, np.repeat(x.reshape(-1, 4).astype(np.uint64).sum(1).astype(np.uint32), 4))
        for T in (4, 8, 16, 32):
            got = dm.dev_map(f"gang_sum{T}_u32", x)
            want = np.repeat((x.reshape(-1, T).astype(np.uint64).sum(1) & np.uint64(0xFFFFFFFF)).astype(np.uint32), T)
            assert np.array_equal(got, want), T


def random_words(rng, ut, n):
    """Distinct random bit patterns: NaN payloads, denormals and infinities among them, plus -0 and NaNs."""
    top = np.iinfo(ut).max
    w = rng.integers(0, top, n, dtype=ut, endpoint=True)
    if ut == np.uint32:
        w[:6] = [0x80000000, 0x7FC00001, 0xFFC12345, 0x7F800001, 0x00000001, 0xFF800000]
    else:
        w[:6] = [0x8000000000000000, 0x7FF8000000000001, 0xFFF8123456789ABC, 0x7FF0000000000001, 1, 0xFFF0000000000000]
    w = rng.permutation(w)
    assert np.unique(w).size == n
    return w


@pytest.mark.parametrize("K", [0, 1, 2, 3])
def test_quad_bcast(K):
    """quad_bcast<K> (float, double, int) and quad_bcast_f64<K>: every lane of quad q holds lane 4 q + K's
    bits -- NaN payloads, -0 and denormals included."""
    rng = np.random.default_rng(40 + K)
    for name, dt, ut in ((f"quad_bcast{K}_f32", np.float32, np.uint32), (f"quad_bcast{K}_i32", np.int32, np.uint32),
                         (f"quad_bcast{K}_f64", np.float64, np.uint64), (f"quad_bcast_f64_{K}", np.float64, np.uint64)):
        w = random_words(rng, ut, NL)
        got = dm.dev_map(name, w.view(dt)).view(ut)
        assert np.array_equal(got, np.repeat(w.reshape(-1, 4)[:, K], 4)), name


@pytest.mark.parametrize("ty,dt,ut", [("f32", np.float32, np.uint32), ("u32", np.uint32, np.uint32),
                                      ("f64", np.float64, np.uint64)], ids=["f32", "u32", "f64"])
def test_row_pair_swap(ty, dt, ut):
    """row_pair_swap(a, b) with a = b = x, x uniform within each 16-lane row: a holds the even row's value
    and b the odd row's, in both rows of each pair -- all 32 (64) bits, NaN payloads included."""
    rows = random_words(np.random.default_rng(16), ut, NL // 16)
    x = np.repeat(rows, 16)
    a, b = dm.dev_map(f"row_pair_swap_{ty}", x.view(dt), 2)
    assert np.array_equal(a.view(ut), np.repeat(rows[0::2], 32))
    assert np.array_equal(b.view(ut), np.repeat(rows[1::2], 32))


# ================================================================== evolution-strategy noise
def box_muller_reference(a, b):
    """include/pbg.h "Noise contract" in float64, rounded once; cospi / sinpi exact at the quadrant
    boundaries (t = 2 u2 is a binary fraction: reduced exactly)."""
    u1 = (a >> np.uint32(9)).astype(np.float64) * 2.0 ** -23 + 2.0 ** -24
    t = 2.0 * ((b >> np.uint32(8)).astype(np.float64) * 2.0 ** -24)
    r = np.sqrt(-2.0 * np.log(u1))
    k = np.rint(2.0 * t)
    f = t - 0.5 * k  # exact, |f| <= 1/4
    s0, c0 = np.sin(np.pi * f), np.cos(np.pi * f)
    q = k.astype(np.int64) & 3
    s = np.where(q == 0, s0, np.where(q == 1, c0, np.where(q == 2, -s0, -c0)))
    c = np.where(q == 0, c0, np.where(q == 1, -s0, np.where(q == 2, -c0, s0)))
    return (r * c).astype(np.float32), (r * s).astype(np.float32)


def test_box_muller_edges_and_random():
    """es_box_muller on the words Philox rarely produces -- u1 = 2^-24 and 1 - 2^-24, u2 on and next to the
    quadrant boundaries -- and on 2^16 random pairs, against the contract in float64: |d| <= 1e-5
    (derived in pbg.h), every output finite and |n| <= 5.77 + 1e-5.
    Measured on an MI355X: 4.77e-7 on the 91 edge pairs and on the random ones, max |n| = 5.7681."""
    A = np.array([0, 0x1FF, 0x200, 0x7FFFFFFF, 0x80000000, 0xFFFFFE00, 0xFFFFFFFF], np.uint32)
    quad = np.array([0, 0x40000000, 0x80000000, 0xC0000000], np.int64)
    B = np.concatenate([quad, (quad + 0x100) & 0xFFFFFFFF, (quad - 0x100) & 0xFFFFFFFF, [0xFFFFFFFF]]).astype(np.uint32)
    ea, eb = [v.reshape(-1) for v in np.meshgrid(A, B, indexing="ij")]
    rng = np.random.default_rng(0xE5)
    a = np.concatenate([ea, rng.integers(0, 1 << 32, 1 << 16, dtype=np.uint32)])
    b = np.concatenate([eb, rng.integers(0, 1 << 32, 1 << 16, dtype=np.uint32)])
    ta, tb = (torch.from_numpy(v.view(np.int32)).cuda() for v in (a, b))
    n0, n1 = torch.zeros(a.size, dtype=torch.float32, device="cuda"), torch.zeros(a.size, dtype=torch.float32, device="cuda")
    dm.dev_call("box_muller", ta, tb, n0, n1)
    n0, n1 = n0.cpu().numpy(), n1.cpu().numpy()
    r0, r1 = box_muller_reference(a, b)
    d = np.maximum(np.abs(n0.astype(np.float64) - r0), np.abs(n1.astype(np.float64) - r1))
    ne = ea.size
    print(f"es_box_muller: max |device - float64| = {d[:ne].max():.3e} on the {ne} edge pairs, {d[ne:].max():.3e} on "
          f"{a.size - ne} random pairs; max |n| = {max(np.abs(n0).max(), np.abs(n1).max()):.4f}")
    assert np.isfinite(n0).all() and np.isfinite(n1).all()
    assert max(np.abs(n0).max(), np.abs(n1).max()) <= 5.77 + 1e-5
    i = int(np.argmax(d))
    assert d[i] <= 1e-5, (hex(int(a[i])), hex(int(b[i])), n0[i], r0[i], n1[i], r1[i])
    # the largest radius is reached: a = 0 gives u1 = 2^-24, r = sqrt(48 ln 2)
    assert abs(float(np.hypot(n0[0].astype(np.float64), n1[0].astype(np.float64))) - np.sqrt(48 * np.log(2))) <= 1e-5
