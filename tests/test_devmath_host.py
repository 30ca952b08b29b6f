"""The kernels' sin / cos at their own stated accuracy, on the host (no GPU): the host entry points of the
test-only library libpbg_devtest.so evaluate the same source text the device compiles
(pbg_math.h sincos_fast(float), pbg_sincos64.h pbg::sincos_reduced64).  tests/test_devmath_gpu.py holds
the device build to the same bounds and, for float, to these very bits.

float64 contract: |err| <= 1 ulp(ref) + (|n| + 1) 2^-87, n = rint(x 2/pi); the second term is the
reduction's (pio2_1 + pio2_1t carry pi/2 to ~86 bits) and is all of the error next to a multiple of pi/2,
which random sampling never hits: the directed arguments fl(n pi/2) and neighbours do, against mpmath.

float32 bounds: measured on the host over EVERY float in [0, 1e5] against float64 libm -- 9.31e-8 absolute,
1.55 ulp up to 3.2 -- with 10 % headroom for the arguments this test's stride skips: 1.03e-7 and 1.7 ulp.
"""
import numpy as np

import devmath as dm


def test_sincos64_directed_near_multiples_of_half_pi():
    """fl(n pi/2) and both neighbours, every |n| <= 4,096 and every 16th n to 63,662, against mpmath at 50
    digits: within the contract (measured on the host: 0.545 of the bound; the relative error reaches 1.06e9 ulp
    on this set)."""
    x = dm.directed64()[0]
    assert x.size == 3 * (8193 + 2 * 3723) and np.abs(x).max() < 1e5 + 0.04
    s, c = dm.host_sincos(x)
    worst, worst_ulp = dm.check_directed64(s, c, "host")
    assert worst_ulp > 1e5  # the arguments do reach where a plain ulp bound is false (fl(pi): 3e5 ulp)


def test_sincos64_pi_example():
    """The header's example: sin(fl(pi)) is 1.2246467991473532e-16, the function gives ...0769e-16."""
    s, c = dm.host_sincos(np.array([np.pi]))
    assert c[0] == -1.0
    assert abs(s[0] - 1.2246467991473532e-16) <= 3 * 2.0 ** -87
    assert abs(s[0] - 1.2246467991473532e-16) > 1e4 * np.spacing(1.2246467991473532e-16)


def test_sincos64_edge_values():
    tiny = 5e-324
    s, c = dm.host_sincos(np.array([0.0, -0.0, tiny, -tiny]))
    assert np.array_equal(c, [1.0, 1.0, 1.0, 1.0])
    assert s[0] == 0.0 and not np.signbit(s[0])
    assert s[1] == 0.0 and not np.signbit(s[1])  # sin(-0) = +0: documented, not the C library's -0
    assert s[2] == tiny and s[3] == -tiny
    s, c = dm.host_sincos(np.array([np.nan, np.inf, -np.inf]))
    assert np.isnan(s).all() and np.isnan(c).all()
    # huge finite arguments: no Payne-Hanek path; NaN once the unreduced remainder's square overflows
    big = np.array([1e171, 1e200, 1e300, np.finfo(np.float64).max])
    s, c = dm.host_sincos(np.concatenate([big, -big]))
    assert np.isnan(s).all() and np.isnan(c).all()


def _f32_errors(x, s, c):
    rs, rc = np.sin(x.astype(np.float64)), np.cos(x.astype(np.float64))
    es, ec = np.abs(s - rs), np.abs(c - rc)
    return np.maximum(es, ec), np.maximum(es / dm.ulp32(rs), ec / dm.ulp32(rc))


def test_sincos32_accuracy_and_symmetry():
    """Every 64th float in [0, 1e5], both signs, and the floats at n pi/2 with neighbours, against numpy
    float64: 1.03e-7 absolute everywhere, 1.7 ulp for |x| <= 3.2; sin odd and cos even bit for bit."""
    max_abs, max_ulp, n = 0.0, 0.0, 0
    halves = {}
    for x in list(dm.f32_stride_chunks()) + [dm.f32_directed()]:
        s, c = dm.host_sincos(x)
        assert np.isfinite(s).all() and np.isfinite(c).all()
        ea, eu = _f32_errors(x, s, c)
        small = np.abs(x) <= np.float32(3.2)
        max_abs = max(max_abs, float(ea.max()))
        if small.any():
            max_ulp = max(max_ulp, float(eu[small].max()))
        n += x.size
        # symmetry: the stride chunks come as a positive half, then the same magnitudes negated
        key = (x.size, float(np.abs(x[0])), float(np.abs(x[-1])))
        if key in halves:
            s0, c0 = halves.pop(key)
            assert np.array_equal(c0.view(np.uint32), c.view(np.uint32))
            nz = s0 != 0
            assert np.array_equal((-s0[nz]).view(np.uint32), s[nz].view(np.uint32))
            assert (s[~nz] == 0).all() and not np.signbit(s[~nz]).any()  # sin(-0) = +0
        elif x is not dm.f32_directed():
            halves[key] = (s, c)
    assert not halves
    print(f"sincos_fast(float) host: {n} arguments, max abs err {max_abs:.3e}, max err for |x| <= 3.2 {max_ulp:.3f} ulp")
    assert max_abs <= 1.03e-7
    assert max_ulp <= 1.7
    # the directed set is symmetric in itself (n and -n)
    x = dm.f32_directed()
    s, c = dm.host_sincos(x)
    sm, cm = dm.host_sincos(-x)
    assert np.array_equal(c.view(np.uint32), cm.view(np.uint32))
    nz = s != 0
    assert np.array_equal((-s[nz]).view(np.uint32), sm[nz].view(np.uint32))
    assert not np.signbit(s[~nz]).any() and not np.signbit(sm[~nz]).any()


def test_sincos32_edge_values():
    den = np.array([0x00000001, 0x00000200, 0x007FFFFF], np.uint32).view(np.float32)
    x = np.concatenate([np.array([0.0, -0.0], np.float32), den, -den])
    s, c = dm.host_sincos(x)
    assert np.array_equal(c, np.ones(8, np.float32))
    assert np.array_equal(s[:2].view(np.uint32), [0, 0])  # sin(+-0) = +0
    assert np.array_equal(s[2:].view(np.uint32), x[2:].view(np.uint32))  # sin(denormal) = the denormal
    s, c = dm.host_sincos(dm.F32_NONFINITE)
    assert np.isnan(s).all() and np.isnan(c).all()
