// pbg_sincos64.h -- float64 sin/cos for the physics of the float64 kernels (joint rotations, the base's
// exponential map).  The device library's double sincos carries a Payne-Hanek large-argument path and
// costs ~150 VALU instructions per call (108 of them float64, half-rate); the physics' arguments are
// joint angles and half-angle increments.  Here: Cody-Waite reduction by pi/2 (fdlibm's pio2_1 +
// pio2_1t split, the reduced argument carried as a double-double), then the minimax kernels of FreeBSD
// msun's k_sin.c / k_cos.c on [-pi/4, pi/4] (the published coefficients), ~45 instructions, no branch.
//
// Accuracy, for |x| <= 1e5 and n = rint(x 2/pi):   |err| <= 1 ulp(exact) + (|n| + 1) 2^-87.
// The second term is the reduction's: pio2_1 + pio2_1t carry pi/2 to ~86 bits (2^-87 is half an ulp of
// pio2_1t), so the reduced argument is off by up to that times n.  Away from the multiples of pi/2 it
// vanishes under the first (random arguments: 0.77 ulp, the C library 0.52); next to one, where the result
// is tiny, it is all of the error: x = fl(pi) gives sin = 1.224646799076922e-16 for 1.2246467991473532e-16,
// 3e5 ulp, and over fl(n pi/2) and its neighbours up to 1e5 the relative error reaches 4e9 ulp while the
// absolute one stays below 0.55 of the bound.  1e-15 absolute up to 1e6.  The float64 parity bound of the
// physics is 1e-9.
// The reduction's TwoProd / TwoSum lines are error-free only as written: contracted (hipcc's default on
// the device), r = r1 - p and p + bb become fmas of n and pio2_1t, r is then the rounding of the exact
// r1 - n pio2_1t and y subtracts pe a second time -- measured on an MI355X, 2.44 times the bound on the
// directed arguments.  sincos_reduced64 therefore switches contraction off for its own body (the
// polynomial kernels keep the build's setting); with it the device meets the bound like the host builds.
// Special values: sin(-0) is +0 (n = -0 makes the reduced argument +0; the C library returns -0); NaN and
// +-inf give NaN; the smallest denormal returns (x, 1).  Huge finite arguments get no Payne-Hanek
// reduction: from about 1e16 (n no longer exact) the remainder is not reduced and the polynomials return
// garbage of any magnitude (+-inf from ~1e40), and NaN once the remainder's square overflows (every
// |x| >= 1e171; in practice from ~1e120).  The physics stays below 1e5.
// tests/test_sincos64.py and tests/test_devmath_host.py check the host build (with mpmath on the directed
// arguments next to n pi/2), tests/test_devmath_gpu.py the device build under the product's flags.
// Plain C++ (no HIP types), so the host test compiles it with g++.
#pragma once

#ifndef PBG_SC64_FN
#define PBG_SC64_FN inline
#endif

namespace pbg {
// r + y in [-pi/4, pi/4] (y: the reduction's tail, |y| <= ulp(r)): (sin, cos) of r + y
PBG_SC64_FN void sincos_kernel64(double r, double y, double* sp, double* cp) {
  const double z = r * r, w = z * z;
  // k_sin.c: S1..S6 (sin(r + y) = r + v S1 + ... with the tail's first-order terms)
  const double sr = 8.33333333332248946124e-03 + z * (-1.98412698298579493134e-04 + z * 2.75573137070700676789e-06) +
                    z * w * (-2.50507602534068634195e-08 + z * 1.58969099521155010221e-10);
  const double v = z * r;
  *sp = r - ((z * (0.5 * y - v * sr) - y) - v * -1.66666666666666324348e-01);
  // k_cos.c: C1..C6, 1 - z/2 + z cr - r y with the rounding of 1 - z/2 recovered
  const double cr = z * (4.16666666666666019037e-02 + z * (-1.38888888888741095749e-03 + z * 2.48015872894767294178e-05)) +
                    w * w * (-2.75573143513906633035e-07 + z * (2.08757232129817482790e-09 + z * -1.13596475577881948265e-11));
  const double hz = 0.5 * z, one_m = 1.0 - hz;
  *cp = one_m + (((1.0 - one_m) - hz) + (z * cr - r * y));
}
// x = n pi/2 + (r + y), r + y a double-double (fdlibm's
// __ieee754_rem_pio2 medium case with FMAs: n pio2_1 is exact, the product n pio2_1t and the
// subtraction are carried exactly by TwoProd / TwoSum), then the quadrant
PBG_SC64_FN void sincos_reduced64(double x, double* sp, double* cp) {
#if defined(__clang__)
#pragma clang fp contract(off)  // p, r, bb, y below must round exactly as written (header comment)
#endif
  const double n = __builtin_rint(x * 6.36619772367581382433e-01);  // 2 / pi
  const double r1 = __builtin_fma(-n, 1.57079632673412561417e+00, x);  // pio2_1: pi/2, first 33 bits
  const double p = n * 6.07710050650619224932e-11;                     // pio2_1t = pi/2 - pio2_1
  const double pe = __builtin_fma(n, 6.07710050650619224932e-11, -p);
  const double r = r1 - p, bb = r - r1;
  const double y = ((r1 - (r - bb)) - (p + bb)) - pe;
  double s, c;
  sincos_kernel64(r, y, &s, &c);
  const int q = (int)n & 3;
  const double s0 = (q & 1) ? c : s, c0 = (q & 1) ? s : c;
  *sp = (q & 2) ? -s0 : s0;
  *cp = ((q + 1) & 2) ? -c0 : c0;
}
}  // namespace pbg
