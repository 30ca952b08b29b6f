// pbg_lanes.h -- the cross-lane primitives of the quad and gang kernels: DPP permutations within a quad
// or a 16-lane row, the gfx950 row-pair swap, and the all-reduces and broadcasts built on them.  One
// header so that the test unit (pbg_devtest.hip, tests/test_devmath_gpu.py) runs the very text the step
// kernels include; the three groups below are verbatim what pbg_team.hip, pbg_gang.hip and pbg_step.hip
// held (same names, same duplicates: the kernels' device code is byte-identical).
// Every helper expects the full EXEC mask of its quad / row segment / row pair.
#pragma once
#include "pbg_math.h"

namespace pbg {

// ------------------------------------------------------------------ quad (DPP) helpers (pbg_team.hip)
// bound_ctrl set: every permutation used here reads a valid lane, and with it the
// compiler folds `x + mov_dpp(x)` into one v_add_f32_dpp (no mov, no DPP hazard nop).
template <int CTRL>
PBG_DEV float qperm(float x) {
  return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, x), CTRL, 0xF, 0xF, true));
}
template <int CTRL>
PBG_DEV int qperm_i(int x) {
  return __builtin_amdgcn_mov_dpp(x, CTRL, 0xF, 0xF, true);
}
// sum over the quad; identical bits in all four lanes ((x0+x1)+(x2+x3), addition commutes)
PBG_DEV float quad_sum(float x) {
  x = x + qperm<0xB1>(x);  // quad_perm [1,0,3,2]
  return x + qperm<0x4E>(x);  // quad_perm [2,3,0,1]
}
PBG_DEV int quad_sum_i(int x) {
  x = x + qperm_i<0xB1>(x);
  return x + qperm_i<0x4E>(x);
}
template <int K>
PBG_DEV float quad_bcast(float x) { return qperm<K | (K << 2) | (K << 4) | (K << 6)>(x); }
template <int K>
PBG_DEV int quad_bcast_i(int x) { return qperm_i<K | (K << 2) | (K << 4) | (K << 6)>(x); }
// float64 (F64<R>: the reference-precision path): a double moves as its two dwords
template <int CTRL>
PBG_DEV double qperm(double x) {
  const uint64_t u = __builtin_bit_cast(uint64_t, x);
  const uint32_t lo = (uint32_t)__builtin_amdgcn_mov_dpp((int)(uint32_t)u, CTRL, 0xF, 0xF, true);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_mov_dpp((int)(uint32_t)(u >> 32), CTRL, 0xF, 0xF, true);
  return __builtin_bit_cast(double, ((uint64_t)hi << 32) | lo);
}
PBG_DEV double quad_sum(double x) {
  x = x + qperm<0xB1>(x);
  return x + qperm<0x4E>(x);
}
template <int K>
PBG_DEV double quad_bcast(double x) { return qperm<K | (K << 2) | (K << 4) | (K << 6)>(x); }

// ------------------------------------------------------------------ pack (pbg_step.hip)
// Broadcast lane K of each DPP quad (a float64 as two dword moves).
template <int K>
PBG_DEV double quad_bcast_f64(double x) {
  constexpr int CTRL = K * 85;  // quad_perm [K, K, K, K]
  const uint64_t u = __builtin_bit_cast(uint64_t, x);
  const uint32_t lo = (uint32_t)__builtin_amdgcn_mov_dpp((int)(uint32_t)u, CTRL, 0xF, 0xF, true);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_mov_dpp((int)(uint32_t)(u >> 32), CTRL, 0xF, 0xF, true);
  return __builtin_bit_cast(double, ((uint64_t)hi << 32) | lo);
}

// ------------------------------------------------------------------ gang (row) helpers (pbg_gang.hip)
// bound_ctrl set: every permutation used here reads a valid lane, and with it the
// compiler folds `x + mov_dpp(x)` into one v_add_f32_dpp (no mov, no DPP hazard nop).
template <int CTRL>
PBG_DEV float dpp_f(float x) {
  return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, x), CTRL, 0xF, 0xF, true));
}
// float64: the two dwords moved by the same permutation
template <int CTRL>
PBG_DEV double dpp_f(double x) {
  const uint64_t u = __builtin_bit_cast(uint64_t, x);
  const uint32_t lo = (uint32_t)__builtin_amdgcn_mov_dpp((int)(uint32_t)u, CTRL, 0xF, 0xF, true);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_mov_dpp((int)(uint32_t)(u >> 32), CTRL, 0xF, 0xF, true);
  return __builtin_bit_cast(double, ((uint64_t)hi << 32) | lo);
}
// gfx950 v_permlane16_swap_b32 a, b: the odd rows of a trade places with the even rows of b.
// With a = b = x (x uniform within each row) a ends up holding the even row's value and b the odd
// row's, in both rows of each pair.  Inline asm because this ROCm's builtin
// (__builtin_amdgcn_permlane16_swap) returns the first register for both of its results.  The
// compiler's hazard recognizer cannot see inside the asm, so the s_nop 3 (4 wait states) covers
// both hazards a preceding VALU instruction can leave for a permlane: a VALU write of an operand
// register, and a VALU write of EXEC (v_cmpx) -- the latter needs 4 wait states on gfx950.
// gang_sum<32> is only called from the 32-lane kernel's row reductions, all reached with the
// gang's full EXEC mask (wave-uniform control flow).
PBG_DEV void row_pair_swap(float& a, float& b) {
  asm volatile("s_nop 3\n\tv_permlane16_swap_b32 %0, %1" : "+v"(a), "+v"(b));
}
PBG_DEV void row_pair_swap_u(uint32_t& a, uint32_t& b) {
  asm volatile("s_nop 3\n\tv_permlane16_swap_b32 %0, %1" : "+v"(a), "+v"(b));
}
PBG_DEV void row_pair_swap(double& a, double& b) {  // the two dwords of each
  uint64_t ua = __builtin_bit_cast(uint64_t, a), ub = __builtin_bit_cast(uint64_t, b);
  uint32_t al = (uint32_t)ua, ah = (uint32_t)(ua >> 32), bl = (uint32_t)ub, bh = (uint32_t)(ub >> 32);
  row_pair_swap_u(al, bl);
  row_pair_swap_u(ah, bh);
  a = __builtin_bit_cast(double, ((uint64_t)ah << 32) | al);
  b = __builtin_bit_cast(double, ((uint64_t)bh << 32) | bl);
}
// all-reduce over the T (4, 8, 16 or 32) lanes of a DPP row segment (T = 32: a row pair);
// identical bits in every lane (each step adds a value and its mirror image: a + b == b + a;
// the row-pair step adds the even row's sum to the odd row's in that order in both rows)
template <int T, class V>
PBG_DEV V gang_sum(V x) {
  x = x + dpp_f<0xB1>(x);  // quad_perm [1,0,3,2]
  x = x + dpp_f<0x4E>(x);  // quad_perm [2,3,0,1]
  if constexpr (T >= 8) x = x + dpp_f<0x141>(x);   // row_half_mirror
  if constexpr (T >= 16) x = x + dpp_f<0x140>(x);  // row_mirror
  if constexpr (T >= 32) {
    V a = x, b = x;
    row_pair_swap(a, b);  // a: the even row's value, b: the odd row's, in both rows of the pair
    x = a + b;
  }
  return x;
}
template <int CTRL>
PBG_DEV uint32_t dpp_u(uint32_t x) {
  return (uint32_t)__builtin_amdgcn_mov_dpp((int)x, CTRL, 0xF, 0xF, true);
}
// integer sum over the T lanes of a DPP row segment (mod 2^32), same in every lane
template <int T>
PBG_DEV uint32_t gang_sum_u32(uint32_t x) {
  x += dpp_u<0xB1>(x);
  x += dpp_u<0x4E>(x);
  if constexpr (T >= 8) x += dpp_u<0x141>(x);
  if constexpr (T >= 16) x += dpp_u<0x140>(x);
  if constexpr (T >= 32) {
    uint32_t a = x, b = x;
    row_pair_swap_u(a, b);
    x = a + b;
  }
  return x;
}

}  // namespace pbg
