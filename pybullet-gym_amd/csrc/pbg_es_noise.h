// pbg_es_noise.h -- the counter-based normals (include/pbg.h "Noise contract"): es_box_muller and es_normals4
// on the device, in a header so that the evolution strategy's kernels (pbg_population.hip), the sampling actor
// (pbg_policy_dev.h) and the test unit (pbg_devtest.hip, tests/test_devmath_gpu.py, which feeds es_box_muller
// the contract's edge words directly) call the same function; the streams differ by the counter's fourth
// word.  The host counterparts of both streams (float64, rounded once) are here as well.
#pragma once
#include <math.h>

#include "pbg_math.h"

namespace pbg {
namespace es {

constexpr uint32_t ES_TAG = 0xE5u;      // fourth counter word of the evolution strategy's noise stream
constexpr uint32_t ACTION_TAG = 0xACu;  // of the action noise's (pbg.h "Stochastic Gaussian actions")

// Two normals from two Philox words (pbg.h "Noise contract").  u1 = (a >> 9 + 1/2) 2^-23 lies in (0, 1)
// and is exact; -2 logf, 2 u2 and the two r * trig products feed no add.
__device__ __forceinline__ void es_box_muller(uint32_t a, uint32_t b, float& n0, float& n1) {
  const float u1 = __builtin_fmaf((float)(a >> 9), 0x1p-23f, 0x1p-24f);
  const float u2 = (float)(b >> 8) * 0x1p-24f;
  const float r = sqrtf(-2.0f * logf(u1));
  const float t = 2.0f * u2;
  n0 = r * cospif(t);
  n1 = r * sinpif(t);
}

// The four normals of parameters 4 b .. 4 b + 3 of the global pair `pair` in `generation` (tag ES_TAG); of
// action components 4 b .. 4 b + 3 of the global env `pair` at step count `generation` (tag ACTION_TAG).
__device__ __forceinline__ void es_normals4(uint32_t k0, uint32_t k1, uint32_t b, uint32_t pair, uint32_t generation,
                                            uint32_t tag, float e[4]) {
  u4 c;
  c.x = b;
  c.y = pair;
  c.z = generation;
  c.w = tag;
  const u4 x = philox4x32_10(c, k0, k1);
  es_box_muller(x.x, x.y, e[0], e[1]);
  es_box_muller(x.z, x.w, e[2], e[3]);
}

// ---------------------------------------------------------------- the host counterparts (float64, rounded once)
inline void host_philox(uint32_t c[4], uint32_t k0, uint32_t k1) {
  for (int r = 0; r < 10; r++) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n1 = (uint32_t)p1;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1, n3 = (uint32_t)p0;
    c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
}

inline void host_box_muller(uint32_t a, uint32_t b, float* n0, float* n1) {
  const double u1 = (double)(a >> 9) * 0x1p-23 + 0x1p-24;
  const double u2 = (double)(b >> 8) * 0x1p-24;
  const double r = sqrt(-2.0 * log(u1));
  const double ang = 2.0 * M_PI * u2;
  *n0 = (float)(r * cos(ang));
  *n1 = (float)(r * sin(ang));
}

// es_normals4 on the host: the block at counter (b, pair, generation, tag)
inline void host_normals4(uint32_t k0, uint32_t k1, uint32_t b, uint32_t pair, uint32_t generation, uint32_t tag,
                          float e[4]) {
  uint32_t c[4] = {b, pair, generation, tag};
  host_philox(c, k0, k1);
  host_box_muller(c[0], c[1], &e[0], &e[1]);
  host_box_muller(c[2], c[3], &e[2], &e[3]);
}

}  // namespace es
}  // namespace pbg
