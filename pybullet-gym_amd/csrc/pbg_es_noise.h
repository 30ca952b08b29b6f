// pbg_es_noise.h -- the device side of the evolution-strategy noise (include/pbg.h "Noise contract"):
// es_box_muller and es_normals4, verbatim what pbg_population.hip held in its anonymous namespace, in a
// header so that the test unit (pbg_devtest.hip, tests/test_devmath_gpu.py) feeds es_box_muller the
// contract's edge words directly.
#pragma once
#include "pbg_math.h"

namespace pbg {
namespace es {

constexpr uint32_t ES_TAG = 0xE5u;  // fourth counter word of the noise stream

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

// The four normals of parameters 4 b .. 4 b + 3 of the global pair `pair` in `generation`.
__device__ __forceinline__ void es_normals4(uint32_t k0, uint32_t k1, uint32_t b, uint32_t pair, uint32_t generation,
                                            float e[4]) {
  u4 c;
  c.x = b;
  c.y = pair;
  c.z = generation;
  c.w = ES_TAG;
  const u4 x = philox4x32_10(c, k0, k1);
  es_box_muller(x.x, x.y, e[0], e[1]);
  es_box_muller(x.z, x.w, e[2], e[3]);
}

}  // namespace es
}  // namespace pbg
