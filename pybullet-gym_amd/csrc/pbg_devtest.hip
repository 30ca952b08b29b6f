// pbg_devtest.hip -- test-only library libpbg_devtest.so (`make devtest`): the step kernels' device math
// and cross-lane primitives, each alone in a trivial kernel, for tests/test_devmath_host.py and
// tests/test_devmath_gpu.py.  Never linked into libpbg_amd.so and never loaded by _native.lib().
// Built with exactly the product's flags, so contraction (a * b + c -> fma) and code generation are
// the product's.
//
// pbgdt_<name>_dev(device pointers..., n, stream): a lane per element, no shared state, block 64;
//     returns the hipError_t of the launch (the caller synchronises).
// pbgdt_<name>_host(host pointers..., n): the same source text compiled for the host, where the
//     primitive is plain C++ (sincos_fast(float), pbg::sincos_reduced64).
// The lane entry points take n = a multiple of 64: whole waves, so every helper sees the full EXEC mask
// its contract requires (anything else is refused with hipErrorInvalidValue before any launch).
// pbgdt_lds_peek_dev: what a workgroup finds in its LDS, the witness of tests/poison.py's LDS poison
// (tests/test_learner_invariance_gpu.py).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pbg_math.h"
#include "pbg_lanes.h"
#include "pbg_es_noise.h"

namespace {

template <class F>
__global__ __launch_bounds__(64) void map_kernel(long n, F f) {
  const long i = (long)blockIdx.x * 64 + threadIdx.x;
  if (i < n) f(i);
}
// whole waves only: no lane is masked off (n % 64 == 0, checked by the caller)
template <class F>
__global__ __launch_bounds__(64) void wave_kernel(F f) {
  f((long)blockIdx.x * 64 + threadIdx.x);
}
template <class F>
int launch_map(long n, hipStream_t s, F f) {
  if (n < 0 || n > (1L << 24)) return (int)hipErrorInvalidValue;
  if (n == 0) return 0;
  hipLaunchKernelGGL(map_kernel<F>, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, s, n, f);
  return (int)hipGetLastError();
}
template <class F>
int launch_waves(long n, hipStream_t s, F f) {
  if (n <= 0 || n % 64 != 0 || n > (1L << 24)) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(wave_kernel<F>, dim3((unsigned)(n / 64)), dim3(64), 0, s, f);
  return (int)hipGetLastError();
}

// tests/poison.py's witness: what a workgroup finds in its LDS.  Dynamic LDS, so the loads cannot be folded away;
// loads only, no LDS word is written.
__global__ __launch_bounds__(256) void lds_peek_kernel(uint32_t* out, int words_per_wg) {
  extern __shared__ uint32_t lds_peek[];
  for (int i = threadIdx.x; i < words_per_wg; i += 256) out[(size_t)blockIdx.x * words_per_wg + i] = lds_peek[i];
}

}  // namespace

extern "C" {

// ---------------------------------------------------------------- the LDS a workgroup starts on
// out[w * words_per_wg + i] = word i of workgroup w's LDS as it found it, n_wg workgroups of 256 lanes with
// words_per_wg words (at most the 160 KiB of a CU) of dynamic LDS each; out: n_wg * words_per_wg words on the device
int pbgdt_lds_peek_dev(uint32_t* out, int words_per_wg, int n_wg, hipStream_t st) {
  if (!out || words_per_wg < 1 || words_per_wg > 163840 / 4 || n_wg < 1 || n_wg > 8192) return (int)hipErrorInvalidValue;
  const hipError_t e = hipFuncSetAttribute((const void*)lds_peek_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                           words_per_wg * 4);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(lds_peek_kernel, dim3((unsigned)n_wg), dim3(256), (size_t)words_per_wg * 4, st, out, words_per_wg);
  return (int)hipGetLastError();
}

// ---------------------------------------------------------------- sin / cos
int pbgdt_sincos32_dev(const float* x, float* s, float* c, long n, hipStream_t st) {
  return launch_map(n, st, [=] __device__(long i) { sincos_fast(x[i], &s[i], &c[i]); });
}
void pbgdt_sincos32_host(const float* x, float* s, float* c, long n) {
  for (long i = 0; i < n; i++) sincos_fast(x[i], &s[i], &c[i]);
}
int pbgdt_sincos64_dev(const double* x, double* s, double* c, long n, hipStream_t st) {
  return launch_map(n, st, [=] __device__(long i) { sincos_fast(x[i], &s[i], &c[i]); });
}
void pbgdt_sincos64_host(const double* x, double* s, double* c, long n) {
  for (long i = 0; i < n; i++) pbg::sincos_reduced64(x[i], &s[i], &c[i]);
}

// ---------------------------------------------------------------- reciprocal, sqrt, rsq, clamp
#define PBGDT_UNARY(name, T, fn)                                                         \
  int pbgdt_##name##_dev(const T* x, T* y, long n, hipStream_t st) {                     \
    return launch_map(n, st, [=] __device__(long i) { y[i] = fn(x[i]); });               \
  }
PBGDT_UNARY(rcp32, float, fast_rcp)
PBGDT_UNARY(sqrt32, float, fast_sqrt)
PBGDT_UNARY(rsq32, float, fast_rsq)
PBGDT_UNARY(rcp64, double, fast_rcp)
PBGDT_UNARY(sqrt64, double, fast_sqrt)
#undef PBGDT_UNARY
int pbgdt_clamp32_dev(const float* x, float lo, float hi, float* y, long n, hipStream_t st) {
  return launch_map(n, st, [=] __device__(long i) { y[i] = clampf<float>(x[i], lo, hi); });
}
int pbgdt_clamp64_dev(const double* x, double lo, double hi, double* y, long n, hipStream_t st) {
  return launch_map(n, st, [=] __device__(long i) { y[i] = clampf<double>(x[i], lo, hi); });
}

// ---------------------------------------------------------------- lane primitives (n % 64 == 0)
#define PBGDT_LANE(name, T, expr)                                                        \
  int pbgdt_##name##_dev(const T* x, T* y, long n, hipStream_t st) {                     \
    return launch_waves(n, st, [=] __device__(long i) { y[i] = expr(x[i]); });           \
  }
PBGDT_LANE(quad_sum_f32, float, pbg::quad_sum)
PBGDT_LANE(quad_sum_f64, double, pbg::quad_sum)
PBGDT_LANE(quad_sum_i32, int, pbg::quad_sum_i)
#define PBGDT_GANG(T)                                               \
  PBGDT_LANE(gang_sum##T##_f32, float, (pbg::gang_sum<T, float>))   \
  PBGDT_LANE(gang_sum##T##_f64, double, (pbg::gang_sum<T, double>)) \
  PBGDT_LANE(gang_sum##T##_u32, uint32_t, pbg::gang_sum_u32<T>)
PBGDT_GANG(4)
PBGDT_GANG(8)
PBGDT_GANG(16)
PBGDT_GANG(32)
#undef PBGDT_GANG
#define PBGDT_BCAST(K)                                           \
  PBGDT_LANE(quad_bcast##K##_f32, float, pbg::quad_bcast<K>)     \
  PBGDT_LANE(quad_bcast##K##_f64, double, pbg::quad_bcast<K>)    \
  PBGDT_LANE(quad_bcast##K##_i32, int, pbg::quad_bcast_i<K>)     \
  PBGDT_LANE(quad_bcast_f64_##K, double, pbg::quad_bcast_f64<K>)
PBGDT_BCAST(0)
PBGDT_BCAST(1)
PBGDT_BCAST(2)
PBGDT_BCAST(3)
#undef PBGDT_BCAST
#undef PBGDT_LANE
// row_pair_swap with a = b = x: a and b out
#define PBGDT_SWAP(name, T, fn)                                                   \
  int pbgdt_##name##_dev(const T* x, T* a, T* b, long n, hipStream_t st) {        \
    return launch_waves(n, st, [=] __device__(long i) {                           \
      T va = x[i], vb = va;                                                       \
      fn(va, vb);                                                                 \
      a[i] = va;                                                                  \
      b[i] = vb;                                                                  \
    });                                                                           \
  }
PBGDT_SWAP(row_pair_swap_f32, float, pbg::row_pair_swap)
PBGDT_SWAP(row_pair_swap_u32, uint32_t, pbg::row_pair_swap_u)
PBGDT_SWAP(row_pair_swap_f64, double, pbg::row_pair_swap)
#undef PBGDT_SWAP

// ---------------------------------------------------------------- evolution-strategy noise
int pbgdt_box_muller_dev(const uint32_t* a, const uint32_t* b, float* n0, float* n1, long n, hipStream_t st) {
  return launch_map(n, st, [=] __device__(long i) { pbg::es::es_box_muller(a[i], b[i], n0[i], n1[i]); });
}

}  // extern "C"
