// pbg_perm.hip -- counter-based permutations of 0 .. B - 1 (include/pbg.h "Counter-based permutations"): the
// pbg_perm object with its device counter, the fill (two launches: the elements, then one lane that advances the
// counter) and the host twin; and the linear learning-rate schedule that the optimiser step reads from device memory
// (pbg_ppo_lr_linear, one lane, with its host twin).
//
// perm(seed, c, B) is an eight-round Feistel network on the smallest even number of bits k that holds B, keyed by
// eight Philox words of (seed, c), cycle-walked into range.  Everything is uint32 arithmetic in one
// __host__ __device__ function, so the host twin gives the device's bits.
//
// The fill kernel: one lane per output element, the permutation index is blockIdx.y.  The eight round keys depend
// on the launch arguments, the counter (one load through a kernel-argument pointer) and blockIdx.y alone: every
// operand is uniform, so the two Philox blocks are scalar instructions on scalar registers, once per wave, and
// the rounds read the keys as scalar operands (no LDS, no barrier).  The cycle walk is a per-lane loop: lanes that
// are in range wait masked for the wave's longest walk (2^k < 4 B: under four passes on average).
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include <new>

#include "pbg_policy_dev.h"

struct pbg_perm {
  int device;
  uint64_t seed;
  uint32_t* counter;  // DEVICE, one word
};

namespace {

using namespace pbg::policy;
using pbg::DeviceGuard;

constexpr int PERM_LANES = 256;       // the fill's workgroup
constexpr uint32_t PERM_TAG = 0x9Eu;  // fourth counter word: apart from 0xE5, 0xAC, 0xAC7, 0x5EED
constexpr int MAX_PERMS = 65535;      // the grid's second dimension

struct PermKeys {
  uint32_t k[8];
};

// the Feistel geometry of B: the half-width in bits and its mask
struct PermGeom {
  uint32_t half, mask;
};

inline PermGeom perm_geom(uint32_t B) {
  uint32_t k = 0;
  for (uint32_t v = B - 1u; v; v >>= 1) k++;  // bit_length(B - 1)
  if (k < 2u) k = 2u;
  k += k & 1u;
  return PermGeom{k / 2u, (1u << (k / 2u)) - 1u};
}

// murmur3's finaliser (sim_params.h's contact hash ends with it)
__host__ __device__ __forceinline__ uint32_t fmix32(uint32_t h) {
  h ^= h >> 16;
  h *= 0x85EBCA6Bu;
  h ^= h >> 13;
  h *= 0xC2B2AE35u;
  h ^= h >> 16;
  return h;
}

// pbg.h's walk from i < B: it stays on i's cycle of the bijection of [0, 2^k), which holds i < B, so it ends
__host__ __device__ __forceinline__ uint32_t perm_walk(uint32_t i, uint32_t B, uint32_t half, uint32_t mask, const PermKeys& K) {
  uint32_t x = i;
  do {
    uint32_t L = x >> half, R = x & mask;
#pragma unroll
    for (int r = 0; r < 8; r++) {
      const uint32_t F = fmix32(R + K.k[r]) & mask;
      const uint32_t nR = L ^ F;
      L = R;
      R = nR;
    }
    x = (L << half) | R;
  } while (x >= B);
  return x;
}

__device__ __forceinline__ PermKeys perm_keys_dev(uint32_t k0, uint32_t k1, uint32_t c) {
  PermKeys K;
#pragma unroll
  for (uint32_t j = 0; j < 2; j++) {
    u4 ctr;
    ctr.x = c;
    ctr.y = j;
    ctr.z = 0u;
    ctr.w = PERM_TAG;
    const u4 r = philox4x32_10(ctr, k0, k1);
    K.k[4 * j] = r.x;
    K.k[4 * j + 1] = r.y;
    K.k[4 * j + 2] = r.z;
    K.k[4 * j + 3] = r.w;
  }
  return K;
}

inline PermKeys perm_keys_host(uint32_t k0, uint32_t k1, uint32_t c) {
  PermKeys K;
  for (uint32_t j = 0; j < 2; j++) {
    uint32_t ctr[4] = {c, j, 0u, PERM_TAG};
    pbg::es::host_philox(ctr, k0, k1);
    for (int t = 0; t < 4; t++) K.k[4 * j + t] = ctr[t];
  }
  return K;
}

// launch 1: out[j][i] = perm(seed, *counter + j, B)[i], j = blockIdx.y; reads the counter, never writes it
__global__ __launch_bounds__(PERM_LANES) void perm_fill_kernel(uint32_t B, uint32_t half, uint32_t mask, uint32_t k0,
                                                               uint32_t k1, const uint32_t* __restrict__ counter,
                                                               int64_t* __restrict__ out) {
  const uint32_t c = *counter + blockIdx.y;  // uint32: wraps
  const PermKeys K = perm_keys_dev(k0, k1, c);
  const uint32_t i = blockIdx.x * PERM_LANES + threadIdx.x;
  if (i >= B) return;
  out[(size_t)blockIdx.y * B + i] = (int64_t)perm_walk(i, B, half, mask, K);
}

// launch 2: one lane, after every workgroup of launch 1 has read the counter
__global__ void perm_advance_kernel(uint32_t* counter, uint32_t add) {
  if (blockIdx.x == 0 && threadIdx.x == 0) *counter += add;
}

__global__ void perm_set_kernel(uint32_t* counter, uint32_t value) {
  if (blockIdx.x == 0 && threadIdx.x == 0) *counter = value;
}

// pbg.h's linear schedule, host and device: float64, nothing contracted
__host__ __device__ __forceinline__ double lr_linear(uint32_t it, uint32_t n_total, double lr0) {
#pragma clang fp contract(off)
  const uint32_t m = it < n_total ? it : n_total;
  const double q = (double)m / (double)n_total;
  return lr0 * (1.0 - q);
}

__global__ void lr_linear_kernel(const uint32_t* __restrict__ it, uint32_t n_total, double lr0, double* __restrict__ lr_out) {
  if (blockIdx.x == 0 && threadIdx.x == 0) *lr_out = lr_linear(*it, n_total, lr0);
}

int fill_args(const char* who, int n_rows, int n_perms, const int64_t* out) {
  if (n_rows < 1 || n_perms < 1 || n_perms > MAX_PERMS || !out) {
    char msg[200];
    snprintf(msg, sizeof(msg), "%s: n_rows %d must be >= 1, n_perms %d in 1 .. %d and out not NULL", who, n_rows, n_perms,
             MAX_PERMS);
    return pbg::capi_fail(PBG_E_ARG, msg);
  }
  return PBG_OK;
}

}  // namespace

extern "C" {

int pbg_perm_create(int device, uint64_t seed, pbg_perm** out) {
  if (!out) return pbg::capi_fail(PBG_E_ARG, "pbg_perm_create: out is NULL");
  *out = nullptr;
  if (device < 0) return pbg::capi_fail(PBG_E_ARG, "pbg_perm_create: device < 0");
  if (const int rc = check_device("pbg_perm_create", device)) return rc;
  pbg_perm* p = new (std::nothrow) pbg_perm();
  if (!p) return pbg::capi_fail(PBG_E_NOMEM, "pbg_perm_create: out of host memory");
  p->device = device;
  p->seed = seed;
  p->counter = nullptr;
  DeviceGuard dg(device);
  int e = (int)hipMalloc(&p->counter, 16);
  if (e) {
    delete p;
    return hip_fail(e, "pbg_perm_create: storage");
  }
  // the counter by a kernel of this unit: its code object is then loaded before a first fill, which may be one
  // that a stream capture records
  hipLaunchKernelGGL(perm_set_kernel, dim3(1), dim3(64), 0, (hipStream_t) nullptr, p->counter, 0u);
  e = (int)hipGetLastError();
  if (!e) e = (int)hipStreamSynchronize(nullptr);
  if (e) {
    pbg_perm_destroy(p);
    return hip_fail(e, "pbg_perm_create: counter");
  }
  *out = p;
  return PBG_OK;
}

void pbg_perm_destroy(pbg_perm* p) {
  if (!p) return;
  if (p->counter) {
    DeviceGuard dg(p->device);
    (void)hipFree(p->counter);
  }
  delete p;
}

int pbg_perm_fill(pbg_perm* p, int n_rows, int n_perms, int64_t* out, void* stream) {
  if (!p) return pbg::capi_fail(PBG_E_ARG, "pbg_perm_fill: the object is NULL");
  if (const int rc = fill_args("pbg_perm_fill", n_rows, n_perms, out)) return rc;
  const PermGeom g = perm_geom((uint32_t)n_rows);
  DeviceGuard dg(p->device);
  const dim3 grid((unsigned)(((long long)n_rows + PERM_LANES - 1) / PERM_LANES), (unsigned)n_perms);
  hipLaunchKernelGGL(perm_fill_kernel, grid, dim3(PERM_LANES), 0, (hipStream_t)stream, (uint32_t)n_rows, g.half, g.mask,
                     (uint32_t)p->seed, (uint32_t)(p->seed >> 32), p->counter, out);
  if (const int rc = launched("perm_fill_kernel launch")) return rc;
  hipLaunchKernelGGL(perm_advance_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, p->counter, (uint32_t)n_perms);
  return launched("perm_advance_kernel launch");
}

int pbg_perm_set_counter(pbg_perm* p, uint32_t c, void* stream) {
  if (!p) return pbg::capi_fail(PBG_E_ARG, "pbg_perm_set_counter: the object is NULL");
  DeviceGuard dg(p->device);
  hipLaunchKernelGGL(perm_set_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, p->counter, c);
  return launched("perm_set_kernel launch");
}

int pbg_perm_get_counter(const pbg_perm* p, uint32_t* c_out, void* stream) {
  if (!p || !c_out) return pbg::capi_fail(PBG_E_ARG, "pbg_perm_get_counter: NULL object or c_out");
  DeviceGuard dg(p->device);
  const int e = (int)hipMemcpyAsync(c_out, p->counter, sizeof(uint32_t), hipMemcpyDeviceToDevice, (hipStream_t)stream);
  return e ? hip_fail(e, "pbg_perm_get_counter: copy") : PBG_OK;
}

int pbg_perm_host(uint64_t seed, uint32_t counter, int n_rows, int n_perms, int64_t* out) {
  if (const int rc = fill_args("pbg_perm_host", n_rows, n_perms, out)) return rc;
  const uint32_t B = (uint32_t)n_rows;
  const PermGeom g = perm_geom(B);
  for (int j = 0; j < n_perms; j++) {
    const PermKeys K = perm_keys_host((uint32_t)seed, (uint32_t)(seed >> 32), counter + (uint32_t)j);
    int64_t* row = out + (size_t)j * B;
    for (uint32_t i = 0; i < B; i++) row[i] = (int64_t)perm_walk(i, B, g.half, g.mask, K);
  }
  return PBG_OK;
}

int pbg_ppo_lr_linear(const uint32_t* it, uint32_t n_total, double lr0, double* lr_out, void* stream) {
  if (!it || !lr_out || n_total < 1u) return pbg::capi_fail(PBG_E_ARG, "pbg_ppo_lr_linear: it or lr_out NULL or n_total < 1");
  hipLaunchKernelGGL(lr_linear_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, it, n_total, lr0, lr_out);
  return launched("lr_linear_kernel launch");
}

int pbg_ppo_lr_linear_host(const uint32_t* it, uint32_t n_total, double lr0, double* lr_out) {
  if (!it || !lr_out || n_total < 1u)
    return pbg::capi_fail(PBG_E_ARG, "pbg_ppo_lr_linear_host: it or lr_out NULL or n_total < 1");
  *lr_out = lr_linear(*it, n_total, lr0);
  return PBG_OK;
}

}  // extern "C"
