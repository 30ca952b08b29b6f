// pbg_retstats.hip -- reward scaling by a running standard deviation of the discounted return (include/pbg.h "Return
// statistics"): the pbg_ret_stats object, its three launches (walk, finalize, apply), the copy
// and reset launches of its accessors, and the host twin (an object created with device -1, whose state is host
// memory and whose calls run the same functions in the same order on the calling thread).
//
// Order of every sum (pbg.h): a lane per env walks t ascending (ret_step, host and device); the 32 lanes of a tile
// meet in the tree x[l] += x[l + s], s = 16 .. 1, and lane 0 overwrites the tile's slot; finalize adds the used slots
// in ascending order onto (0, +0.0, +0.0) in one lane, then that onto the totals.  No atomics anywhere, nothing read
// back, all float64 arithmetic uncontracted.
//
// The walk's workgroup is one wave of 64 lanes (two tiles): at 16,384 envs that is 256 workgroups, one per CU, where
// 256-lane workgroups would occupy 64 of the 256 CUs.  A lane's loads of rew_traj[t][e] and done_traj[t][e] do not
// depend on the running return, so they are issued WALK_AHEAD steps at a time in front of the dependent chain; across
// lanes they are consecutive addresses.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <new>

#include "pbg_policy_dev.h"

// One allocation of 8-byte words (device memory, or host memory for device -1):
// tot_count [1] | tot_sums [2] | scale (a float32 in the first half of a word) | carry [n_envs] | slot_count [n_slots] |
// slot_sums [n_slots, 2]
struct pbg_ret_stats {
  int device, n_envs, n_slots;
  double gamma;
  int64_t* tot_count;
  double* tot_sums;
  float* scale;
  double* carry;
  int64_t* slot_count;
  double* slot_sums;

  size_t words() const { return 4 + (size_t)n_envs + 3 * (size_t)n_slots; }
};

namespace {

using namespace pbg::policy;
using pbg::DeviceGuard;

constexpr int TILE = 32;        // the envs of one slot
constexpr int WALK_LANES = 64;  // the walk's workgroup: one wave, two tiles
constexpr int WALK_AHEAD = 8;   // the steps whose loads a lane issues in front of its chain
constexpr int FIN_LANES = 64;   // finalize's one workgroup: the slots it stages per pass
constexpr int APPLY_LANES = 256;
constexpr int APPLY_MAX_WG = 2048;  // apply's grid: 256 CUs x 8, the rest by stride

// pbg.h's step of env e's discounted return, host and device: two roundings for R, the product R * R rounded before
// its add
__host__ __device__ __forceinline__ void ret_step(double gamma, float r, uint8_t d, double& R, long long& c, double& s1,
                                                  double& s2) {
#pragma clang fp contract(off)
  const double g = gamma * R;
  R = g + (double)r;
  const bool fin = __builtin_isfinite(R);
  if (fin) {
    const double q = R * R;
    c += 1;
    s1 += R;
    s2 += q;
  }
  if (!fin || d != 0) R = 0.0;
}

// pbg.h's scale from the batch's slot sum (bc, b1, b2), host and device: the totals advance, and the scale follows
// them unless they are still empty
__host__ __device__ __forceinline__ void ret_finish(long long bc, double b1, double b2, double var_floor, int64_t* tot_count,
                                                    double* tot_sums, float* scale) {
#pragma clang fp contract(off)
  const long long tc = (long long)*tot_count + bc;
  const double t1 = tot_sums[0] + b1;
  const double t2 = tot_sums[1] + b2;
  *tot_count = (int64_t)tc;
  tot_sums[0] = t1;
  tot_sums[1] = t2;
  if (tc == 0) return;
  const double cnt = (double)tc;
  const double m = t1 / cnt;
  const double mm = m * m;
  double var = t2 / cnt - mm;
  var = var > var_floor ? var : var_floor;  // a NaN variance takes the floor too
  *scale = (float)(1.0 / sqrt(var));
}

// pbg.h's scaled and clipped reward: one float32 rounding, a NaN passes
__host__ __device__ __forceinline__ float ret_apply(float r, float sc, float clip) {
#pragma clang fp contract(off)
  const float v = r * sc;
  return v < -clip ? -clip : (v > clip ? clip : v);
}

// grid = ceil(n / 64) workgroups of one wave: lane e walks env e, then each half of the wave is a tile's tree
__global__ __launch_bounds__(WALK_LANES) void ret_walk_kernel(int T, int n, int slot_offset, double gamma,
                                                              const float* __restrict__ rew, const uint8_t* __restrict__ done,
                                                              double* __restrict__ carry, int64_t* __restrict__ slot_count,
                                                              double* __restrict__ slot_sums) {
#pragma clang fp contract(off)
  const int e = blockIdx.x * WALK_LANES + threadIdx.x;
  long long c = 0;
  double s1 = 0.0, s2 = 0.0;
  if (e < n) {
    double R = carry[e];
    const float* rp = rew + e;
    const uint8_t* dp = done + e;
    int t = 0;
    for (; t + WALK_AHEAD <= T; t += WALK_AHEAD) {
      float r[WALK_AHEAD];
      uint8_t d[WALK_AHEAD];
#pragma unroll
      for (int k = 0; k < WALK_AHEAD; k++) {
        r[k] = rp[(size_t)(t + k) * n];
        d[k] = dp[(size_t)(t + k) * n];
      }
#pragma unroll
      for (int k = 0; k < WALK_AHEAD; k++) ret_step(gamma, r[k], d[k], R, c, s1, s2);
    }
    for (; t < T; t++) ret_step(gamma, rp[(size_t)t * n], dp[(size_t)t * n], R, c, s1, s2);
    carry[e] = R;
  }
  // every lane of the wave is here: a lane past n holds (0, +0.0, +0.0).  Lane l < s of a tile takes lane l + s of the
  // same tile (width 32); what the lanes l >= s compute is never read by lane 0's chain
#pragma unroll
  for (int s = TILE / 2; s >= 1; s >>= 1) {
    c += __shfl_down(c, s, TILE);
    s1 += __shfl_down(s1, s, TILE);
    s2 += __shfl_down(s2, s, TILE);
  }
  if ((threadIdx.x & (TILE - 1)) == 0 && e < n) {
    const size_t at = (size_t)slot_offset + (size_t)(e / TILE);
    slot_count[at] = (int64_t)c;
    slot_sums[2 * at] = s1;
    slot_sums[2 * at + 1] = s2;
  }
}

// one workgroup: its lanes stage FIN_LANES slots a pass in LDS, lane 0 adds them in ascending order and finishes
__global__ __launch_bounds__(FIN_LANES) void ret_finalize_kernel(int n_used, double var_floor,
                                                                 const int64_t* __restrict__ slot_count,
                                                                 const double* __restrict__ slot_sums,
                                                                 int64_t* __restrict__ tot_count, double* __restrict__ tot_sums,
                                                                 float* __restrict__ scale) {
#pragma clang fp contract(off)
  __shared__ long long lc[FIN_LANES];
  __shared__ double l1[FIN_LANES];
  __shared__ double l2[FIN_LANES];
  const int tid = threadIdx.x;
  long long bc = 0;
  double b1 = 0.0, b2 = 0.0;
  for (int g0 = 0; g0 < n_used; g0 += FIN_LANES) {
    const int g = g0 + tid;
    if (g < n_used) {
      lc[tid] = (long long)slot_count[g];
      l1[tid] = slot_sums[2 * (size_t)g];
      l2[tid] = slot_sums[2 * (size_t)g + 1];
    }
    __syncthreads();
    if (tid == 0) {
      const int m = min(FIN_LANES, n_used - g0);
      for (int i = 0; i < m; i++) {
        bc += lc[i];
        b1 += l1[i];
        b2 += l2[i];
      }
    }
    __syncthreads();
  }
  if (tid == 0) ret_finish(bc, b1, b2, var_floor, tot_count, tot_sums, scale);
}

// VEC: count4 groups of four through float4 (both pointers 16-byte aligned), then the count - 4 count4 tail by the first
// lanes of workgroup 0; otherwise element by element.  The same expression per element either way
template <bool VEC>
__global__ __launch_bounds__(APPLY_LANES) void ret_apply_kernel(long long count, float clip, const float* __restrict__ scale,
                                                                const float* __restrict__ in, float* __restrict__ out) {
  const float sc = *scale;
  const long long i0 = (long long)blockIdx.x * APPLY_LANES + threadIdx.x, stride = (long long)gridDim.x * APPLY_LANES;
  if (VEC) {
    const long long count4 = count / 4;
    const float4* in4 = reinterpret_cast<const float4*>(in);
    float4* out4 = reinterpret_cast<float4*>(out);
    for (long long i = i0; i < count4; i += stride) {
      const float4 v = in4[i];
      float4 w;
      w.x = ret_apply(v.x, sc, clip);
      w.y = ret_apply(v.y, sc, clip);
      w.z = ret_apply(v.z, sc, clip);
      w.w = ret_apply(v.w, sc, clip);
      out4[i] = w;
    }
    const long long at = 4 * count4 + i0;
    if (i0 < 4 && at < count) out[at] = ret_apply(in[at], sc, clip);
  } else {
    for (long long i = i0; i < count; i += stride) out[i] = ret_apply(in[i], sc, clip);
  }
}

// the accessors' copy: n 4-byte words, a lane per word
__global__ __launch_bounds__(256) void ret_copy_kernel(long long n, const uint32_t* __restrict__ src, uint32_t* __restrict__ dst) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) dst[i] = src[i];
}

// pbg_ret_stats_reset: every 8-byte word of the object to zero (count 0, +0.0), then the scale to 1
__global__ __launch_bounds__(256) void ret_reset_kernel(long long words, uint64_t* __restrict__ base, float* __restrict__ scale) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < words) base[i] = 0u;
  // the scale's word is word 3 of the object: the lane that zeroed it writes the float, so no two lanes meet
  if (i == 3) *scale = 1.0f;
}

int tiles(int n) { return (n + TILE - 1) / TILE; }

// bytes from src to dst on the object's side: a launch on `stream`, or memcpy for a host object
int copy_words(const pbg_ret_stats* s, const void* src, void* dst, size_t bytes, void* stream, const char* what) {
  if (bytes == 0) return PBG_OK;
  if (s->device < 0) {
    memcpy(dst, src, bytes);
    return PBG_OK;
  }
  DeviceGuard dg(s->device);
  const long long n = (long long)(bytes / 4);
  hipLaunchKernelGGL(ret_copy_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, n,
                     (const uint32_t*)src, (uint32_t*)dst);
  return launched(what);
}

int check_slots(const char* who, const pbg_ret_stats* s, int first, int count, const void* counts, const void* sums) {
  char msg[200];
  if (!s || !counts || !sums) {
    snprintf(msg, sizeof(msg), "%s: NULL stats, counts or sums", who);
    return pbg::capi_fail(PBG_E_ARG, msg);
  }
  if (first < 0 || count < 0 || (long long)first + count > (long long)s->n_slots) {
    snprintf(msg, sizeof(msg), "%s: slots %d .. %d + %d are outside the object's 0 .. %d", who, first, first, count, s->n_slots);
    return pbg::capi_fail(PBG_E_ARG, msg);
  }
  return PBG_OK;
}

}  // namespace

extern "C" {

int pbg_ret_stats_create(int device, int n_envs, int n_slots, double gamma, pbg_ret_stats** out) {
  if (!out) return pbg::capi_fail(PBG_E_ARG, "pbg_ret_stats_create: out is NULL");
  *out = nullptr;
  if (n_envs < 1 || n_slots < tiles(n_envs < 1 ? 1 : n_envs) || !(gamma >= 0.0 && gamma <= 1.0) || device < -1) {
    char msg[200];
    snprintf(msg, sizeof(msg), "pbg_ret_stats_create: n_envs %d < 1, n_slots %d below a slot per %d envs, gamma %g outside [0, 1] "
             "or device %d < -1", n_envs, n_slots, TILE, gamma, device);
    return pbg::capi_fail(PBG_E_ARG, msg);
  }
  if (device >= 0)
    if (const int rc = check_device("pbg_ret_stats_create", device)) return rc;
  pbg_ret_stats* s = new (std::nothrow) pbg_ret_stats();
  if (!s) return pbg::capi_fail(PBG_E_NOMEM, "pbg_ret_stats_create: out of host memory");
  s->device = device;
  s->n_envs = n_envs;
  s->n_slots = n_slots;
  s->gamma = gamma;
  s->tot_count = nullptr;
  uint64_t* base = nullptr;
  if (device < 0) {
    base = (uint64_t*)calloc(s->words(), 8);
    if (!base) {
      delete s;
      return pbg::capi_fail(PBG_E_NOMEM, "pbg_ret_stats_create: out of host memory");
    }
  } else {
    DeviceGuard dg(device);
    const int e = (int)hipMalloc(&base, s->words() * 8);
    if (e) {
      delete s;
      return hip_fail(e, "pbg_ret_stats_create: storage");
    }
  }
  s->tot_count = reinterpret_cast<int64_t*>(base);
  s->tot_sums = reinterpret_cast<double*>(base + 1);
  s->scale = reinterpret_cast<float*>(base + 3);
  s->carry = reinterpret_cast<double*>(base + 4);
  s->slot_count = reinterpret_cast<int64_t*>(base + 4 + (size_t)n_envs);
  s->slot_sums = reinterpret_cast<double*>(base + 4 + (size_t)n_envs + (size_t)n_slots);
  // the initial state by this unit's reset kernel: its code object is then loaded before a first launch that a
  // stream capture may record
  int rc = pbg_ret_stats_reset(s, nullptr);
  if (!rc && device >= 0) {
    DeviceGuard dg(device);
    const int e = (int)hipStreamSynchronize(nullptr);
    if (e) rc = hip_fail(e, "pbg_ret_stats_create: reset");
  }
  if (rc) {
    pbg_ret_stats_destroy(s);
    return rc;
  }
  *out = s;
  return PBG_OK;
}

void pbg_ret_stats_destroy(pbg_ret_stats* s) {
  if (!s) return;
  if (s->tot_count) {
    if (s->device < 0) {
      free(s->tot_count);
    } else {
      DeviceGuard dg(s->device);
      (void)hipFree(s->tot_count);
    }
  }
  delete s;
}

int pbg_ret_stats_reset(pbg_ret_stats* s, void* stream) {
  if (!s) return pbg::capi_fail(PBG_E_ARG, "pbg_ret_stats_reset: stats is NULL");
  if (s->device < 0) {
    memset(s->tot_count, 0, s->words() * 8);
    *s->scale = 1.0f;
    return PBG_OK;
  }
  DeviceGuard dg(s->device);
  const long long w = (long long)s->words();
  hipLaunchKernelGGL(ret_reset_kernel, dim3((unsigned)((w + 255) / 256)), dim3(256), 0, (hipStream_t)stream, w,
                     reinterpret_cast<uint64_t*>(s->tot_count), s->scale);
  return launched("ret_reset_kernel launch");
}

int pbg_ret_stats_walk(pbg_ret_stats* s, int T, int n, int slot_offset, const float* rew_traj, const uint8_t* done_traj,
                       void* stream) {
  if (!s || !rew_traj || !done_traj) return pbg::capi_fail(PBG_E_ARG, "pbg_ret_stats_walk: NULL stats, rew_traj or done_traj");
  char msg[200];
  if (T < 1 || n < 1 || n > s->n_envs) {
    snprintf(msg, sizeof(msg), "pbg_ret_stats_walk: T = %d must be >= 1 and n = %d in 1 .. the object's %d envs", T, n, s->n_envs);
    return pbg::capi_fail(PBG_E_ARG, msg);
  }
  if (slot_offset < 0 || (long long)slot_offset + tiles(n) > (long long)s->n_slots) {
    snprintf(msg, sizeof(msg), "pbg_ret_stats_walk: the %d slots from %d are outside the object's 0 .. %d", tiles(n), slot_offset,
             s->n_slots);
    return pbg::capi_fail(PBG_E_ARG, msg);
  }
  if (s->device < 0) {
    // the device's lanes one after the other: lane l of tile b is env 32 b + l, a lane past n holds (0, +0.0, +0.0)
    for (int b = 0; b < tiles(n); b++) {
      long long c[TILE];
      double s1[TILE], s2[TILE];
      for (int l = 0; l < TILE; l++) {
        const int e = b * TILE + l;
        c[l] = 0;
        s1[l] = s2[l] = 0.0;
        if (e >= n) continue;
        double R = s->carry[e];
        for (int t = 0; t < T; t++)
          ret_step(s->gamma, rew_traj[(size_t)t * n + e], done_traj[(size_t)t * n + e], R, c[l], s1[l], s2[l]);
        s->carry[e] = R;
      }
      for (int st = TILE / 2; st >= 1; st >>= 1)
        for (int l = 0; l < st; l++) {
          c[l] += c[l + st];
          s1[l] += s1[l + st];
          s2[l] += s2[l + st];
        }
      const size_t at = (size_t)slot_offset + (size_t)b;
      s->slot_count[at] = (int64_t)c[0];
      s->slot_sums[2 * at] = s1[0];
      s->slot_sums[2 * at + 1] = s2[0];
    }
    return PBG_OK;
  }
  DeviceGuard dg(s->device);
  hipLaunchKernelGGL(ret_walk_kernel, dim3((unsigned)((n + WALK_LANES - 1) / WALK_LANES)), dim3(WALK_LANES), 0,
                     (hipStream_t)stream, T, n, slot_offset, s->gamma, rew_traj, done_traj, s->carry, s->slot_count, s->slot_sums);
  return launched("ret_walk_kernel launch");
}

int pbg_ret_stats_finalize(pbg_ret_stats* s, int n_used_slots, double var_floor, void* stream) {
  if (!s) return pbg::capi_fail(PBG_E_ARG, "pbg_ret_stats_finalize: stats is NULL");
  if (n_used_slots < 0 || n_used_slots > s->n_slots || !(var_floor > 0.0)) {
    char msg[200];
    snprintf(msg, sizeof(msg), "pbg_ret_stats_finalize: n_used_slots %d outside 0 .. %d or var_floor %g not > 0", n_used_slots,
             s->n_slots, var_floor);
    return pbg::capi_fail(PBG_E_ARG, msg);
  }
  if (s->device < 0) {
    long long bc = 0;
    double b1 = 0.0, b2 = 0.0;
    for (int g = 0; g < n_used_slots; g++) {
      bc += (long long)s->slot_count[g];
      b1 += s->slot_sums[2 * (size_t)g];
      b2 += s->slot_sums[2 * (size_t)g + 1];
    }
    ret_finish(bc, b1, b2, var_floor, s->tot_count, s->tot_sums, s->scale);
    return PBG_OK;
  }
  DeviceGuard dg(s->device);
  hipLaunchKernelGGL(ret_finalize_kernel, dim3(1), dim3(FIN_LANES), 0, (hipStream_t)stream, n_used_slots, var_floor,
                     s->slot_count, s->slot_sums, s->tot_count, s->tot_sums, s->scale);
  return launched("ret_finalize_kernel launch");
}

int pbg_ret_stats_apply(const pbg_ret_stats* s, int count, float clip, const float* rew_in, float* rew_out, void* stream) {
  if (!s || !rew_in || !rew_out) return pbg::capi_fail(PBG_E_ARG, "pbg_ret_stats_apply: NULL stats, rew_in or rew_out");
  if (count < 1 || !(clip > 0.f)) {
    char msg[160];
    snprintf(msg, sizeof(msg), "pbg_ret_stats_apply: count %d < 1 or clip %g not > 0", count, (double)clip);
    return pbg::capi_fail(PBG_E_ARG, msg);
  }
  const uintptr_t a = (uintptr_t)rew_in, b = (uintptr_t)rew_out, bytes = (uintptr_t)count * 4u;
  if (a < b + bytes && b < a + bytes)
    return pbg::capi_fail(PBG_E_ARG, "pbg_ret_stats_apply: rew_out overlaps rew_in (the raw rewards stay as they are)");
  if (s->device < 0) {
    const float sc = *s->scale;
    for (int i = 0; i < count; i++) rew_out[i] = ret_apply(rew_in[i], sc, clip);
    return PBG_OK;
  }
  DeviceGuard dg(s->device);
  const bool vec = ((a | b) & 15u) == 0;
  const long long work = vec ? ((long long)count + 3) / 4 : (long long)count;
  long long wg = (work + APPLY_LANES - 1) / APPLY_LANES;
  if (wg > APPLY_MAX_WG) wg = APPLY_MAX_WG;
  hipLaunchKernelGGL(vec ? ret_apply_kernel<true> : ret_apply_kernel<false>, dim3((unsigned)wg), dim3(APPLY_LANES), 0,
                     (hipStream_t)stream, (long long)count, clip, s->scale, rew_in, rew_out);
  return launched("ret_apply_kernel launch");
}

int pbg_ret_stats_get_slots(const pbg_ret_stats* s, int first, int count, int64_t* counts_out, double* sums_out, void* stream) {
  if (const int rc = check_slots("pbg_ret_stats_get_slots", s, first, count, counts_out, sums_out)) return rc;
  if (const int rc = copy_words(s, s->slot_count + first, counts_out, (size_t)count * 8, stream, "pbg_ret_stats_get_slots: counts"))
    return rc;
  return copy_words(s, s->slot_sums + 2 * (size_t)first, sums_out, (size_t)count * 16, stream, "pbg_ret_stats_get_slots: sums");
}

int pbg_ret_stats_set_slots(pbg_ret_stats* s, int first, int count, const int64_t* counts, const double* sums, void* stream) {
  if (const int rc = check_slots("pbg_ret_stats_set_slots", s, first, count, counts, sums)) return rc;
  if (const int rc = copy_words(s, counts, s->slot_count + first, (size_t)count * 8, stream, "pbg_ret_stats_set_slots: counts"))
    return rc;
  return copy_words(s, sums, s->slot_sums + 2 * (size_t)first, (size_t)count * 16, stream, "pbg_ret_stats_set_slots: sums");
}

int pbg_ret_stats_get_totals(const pbg_ret_stats* s, int64_t* count_out, double* sums_out, void* stream) {
  if (!s || !count_out || !sums_out) return pbg::capi_fail(PBG_E_ARG, "pbg_ret_stats_get_totals: NULL stats, count_out or sums_out");
  if (const int rc = copy_words(s, s->tot_count, count_out, 8, stream, "pbg_ret_stats_get_totals: count")) return rc;
  return copy_words(s, s->tot_sums, sums_out, 16, stream, "pbg_ret_stats_get_totals: sums");
}

int pbg_ret_stats_set_totals(pbg_ret_stats* s, const int64_t* count, const double* sums, void* stream) {
  if (!s || !count || !sums) return pbg::capi_fail(PBG_E_ARG, "pbg_ret_stats_set_totals: NULL stats, count or sums");
  if (const int rc = copy_words(s, count, s->tot_count, 8, stream, "pbg_ret_stats_set_totals: count")) return rc;
  return copy_words(s, sums, s->tot_sums, 16, stream, "pbg_ret_stats_set_totals: sums");
}

int pbg_ret_stats_get_carry(const pbg_ret_stats* s, double* carry_out, void* stream) {
  if (!s || !carry_out) return pbg::capi_fail(PBG_E_ARG, "pbg_ret_stats_get_carry: NULL stats or carry_out");
  return copy_words(s, s->carry, carry_out, (size_t)s->n_envs * 8, stream, "pbg_ret_stats_get_carry");
}

int pbg_ret_stats_set_carry(pbg_ret_stats* s, const double* carry, void* stream) {
  if (!s || !carry) return pbg::capi_fail(PBG_E_ARG, "pbg_ret_stats_set_carry: NULL stats or carry");
  return copy_words(s, carry, s->carry, (size_t)s->n_envs * 8, stream, "pbg_ret_stats_set_carry");
}

int pbg_ret_stats_get_scale(const pbg_ret_stats* s, float* scale_out, void* stream) {
  if (!s || !scale_out) return pbg::capi_fail(PBG_E_ARG, "pbg_ret_stats_get_scale: NULL stats or scale_out");
  return copy_words(s, s->scale, scale_out, 4, stream, "pbg_ret_stats_get_scale");
}

int pbg_ret_stats_set_scale(pbg_ret_stats* s, const float* scale, void* stream) {
  if (!s || !scale) return pbg::capi_fail(PBG_E_ARG, "pbg_ret_stats_set_scale: NULL stats or scale");
  return copy_words(s, scale, s->scale, 4, stream, "pbg_ret_stats_set_scale");
}

}  // extern "C"
