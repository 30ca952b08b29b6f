// pbg_obsnorm.hip -- running observation statistics (include/pbg.h pbg_obs_stats_*): the object, the
// stand-alone update kernel and the finalize kernel.  The tile accumulation itself (stats_tile) and the
// tile load that sets the flags (load_tile) are pbg_policy_dev.h's, the very functions the actor kernel runs
// during a rollout: the stand-alone kernel is those two around one barrier.
//
// Order of every sum (pbg.h): inside a slot (launch ascending, row-in-tile ascending), written by one lane
// per component; finalize folds slot 0, 1, ... into the totals with sequential float64 adds, one lane per
// component.  No atomics anywhere.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>

#include <new>

#include "pbg_policy_dev.h"

namespace {

using namespace pbg::policy;
using pbg::DeviceGuard;

// grid = groups * tpm workgroups, tpm = ceil(G / PT): workgroup b owns the rows of tile_of(b), as in the
// actor kernel (G = n: a shared-weight policy's tiling); `active` NULL = every row
__global__ __launch_bounds__(PB) void obs_stats_update_kernel(Slot st, int K, int G, int tpm, const float* __restrict__ obs,
                                                              const uint8_t* __restrict__ active) {
  __shared__ __attribute__((aligned(16))) float xT[PD * PT];
  __shared__ int fl[FLAG_WORDS];
  const int tid = threadIdx.x;
  const Tile t = tile_of(blockIdx.x, G, tpm);
  if (tid < PT) fl[tid] = tid < t.rows && (!active || active[t.row0 + tid] != 0) ? 1 : 0;
  load_tile(K, t.row0, t.rows, obs, nullptr, Norm{nullptr, nullptr, 0.f}, xT, fl);
  __syncthreads();
  stats_tile(slot_at(st, K, blockIdx.x), K, xT, fl);
}

// one workgroup; lane k < K folds the slots' component k into the totals, slot ascending, zeroes them and
// writes the outputs; lane 0 also sums the int64 counts exactly and adds them to count as one float64.
// Every lane needs the new count: it is computed by each lane for itself from the same values (the counts
// are zeroed only after a barrier).
__global__ __launch_bounds__(PB) void obs_stats_finalize_kernel(int K, int n_slots, double* __restrict__ totals,
                                                                double* __restrict__ slot_sum, double* __restrict__ slot_sumsq,
                                                                int64_t* __restrict__ slot_count, float* __restrict__ mean_out,
                                                                float* __restrict__ inv_std_out) {
#pragma clang fp contract(off)
  const int k = threadIdx.x;
  int64_t added = 0;
  for (int s = 0; s < n_slots; s++) added += slot_count[s];
  const double count = totals[0] + (double)added;
  if (k < K) {
    double a = totals[1 + k], q = totals[1 + K + k];
    for (int s = 0; s < n_slots; s++) {
      a += slot_sum[(size_t)s * K + k];
      q += slot_sumsq[(size_t)s * K + k];
      slot_sum[(size_t)s * K + k] = 0.0;
      slot_sumsq[(size_t)s * K + k] = 0.0;
    }
    totals[1 + k] = a;
    totals[1 + K + k] = q;
    const double m = a / count;
    const double mm = m * m;
    double var = q / count - mm;
    var = var > 1e-2 ? var : 1e-2;  // a NaN variance takes the floor too
    if (mean_out) mean_out[k] = (float)m;
    if (inv_std_out) inv_std_out[k] = (float)(1.0 / sqrt(var));
  }
  __syncthreads();  // every lane has read count's inputs
  if (k == 0) totals[0] = count;
  for (int s = k; s < n_slots; s += PB) slot_count[s] = 0;
}

}  // namespace

extern "C" {

int pbg_obs_stats_create(int device, int obs_dim, int n_slots, pbg_obs_stats** out) {
  if (!out) return pbg::capi_fail(PBG_E_ARG, "pbg_obs_stats_create: out is NULL");
  *out = nullptr;
  if (obs_dim < 1 || obs_dim > PBG_POLICY_MAX_DIM || n_slots < 1 || device < 0) {
    char msg[160];
    snprintf(msg, sizeof(msg), "pbg_obs_stats_create: obs_dim %d outside 1..%d, n_slots %d < 1 or device %d < 0", obs_dim,
             PBG_POLICY_MAX_DIM, n_slots, device);
    return pbg::capi_fail(PBG_E_ARG, msg);
  }
  if (const int rc = check_device("pbg_obs_stats_create", device)) return rc;
  pbg_obs_stats* s = new (std::nothrow) pbg_obs_stats();
  if (!s) return pbg::capi_fail(PBG_E_NOMEM, "pbg_obs_stats_create: out of host memory");
  const size_t K = (size_t)obs_dim, nt = 1 + 2 * K, words = nt + (2 * K + 1) * (size_t)n_slots;
  s->device = device;
  s->obs_dim = obs_dim;
  s->n_slots = n_slots;
  s->totals = nullptr;
  DeviceGuard dg(device);
  double* init = (double*)calloc(nt, sizeof(double));  // RunningStat(eps = 1e-2): count, sum = 0, sumsq
  int e = init ? (int)hipMalloc(&s->totals, words * sizeof(double)) : (int)hipErrorOutOfMemory;
  if (!e) {
    init[0] = 1e-2;
    for (size_t k = 0; k < K; k++) init[1 + K + k] = 1e-2;
    e = (int)hipMemset(s->totals, 0, words * sizeof(double));
    if (!e) e = (int)hipMemcpy(s->totals, init, nt * sizeof(double), hipMemcpyHostToDevice);
  }
  free(init);
  if (e) {
    pbg_obs_stats_destroy(s);
    return hip_fail(e, "pbg_obs_stats_create: storage");
  }
  s->slot_sum = s->totals + nt;
  s->slot_sumsq = s->slot_sum + K * (size_t)n_slots;
  s->slot_count = reinterpret_cast<int64_t*>(s->slot_sumsq + K * (size_t)n_slots);
  *out = s;
  return PBG_OK;
}

void pbg_obs_stats_destroy(pbg_obs_stats* s) {
  if (!s) return;
  if (s->totals) {
    DeviceGuard dg(s->device);
    (void)hipFree(s->totals);
  }
  delete s;
}

int pbg_obs_stats_update(pbg_obs_stats* s, int n, int group, const float* obs, const uint8_t* active, void* stream) {
  if (!s) return pbg::capi_fail(PBG_E_ARG, "pbg_obs_stats_update: stats is NULL");
  if (n < 0 || group < 0 || (n > 0 && !obs)) return pbg::capi_fail(PBG_E_ARG, "pbg_obs_stats_update: bad arguments");
  if (n == 0) return PBG_OK;
  const int G = group ? group : n;
  char msg[160];
  if (n % G != 0) {
    snprintf(msg, sizeof(msg), "pbg_obs_stats_update: n = %d is no multiple of group = %d", n, G);
    return pbg::capi_fail(PBG_E_ARG, msg);
  }
  const long long need = tiles_of(n, G);
  if (need > (long long)s->n_slots) {
    snprintf(msg, sizeof(msg), "pbg_obs_stats_update: %d rows in groups of %d need %lld slots, the object has %d", n, G, need,
             s->n_slots);
    return pbg::capi_fail(PBG_E_ARG, msg);
  }
  DeviceGuard dg(s->device);
  hipLaunchKernelGGL(obs_stats_update_kernel, dim3((unsigned)need), dim3(PB), 0, (hipStream_t)stream, s->slot0(), s->obs_dim,
                     G, (G + PT - 1) / PT, obs, active);
  const int e = (int)hipGetLastError();
  return e ? hip_fail(e, "obs_stats_update_kernel launch") : PBG_OK;
}

int pbg_obs_stats_finalize(pbg_obs_stats* s, float* mean_out, float* inv_std_out, void* stream) {
  if (!s) return pbg::capi_fail(PBG_E_ARG, "pbg_obs_stats_finalize: stats is NULL");
  DeviceGuard dg(s->device);
  hipLaunchKernelGGL(obs_stats_finalize_kernel, dim3(1), dim3(PB), 0, (hipStream_t)stream, s->obs_dim, s->n_slots, s->totals,
                     s->slot_sum, s->slot_sumsq, s->slot_count, mean_out, inv_std_out);
  const int e = (int)hipGetLastError();
  return e ? hip_fail(e, "obs_stats_finalize_kernel launch") : PBG_OK;
}

int pbg_obs_stats_get_totals(const pbg_obs_stats* s, double* totals_out, void* stream) {
  if (!s || !totals_out) return pbg::capi_fail(PBG_E_ARG, "pbg_obs_stats_get_totals: NULL stats or totals_out");
  DeviceGuard dg(s->device);
  const int e = (int)hipMemcpyAsync(totals_out, s->totals, (1 + 2 * (size_t)s->obs_dim) * sizeof(double),
                                    hipMemcpyDeviceToDevice, (hipStream_t)stream);
  return e ? hip_fail(e, "pbg_obs_stats_get_totals: copy") : PBG_OK;
}

int pbg_obs_stats_set_totals(pbg_obs_stats* s, const double* totals, void* stream) {
  if (!s || !totals) return pbg::capi_fail(PBG_E_ARG, "pbg_obs_stats_set_totals: NULL stats or totals");
  DeviceGuard dg(s->device);
  const int e = (int)hipMemcpyAsync(s->totals, totals, (1 + 2 * (size_t)s->obs_dim) * sizeof(double),
                                    hipMemcpyDeviceToDevice, (hipStream_t)stream);
  return e ? hip_fail(e, "pbg_obs_stats_set_totals: copy") : PBG_OK;
}

}  // extern "C"
