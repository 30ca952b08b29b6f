// pbg_obsslots.hip -- the slots of a pbg_obs_stats as arrays (include/pbg.h pbg_obs_stats_get_slots,
// pbg_obs_stats_set_slots): what a data-parallel learner moves between ranks so that one object can finalize the
// statistics every rank gathered.  The object, its update and its finalize are pbg_obsnorm.hip's.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include "pbg_policy_dev.h"

namespace {

using namespace pbg::policy;
using pbg::DeviceGuard;

// `count` slots from `first` <-> the caller's counts [count] and sums [count, 2 K] (sum[K] | sumsq[K] per slot): a lane
// per double, the first count lanes the int64 too.  SET: the caller's values overwrite the slots; otherwise the slots
// are copied out and left as they are.
template <bool SET>
__global__ __launch_bounds__(256) void obs_stats_slots_kernel(int K, int first, int count, double* __restrict__ slot_sum,
                                                              double* __restrict__ slot_sumsq, int64_t* __restrict__ slot_count,
                                                              int64_t* __restrict__ counts, double* __restrict__ sums) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)count * 2 * K) return;
  const int sl = (int)(i / (2 * K)), c = (int)(i - (long long)sl * 2 * K);
  double* at = c < K ? slot_sum + (size_t)(first + sl) * K + c : slot_sumsq + (size_t)(first + sl) * K + (c - K);
  if (SET) *at = sums[i];
  else sums[i] = *at;
  if (i < count) {
    if (SET) slot_count[first + i] = counts[i];
    else counts[i] = slot_count[first + i];
  }
}

// what get_slots and set_slots check alike
int check_slots(const char* who, const pbg_obs_stats* s, int first, int count, const void* counts, const void* sums) {
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

template <bool SET>
int launch_slots(pbg_obs_stats* s, int first, int count, int64_t* counts, double* sums, void* stream) {
  if (count == 0) return PBG_OK;
  DeviceGuard dg(s->device);
  const long long n = (long long)count * 2 * s->obs_dim;
  hipLaunchKernelGGL(obs_stats_slots_kernel<SET>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     s->obs_dim, first, count, s->slot_sum, s->slot_sumsq, s->slot_count, counts, sums);
  const int e = (int)hipGetLastError();
  return e ? hip_fail(e, "obs_stats_slots_kernel launch") : PBG_OK;
}

}  // namespace

extern "C" {

int pbg_obs_stats_get_slots(const pbg_obs_stats* s, int first, int count, int64_t* counts_out, double* sums_out, void* stream) {
  if (const int rc = check_slots("pbg_obs_stats_get_slots", s, first, count, counts_out, sums_out)) return rc;
  return launch_slots<false>(const_cast<pbg_obs_stats*>(s), first, count, counts_out, sums_out, stream);
}

int pbg_obs_stats_set_slots(pbg_obs_stats* s, int first, int count, const int64_t* counts, const double* sums, void* stream) {
  if (const int rc = check_slots("pbg_obs_stats_set_slots", s, first, count, counts, sums)) return rc;
  return launch_slots<true>(s, first, count, const_cast<int64_t*>(counts), const_cast<double*>(sums), stream);
}

}  // extern "C"
