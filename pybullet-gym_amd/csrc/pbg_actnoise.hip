// pbg_actnoise.hip -- what a policy-gradient learner needs from the device side of the loop (include/pbg.h
// "Stochastic Gaussian actions and advantage estimation"): the pbg_action_noise object, the stand-alone fill
// kernel and its host counterpart, and generalised advantage estimation (pbg_gae, pbg_gae_host).
//
// The sampling itself happens inside the actor launch (pbg_policy_dev.h act_tile<MODE, true>); this unit's
// fill kernel calls the same device function (action_normals4) with the same counter, so a test or a learner
// that regenerates the noise of a rollout step sees the bits the actor added.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stddef.h>
#include <stdio.h>

#include <new>

#include "pbg_policy_dev.h"

namespace {

using namespace pbg::policy;
using pbg::DeviceGuard;

// a lane per (env, block of 4 components): eps [n, act_dim]
__global__ __launch_bounds__(256) void action_noise_fill_kernel(int n, int act_dim, uint32_t k0, uint32_t k1, uint32_t env_offset,
                                                                uint32_t step, float* __restrict__ eps) {
  const int nb = (act_dim + 3) / 4;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)n * nb) return;
  const int e = (int)(i / nb), b = (int)(i - (long long)e * nb);
  float z[4];
  action_normals4(k0, k1, (uint32_t)b, env_offset + (uint32_t)e, step, z);
  float* out = eps + (size_t)e * act_dim;
#pragma unroll
  for (int t = 0; t < 4; t++)
    if (4 * b + t < act_dim) out[4 * b + t] = z[t];
}

// a lane per env: every row access is coalesced over the envs; the scan is pbg_policy_dev.h's gae_env, without
// the truncation lines (pbg_trunc.hip's kernel runs it with them)
__global__ __launch_bounds__(256) void gae_kernel(int T, int n, const float* __restrict__ rew, const uint8_t* __restrict__ done,
                                                  const float* __restrict__ value, double gamma, double gl,
                                                  float* __restrict__ adv, float* __restrict__ ret) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e < n) gae_env<false>(T, n, e, rew, done, nullptr, value, nullptr, gamma, gl, adv, ret);
}

bool gae_args_ok(int T, int n, const void* rew, const void* done, const void* value, const void* adv, const void* ret) {
  return T >= 1 && n >= 1 && rew && done && value && adv && ret;
}

}  // namespace

extern "C" {

int pbg_action_noise_create(int device, int act_dim, uint64_t seed, pbg_action_noise** out) {
  if (!out) return pbg::capi_fail(PBG_E_ARG, "pbg_action_noise_create: out is NULL");
  *out = nullptr;
  if (act_dim < 1 || act_dim > PBG_POLICY_MAX_ACT || device < 0) {
    char msg[128];
    snprintf(msg, sizeof(msg), "pbg_action_noise_create: act_dim %d outside 1..%d or device %d < 0", act_dim, PBG_POLICY_MAX_ACT,
             device);
    return pbg::capi_fail(PBG_E_ARG, msg);
  }
  if (const int rc = check_device("pbg_action_noise_create", device)) return rc;
  pbg_action_noise* z = new (std::nothrow) pbg_action_noise();
  if (!z) return pbg::capi_fail(PBG_E_NOMEM, "pbg_action_noise_create: out of host memory");
  z->device = device;
  z->act_dim = act_dim;
  z->seed = seed;
  z->std = nullptr;
  z->eps2_traj = nullptr;
  DeviceGuard dg(device);
  const size_t bytes = ((size_t)act_dim + 1) * sizeof(float);  // std [act_dim], then the counter
  int e = (int)hipMalloc(&z->std, bytes);
  if (!e) e = (int)hipMemset(z->std, 0, bytes);
  if (e) {
    pbg_action_noise_destroy(z);
    return hip_fail(e, "pbg_action_noise_create: storage");
  }
  z->counter = reinterpret_cast<uint32_t*>(z->std + act_dim);
  *out = z;
  return PBG_OK;
}

void pbg_action_noise_destroy(pbg_action_noise* z) {
  if (!z) return;
  if (z->std) {
    DeviceGuard dg(z->device);
    (void)hipFree(z->std);
  }
  delete z;
}

int pbg_action_noise_set_std(pbg_action_noise* z, const float* std, void* stream) {
  if (!z || !std) return pbg::capi_fail(PBG_E_ARG, "pbg_action_noise_set_std: NULL noise or std");
  DeviceGuard dg(z->device);
  const int e = (int)hipMemcpyAsync(z->std, std, (size_t)z->act_dim * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream);
  return e ? hip_fail(e, "pbg_action_noise_set_std: copy") : PBG_OK;
}

int pbg_action_noise_set_counter(pbg_action_noise* z, uint32_t counter, void* stream) {
  if (!z) return pbg::capi_fail(PBG_E_ARG, "pbg_action_noise_set_counter: noise is NULL");
  DeviceGuard dg(z->device);
  const int e = (int)hipMemsetD32Async((hipDeviceptr_t)z->counter, (int)counter, 1, (hipStream_t)stream);
  return e ? hip_fail(e, "pbg_action_noise_set_counter: memset") : PBG_OK;
}

int pbg_action_noise_get_counter(const pbg_action_noise* z, uint32_t* counter_out, void* stream) {
  if (!z || !counter_out) return pbg::capi_fail(PBG_E_ARG, "pbg_action_noise_get_counter: NULL noise or counter_out");
  DeviceGuard dg(z->device);
  const int e = (int)hipMemcpyAsync(counter_out, z->counter, sizeof(uint32_t), hipMemcpyDeviceToDevice, (hipStream_t)stream);
  return e ? hip_fail(e, "pbg_action_noise_get_counter: copy") : PBG_OK;
}

int pbg_action_noise_set_eps2_traj(pbg_action_noise* z, double* eps2_traj) {
  if (!z) return pbg::capi_fail(PBG_E_ARG, "pbg_action_noise_set_eps2_traj: noise is NULL");
  z->eps2_traj = eps2_traj;
  return PBG_OK;
}

int pbg_action_noise_fill(const pbg_action_noise* z, int n, int env_offset, uint32_t step, float* eps_out, void* stream) {
  if (!z || n < 0 || env_offset < 0 || env_offset > INT_MAX - n || (n > 0 && !eps_out))
    return pbg::capi_fail(PBG_E_ARG, "pbg_action_noise_fill: NULL noise or eps_out, n < 0 or env_offset < 0");
  if (n == 0) return PBG_OK;
  DeviceGuard dg(z->device);
  const long long lanes = (long long)n * ((z->act_dim + 3) / 4);
  hipLaunchKernelGGL(action_noise_fill_kernel, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, (hipStream_t)stream, n,
                     z->act_dim, (uint32_t)z->seed, (uint32_t)(z->seed >> 32), (uint32_t)env_offset, step, eps_out);
  return launched("action_noise_fill_kernel launch");
}

int pbg_action_noise_host(int act_dim, uint64_t seed, int n, int env_offset, uint32_t step, float* eps_out) {
  if (act_dim < 1 || act_dim > PBG_POLICY_MAX_ACT || n < 0 || env_offset < 0 || env_offset > INT_MAX - n || (n > 0 && !eps_out))
    return pbg::capi_fail(PBG_E_ARG, "pbg_action_noise_host: act_dim outside 1..64, n < 0, env_offset < 0 or eps_out NULL");
  const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
  for (int e = 0; e < n; e++) {
    float* row = eps_out + (size_t)e * act_dim;
    for (int b = 0; 4 * b < act_dim; b++) {
      float z[4];
      pbg::es::host_normals4(k0, k1, (uint32_t)b, (uint32_t)env_offset + (uint32_t)e, step, pbg::es::ACTION_TAG, z);
      for (int t = 0; t < 4 && 4 * b + t < act_dim; t++) row[4 * b + t] = z[t];
    }
  }
  return PBG_OK;
}

int pbg_gae(int T, int n, const float* rew_traj, const uint8_t* done_traj, const float* value, double gamma, double lambda,
            float* adv_out, float* ret_out, void* stream) {
  if (!gae_args_ok(T, n, rew_traj, done_traj, value, adv_out, ret_out))
    return pbg::capi_fail(PBG_E_ARG, "pbg_gae: T and n must be >= 1 and no array NULL");
  const double gl = gamma * lambda;
  hipLaunchKernelGGL(gae_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, T, n, rew_traj, done_traj,
                     value, gamma, gl, adv_out, ret_out);
  return launched("gae_kernel launch");
}

int pbg_gae_host(int T, int n, const float* rew_traj, const uint8_t* done_traj, const float* value, double gamma, double lambda,
                 float* adv_out, float* ret_out) {
  if (!gae_args_ok(T, n, rew_traj, done_traj, value, adv_out, ret_out))
    return pbg::capi_fail(PBG_E_ARG, "pbg_gae_host: T and n must be >= 1 and no array NULL");
  const double gl = gamma * lambda;
  for (int e = 0; e < n; e++) gae_env<false>(T, n, e, rew_traj, done_traj, nullptr, value, nullptr, gamma, gl, adv_out, ret_out);
  return PBG_OK;
}

}  // extern "C"
