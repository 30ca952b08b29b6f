// pbg_population.hip -- policy populations and the evolution-strategy kernels (include/pbg.h
// pbg_population_*, pbg_rollout_population).  A population is P = 2 n_pairs weight sets of one MLP shape
// in device memory, member m's flat parameter vector at members + m D (pbg.h "Flat parameter layout").
//
// The actor is pbg_policy.hip's (pbg_policy_dev.h Actor, launch_actor): the grid over (member, tile of that
// member's G envs), so a tile never straddles two members and the workgroup's weight pointers start at its
// member; a population adds only its pair bookkeeping to the Actor.  The once-per-
// generation kernels (noise, perturb, grad, fitness, member copies) are written for the stated summation
// order, not for speed.
//
// Same-bits rule: es_normals4 (pbg_es_noise.h) is the only place the device computes the noise; noise, perturb and grad
// call it with the same counter and so see the same floats.  Every multiply-add in this file is either a
// spelled-out fma or cannot be contracted (a product that feeds no add).
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stddef.h>
#include <stdio.h>
#include <string.h>

#include <new>

#include "pbg_math.h"
#include "pbg_es_noise.h"
#include "pbg_policy_dev.h"

namespace {

using namespace pbg::policy;
using namespace pbg::es;  // es_box_muller, es_normals4, ES_TAG (pbg_es_noise.h)
using pbg::DeviceGuard;

// grid (n_pairs, ceil(nb / 256)): a lane per (pair, block of 4 parameters)
__global__ __launch_bounds__(256) void noise_kernel(int D, uint32_t k0, uint32_t k1, uint32_t pair0, uint32_t generation,
                                                    float* __restrict__ eps) {
  const int i = blockIdx.x;
  const int b = blockIdx.y * 256 + threadIdx.x;
  if (4 * b >= D) return;
  float e[4];
  es_normals4(k0, k1, (uint32_t)b, pair0 + (uint32_t)i, generation, ES_TAG, e);
  float* out = eps + (size_t)i * D;
#pragma unroll
  for (int t = 0; t < 4; t++)
    if (4 * b + t < D) out[4 * b + t] = e[t];
}

// members 2 i and 2 i + 1 = theta +- sigma eps_i, in float64 (the product of two floats is exact there),
// rounded once
__global__ __launch_bounds__(256) void perturb_kernel(int D, const float* __restrict__ theta, float sigma, uint32_t k0,
                                                      uint32_t k1, uint32_t pair0, uint32_t generation,
                                                      float* __restrict__ members) {
  const int i = blockIdx.x;
  const int b = blockIdx.y * 256 + threadIdx.x;
  if (4 * b >= D) return;
  float e[4];
  es_normals4(k0, k1, (uint32_t)b, pair0 + (uint32_t)i, generation, ES_TAG, e);
  float* plus = members + (size_t)(2 * i) * D;
  float* minus = plus + D;
  const double s = (double)sigma;
#pragma unroll
  for (int t = 0; t < 4; t++) {
    const int d = 4 * b + t;
    if (d < D) {
      const double th = (double)theta[d];
      plus[d] = (float)__builtin_fma(s, (double)e[t], th);
      minus[d] = (float)__builtin_fma(-s, (double)e[t], th);
    }
  }
}

// g[d] = sum over the pairs, ascending, of w[i] eps_i[d] in float64 (exact products, one rounding per
// add); a lane per block of 4 parameters regenerates the noise pair by pair
__global__ __launch_bounds__(256) void grad_kernel(int D, int n_pairs, const float* __restrict__ w, uint32_t k0, uint32_t k1,
                                                   uint32_t pair0, uint32_t generation, float* __restrict__ g) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (4 * b >= D) return;
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  for (int i = 0; i < n_pairs; i++) {
    float e[4];
    es_normals4(k0, k1, (uint32_t)b, pair0 + (uint32_t)i, generation, ES_TAG, e);
    const double wi = (double)w[i];
#pragma unroll
    for (int t = 0; t < 4; t++) acc[t] = __builtin_fma(wi, (double)e[t], acc[t]);
  }
#pragma unroll
  for (int t = 0; t < 4; t++)
    if (4 * b + t < D) g[4 * b + t] = (float)acc[t];
}

// fitness[m] = (sum over member m's G envs, ascending, of done_return + cur_return) / G; a lane per member
__global__ __launch_bounds__(256) void fitness_kernel(int P, int G, const double* __restrict__ cur_return,
                                                      const double* __restrict__ done_return, double* __restrict__ fitness) {
  const int m = blockIdx.x * 256 + threadIdx.x;
  if (m >= P) return;
  double s = 0.0;
  for (int k = 0; k < G; k++) {
    const size_t e = (size_t)m * G + k;
    s += done_return[e] + cur_return[e];
  }
  fitness[m] = s / (double)G;
}

// dst[r, :] = src[r * src_stride + :] for r < rows (src_stride 0: every row takes the same vector)
__global__ __launch_bounds__(256) void copy_rows_kernel(int D, size_t src_stride, const float* __restrict__ src,
                                                        float* __restrict__ dst) {
  const int d = blockIdx.y * 256 + threadIdx.x;
  if (d < D) dst[(size_t)blockIdx.x * D + d] = src[(size_t)blockIdx.x * src_stride + d];
}

// ---------------------------------------------------------------- host side
// the largest population whose member count and whose global pair indices stay inside an int
bool pairs_ok(int n_pairs, int pair0) { return n_pairs >= 1 && n_pairs <= INT_MAX / 2 && pair0 >= 0 && pair0 <= INT_MAX - n_pairs; }

dim3 pair_grid(const pbg_population* p) { return dim3((unsigned)p->n_pairs, (unsigned)(((p->a.D + 3) / 4 + 255) / 256)); }

}  // namespace

extern "C" {

int pbg_population_create(int device, int obs_dim, int h1, int h2, int act_dim, int n_pairs, int pair0,
                          pbg_population** out) {
  if (!out) return pbg::capi_fail(PBG_E_ARG, "pbg_population_create: out is NULL");
  *out = nullptr;
  if (const int rc = check_dims("pbg_population_create", obs_dim, h1, h2, act_dim)) return rc;
  if (!pairs_ok(n_pairs, pair0)) {
    char msg[160];
    snprintf(msg, sizeof(msg), "pbg_population_create: n_pairs %d must be >= 1 and pair0 %d >= 0 (and their sum an int)",
             n_pairs, pair0);
    return pbg::capi_fail(PBG_E_ARG, msg);
  }
  if (device < 0) return pbg::capi_fail(PBG_E_ARG, "pbg_population_create: device must be >= 0 (the members live on a GPU)");
  pbg_population* p = new (std::nothrow) pbg_population();
  if (!p) return pbg::capi_fail(PBG_E_NOMEM, "pbg_population_create: out of host memory");
  p->n_pairs = n_pairs;
  p->pair0 = pair0;
  if (const int rc = actor_init("pbg_population_create", p->a, device, obs_dim, h1, h2, act_dim, 2 * n_pairs)) {
    delete p;
    return rc;
  }
  *out = p;
  return PBG_OK;
}

void pbg_population_destroy(pbg_population* p) {
  if (!p) return;
  actor_free(p->a);
  delete p;
}

int pbg_population_set_obs_norm(pbg_population* p, const float* mean, const float* inv_std, float clip, void* stream) {
  if (!p) return pbg::capi_fail(PBG_E_ARG, "pbg_population_set_obs_norm: population is NULL");
  const int r = norm_args("pbg_population_set_obs_norm", p->a, mean, inv_std, clip);
  if (r) return r > 0 ? PBG_OK : r;
  DeviceGuard dg(p->a.device);
  const size_t bytes = (size_t)p->a.obs_dim * sizeof(float);
  int e = (int)hipMemcpyAsync(p->a.norm, mean, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream);
  if (!e) e = (int)hipMemcpyAsync(p->a.norm + p->a.obs_dim, inv_std, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream);
  if (e) return hip_fail(e, "pbg_population_set_obs_norm: copy");
  p->a.clip = clip;
  p->a.norm_on = 1;
  return PBG_OK;
}

int pbg_population_attach_obs_stats(pbg_population* p, pbg_obs_stats* s) {
  if (!p) return pbg::capi_fail(PBG_E_ARG, "pbg_population_attach_obs_stats: population is NULL");
  p->a.stats = s;
  return PBG_OK;
}

int pbg_population_attach_action_noise(pbg_population* p, pbg_action_noise* z) {
  if (!p) return pbg::capi_fail(PBG_E_ARG, "pbg_population_attach_action_noise: population is NULL");
  p->a.noise = z;
  return PBG_OK;
}

int pbg_population_noise_host(int obs_dim, int h1, int h2, int act_dim, uint64_t seed, uint32_t generation, int pair0,
                              int n_pairs, float* eps_out) {
  if (const int rc = check_dims("pbg_population_noise_host", obs_dim, h1, h2, act_dim)) return rc;
  if (!pairs_ok(n_pairs, pair0) || !eps_out)
    return pbg::capi_fail(PBG_E_ARG, "pbg_population_noise_host: n_pairs must be >= 1, pair0 >= 0 and eps_out not NULL");
  const int D = param_count(obs_dim, h1, h2, act_dim);
  const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
  for (int i = 0; i < n_pairs; i++) {
    float* row = eps_out + (size_t)i * D;
    for (int b = 0; 4 * b < D; b++) {
      float e[4];
      host_normals4(k0, k1, (uint32_t)b, (uint32_t)pair0 + (uint32_t)i, generation, ES_TAG, e);
      for (int t = 0; t < 4 && 4 * b + t < D; t++) row[4 * b + t] = e[t];
    }
  }
  return PBG_OK;
}

int pbg_population_noise(const pbg_population* p, uint64_t seed, uint32_t generation, float* eps_out, void* stream) {
  if (!p || !eps_out) return pbg::capi_fail(PBG_E_ARG, "pbg_population_noise: NULL population or eps_out");
  DeviceGuard dg(p->a.device);
  hipLaunchKernelGGL(noise_kernel, pair_grid(p), dim3(256), 0, (hipStream_t)stream, p->a.D, (uint32_t)seed,
                     (uint32_t)(seed >> 32), (uint32_t)p->pair0, generation, eps_out);
  return launched("noise_kernel launch");
}

int pbg_population_perturb(pbg_population* p, const float* theta, float sigma, uint64_t seed, uint32_t generation,
                           void* stream) {
  if (!p || !theta) return pbg::capi_fail(PBG_E_ARG, "pbg_population_perturb: NULL population or theta");
  DeviceGuard dg(p->a.device);
  hipLaunchKernelGGL(perturb_kernel, pair_grid(p), dim3(256), 0, (hipStream_t)stream, p->a.D, theta, sigma, (uint32_t)seed,
                     (uint32_t)(seed >> 32), (uint32_t)p->pair0, generation, p->a.params);
  return launched("perturb_kernel launch");
}

int pbg_population_set_member(pbg_population* p, int m, const float* theta, void* stream) {
  if (!p || !theta) return pbg::capi_fail(PBG_E_ARG, "pbg_population_set_member: NULL population or theta");
  const int P = p->a.n_members;
  if (m < -1 || m >= P) {
    char msg[96];
    snprintf(msg, sizeof(msg), "pbg_population_set_member: member %d outside 0..%d (or -1 for every member)", m, P - 1);
    return pbg::capi_fail(PBG_E_ARG, msg);
  }
  DeviceGuard dg(p->a.device);
  const unsigned rows = m < 0 ? (unsigned)P : 1u;
  float* dst = p->a.params + (m < 0 ? (size_t)0 : (size_t)m * p->a.D);
  hipLaunchKernelGGL(copy_rows_kernel, dim3(rows, (unsigned)((p->a.D + 255) / 256)), dim3(256), 0, (hipStream_t)stream, p->a.D,
                     (size_t)0, theta, dst);
  return launched("set_member launch");
}

int pbg_population_get_member(const pbg_population* p, int m, float* theta_out, void* stream) {
  if (!p || !theta_out) return pbg::capi_fail(PBG_E_ARG, "pbg_population_get_member: NULL population or theta_out");
  const int P = p->a.n_members;
  if (m < 0 || m >= P) {
    char msg[96];
    snprintf(msg, sizeof(msg), "pbg_population_get_member: member %d outside 0..%d", m, P - 1);
    return pbg::capi_fail(PBG_E_ARG, msg);
  }
  DeviceGuard dg(p->a.device);
  hipLaunchKernelGGL(copy_rows_kernel, dim3(1u, (unsigned)((p->a.D + 255) / 256)), dim3(256), 0, (hipStream_t)stream, p->a.D,
                     (size_t)0, p->a.params + (size_t)m * p->a.D, theta_out);
  return launched("get_member launch");
}

int pbg_population_act(const pbg_population* p, int n, const float* obs, float* act, void* stream) {
  if (!p) return pbg::capi_fail(PBG_E_ARG, "pbg_population_act: population is NULL");
  const int P = p->a.n_members;
  if (n < 0 || n % P != 0 || (n > 0 && (!obs || !act))) {
    char msg[128];
    snprintf(msg, sizeof(msg), "pbg_population_act: n = %d must be a multiple of the %d members, obs and act not NULL", n, P);
    return pbg::capi_fail(PBG_E_ARG, msg);
  }
  if (n == 0) return PBG_OK;
  DeviceGuard dg(p->a.device);
  Book none;
  memset(&none, 0, sizeof(none));
  const int e = launch_actor(p->a, n, obs, act, nullptr, nullptr, none, false, Noise{}, (hipStream_t)stream);
  return e ? hip_fail(e, "actor_kernel launch") : PBG_OK;
}

int pbg_rollout_population(pbg_handle* h, const pbg_population* p, const pbg_rollout_io_t* io, void* stream) {
  if (!h || !p || !io) return pbg::capi_fail(PBG_E_ARG, "pbg_rollout_population: NULL handle, population or io");
  return rollout_loop("pbg_rollout_population", h, io, stream, p->a);
}

int pbg_population_fitness(const pbg_population* p, int n, const double* cur_return, const double* done_return,
                           double* fitness_out, void* stream) {
  if (!p || !cur_return || !done_return || !fitness_out)
    return pbg::capi_fail(PBG_E_ARG, "pbg_population_fitness: NULL population or buffer");
  const int P = p->a.n_members;
  if (n < P || n % P != 0) {
    char msg[128];
    snprintf(msg, sizeof(msg), "pbg_population_fitness: n = %d must be a positive multiple of the %d members", n, P);
    return pbg::capi_fail(PBG_E_ARG, msg);
  }
  DeviceGuard dg(p->a.device);
  hipLaunchKernelGGL(fitness_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, (hipStream_t)stream, P, n / P, cur_return,
                     done_return, fitness_out);
  return launched("fitness_kernel launch");
}

int pbg_population_grad(const pbg_population* p, const float* w, uint64_t seed, uint32_t generation, float* g_out,
                        void* stream) {
  if (!p || !w || !g_out) return pbg::capi_fail(PBG_E_ARG, "pbg_population_grad: NULL population, w or g_out");
  DeviceGuard dg(p->a.device);
  const int nb = (p->a.D + 3) / 4;
  hipLaunchKernelGGL(grad_kernel, dim3((unsigned)((nb + 255) / 256)), dim3(256), 0, (hipStream_t)stream, p->a.D, p->n_pairs, w,
                     (uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)p->pair0, generation, g_out);
  return launched("grad_kernel launch");
}

}  // extern "C"
