// pbg_trunc.hip -- bootstrapping through TimeLimit truncations (include/pbg.h "Truncation bootstrapping", DESIGN.md
// section 19): the masked actor launch that values the flagged rows of a trajectory alone (pbg_population_act_where)
// and the advantage scan that uses those values (pbg_gae_trunc, pbg_gae_trunc_host).  The rollout's side, the two
// trajectories of pbg_rollout_io_t version 2, is pbg_policy.hip's rollout_loop.
//
// Nothing of the numeric contracts is restated here: the masked tile runs pbg_policy_dev.h's `layer` (the actor's
// k-ascending fmaf chain) and `normalise`, the scan is that header's gae_env with its truncation lines switched on.
// A row's chain takes nothing from the tile's other rows, so a row that sits between zero-filled ones has the bits
// it has in pbg_population_act's dense tile.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stddef.h>
#include <stdio.h>

#include "pbg_policy_dev.h"

namespace {

using namespace pbg::policy;
using pbg::DeviceGuard;

static_assert(PT <= WAVE, "a lane of every wave per flag byte of the tile");

// out[T, n, act_dim] under flags[T, n]: grid = T * tpt workgroups, tpt = n_members * tpm the tiles of one time step
// (tile_of: they never straddle a member).  Workgroup ts * tpt + b owns tile b of time step ts, the rows
// ts n + row0 .. + rows of the flat [T n] batch.  MODE: PLAIN or NORM (pbg_policy_dev.h; nothing is collected here).
template <int MODE>
__global__ __launch_bounds__(PB) void actor_where_kernel(const float* __restrict__ params, int obs_dim, int h1, int h2,
                                                         int act_dim, int D, int G, int tpm, int tpt, int n, Norm nm,
                                                         const uint8_t* __restrict__ flags, const float* __restrict__ obs,
                                                         float* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) float bufA[PD * PT];
  __shared__ __attribute__((aligned(16))) float bufB[PD * PT];
  const int tid = threadIdx.x;
  const unsigned ts = blockIdx.x / (unsigned)tpt;
  const Tile t = tile_of(blockIdx.x - ts * (unsigned)tpt, G, tpm);
  const size_t row0 = (size_t)ts * n + t.row0;
  // Every wave reads the tile's flag bytes and votes: the four masks come from the same bytes, so the branch below
  // is uniform over the workgroup and no barrier sits under divergent control flow.  Bit e: row e is flagged.
  const int lane = tid & (WAVE - 1);
  const unsigned mask = (unsigned)__ballot(lane < t.rows && flags[row0 + lane] != 0);
  const int NA = act_dim;
  float* orow = out + row0 * NA;
  if (mask == 0u) {  // the common case: nothing to value, the weights are never touched
    for (int i = tid; i < t.rows * NA; i += PB) orow[i] = 0.f;
    return;
  }
  // load_tile with a row mask: an unflagged row is zero-filled in LDS like a row past `rows`, and not read
  const int K0 = obs_dim;
  const float* xrow = obs + row0 * K0;
  for (int i = tid; i < PT * K0; i += PB) {
    const int e = i / K0, k = i - e * K0;
    float v = 0.f;
    if ((mask >> e) & 1u) {
      v = xrow[i];
      if (MODE == NORM) v = normalise(v, nm.mean[k], nm.inv_std[k], nm.clip);
    }
    bufA[k * PT + e] = v;
  }
  const Weights P = weights_at(params + (size_t)t.m * D, obs_dim, h1, h2, act_dim);
  __syncthreads();
  layer(P.w1, P.b1, K0, P.h1, true, bufA, bufB);
  __syncthreads();
  layer(P.w2, P.b2, P.h1, P.h2, true, bufB, bufA);
  __syncthreads();
  layer(P.w3, P.b3, P.h2, NA, false, bufA, bufB);
  __syncthreads();
  for (int i = tid; i < t.rows * NA; i += PB) {
    const int e = i / NA, j = i - e * NA;
    orow[i] = (mask >> e) & 1u ? bufB[j * PT + e] : 0.f;
  }
}

// a lane per env, pbg_actnoise.hip's gae_kernel with the truncation lines
__global__ __launch_bounds__(256) void gae_trunc_kernel(int T, int n, const float* __restrict__ rew,
                                                        const uint8_t* __restrict__ done, const uint8_t* __restrict__ trunc,
                                                        const float* __restrict__ value, const float* __restrict__ term_value,
                                                        double gamma, double gl, float* __restrict__ adv,
                                                        float* __restrict__ ret) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e < n) gae_env<true>(T, n, e, rew, done, trunc, value, term_value, gamma, gl, adv, ret);
}

bool gae_trunc_args_ok(int T, int n, const void* rew, const void* done, const void* trunc, const void* value,
                       const void* term_value, const void* adv, const void* ret) {
  return T >= 1 && n >= 1 && rew && done && trunc && value && term_value && adv && ret;
}

}  // namespace

extern "C" {

int pbg_population_act_where(const pbg_population* p, int T, int n, const uint8_t* flags, const float* obs, float* out,
                             void* stream) {
  if (!p || !flags || !obs || !out) return pbg::capi_fail(PBG_E_ARG, "pbg_population_act_where: NULL population, flags, obs or out");
  const Actor& a = p->a;
  char msg[200];
  if (a.device < 0) return pbg::capi_fail(PBG_E_ARG, "pbg_population_act_where: host-only population");
  if (T < 1 || n < 1 || n % a.n_members != 0) {
    snprintf(msg, sizeof(msg), "pbg_population_act_where: T = %d must be >= 1 and n = %d a positive multiple of the %d members", T,
             n, a.n_members);
    return pbg::capi_fail(PBG_E_ARG, msg);
  }
  const int G = n / a.n_members;
  const long long tpt = tiles_of(n, G), grid = (long long)T * tpt;
  if (grid > (long long)INT_MAX) {
    snprintf(msg, sizeof(msg), "pbg_population_act_where: %d steps of %lld tiles are more workgroups than a launch takes", T, tpt);
    return pbg::capi_fail(PBG_E_ARG, msg);
  }
  DeviceGuard dg(a.device);
  const Norm nm = a.norm_on ? Norm{a.norm, a.norm + a.obs_dim, a.clip} : Norm{nullptr, nullptr, 0.f};
  hipLaunchKernelGGL(nm.mean ? actor_where_kernel<NORM> : actor_where_kernel<PLAIN>, dim3((unsigned)grid), dim3(PB), 0,
                     (hipStream_t)stream, a.params, a.obs_dim, a.h1, a.h2, a.act_dim, a.D, G, (G + PT - 1) / PT, (int)tpt, n, nm, flags,
                     obs, out);
  return launched("actor_where_kernel launch");
}

int pbg_gae_trunc(int T, int n, const float* rew_traj, const uint8_t* done_traj, const uint8_t* trunc_traj, const float* value,
                  const float* term_value, double gamma, double lambda, float* adv_out, float* ret_out, void* stream) {
  if (!gae_trunc_args_ok(T, n, rew_traj, done_traj, trunc_traj, value, term_value, adv_out, ret_out))
    return pbg::capi_fail(PBG_E_ARG, "pbg_gae_trunc: T and n must be >= 1 and no array NULL");
  const double gl = gamma * lambda;
  hipLaunchKernelGGL(gae_trunc_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, T, n, rew_traj,
                     done_traj, trunc_traj, value, term_value, gamma, gl, adv_out, ret_out);
  return launched("gae_trunc_kernel launch");
}

int pbg_gae_trunc_host(int T, int n, const float* rew_traj, const uint8_t* done_traj, const uint8_t* trunc_traj,
                       const float* value, const float* term_value, double gamma, double lambda, float* adv_out,
                       float* ret_out) {
  if (!gae_trunc_args_ok(T, n, rew_traj, done_traj, trunc_traj, value, term_value, adv_out, ret_out))
    return pbg::capi_fail(PBG_E_ARG, "pbg_gae_trunc_host: T and n must be >= 1 and no array NULL");
  const double gl = gamma * lambda;
  for (int e = 0; e < n; e++)
    gae_env<true>(T, n, e, rew_traj, done_traj, trunc_traj, value, term_value, gamma, gl, adv_out, ret_out);
  return PBG_OK;
}

}  // extern "C"
