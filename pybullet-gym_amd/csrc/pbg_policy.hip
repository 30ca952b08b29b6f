// pbg_policy.hip -- the pretrained-policy MLP (include/pbg.h pbg_policy_*), the actor kernel and its launch,
// and the closed-loop rollout (pbg_rollout).  The reference's enjoy scripts evaluate SmallReactivePolicy.act
// (examples/roboschool-weights/enjoy_TF_*.py:25-31) once per env per step on the host; here one
// launch evaluates all three layers for every env, the hidden activations never leave LDS.
//
// One kernel serves every actor (pbg_policy_dev.h Actor): a pbg_policy is the population of one member whose
// group is the whole batch, pbg_population.hip launches the same kernel with its 2 n_pairs members.  The MLP
// tile, its numeric contract and geometry, the bookkeeping and the declarations are in pbg_policy_dev.h.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <new>

#include "pbg_policy_dev.h"

using namespace pbg::policy;
using pbg::DeviceGuard;

namespace {

// the call's closing launch; BUMP: lane 0 also adds the call's T steps to the attached noise's step counter
template <bool BUMP>
__global__ __launch_bounds__(256) void book_kernel(Book b, int n, uint32_t* counter, uint32_t steps) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e < n) book_env(b, e);
  if (BUMP && e == 0) *counter += steps;
}

// act[n, act_dim] = pi_m(obs[n, obs_dim]), n = n_members G rows: grid = n_members * tpm workgroups, workgroup
// (m, t) (tile_of) runs its rows through member m's weights, params + m D in the flat layout (a shared-weight
// policy: one member, G = n, tpm = the grid).  Optional copies of observation and action into the rollout's
// trajectories; the bookkeeping of the previous env step (bk.rew64 != NULL) for the tile's envs comes first.
// nm: the actor's normaliser (mean NULL: none); st: slot 0 of the statistics to collect into (sum NULL:
// none), workgroup b adds to slot b; MODE (pbg_policy_dev.h) says which of the two the instantiation looks at.
// nz: the launch's action noise, which only a SAMPLE instantiation looks at (the last argument, so that the
// others read theirs where they did before it existed).
template <int MODE, bool SAMPLE>
__global__ __launch_bounds__(PB) void actor_kernel(const float* __restrict__ params, int obs_dim, int h1, int h2, int act_dim,
                                                   int D, int G, int tpm, Norm nm, Slot st, const float* __restrict__ obs,
                                                   float* __restrict__ act, float* __restrict__ obs_traj,
                                                   float* __restrict__ act_traj, Book bk, Noise nz) {
  __shared__ __attribute__((aligned(16))) float bufA[PD * PT];
  __shared__ __attribute__((aligned(16))) float bufB[PD * PT];
  const Tile t = tile_of(blockIdx.x, G, tpm);
  act_tile<MODE, SAMPLE>(weights_at(params + (size_t)t.m * D, obs_dim, h1, h2, act_dim), nm, slot_at(st, obs_dim, blockIdx.x), nz,
                         t.row0, t.rows, obs, act, obs_traj, act_traj, bk, bufA, bufB);
}

// the actor's normaliser with its arrays at `base` (the device's, or a policy's host copy)
Norm norm_of(const Actor& a, const float* base) {
  if (!a.norm_on) return Norm{nullptr, nullptr, 0.f};
  return Norm{base, base + a.obs_dim, a.clip};
}

}  // namespace

// an Actor with one member, plus the host's copies: pbg_policy_act_host and host-only policies run on them
struct pbg_policy {
  Actor a;
  float* host;       // [D], the flat layout
  float* norm_host;  // mean [obs_dim] then inv_std [obs_dim]
};

int pbg::policy::launch_actor(const Actor& a, int n, const float* obs, float* act, float* obs_traj, float* act_traj,
                              const Book& bk, bool collect, const Noise& nz, hipStream_t stream) {
  const int G = n / a.n_members;  // the callers have checked n % n_members == 0 and n > 0
  const Norm nm = norm_of(a, a.norm);
  const Slot st = collect && a.stats ? a.stats->slot0() : Slot{nullptr, nullptr, nullptr};
  decltype(&actor_kernel<PLAIN, false>) kernel = nullptr;
  switch (2 * mode_of(nm, st) + (nz.std ? 1 : 0)) {
    case 2 * PLAIN: kernel = actor_kernel<PLAIN, false>; break;
    case 2 * NORM: kernel = actor_kernel<NORM, false>; break;
    case 2 * COLLECT: kernel = actor_kernel<COLLECT, false>; break;
    case 2 * PLAIN + 1: kernel = actor_kernel<PLAIN, true>; break;
    case 2 * NORM + 1: kernel = actor_kernel<NORM, true>; break;
    case 2 * COLLECT + 1: kernel = actor_kernel<COLLECT, true>; break;
  }
  hipLaunchKernelGGL(kernel, dim3((unsigned)tiles_of(n, G)), dim3(PB), 0, stream, a.params, a.obs_dim, a.h1, a.h2, a.act_dim, a.D,
                     G, (G + PT - 1) / PT, nm, st, obs, act, obs_traj, act_traj, bk, nz);
  return (int)hipGetLastError();
}

int pbg::policy::actor_init(const char* who, Actor& a, int device, int obs_dim, int h1, int h2, int act_dim, int n_members) {
  a = Actor{device, obs_dim, h1, h2, act_dim, n_members, param_count(obs_dim, h1, h2, act_dim), nullptr, nullptr, 0.f, 0, nullptr,
            nullptr};
  if (device < 0) return PBG_OK;
  if (const int rc = check_device(who, device)) return rc;
  DeviceGuard dg(device);
  const size_t bytes = (size_t)n_members * a.D * sizeof(float), norm_bytes = (size_t)2 * obs_dim * sizeof(float);
  int e = (int)hipMalloc(&a.params, bytes);
  if (!e) e = (int)hipMemset(a.params, 0, bytes);
  if (!e) e = (int)hipMalloc(&a.norm, norm_bytes);
  if (!e) e = (int)hipMemset(a.norm, 0, norm_bytes);
  if (!e) return PBG_OK;
  actor_free(a);
  char what[96];
  snprintf(what, sizeof(what), "%s: actor storage", who);
  return hip_fail(e, what);
}

void pbg::policy::actor_free(Actor& a) {
  if (!a.params && !a.norm) return;
  DeviceGuard dg(a.device);
  (void)hipFree(a.params);
  (void)hipFree(a.norm);
  a.params = a.norm = nullptr;
}

int pbg::policy::norm_args(const char* who, Actor& a, const float* mean, const float* inv_std, float clip) {
  if (!mean && !inv_std) {
    a.norm_on = 0;
    return 1;
  }
  char msg[128];
  if (!mean || !inv_std) {
    snprintf(msg, sizeof(msg), "%s: mean and inv_std must both be given (or both NULL)", who);
    return pbg::capi_fail(PBG_E_ARG, msg);
  }
  if (clip > 0.f) return 0;
  snprintf(msg, sizeof(msg), "%s: clip must be > 0", who);
  return pbg::capi_fail(PBG_E_ARG, msg);
}

extern "C" {

int pbg_policy_create(int device, int obs_dim, int h1, int h2, int act_dim, const float* w1, const float* b1,
                      const float* w2, const float* b2, const float* w3, const float* b3, pbg_policy** out) {
  if (!out) return pbg::capi_fail(PBG_E_ARG, "pbg_policy_create: out is NULL");
  *out = nullptr;
  if (const int rc = check_dims("pbg_policy_create", obs_dim, h1, h2, act_dim)) return rc;
  if (!w1 || !b1 || !w2 || !b2 || !w3 || !b3) return pbg::capi_fail(PBG_E_ARG, "pbg_policy_create: NULL weight array");
  if (device < -1) return pbg::capi_fail(PBG_E_ARG, "pbg_policy_create: device must be >= 0, or -1 for a host-only policy");
  pbg_policy* p = new (std::nothrow) pbg_policy();
  const int D = param_count(obs_dim, h1, h2, act_dim);
  if (p) p->host = (float*)calloc((size_t)D, sizeof(float));
  if (p) p->norm_host = (float*)calloc((size_t)2 * obs_dim, sizeof(float));
  if (!p || !p->host || !p->norm_host) {
    pbg_policy_destroy(p);
    return pbg::capi_fail(PBG_E_NOMEM, "pbg_policy_create: out of host memory");
  }
  const Weights H = weights_at(p->host, obs_dim, h1, h2, act_dim);
  const float* src[6] = {w1, b1, w2, b2, w3, b3};
  const float* dst[7] = {H.w1, H.b1, H.w2, H.b2, H.w3, H.b3, p->host + D};
  for (int i = 0; i < 6; i++) memcpy(p->host + (dst[i] - dst[0]), src[i], (size_t)(dst[i + 1] - dst[i]) * sizeof(float));
  if (const int rc = actor_init("pbg_policy_create", p->a, device, obs_dim, h1, h2, act_dim, 1)) {
    pbg_policy_destroy(p);
    return rc;
  }
  if (device >= 0) {
    DeviceGuard dg(device);
    const int e = (int)hipMemcpy(p->a.params, p->host, (size_t)D * sizeof(float), hipMemcpyHostToDevice);
    if (e) {
      pbg_policy_destroy(p);
      return hip_fail(e, "pbg_policy_create: weight upload");
    }
  }
  *out = p;
  return PBG_OK;
}

void pbg_policy_destroy(pbg_policy* p) {
  if (!p) return;
  actor_free(p->a);
  free(p->norm_host);
  free(p->host);
  delete p;
}

int pbg_policy_set_obs_norm(pbg_policy* p, const float* mean, const float* inv_std, float clip) {
  if (!p) return pbg::capi_fail(PBG_E_ARG, "pbg_policy_set_obs_norm: policy is NULL");
  const int r = norm_args("pbg_policy_set_obs_norm", p->a, mean, inv_std, clip);
  if (r) return r > 0 ? PBG_OK : r;
  const size_t K = (size_t)p->a.obs_dim;
  if (p->a.device >= 0) {
    // a launch enqueued earlier may still read the device copy: upload through the (synchronous) null-stream
    // copy into place only after every stream of the device has drained
    DeviceGuard dg(p->a.device);
    int e = (int)hipDeviceSynchronize();
    if (!e) e = (int)hipMemcpy(p->a.norm, mean, K * sizeof(float), hipMemcpyHostToDevice);
    if (!e) e = (int)hipMemcpy(p->a.norm + K, inv_std, K * sizeof(float), hipMemcpyHostToDevice);
    if (e) {
      p->a.norm_on = 0;
      return hip_fail(e, "pbg_policy_set_obs_norm: upload");
    }
  }
  memcpy(p->norm_host, mean, K * sizeof(float));
  memcpy(p->norm_host + K, inv_std, K * sizeof(float));
  p->a.clip = clip;
  p->a.norm_on = 1;
  return PBG_OK;
}

int pbg_policy_attach_obs_stats(pbg_policy* p, pbg_obs_stats* s) {
  if (!p) return pbg::capi_fail(PBG_E_ARG, "pbg_policy_attach_obs_stats: policy is NULL");
  p->a.stats = s;
  return PBG_OK;
}

int pbg_policy_attach_action_noise(pbg_policy* p, pbg_action_noise* z) {
  if (!p) return pbg::capi_fail(PBG_E_ARG, "pbg_policy_attach_action_noise: policy is NULL");
  p->a.noise = z;
  return PBG_OK;
}

int pbg_policy_act_host(const pbg_policy* p, int n, const float* obs, float* act) {
  if (!p || n < 0 || (n > 0 && (!obs || !act))) return pbg::capi_fail(PBG_E_ARG, "pbg_policy_act_host: bad arguments");
  const Weights P = weights_at(p->host, p->a.obs_dim, p->a.h1, p->a.h2, p->a.act_dim);
  const Norm nm = norm_of(p->a, p->norm_host);
  float a[PBG_POLICY_MAX_DIM], b[PBG_POLICY_MAX_DIM];
  for (int i = 0; i < n; i++) {
    const float* x = obs + (size_t)i * P.obs_dim;
    if (nm.mean) {
      for (int k = 0; k < P.obs_dim; k++) b[k] = normalise(x[k], nm.mean[k], nm.inv_std[k], nm.clip);
      x = b;
    }
    host_layer(P.w1, P.b1, P.obs_dim, P.h1, true, x, a);
    host_layer(P.w2, P.b2, P.h1, P.h2, true, a, b);
    host_layer(P.w3, P.b3, P.h2, P.act_dim, false, b, act + (size_t)i * P.act_dim);
  }
  return PBG_OK;
}

int pbg_policy_act(const pbg_policy* p, int n, const float* obs, float* act, void* stream) {
  if (!p) return pbg::capi_fail(PBG_E_ARG, "pbg_policy_act: policy is NULL");
  if (p->a.device < 0)
    return pbg::capi_fail(PBG_E_ARG, "pbg_policy_act: host-only policy (device -1): use pbg_policy_act_host");
  if (n < 0 || (n > 0 && (!obs || !act))) return pbg::capi_fail(PBG_E_ARG, "pbg_policy_act: bad arguments");
  if (n == 0) return PBG_OK;
  DeviceGuard dg(p->a.device);
  Book none;
  memset(&none, 0, sizeof(none));
  const int e = launch_actor(p->a, n, obs, act, nullptr, nullptr, none, false, Noise{}, (hipStream_t)stream);
  return e ? hip_fail(e, "actor_kernel launch") : PBG_OK;
}

int pbg_rollout(pbg_handle* h, const pbg_policy* p, const pbg_rollout_io_t* uio, void* stream) {
  if (!h || !p || !uio) return pbg::capi_fail(PBG_E_ARG, "pbg_rollout: NULL handle, policy or io");
  if (p->a.device < 0) return pbg::capi_fail(PBG_E_ARG, "pbg_rollout: host-only policy");
  return rollout_loop("pbg_rollout", h, uio, stream, p->a);
}

}  // extern "C"

int pbg::policy::rollout_loop(const char* who, pbg_handle* h, const pbg_rollout_io_t* uio, void* stream, const Actor& a) {
  char msg[200];
  // versioned like pbg_create_opts_t: the first version ends with done_traj, the second with term_obs_traj; read
  // only what the caller's struct holds, fields appended later take zero (their default) for an older caller
  constexpr uint32_t v1_size = (uint32_t)(offsetof(pbg_rollout_io_t, done_traj) + sizeof(uint8_t*));
  constexpr uint32_t v2_size = (uint32_t)(offsetof(pbg_rollout_io_t, term_obs_traj) + sizeof(float*));
  static_assert(v2_size == sizeof(pbg_rollout_io_t), "a field appended to pbg_rollout_io_t needs its version here");
  pbg_rollout_io_t io_copy;
  if (const int rc = pbg::read_versioned(who, "pbg_rollout_io_t", uio, {v1_size, v2_size}, &io_copy)) return rc;
  const pbg_rollout_io_t* io = &io_copy;
  const int dev = pbg::handle_device(h);
  if (a.device != dev) {
    snprintf(msg, sizeof(msg), "%s: the policy lives on another device than the handle", who);
    return pbg::capi_fail(PBG_E_ARG, msg);
  }
  pbg_info_t info;
  if (pbg_info(h, &info)) return PBG_E_ARG;
  if (a.obs_dim != info.obs_dim || a.act_dim != info.action_dim) {
    snprintf(msg, sizeof(msg), "%s: policy maps %d -> %d, the env's obs_dim / action_dim are %d / %d", who, a.obs_dim,
             a.act_dim, info.obs_dim, info.action_dim);
    return pbg::capi_fail(PBG_E_ARG, msg);
  }
  if (info.n_envs % a.n_members != 0) {
    snprintf(msg, sizeof(msg), "%s: the handle's %d envs are not a multiple of the population's %d members", who,
             info.n_envs, a.n_members);
    return pbg::capi_fail(PBG_E_ARG, msg);
  }
  if (a.stats) {
    const long long need = tiles_of(info.n_envs, info.n_envs / a.n_members);
    if (a.stats->device != dev || a.stats->obs_dim != a.obs_dim || (long long)a.stats->n_slots < need) {
      snprintf(msg, sizeof(msg), "%s: the attached obs stats (device %d, obs_dim %d, %d slots) do not fit device %d, obs_dim "
               "%d and the actor's %lld workgroups", who, a.stats->device, a.stats->obs_dim, a.stats->n_slots, dev, a.obs_dim,
               need);
      return pbg::capi_fail(PBG_E_ARG, msg);
    }
  }
  if (a.noise && (a.noise->device != dev || a.noise->act_dim != a.act_dim)) {
    snprintf(msg, sizeof(msg), "%s: the attached action noise (device %d, act_dim %d) does not fit device %d and act_dim %d", who,
             a.noise->device, a.noise->act_dim, dev, a.act_dim);
    return pbg::capi_fail(PBG_E_ARG, msg);
  }
  if (io->n_steps < 1) {
    snprintf(msg, sizeof(msg), "%s: n_steps must be >= 1", who);
    return pbg::capi_fail(PBG_E_ARG, msg);
  }
  if (!io->obs || !io->act || !io->rew64 || (!io->rew && !io->rew_traj) || (!io->done && !io->done_traj) ||
      !io->cur_return || !io->cur_length || !io->done_return || !io->done_length || !io->done_episodes) {
    snprintf(msg, sizeof(msg), "%s: NULL required buffer", who);
    return pbg::capi_fail(PBG_E_ARG, msg);
  }
  if ((io->trunc_traj != nullptr) != (io->term_obs_traj != nullptr) || (io->trunc_traj && !io->autoreset)) {
    snprintf(msg, sizeof(msg), "%s: trunc_traj and term_obs_traj go together (both or neither) and need autoreset != 0", who);
    return pbg::capi_fail(PBG_E_ARG, msg);
  }
  DeviceGuard dg(dev);
  hipStream_t s = (hipStream_t)stream;
  const int n = info.n_envs;
  const size_t no = (size_t)n * info.obs_dim, na = (size_t)n * info.action_dim;
  Book bk{nullptr, nullptr, io->cur_return, io->cur_length, io->done_return, io->done_length, io->done_episodes,
          io->autoreset ? 1 : 0};
  pbg_step_io_t st;
  memset(&st, 0, sizeof(st));
  st.act = io->act;
  st.obs = io->obs;
  st.rew64 = io->rew64;
  st.autoreset = io->autoreset ? 1 : 0;
  Noise nz{};
  if (a.noise)
    nz = Noise{a.noise->std, a.noise->counter, nullptr, (uint32_t)a.noise->seed, (uint32_t)(a.noise->seed >> 32),
               (uint32_t)pbg::handle_env_offset(h), 0u};
  for (int t = 0; t < io->n_steps; t++) {
    if (a.noise) {
      nz.step = (uint32_t)t;
      nz.eps2 = a.noise->eps2_traj ? a.noise->eps2_traj + (size_t)t * n : nullptr;
    }
    // actor: the bookkeeping of step t - 1, then act = pi(obs)
    int e = launch_actor(a, n, io->obs, io->act, io->obs_traj ? io->obs_traj + (size_t)t * no : nullptr,
                         io->act_traj ? io->act_traj + (size_t)t * na : nullptr, bk, a.stats != nullptr, nz, s);
    if (e) return hip_fail(e, "actor kernel launch");
    // the step writes reward and done straight into the trajectory rows when there are any
    st.rew = io->rew_traj ? io->rew_traj + (size_t)t * n : io->rew;
    st.done = io->done_traj ? io->done_traj + (size_t)t * n : io->done;
    // version 2: the step writes the truncation flags and, for the envs it resets, the observation before the reset
    st.trunc = io->trunc_traj ? io->trunc_traj + (size_t)t * n : nullptr;
    st.term_obs = io->term_obs_traj ? io->term_obs_traj + (size_t)t * no : nullptr;
    const int rc = pbg_step_ex(h, &st, stream);
    if (rc) return rc;
    bk.rew64 = io->rew64;
    bk.done = st.done;
  }
  const dim3 bgrid((unsigned)((n + 255) / 256));
  if (a.noise)
    hipLaunchKernelGGL(book_kernel<true>, bgrid, dim3(256), 0, s, bk, n, a.noise->counter, (uint32_t)io->n_steps);
  else
    hipLaunchKernelGGL(book_kernel<false>, bgrid, dim3(256), 0, s, bk, n, (uint32_t*)nullptr, 0u);
  const int e = (int)hipGetLastError();
  return e ? hip_fail(e, "rollout bookkeeping launch") : PBG_OK;
}
