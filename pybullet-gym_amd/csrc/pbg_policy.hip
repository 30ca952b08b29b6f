// pbg_policy.hip -- the pretrained-policy MLP (include/pbg.h pbg_policy_*) and the closed-loop
// rollout (pbg_rollout).  The reference's enjoy scripts evaluate SmallReactivePolicy.act
// (examples/roboschool-weights/enjoy_TF_*.py:25-31) once per env per step on the host; here one
// launch evaluates all three layers for every env, the hidden activations never leave LDS.
//
// The MLP tile, its numeric contract and geometry, the bookkeeping and the loop's declaration are in
// pbg_policy_dev.h, shared with the population actor (pbg_population.hip).
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <new>

#include "pbg_policy_dev.h"

namespace {

using namespace pbg::policy;

__global__ __launch_bounds__(256) void book_kernel(Book b, int n) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e < n) book_env(b, e);
}

// act[n, act_dim] = pi(obs[n, obs_dim]); optional copies of both into the rollout's trajectories; the
// bookkeeping of the previous env step (bk.rew64 != NULL) for the tile's envs comes first.
// nm: the policy's normaliser (mean NULL: none); st: slot 0 of the statistics to collect into (sum NULL:
// none), workgroup b adds to slot b; MODE (pbg_policy_dev.h) says which of the two the instantiation looks at.
template <int MODE>
__global__ __launch_bounds__(PB) void policy_act_kernel(Weights P, Norm nm, Slot st, int n, const float* __restrict__ obs,
                                                        float* __restrict__ act, float* __restrict__ obs_traj,
                                                        float* __restrict__ act_traj, Book bk) {
  __shared__ __attribute__((aligned(16))) float bufA[PD * PT];
  __shared__ __attribute__((aligned(16))) float bufB[PD * PT];
  const int env0 = blockIdx.x * PT;
  act_tile<MODE>(P, nm, slot_at(st, P.obs_dim, blockIdx.x), env0, min(PT, n - env0), obs, act, obs_traj, act_traj, bk, bufA,
           bufB);  // rows >= 1: the grid is ceil(n / PT)
}

}  // namespace

struct pbg_policy {
  int device;  // -1: host only
  int obs_dim, h1, h2, act_dim;
  size_t off[6], words;  // w1 b1 w2 b2 w3 b3 inside one array
  float* host;
  float* dev;
  // the normaliser (pbg_policy_set_obs_norm): mean [obs_dim] then inv_std [obs_dim], on the host and, for a
  // device policy, on the device; norm_on 0 = none
  float* norm_host;
  float* norm_dev;
  float clip;
  int norm_on;
  pbg_obs_stats* stats;  // attached (pbg_policy_attach_obs_stats), not owned
};

namespace {

Weights weights_at(const pbg_policy* p, const float* base) {
  return Weights{base + p->off[0], base + p->off[1], base + p->off[2], base + p->off[3], base + p->off[4],
                 base + p->off[5], p->obs_dim, p->h1, p->h2, p->act_dim};
}

Norm norm_at(const pbg_policy* p, const float* base) {
  if (!p->norm_on) return Norm{nullptr, nullptr, 0.f};
  return Norm{base, base + p->obs_dim, p->clip};
}

int launch_act(const pbg_policy* p, int n, const float* obs, float* act, float* obs_traj, float* act_traj,
               const Book& bk, bool collect, hipStream_t stream) {
  const unsigned grid = (unsigned)((n + PT - 1) / PT);
  const Slot st = collect && p->stats ? p->stats->slot0() : Slot{nullptr, nullptr, nullptr};
  const Norm nm = norm_at(p, p->norm_dev);
  const Weights W = weights_at(p, p->dev);
  switch (mode_of(nm, st)) {
    case PLAIN:
      hipLaunchKernelGGL(policy_act_kernel<PLAIN>, dim3(grid), dim3(PB), 0, stream, W, nm, st, n, obs, act, obs_traj, act_traj, bk);
      break;
    case NORM:
      hipLaunchKernelGGL(policy_act_kernel<NORM>, dim3(grid), dim3(PB), 0, stream, W, nm, st, n, obs, act, obs_traj, act_traj, bk);
      break;
    case COLLECT:
      hipLaunchKernelGGL(policy_act_kernel<COLLECT>, dim3(grid), dim3(PB), 0, stream, W, nm, st, n, obs, act, obs_traj, act_traj,
                         bk);
      break;
  }
  return (int)hipGetLastError();
}

int act_of_policy(const void* actor, int n, const float* obs, float* act, float* obs_traj, float* act_traj,
                  const Book& bk, bool collect, hipStream_t stream) {
  return launch_act(static_cast<const pbg_policy*>(actor), n, obs, act, obs_traj, act_traj, bk, collect, stream);
}

int hip_fail(int e, const char* what) {
  char msg[160];
  snprintf(msg, sizeof(msg), "%s: HIP error %d", what, e);
  return pbg::capi_fail(PBG_E_HIP, msg);
}

using pbg::DeviceGuard;

// the contract's chain on the CPU: y[j] = fmaf chain over k ascending from the bias
void host_layer(const float* W, const float* b, int K, int H, bool relu, const float* x, float* y) {
  for (int j = 0; j < H; j++) y[j] = b[j];
  for (int k = 0; k < K; k++) {
    const float xk = x[k];
    const float* w = W + (size_t)k * H;
    for (int j = 0; j < H; j++) y[j] = __builtin_fmaf(xk, w[j], y[j]);
  }
  if (relu)
    for (int j = 0; j < H; j++) y[j] = y[j] < 0.f ? 0.f : y[j];
}

}  // namespace

extern "C" {

int pbg_policy_create(int device, int obs_dim, int h1, int h2, int act_dim, const float* w1, const float* b1,
                      const float* w2, const float* b2, const float* w3, const float* b3, pbg_policy** out) {
  if (!out) return pbg::capi_fail(PBG_E_ARG, "pbg_policy_create: out is NULL");
  *out = nullptr;
  if (obs_dim < 1 || obs_dim > PBG_POLICY_MAX_DIM || h1 < 1 || h1 > PBG_POLICY_MAX_DIM || h2 < 1 ||
      h2 > PBG_POLICY_MAX_DIM || act_dim < 1 || act_dim > PBG_POLICY_MAX_ACT) {
    char msg[200];
    snprintf(msg, sizeof(msg), "pbg_policy_create: dims (%d, %d, %d, %d) outside 1..%d (obs_dim, h1, h2), 1..%d (act_dim)",
             obs_dim, h1, h2, act_dim, PBG_POLICY_MAX_DIM, PBG_POLICY_MAX_ACT);
    return pbg::capi_fail(PBG_E_ARG, msg);
  }
  if (!w1 || !b1 || !w2 || !b2 || !w3 || !b3) return pbg::capi_fail(PBG_E_ARG, "pbg_policy_create: NULL weight array");
  if (device < -1) return pbg::capi_fail(PBG_E_ARG, "pbg_policy_create: device must be >= 0, or -1 for a host-only policy");
  pbg_policy* p = new (std::nothrow) pbg_policy();
  if (!p) return pbg::capi_fail(PBG_E_NOMEM, "pbg_policy_create: out of host memory");
  p->device = device;
  p->obs_dim = obs_dim; p->h1 = h1; p->h2 = h2; p->act_dim = act_dim;
  const size_t cnt[6] = {(size_t)obs_dim * h1, (size_t)h1, (size_t)h1 * h2, (size_t)h2, (size_t)h2 * act_dim,
                         (size_t)act_dim};
  const float* src[6] = {w1, b1, w2, b2, w3, b3};
  size_t at = 0;
  for (int i = 0; i < 6; i++) {
    p->off[i] = at;
    at += (cnt[i] + 3) & ~(size_t)3;  // each array 16-byte aligned
  }
  p->words = at;
  p->dev = nullptr;
  p->norm_host = p->norm_dev = nullptr;
  p->clip = 0.f;
  p->norm_on = 0;
  p->stats = nullptr;
  p->host = (float*)calloc(at, sizeof(float));
  if (!p->host) {
    delete p;
    return pbg::capi_fail(PBG_E_NOMEM, "pbg_policy_create: out of host memory");
  }
  for (int i = 0; i < 6; i++) memcpy(p->host + p->off[i], src[i], cnt[i] * sizeof(float));
  if (device >= 0) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device >= ndev) {
      (void)hipGetLastError();
      pbg_policy_destroy(p);
      char msg[64];
      snprintf(msg, sizeof(msg), "pbg_policy_create: no HIP device %d", device);
      return pbg::capi_fail(PBG_E_HIP, msg);
    }
    DeviceGuard dg(device);
    int e = (int)hipMalloc(&p->dev, at * sizeof(float));
    if (!e) e = (int)hipMemcpy(p->dev, p->host, at * sizeof(float), hipMemcpyHostToDevice);
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
  if (p->dev) {
    DeviceGuard dg(p->device);
    (void)hipFree(p->dev);
  }
  if (p->norm_dev) {
    DeviceGuard dg(p->device);
    (void)hipFree(p->norm_dev);
  }
  free(p->norm_host);
  free(p->host);
  delete p;
}

int pbg_policy_set_obs_norm(pbg_policy* p, const float* mean, const float* inv_std, float clip) {
  if (!p) return pbg::capi_fail(PBG_E_ARG, "pbg_policy_set_obs_norm: policy is NULL");
  if (!mean && !inv_std) {
    p->norm_on = 0;
    return PBG_OK;
  }
  if (!mean || !inv_std) return pbg::capi_fail(PBG_E_ARG, "pbg_policy_set_obs_norm: mean and inv_std must both be given (or both NULL)");
  if (!(clip > 0.f)) return pbg::capi_fail(PBG_E_ARG, "pbg_policy_set_obs_norm: clip must be > 0");
  const size_t K = (size_t)p->obs_dim;
  if (!p->norm_host) {
    p->norm_host = (float*)calloc(2 * K, sizeof(float));
    if (!p->norm_host) return pbg::capi_fail(PBG_E_NOMEM, "pbg_policy_set_obs_norm: out of host memory");
  }
  if (p->device >= 0) {
    // a launch enqueued earlier may still read the device copy: upload through the (synchronous) null-stream
    // copy into place only after every stream of the device has drained
    DeviceGuard dg(p->device);
    int e = p->norm_dev ? 0 : (int)hipMalloc(&p->norm_dev, 2 * K * sizeof(float));
    if (!e) e = (int)hipDeviceSynchronize();
    if (!e) e = (int)hipMemcpy(p->norm_dev, mean, K * sizeof(float), hipMemcpyHostToDevice);
    if (!e) e = (int)hipMemcpy(p->norm_dev + K, inv_std, K * sizeof(float), hipMemcpyHostToDevice);
    if (e) {
      p->norm_on = 0;
      return hip_fail(e, "pbg_policy_set_obs_norm: upload");
    }
  }
  memcpy(p->norm_host, mean, K * sizeof(float));
  memcpy(p->norm_host + K, inv_std, K * sizeof(float));
  p->clip = clip;
  p->norm_on = 1;
  return PBG_OK;
}

int pbg_policy_attach_obs_stats(pbg_policy* p, pbg_obs_stats* s) {
  if (!p) return pbg::capi_fail(PBG_E_ARG, "pbg_policy_attach_obs_stats: policy is NULL");
  p->stats = s;
  return PBG_OK;
}

int pbg_policy_act_host(const pbg_policy* p, int n, const float* obs, float* act) {
  if (!p || n < 0 || (n > 0 && (!obs || !act))) return pbg::capi_fail(PBG_E_ARG, "pbg_policy_act_host: bad arguments");
  const Weights P = weights_at(p, p->host);
  const Norm nm = norm_at(p, p->norm_host);
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
  if (p->device < 0 || !p->dev)
    return pbg::capi_fail(PBG_E_ARG, "pbg_policy_act: host-only policy (device -1): use pbg_policy_act_host");
  if (n < 0 || (n > 0 && (!obs || !act))) return pbg::capi_fail(PBG_E_ARG, "pbg_policy_act: bad arguments");
  if (n == 0) return PBG_OK;
  DeviceGuard dg(p->device);
  Book none;
  memset(&none, 0, sizeof(none));
  const int e = launch_act(p, n, obs, act, nullptr, nullptr, none, false, (hipStream_t)stream);
  return e ? hip_fail(e, "policy_act_kernel launch") : PBG_OK;
}

int pbg_rollout(pbg_handle* h, const pbg_policy* p, const pbg_rollout_io_t* uio, void* stream) {
  if (!h || !p || !uio) return pbg::capi_fail(PBG_E_ARG, "pbg_rollout: NULL handle, policy or io");
  if (p->device < 0 || !p->dev) return pbg::capi_fail(PBG_E_ARG, "pbg_rollout: host-only policy");
  return rollout_loop("pbg_rollout", h, uio, stream, p->device, p->obs_dim, p->act_dim, 1, act_of_policy, p, p->stats);
}

}  // extern "C"

int pbg::policy::rollout_loop(const char* who, pbg_handle* h, const pbg_rollout_io_t* uio, void* stream, int actor_device,
                              int obs_dim, int act_dim, int group, ActLaunch launch, const void* actor,
                              const pbg_obs_stats* stats) {
  char msg[200];
  // versioned like pbg_create_opts_t: the first version ends with done_traj; read only what the caller's
  // struct holds, fields appended later take zero (their default) for an older caller
  constexpr uint32_t v1_size = (uint32_t)(offsetof(pbg_rollout_io_t, done_traj) + sizeof(uint8_t*));
  if (uio->struct_size < v1_size || uio->struct_size > (uint32_t)sizeof(pbg_rollout_io_t) || uio->struct_size % 4u != 0u) {
    snprintf(msg, sizeof(msg), "%s: io->struct_size %u is not a pbg_rollout_io_t size", who, uio->struct_size);
    return pbg::capi_fail(PBG_E_ARG, msg);
  }
  pbg_rollout_io_t io_copy;
  memset(&io_copy, 0, sizeof(io_copy));
  memcpy(&io_copy, uio, uio->struct_size);
  const pbg_rollout_io_t* io = &io_copy;
  const int dev = pbg::handle_device(h);
  if (actor_device != dev) {
    snprintf(msg, sizeof(msg), "%s: the policy lives on another device than the handle", who);
    return pbg::capi_fail(PBG_E_ARG, msg);
  }
  pbg_info_t info;
  if (pbg_info(h, &info)) return PBG_E_ARG;
  if (obs_dim != info.obs_dim || act_dim != info.action_dim) {
    snprintf(msg, sizeof(msg), "%s: policy maps %d -> %d, the env's obs_dim / action_dim are %d / %d", who, obs_dim,
             act_dim, info.obs_dim, info.action_dim);
    return pbg::capi_fail(PBG_E_ARG, msg);
  }
  if (group > 1 && info.n_envs % group != 0) {
    snprintf(msg, sizeof(msg), "%s: the handle's %d envs are not a multiple of the population's %d members", who,
             info.n_envs, group);
    return pbg::capi_fail(PBG_E_ARG, msg);
  }
  if (stats) {
    const long long need = tiles_of(info.n_envs, info.n_envs / (group > 1 ? group : 1));
    if (stats->device != dev || stats->obs_dim != obs_dim || (long long)stats->n_slots < need) {
      snprintf(msg, sizeof(msg), "%s: the attached obs stats (device %d, obs_dim %d, %d slots) do not fit device %d, obs_dim "
               "%d and the actor's %lld workgroups", who, stats->device, stats->obs_dim, stats->n_slots, dev, obs_dim, need);
      return pbg::capi_fail(PBG_E_ARG, msg);
    }
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
  for (int t = 0; t < io->n_steps; t++) {
    // actor: the bookkeeping of step t - 1, then act = pi(obs)
    int e = launch(actor, n, io->obs, io->act, io->obs_traj ? io->obs_traj + (size_t)t * no : nullptr,
                   io->act_traj ? io->act_traj + (size_t)t * na : nullptr, bk, stats != nullptr, s);
    if (e) return hip_fail(e, "actor kernel launch");
    // the step writes reward and done straight into the trajectory rows when there are any
    st.rew = io->rew_traj ? io->rew_traj + (size_t)t * n : io->rew;
    st.done = io->done_traj ? io->done_traj + (size_t)t * n : io->done;
    const int rc = pbg_step_ex(h, &st, stream);
    if (rc) return rc;
    bk.rew64 = io->rew64;
    bk.done = st.done;
  }
  hipLaunchKernelGGL(book_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, bk, n);
  const int e = (int)hipGetLastError();
  return e ? hip_fail(e, "rollout bookkeeping launch") : PBG_OK;
}
