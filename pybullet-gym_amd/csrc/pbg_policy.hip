// pbg_policy.hip -- the pretrained-policy MLP (include/pbg.h pbg_policy_*) and the closed-loop
// rollout (pbg_rollout).  The reference's enjoy scripts evaluate SmallReactivePolicy.act
// (examples/roboschool-weights/enjoy_TF_*.py:25-31) once per env per step on the host; here one
// launch evaluates all three layers for every env, the hidden activations never leave LDS.
//
// Numeric contract (pbg.h): out[j] = fmaf-chain over k ascending, started from b[j]; ReLU as
// `v < 0 ? 0 : v`.  Host and device spell the same chain with __builtin_fmaf, one fma per (k, j, env),
// so they agree bit for bit; nothing is split over k and nothing is left for the compiler to contract.
//
// Geometry (DESIGN.md "Policy kernel"): a workgroup of 256 lanes owns a tile of 16 envs.  Inside a
// layer a lane owns one output column j and EL of the tile's envs: its weight reads W[k][j] are
// coalesced over the lanes (the reference's row-major [K, H] layout as is, read through L2) and the
// activations x[k][e0 .. e0 + EL) are wave-uniform float4 LDS broadcasts.  A layer of H <= 64 columns
// splits the 16 envs over the four waves (EL = 4), H <= 128 over two wave pairs (EL = 8), wider
// layers give every lane all 16: no wave idles through a narrow layer.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <new>

#include "pbg_internal.h"

namespace {

constexpr int PT = 16;                   // envs per workgroup (tile)
constexpr int PB = 256;                  // lanes per workgroup
constexpr int PD = PBG_POLICY_MAX_DIM;   // widest layer

static_assert(PB == PD, "a lane per column of the widest layer");

// bookkeeping of one finished env step (pbg.h pbg_rollout_io_t); rew64 NULL = nothing to do
struct Book {
  const double* rew64;
  const uint8_t* done;
  double* cur_return;
  int32_t* cur_length;
  double* done_return;
  int32_t* done_length;
  int32_t* done_episodes;
  int autoreset;
};

__device__ __forceinline__ void book_env(const Book& b, int e) {
  const int ep = b.done_episodes[e];
  if (!b.autoreset && ep > 0) return;  // first-episode semantics: a finished env stops accumulating
  double cr = b.cur_return[e] + b.rew64[e];
  int cl = b.cur_length[e] + 1;
  if (b.done[e]) {
    b.done_return[e] += cr;
    b.done_length[e] += cl;
    b.done_episodes[e] = ep + 1;
    cr = 0.0;
    cl = 0;
  }
  b.cur_return[e] = cr;
  b.cur_length[e] = cl;
}

__global__ __launch_bounds__(256) void book_kernel(Book b, int n) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e < n) book_env(b, e);
}

struct Weights {
  const float *w1, *b1, *w2, *b2, *w3, *b3;
  int obs_dim, h1, h2, act_dim;
};

// One layer for this lane's column j and envs e0 .. e0 + EL of the tile: xT [K][PT] -> yT [H][PT], both LDS.
template <int EL>
__device__ __forceinline__ void layer_cols(const float* __restrict__ W, const float* __restrict__ bias, int K, int H,
                                           int j, int e0, bool relu, const float* xT, float* yT) {
  float acc[EL];
  const float bj = bias[j];
#pragma unroll
  for (int e = 0; e < EL; e++) acc[e] = bj;
  const float* wp = W + j;
  const float* xp = xT + e0;
  // (an explicit register double-buffer of the weight rows measured the same as this loop: the kernel
  // is bound by the LDS broadcasts and the fma issue, not by the weights' L2 latency)
#pragma unroll 4
  for (int k = 0; k < K; k++) {
    const float w = wp[(size_t)k * H];
#pragma unroll
    for (int q = 0; q < EL / 4; q++) {
      const float4 x = *reinterpret_cast<const float4*>(xp + k * PT + 4 * q);
      acc[4 * q + 0] = __builtin_fmaf(x.x, w, acc[4 * q + 0]);
      acc[4 * q + 1] = __builtin_fmaf(x.y, w, acc[4 * q + 1]);
      acc[4 * q + 2] = __builtin_fmaf(x.z, w, acc[4 * q + 2]);
      acc[4 * q + 3] = __builtin_fmaf(x.w, w, acc[4 * q + 3]);
    }
  }
#pragma unroll
  for (int q = 0; q < EL / 4; q++) {
    float4 y;
    y.x = acc[4 * q + 0]; y.y = acc[4 * q + 1]; y.z = acc[4 * q + 2]; y.w = acc[4 * q + 3];
    if (relu) {
      y.x = y.x < 0.f ? 0.f : y.x; y.y = y.y < 0.f ? 0.f : y.y;
      y.z = y.z < 0.f ? 0.f : y.z; y.w = y.w < 0.f ? 0.f : y.w;
    }
    *reinterpret_cast<float4*>(yT + j * PT + e0 + 4 * q) = y;
  }
}

// A layer over the whole workgroup: H <= 64 columns -> 4 env groups of 4, <= 128 -> 2 of 8, else 1 of 16.
__device__ __forceinline__ void layer(const float* __restrict__ W, const float* __restrict__ bias, int K, int H, bool relu,
                                      const float* xT, float* yT) {
  const int tid = threadIdx.x;
  if (H <= 64) {
    const int j = tid & 63, g = tid >> 6;
    if (j < H) layer_cols<4>(W, bias, K, H, j, 4 * g, relu, xT, yT);
  } else if (H <= 128) {
    const int j = tid & 127, g = tid >> 7;
    if (j < H) layer_cols<8>(W, bias, K, H, j, 8 * g, relu, xT, yT);
  } else {
    if (tid < H) layer_cols<16>(W, bias, K, H, tid, 0, relu, xT, yT);
  }
}

// act[n, act_dim] = pi(obs[n, obs_dim]); optional copies of both into the rollout's trajectories; the
// bookkeeping of the previous env step (bk.rew64 != NULL) for the tile's envs comes first.
__global__ __launch_bounds__(PB) void policy_act_kernel(Weights P, int n, const float* __restrict__ obs,
                                                        float* __restrict__ act, float* __restrict__ obs_traj,
                                                        float* __restrict__ act_traj, Book bk) {
  __shared__ __attribute__((aligned(16))) float bufA[PD * PT];
  __shared__ __attribute__((aligned(16))) float bufB[PD * PT];
  const int tid = threadIdx.x;
  const int env0 = blockIdx.x * PT;
  const int rows = min(PT, n - env0);  // >= 1: the grid is ceil(n / PT)

  if (bk.rew64 && tid < rows) book_env(bk, env0 + tid);

  // the tile's observations (rows * obs_dim contiguous floats) -> bufA [obs_dim][PT], zero past n
  const int K0 = P.obs_dim;
  for (int i = tid; i < PT * K0; i += PB) {
    const int e = i / K0, k = i - e * K0;
    float v = 0.f;
    if (e < rows) {
      const size_t at = (size_t)env0 * K0 + i;
      v = obs[at];
      if (obs_traj) obs_traj[at] = v;
    }
    bufA[k * PT + e] = v;
  }
  __syncthreads();
  layer(P.w1, P.b1, K0, P.h1, true, bufA, bufB);
  __syncthreads();
  layer(P.w2, P.b2, P.h1, P.h2, true, bufB, bufA);
  __syncthreads();
  layer(P.w3, P.b3, P.h2, P.act_dim, false, bufA, bufB);
  __syncthreads();
  const int NA = P.act_dim;
  for (int i = tid; i < rows * NA; i += PB) {
    const int e = i / NA, j = i - e * NA;
    const float v = bufB[j * PT + e];
    const size_t at = (size_t)env0 * NA + i;
    act[at] = v;
    if (act_traj) act_traj[at] = v;
  }
}

}  // namespace

struct pbg_policy {
  int device;  // -1: host only
  int obs_dim, h1, h2, act_dim;
  size_t off[6], words;  // w1 b1 w2 b2 w3 b3 inside one array
  float* host;
  float* dev;
};

namespace {

Weights weights_at(const pbg_policy* p, const float* base) {
  return Weights{base + p->off[0], base + p->off[1], base + p->off[2], base + p->off[3], base + p->off[4],
                 base + p->off[5], p->obs_dim, p->h1, p->h2, p->act_dim};
}

int launch_act(const pbg_policy* p, int n, const float* obs, float* act, float* obs_traj, float* act_traj,
               const Book& bk, hipStream_t stream) {
  const unsigned grid = (unsigned)((n + PT - 1) / PT);
  hipLaunchKernelGGL(policy_act_kernel, dim3(grid), dim3(PB), 0, stream, weights_at(p, p->dev), n, obs, act, obs_traj,
                     act_traj, bk);
  return (int)hipGetLastError();
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
  free(p->host);
  delete p;
}

int pbg_policy_act_host(const pbg_policy* p, int n, const float* obs, float* act) {
  if (!p || n < 0 || (n > 0 && (!obs || !act))) return pbg::capi_fail(PBG_E_ARG, "pbg_policy_act_host: bad arguments");
  const Weights P = weights_at(p, p->host);
  float a[PBG_POLICY_MAX_DIM], b[PBG_POLICY_MAX_DIM];
  for (int i = 0; i < n; i++) {
    host_layer(P.w1, P.b1, P.obs_dim, P.h1, true, obs + (size_t)i * P.obs_dim, a);
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
  const int e = launch_act(p, n, obs, act, nullptr, nullptr, none, (hipStream_t)stream);
  return e ? hip_fail(e, "policy_act_kernel launch") : PBG_OK;
}

int pbg_rollout(pbg_handle* h, const pbg_policy* p, const pbg_rollout_io_t* uio, void* stream) {
  if (!h || !p || !uio) return pbg::capi_fail(PBG_E_ARG, "pbg_rollout: NULL handle, policy or io");
  // versioned like pbg_create_opts_t: the first version ends with done_traj; read only what the caller's
  // struct holds, fields appended later take zero (their default) for an older caller
  constexpr uint32_t v1_size = (uint32_t)(offsetof(pbg_rollout_io_t, done_traj) + sizeof(uint8_t*));
  if (uio->struct_size < v1_size || uio->struct_size > (uint32_t)sizeof(pbg_rollout_io_t) || uio->struct_size % 4u != 0u) {
    char msg[96];
    snprintf(msg, sizeof(msg), "pbg_rollout: io->struct_size %u is not a pbg_rollout_io_t size", uio->struct_size);
    return pbg::capi_fail(PBG_E_ARG, msg);
  }
  pbg_rollout_io_t io_copy;
  memset(&io_copy, 0, sizeof(io_copy));
  memcpy(&io_copy, uio, uio->struct_size);
  const pbg_rollout_io_t* io = &io_copy;
  if (p->device < 0 || !p->dev) return pbg::capi_fail(PBG_E_ARG, "pbg_rollout: host-only policy");
  const int dev = pbg::handle_device(h);
  if (p->device != dev) return pbg::capi_fail(PBG_E_ARG, "pbg_rollout: the policy lives on another device than the handle");
  pbg_info_t info;
  if (pbg_info(h, &info)) return PBG_E_ARG;
  if (p->obs_dim != info.obs_dim || p->act_dim != info.action_dim) {
    char msg[160];
    snprintf(msg, sizeof(msg), "pbg_rollout: policy maps %d -> %d, the env's obs_dim / action_dim are %d / %d", p->obs_dim,
             p->act_dim, info.obs_dim, info.action_dim);
    return pbg::capi_fail(PBG_E_ARG, msg);
  }
  if (io->n_steps < 1) return pbg::capi_fail(PBG_E_ARG, "pbg_rollout: n_steps must be >= 1");
  if (!io->obs || !io->act || !io->rew64 || (!io->rew && !io->rew_traj) || (!io->done && !io->done_traj) ||
      !io->cur_return || !io->cur_length || !io->done_return || !io->done_length || !io->done_episodes)
    return pbg::capi_fail(PBG_E_ARG, "pbg_rollout: NULL required buffer");
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
    int e = launch_act(p, n, io->obs, io->act, io->obs_traj ? io->obs_traj + (size_t)t * no : nullptr,
                       io->act_traj ? io->act_traj + (size_t)t * na : nullptr, bk, s);
    if (e) return hip_fail(e, "policy_act_kernel launch");
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

}  // extern "C"
