// pbg_ppograd.hip -- the backward pass of the PPO clipped-surrogate update (include/pbg.h "PPO gradient"): the
// pbg_ppo_grad object, the tile kernel, the reduction and the host twin.
//
// Geometry.  The tile kernel is the actor's tile (pbg_policy_dev.h: 256 lanes, 16 rows,
// transposed [width][16] LDS planes, `layer` for the forward) with the activations kept: per tile a workgroup
// gathers its rows by idx into bX, runs the actor's three layers into bH1, bH2, bD, lets lane e < 16 turn row e's
// means into dL/dmu in place (ppo_actor_row), and walks back: per layer the weight gradient (dw_layer: a lane owns
// a column j and every NG-th input row k, holds dy[j][0 .. 16) in registers and reads x[k][0 .. 16) as wave-uniform
// float4 broadcasts) and the masked transposed product (back_layer: the forward's split with the roles of k and
// j swapped).  Then the actor's means once more in float64 for `stats` (actor_forward64: half a tile at a time in
// the planes the backward has left idle), and the same forward and backward for the critic on the same bX.  A
// workgroup owns the tiles b, b + G, ...; its sums over them stay in registers when obs_dim, h1, h2 <= 64 (REG: 16
// per lane and layer) and go through its own partial in global memory otherwise.  The reduction kernel adds the partials in float64.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <new>

#include "pbg_ppograd_dev.h"

namespace {

using namespace pbg::policy;
using namespace pbg::ppograd;  // Args, gather_tile, actor_forward64
using pbg::DeviceGuard;

constexpr int MAX_WG = 512;                       // two workgroups per CU
constexpr size_t MAX_WS_BYTES = (size_t)128 << 20;
constexpr int RK = 16;                            // REG: weight-gradient accumulators per lane and layer

// out[k][e] = act[k][e] > 0 ? sum_j W[k][j] dy[j][e] : 0 for this lane's row k and envs e0 .. e0 + EL
template <int EL>
__device__ __forceinline__ void back_cols(const float* __restrict__ W, int H, int k, int e0, const float* dyT, const float* actT,
                                          float* outT) {
  float acc[EL];
#pragma unroll
  for (int e = 0; e < EL; e++) acc[e] = 0.f;
  const float* wp = W + (size_t)k * H;
  const float* dp = dyT + e0;
#pragma unroll 4
  for (int j = 0; j < H; j++) {
    const float w = wp[j];
#pragma unroll
    for (int q = 0; q < EL / 4; q++) {
      const float4 d = *reinterpret_cast<const float4*>(dp + j * PT + 4 * q);
      acc[4 * q + 0] = __builtin_fmaf(d.x, w, acc[4 * q + 0]);
      acc[4 * q + 1] = __builtin_fmaf(d.y, w, acc[4 * q + 1]);
      acc[4 * q + 2] = __builtin_fmaf(d.z, w, acc[4 * q + 2]);
      acc[4 * q + 3] = __builtin_fmaf(d.w, w, acc[4 * q + 3]);
    }
  }
#pragma unroll
  for (int q = 0; q < EL / 4; q++) {
    const float4 a = *reinterpret_cast<const float4*>(actT + k * PT + e0 + 4 * q);
    float4 y;
    y.x = a.x > 0.f ? acc[4 * q + 0] : 0.f; y.y = a.y > 0.f ? acc[4 * q + 1] : 0.f;
    y.z = a.z > 0.f ? acc[4 * q + 2] : 0.f; y.w = a.w > 0.f ? acc[4 * q + 3] : 0.f;
    *reinterpret_cast<float4*>(outT + k * PT + e0 + 4 * q) = y;
  }
}

// the gradient of a layer's input activations (K rows) from its outputs' (H rows): `layer`'s split over K
__device__ __forceinline__ void back_layer(const float* __restrict__ W, int K, int H, const float* dyT, const float* actT,
                                           float* outT) {
  const int tid = threadIdx.x;
  if (K <= 64) {
    const int k = tid & 63, g = tid >> 6;
    if (k < K) back_cols<4>(W, H, k, 4 * g, dyT, actT, outT);
  } else if (K <= 128) {
    const int k = tid & 127, g = tid >> 7;
    if (k < K) back_cols<8>(W, H, k, 8 * g, dyT, actT, outT);
  } else {
    if (tid < K) back_cols<16>(W, H, tid, 0, dyT, actT, outT);
  }
}

// one element's tile value: the fmaf chain over the tile's rows ascending from zero
__device__ __forceinline__ float dot_rows(const float* xk, const float (&dy)[PT]) {
  float d = 0.f;
#pragma unroll
  for (int q = 0; q < PT / 4; q++) {
    const float4 x = *reinterpret_cast<const float4*>(xk + 4 * q);
    d = __builtin_fmaf(x.x, dy[4 * q + 0], d);
    d = __builtin_fmaf(x.y, dy[4 * q + 1], d);
    d = __builtin_fmaf(x.z, dy[4 * q + 2], d);
    d = __builtin_fmaf(x.w, dy[4 * q + 3], d);
  }
  return d;
}

// The weight and bias gradient of one layer ([K, H] weights) for one tile: lane (j, g) owns column j and the input
// rows k = g, g + NG, ...  REG (K, H <= 64: NG = 4, at most RK rows): the tile's values are added onto aw / ab;
// otherwise onto the workgroup's partial pw (the first tile stores).  The bias sum is always a register.
template <bool REG>
__device__ __forceinline__ void dw_layer(int K, int H, const float* xT, const float* dyT, float* __restrict__ pw, bool first,
                                         float (&aw)[RK], float& ab) {
  const int tid = threadIdx.x;
  int j, g, NG;
  if (REG || H <= 64) { j = tid & 63; g = tid >> 6; NG = 4; }
  else if (H <= 128) { j = tid & 127; g = tid >> 7; NG = 2; }
  else { j = tid; g = 0; NG = 1; }
  if (j >= H) return;
  float dy[PT];
#pragma unroll
  for (int q = 0; q < PT / 4; q++) {
    const float4 d = *reinterpret_cast<const float4*>(dyT + j * PT + 4 * q);
    dy[4 * q + 0] = d.x; dy[4 * q + 1] = d.y; dy[4 * q + 2] = d.z; dy[4 * q + 3] = d.w;
  }
  if (g == 0) {
    float s = 0.f;
#pragma unroll
    for (int e = 0; e < PT; e++) s += dy[e];
    ab += s;
  }
  if (REG) {
#pragma unroll
    for (int kk = 0; kk < RK; kk++) {
      const int k = g + 4 * kk;
      if (k < K) aw[kk] += dot_rows(xT + k * PT, dy);
    }
  } else {
    for (int k = g; k < K; k += NG) {
      const float d = dot_rows(xT + k * PT, dy);
      float* at = pw + (size_t)k * H + j;
      *at = (first ? 0.f : *at) + d;
    }
  }
}

// REG: what dw_layer kept in registers goes to the partial
__device__ __forceinline__ void flush_w(int K, int H, float* __restrict__ pw, const float (&aw)[RK]) {
  const int j = threadIdx.x & 63, g = threadIdx.x >> 6;
  if (j >= H) return;
#pragma unroll
  for (int kk = 0; kk < RK; kk++) {
    const int k = g + 4 * kk;
    if (k < K) pw[(size_t)k * H + j] = aw[kk];
  }
}

// the bias lanes of dw_layer: g == 0
__device__ __forceinline__ void flush_b(int H, float* __restrict__ pb, float ab) {
  const int tid = threadIdx.x;
  const bool lane = H <= 64 ? tid < 64 : (H <= 128 ? tid < 128 : true);
  if (lane && tid < H) pb[tid] = ab;
}

// a network's accumulators over the workgroup's tiles
struct NetAcc {
  float w1[RK], w2[RK], w3[RK];
  float b1, b2, b3;
};

__device__ __forceinline__ void zero(NetAcc& a) {
#pragma unroll
  for (int i = 0; i < RK; i++) a.w1[i] = a.w2[i] = a.w3[i] = 0.f;
  a.b1 = a.b2 = a.b3 = 0.f;
}

struct Planes {
  float *X, *H1, *H2, *E, *D, *D2;
};

// forward of one network on the tile in L.X: H1, H2 and the outputs D [NA][PT]
__device__ __forceinline__ void net_forward(const Weights& P, const Planes& L) {
  layer(P.w1, P.b1, P.obs_dim, P.h1, true, L.X, L.H1);
  __syncthreads();
  layer(P.w2, P.b2, P.h1, P.h2, true, L.H1, L.H2);
  __syncthreads();
  layer(P.w3, P.b3, P.h2, P.act_dim, false, L.H2, L.D);
  __syncthreads();
}

// backward of one network from dL/d(outputs) in L.D (a barrier behind it); G: its arrays of the partial
template <bool REG>
__device__ __forceinline__ void net_backward(const Weights& P, const Weights& G, const Planes& L, bool first, NetAcc& acc) {
  dw_layer<REG>(P.h2, P.act_dim, L.H2, L.D, const_cast<float*>(G.w3), first, acc.w3, acc.b3);
  back_layer(P.w3, P.h2, P.act_dim, L.D, L.H2, L.E);
  __syncthreads();
  dw_layer<REG>(P.h1, P.h2, L.H1, L.E, const_cast<float*>(G.w2), first, acc.w2, acc.b2);
  back_layer(P.w2, P.h1, P.h2, L.E, L.H1, L.H2);  // H2 is free: its mask and its weight gradient are done
  __syncthreads();
  dw_layer<REG>(P.obs_dim, P.h1, L.X, L.H2, const_cast<float*>(G.w1), first, acc.w1, acc.b1);
}

template <bool REG>
__device__ __forceinline__ void net_flush(const Weights& P, const Weights& G, const NetAcc& acc) {
  if (REG) {
    flush_w(P.obs_dim, P.h1, const_cast<float*>(G.w1), acc.w1);
    flush_w(P.h1, P.h2, const_cast<float*>(G.w2), acc.w2);
    flush_w(P.h2, P.act_dim, const_cast<float*>(G.w3), acc.w3);
  }
  flush_b(P.h1, const_cast<float*>(G.b1), acc.b1);
  flush_b(P.h2, const_cast<float*>(G.b2), acc.b2);
  flush_b(P.act_dim, const_cast<float*>(G.b3), acc.b3);
}

// Workgroup b = a.wg0 + blockIdx.x of a.G: the tiles b, b + a.G, ... of the minibatch into row blockIdx.x of a.part.  LDS: four [256][16] planes and
// two [64][16] ones, 72 KiB, plus the row lanes' doubles.
template <bool REG>
__global__ __launch_bounds__(PB) void ppograd_tiles_kernel(const Args a) {
  __shared__ __attribute__((aligned(16))) float bX[PD * PT];
  __shared__ __attribute__((aligned(16))) float bH1[PD * PT];
  __shared__ __attribute__((aligned(16))) float bH2[PD * PT];
  __shared__ __attribute__((aligned(16))) float bE[PD * PT];
  __shared__ __attribute__((aligned(16))) float bDD[2 * NA_MAX * PT];  // bD, bD2; the float64 means span both
  float* const bD = bDD;
  float* const bD2 = bDD + NA_MAX * PT;
  __shared__ double inv_sig[NA_MAX];
  __shared__ double sstat[4 * PT];
  const Planes L{bX, bH1, bH2, bE, bD, bD2};
  if (a.gate && a.gate[0] != 0) return;  // stopped: uniform over the launch, nothing read or written
  const int tid = threadIdx.x, A = a.A;
  const Weights Pa = weights_at(a.theta_a, a.obs_dim, a.h1, a.h2, A);
  const Weights Pc = weights_at(a.theta_c, a.obs_dim, a.h1, a.h2, 1);
  float* part = a.part + (size_t)blockIdx.x * a.Dtot;
  const Weights Ga = weights_at(part, a.obs_dim, a.h1, a.h2, A);
  const Weights Gc = weights_at(part + a.Da, a.obs_dim, a.h1, a.h2, 1);

  if (tid < A) inv_sig[tid] = exp(-(double)a.log_std[tid]);  // read behind the tile's barriers
  double sum_ls = 0.0;
  if (tid < PT)
    for (int j = 0; j < A; j++) sum_ls += (double)a.log_std[j];
  const double inv_bm = 1.0 / (double)a.Bm;
  NetAcc accA, accC;
  zero(accA);
  zero(accC);
  float als = 0.f;                                // lane j < A: log_std's sum
  double st0 = 0.0, st1 = 0.0, st2 = 0.0, st3 = 0.0;  // row lanes: pg, vf, clipped, logp_old - logp

  const int ntiles = (a.Bm + PT - 1) / PT;
  bool first = true;
  for (int t = a.wg0 + (int)blockIdx.x; t < ntiles; t += a.G, first = false) {
    const int row0 = t * PT, rows = min(PT, a.Bm - row0);
    if (!first) __syncthreads();  // the previous tile's last weight gradient reads bX and bH2
    gather_tile(a.obs_dim, a.idx, row0, rows, a.obs, a.nm, bX);
    __syncthreads();
    size_t r = 0;  // row lanes: the batch row
    if (tid < rows) r = a.idx ? (size_t)a.idx[row0 + tid] : (size_t)(row0 + tid);

    // ---- the actor
    net_forward(Pa, L);
    if (tid < PT) {
      if (tid < rows) {
        double ahat = (double)a.adv[r];
        if (a.adv_norm) ahat = (ahat - (double)a.adv_norm[0]) * (double)a.adv_norm[1];
        const double logp = ppo_actor_row(A, bD + tid, bD2 + tid, PT, a.act + r * A, inv_sig, sum_ls, (double)a.logp_old[r],
                                          ahat, (double)a.clip_eps, inv_bm);
        if (a.logp_out) a.logp_out[row0 + tid] = (float)logp;
      } else {
        for (int j = 0; j < A; j++) bD[j * PT + tid] = bD2[j * PT + tid] = 0.f;
      }
    }
    __syncthreads();
    if (tid < A) {
      float s = 0.f;
#pragma unroll
      for (int e = 0; e < PT; e++) s += bD2[tid * PT + e];
      als += s;
    }
    net_backward<REG>(Pa, Ga, L, first, accA);

    // ---- the actor's statistics from a float64 forward: every plane but bX is idle
    __syncthreads();  // the last weight gradient reads bH2
    double* mu64 = reinterpret_cast<double*>(bDD);
    if (a.obs_dim <= PD / 2 && a.h1 <= PD / 2 && a.h2 <= PD / 2)
      actor_forward64<PT>(Pa, a.nm, a.idx, row0, rows, a.obs, bE, bH1, bH2, mu64);
    else
      actor_forward64<PT / 2>(Pa, a.nm, a.idx, row0, rows, a.obs, bE, bH1, bH2, mu64);
    if (tid < rows) {
      double ahat = (double)a.adv[r];
      if (a.adv_norm) ahat = (ahat - (double)a.adv_norm[0]) * (double)a.adv_norm[1];
      double st[3];
      ppo_stats_row(A, mu64 + tid, PT, a.act + r * A, inv_sig, sum_ls, (double)a.logp_old[r], ahat, (double)a.clip_eps, st);
      st0 += st[0];
      st2 += st[1];
      st3 += st[2];
    }

    // ---- the critic on the same bX (its first layer writes bH1, which the actor's last phase does not read)
    net_forward(Pc, L);
    if (tid < PT) {
      float dv = 0.f;
      if (tid < rows) {
        const float v = bD[tid];
        double vf;
        dv = ppo_critic_row(v, a.ret[r], a.value_old ? a.value_old + r : nullptr, (double)a.vf_clip, (double)a.vf_coef, inv_bm,
                            &vf);
        st1 += vf;
        if (a.v_out) a.v_out[row0 + tid] = v;
      }
      bD[tid] = dv;
    }
    __syncthreads();
    net_backward<REG>(Pc, Gc, L, first, accC);
  }

  net_flush<REG>(Pa, Ga, accA);
  net_flush<REG>(Pc, Gc, accC);
  if (tid < A) part[a.Dtot - A + tid] = als;
  if (tid < PT) {
    sstat[0 * PT + tid] = st0;
    sstat[1 * PT + tid] = st1;
    sstat[2 * PT + tid] = st2;
    sstat[3 * PT + tid] = st3;
  }
  __syncthreads();
  if (tid < 4) {
    double s = 0.0;
    for (int e = 0; e < PT; e++) s += sstat[tid * PT + e];
    a.part_stats[(size_t)blockIdx.x * 4 + tid] = s;
  }
}

// a lane per gradient element: the G partials in ascending order, float64; block 0 also folds the stats
__global__ __launch_bounds__(256) void ppograd_reduce_kernel(const float* __restrict__ part, const double* __restrict__ part_stats,
                                                             int G, int Da, int Dc, int Dtot, float ent_coef, int Bm,
                                                             float* __restrict__ grad_actor, float* __restrict__ grad_critic,
                                                             float* __restrict__ grad_log_std, double* __restrict__ stats,
                                                             const int32_t* __restrict__ gate) {
  if (gate && gate[0] != 0) return;  // stopped: the outputs keep what they held
  const int d = blockIdx.x * 256 + threadIdx.x;
  if (d < Dtot) {
    double s = 0.0;
    for (int g = 0; g < G; g++) s += (double)part[(size_t)g * Dtot + d];
    if (d < Da) grad_actor[d] = (float)s;
    else if (d < Da + Dc) grad_critic[d - Da] = (float)s;
    else grad_log_std[d - Da - Dc] = (float)(s - (double)ent_coef);
  }
  if (blockIdx.x == 0 && threadIdx.x < 4) {
    double s = 0.0;
    for (int g = 0; g < G; g++) s += part_stats[(size_t)g * 4 + threadIdx.x];
    stats[threadIdx.x] = s / (double)Bm;
  }
}

// what run and host check alike: the struct's version, then its fields; copies the caller's struct into `io`.
// need_in: the batch, the parameters and the loss's constants (all but reduce); need_out: grad_* and stats (all but
// run_part)
int check_io(const char* who, const pbg_ppo_grad_io_t* uio, pbg_ppo_grad_io_t* io, bool need_in = true, bool need_out = true) {
  char msg[200];
  if (!uio) {
    snprintf(msg, sizeof(msg), "%s: io is NULL", who);
    return pbg::capi_fail(PBG_E_ARG, msg);
  }
  constexpr uint32_t v1_size = (uint32_t)(offsetof(pbg_ppo_grad_io_t, v_out) + sizeof(float*));
  // the two versions: the one that ends with v_out and this library's, which appends value_old, gate and vf_clip (NULL,
  // NULL and 0 for the first)
  if (const int rc = pbg::read_versioned(who, "pbg_ppo_grad_io_t", uio, {v1_size, (uint32_t)sizeof(pbg_ppo_grad_io_t)}, io))
    return rc;
  if (io->mb_rows < 1 || io->batch_rows < 1 || (!io->idx && io->mb_rows > io->batch_rows)) {
    snprintf(msg, sizeof(msg), "%s: mb_rows %d and batch_rows %d must be >= 1, and mb_rows <= batch_rows without idx", who,
             io->mb_rows, io->batch_rows);
    return pbg::capi_fail(PBG_E_ARG, msg);
  }
  if ((need_in && (!io->theta_actor || !io->theta_critic || !io->log_std || !io->obs || !io->act || !io->logp_old || !io->adv ||
                   !io->ret)) ||
      (need_out && (!io->grad_actor || !io->grad_critic || !io->grad_log_std || !io->stats))) {
    snprintf(msg, sizeof(msg), "%s: NULL required pointer", who);
    return pbg::capi_fail(PBG_E_ARG, msg);
  }
  if (!need_in) return PBG_OK;
  if ((io->mean == nullptr) != (io->inv_std == nullptr) || (io->mean && !(io->clip > 0.f))) {
    snprintf(msg, sizeof(msg), "%s: mean and inv_std must both be given with a clip > 0, or both NULL", who);
    return pbg::capi_fail(PBG_E_ARG, msg);
  }
  if (!(io->clip_eps >= 0.f)) {
    snprintf(msg, sizeof(msg), "%s: clip_eps must be >= 0", who);
    return pbg::capi_fail(PBG_E_ARG, msg);
  }
  if (io->value_old && !(io->vf_clip > 0.f)) {
    snprintf(msg, sizeof(msg), "%s: vf_clip must be > 0 when value_old is given", who);
    return pbg::capi_fail(PBG_E_ARG, msg);
  }
  return PBG_OK;
}

// pbg_ppo_grad_create and pbg_ppo_grad_create_ex behind their own checks of `out` and `opts`; max_wg: the path's
// workgroup cap
int create_object(const char* who, int device, int obs_dim, int h1, int h2, int act_dim, int max_rows, int path, int max_wg,
                  pbg_ppo_grad** out) {
  char msg[160];
  if (const int rc = check_dims(who, obs_dim, h1, h2, act_dim)) return rc;
  if (max_rows < 1 || device < 0) {
    snprintf(msg, sizeof(msg), "%s: max_rows %d < 1 or device %d < 0", who, max_rows, device);
    return pbg::capi_fail(PBG_E_ARG, msg);
  }
  if (const int rc = check_device(who, device)) return rc;
  pbg_ppo_grad* g = new (std::nothrow) pbg_ppo_grad();
  if (!g) {
    snprintf(msg, sizeof(msg), "%s: out of host memory", who);
    return pbg::capi_fail(PBG_E_NOMEM, msg);
  }
  g->path = path;
  g->device = device;
  g->obs_dim = obs_dim; g->h1 = h1; g->h2 = h2; g->act_dim = act_dim;
  g->max_rows = max_rows;
  g->Da = param_count(obs_dim, h1, h2, act_dim);
  g->Dc = param_count(obs_dim, h1, h2, 1);
  g->Dtot = g->Da + g->Dc + act_dim;
  const size_t per_wg = (size_t)g->Dtot * sizeof(float) + 4 * sizeof(double);
  long long n = ((long long)max_rows + PT - 1) / PT;
  if (n > max_wg) n = max_wg;
  if (n > (long long)(MAX_WS_BYTES / per_wg)) n = (long long)(MAX_WS_BYTES / per_wg);
  g->n_wg = n < 1 ? 1 : (int)n;
  g->part = nullptr;
  DeviceGuard dg(device);
  // the doubles first: 8-byte aligned whatever Dtot is
  const size_t bytes = (size_t)g->n_wg * per_wg;
  void* ws = nullptr;
  int e = (int)hipMalloc(&ws, bytes);
  if (!e) e = (int)hipMemset(ws, 0, bytes);
  if (e) {
    if (ws) (void)hipFree(ws);
    delete g;
    snprintf(msg, sizeof(msg), "%s: workspace", who);
    return hip_fail(e, msg);
  }
  g->part_stats = reinterpret_cast<double*>(ws);
  g->part = reinterpret_cast<float*>(g->part_stats + (size_t)g->n_wg * 4);
  *out = g;
  return PBG_OK;
}

// the workgroups of a whole gradient over mb_rows rows: min(tiles, n_wg)
int workgroups_of(const pbg_ppo_grad* g, int mb_rows) {
  const int ntiles = (mb_rows + PT - 1) / PT;
  return ntiles < g->n_wg ? ntiles : g->n_wg;
}

int check_rows(const char* who, const pbg_ppo_grad* g, int mb_rows) {
  if (mb_rows <= g->max_rows) return PBG_OK;
  char msg[160];
  snprintf(msg, sizeof(msg), "%s: mb_rows %d exceeds the object's max_rows %d", who, mb_rows, g->max_rows);
  return pbg::capi_fail(PBG_E_ARG, msg);
}

// the tile kernel of the object's path for the workgroups wg0 .. wg0 + count - 1 of G, row i of part / part_stats
// for workgroup wg0 + i
int launch_tiles(const pbg_ppo_grad* g, const pbg_ppo_grad_io_t& io, int wg0, int count, int G, float* part, double* part_stats,
                 hipStream_t s) {
  Args a;
  a.theta_a = io.theta_actor; a.theta_c = io.theta_critic; a.log_std = io.log_std;
  a.nm = io.mean ? Norm{io.mean, io.inv_std, io.clip} : Norm{nullptr, nullptr, 0.f};
  a.obs = io.obs; a.act = io.act; a.logp_old = io.logp_old; a.adv = io.adv; a.ret = io.ret;
  a.idx = io.idx; a.adv_norm = io.adv_norm;
  a.clip_eps = io.clip_eps; a.vf_coef = io.vf_coef;
  a.Bm = io.mb_rows; a.obs_dim = g->obs_dim; a.h1 = g->h1; a.h2 = g->h2; a.A = g->act_dim; a.Da = g->Da; a.Dtot = g->Dtot;
  a.wg0 = wg0; a.G = G;
  a.part = part; a.part_stats = part_stats;
  a.logp_out = io.logp_out; a.v_out = io.v_out;
  a.value_old = io.value_old; a.gate = io.gate; a.vf_clip = io.vf_clip;
  const bool reg = g->obs_dim <= 64 && g->h1 <= 64 && g->h2 <= 64;
  int e;
  if (g->path == PBG_PPO_GRAD_MFMA) {
    e = launch_tiles_mfma(a, count, s);
  } else {
    if (reg)
      hipLaunchKernelGGL(ppograd_tiles_kernel<true>, dim3((unsigned)count), dim3(PB), 0, s, a);
    else
      hipLaunchKernelGGL(ppograd_tiles_kernel<false>, dim3((unsigned)count), dim3(PB), 0, s, a);
    e = (int)hipGetLastError();
  }
  return e ? hip_fail(e, "ppograd_tiles_kernel launch") : PBG_OK;
}

int launch_reduce(const pbg_ppo_grad* g, const pbg_ppo_grad_io_t& io, int G, const float* part, const double* part_stats,
                  hipStream_t s) {
  hipLaunchKernelGGL(ppograd_reduce_kernel, dim3((unsigned)((g->Dtot + 255) / 256)), dim3(256), 0, s, part, part_stats, G, g->Da,
                     g->Dc, g->Dtot, io.ent_coef, io.mb_rows, io.grad_actor, io.grad_critic, io.grad_log_std, io.stats, io.gate);
  const int e = (int)hipGetLastError();
  return e ? hip_fail(e, "ppograd_reduce_kernel launch") : PBG_OK;
}

}  // namespace

extern "C" {

int pbg_ppo_grad_create(int device, int obs_dim, int h1, int h2, int act_dim, int max_rows, pbg_ppo_grad** out) {
  if (!out) return pbg::capi_fail(PBG_E_ARG, "pbg_ppo_grad_create: out is NULL");
  *out = nullptr;
  return create_object("pbg_ppo_grad_create", device, obs_dim, h1, h2, act_dim, max_rows, PBG_PPO_GRAD_FMA, MAX_WG, out);
}

int pbg_ppo_grad_create_ex(int device, int obs_dim, int h1, int h2, int act_dim, int max_rows, const pbg_ppo_grad_opts_t* opts,
                           pbg_ppo_grad** out) {
  if (!out) return pbg::capi_fail(PBG_E_ARG, "pbg_ppo_grad_create_ex: out is NULL");
  *out = nullptr;
  int path = PBG_PPO_GRAD_FMA;
  if (opts) {
    char msg[128];
    if (opts->struct_size != (uint32_t)sizeof(pbg_ppo_grad_opts_t)) {
      snprintf(msg, sizeof(msg), "pbg_ppo_grad_create_ex: opts->struct_size %u is not a pbg_ppo_grad_opts_t size",
               opts->struct_size);
      return pbg::capi_fail(PBG_E_ARG, msg);
    }
    path = opts->path;
    if (path != PBG_PPO_GRAD_FMA && path != PBG_PPO_GRAD_MFMA) {
      snprintf(msg, sizeof(msg), "pbg_ppo_grad_create_ex: opts->path %d is neither PBG_PPO_GRAD_FMA nor PBG_PPO_GRAD_MFMA", path);
      return pbg::capi_fail(PBG_E_ARG, msg);
    }
  }
  if (path == PBG_PPO_GRAD_FMA)
    return create_object("pbg_ppo_grad_create", device, obs_dim, h1, h2, act_dim, max_rows, path, MAX_WG, out);
  return create_object("pbg_ppo_grad_create_ex", device, obs_dim, h1, h2, act_dim, max_rows, path, MFMA_MAX_WG, out);
}

void pbg_ppo_grad_destroy(pbg_ppo_grad* g) {
  if (!g) return;
  if (g->part_stats) {
    DeviceGuard dg(g->device);
    (void)hipFree(g->part_stats);
  }
  delete g;
}

int pbg_ppo_grad_run(pbg_ppo_grad* g, const pbg_ppo_grad_io_t* uio, void* stream) {
  if (!g) return pbg::capi_fail(PBG_E_ARG, "pbg_ppo_grad_run: the object is NULL");
  pbg_ppo_grad_io_t io;
  if (const int rc = check_io("pbg_ppo_grad_run", uio, &io)) return rc;
  if (const int rc = check_rows("pbg_ppo_grad_run", g, io.mb_rows)) return rc;
  DeviceGuard dg(g->device);
  hipStream_t s = (hipStream_t)stream;
  const int G = workgroups_of(g, io.mb_rows);
  if (const int rc = launch_tiles(g, io, 0, G, G, g->part, g->part_stats, s)) return rc;
  return launch_reduce(g, io, G, g->part, g->part_stats, s);
}

int pbg_ppo_grad_geometry(const pbg_ppo_grad* g, int mb_rows, int* G_out, int64_t* dtot_out) {
  if (!g || !G_out || !dtot_out) return pbg::capi_fail(PBG_E_ARG, "pbg_ppo_grad_geometry: NULL object, G_out or dtot_out");
  if (mb_rows < 1) return pbg::capi_fail(PBG_E_ARG, "pbg_ppo_grad_geometry: mb_rows must be >= 1");
  if (const int rc = check_rows("pbg_ppo_grad_geometry", g, mb_rows)) return rc;
  *G_out = workgroups_of(g, mb_rows);
  *dtot_out = (int64_t)g->Dtot;
  return PBG_OK;
}

int pbg_ppo_grad_run_part(pbg_ppo_grad* g, const pbg_ppo_grad_io_t* uio, int wg_first, int wg_count, float* part_out,
                          double* part_stats_out, void* stream) {
  if (!g) return pbg::capi_fail(PBG_E_ARG, "pbg_ppo_grad_run_part: the object is NULL");
  pbg_ppo_grad_io_t io;
  if (const int rc = check_io("pbg_ppo_grad_run_part", uio, &io, true, false)) return rc;
  if (const int rc = check_rows("pbg_ppo_grad_run_part", g, io.mb_rows)) return rc;
  const int G = workgroups_of(g, io.mb_rows);
  char msg[160];
  if (wg_first < 0 || wg_count < 0 || (long long)wg_first + wg_count > (long long)G) {
    snprintf(msg, sizeof(msg), "pbg_ppo_grad_run_part: workgroups %d .. %d + %d are outside 0 .. %d", wg_first, wg_first, wg_count,
             G);
    return pbg::capi_fail(PBG_E_ARG, msg);
  }
  if (wg_count == 0) return PBG_OK;
  if (!part_out || !part_stats_out) return pbg::capi_fail(PBG_E_ARG, "pbg_ppo_grad_run_part: NULL part_out or part_stats_out");
  DeviceGuard dg(g->device);
  return launch_tiles(g, io, wg_first, wg_count, G, part_out, part_stats_out, (hipStream_t)stream);
}

int pbg_ppo_grad_reduce(pbg_ppo_grad* g, const pbg_ppo_grad_io_t* uio, int G, const float* part, const double* part_stats,
                        void* stream) {
  if (!g) return pbg::capi_fail(PBG_E_ARG, "pbg_ppo_grad_reduce: the object is NULL");
  pbg_ppo_grad_io_t io;
  if (const int rc = check_io("pbg_ppo_grad_reduce", uio, &io, false, true)) return rc;
  if (const int rc = check_rows("pbg_ppo_grad_reduce", g, io.mb_rows)) return rc;
  if (G != workgroups_of(g, io.mb_rows)) {
    char msg[160];
    snprintf(msg, sizeof(msg), "pbg_ppo_grad_reduce: G %d is not the %d workgroups of mb_rows %d", G, workgroups_of(g, io.mb_rows),
             io.mb_rows);
    return pbg::capi_fail(PBG_E_ARG, msg);
  }
  if (!part || !part_stats) return pbg::capi_fail(PBG_E_ARG, "pbg_ppo_grad_reduce: NULL part or part_stats");
  DeviceGuard dg(g->device);
  return launch_reduce(g, io, G, part, part_stats, (hipStream_t)stream);
}

int pbg_ppo_grad_host(int obs_dim, int h1, int h2, int act_dim, const pbg_ppo_grad_io_t* uio) {
  if (const int rc = check_dims("pbg_ppo_grad_host", obs_dim, h1, h2, act_dim)) return rc;
  pbg_ppo_grad_io_t io;
  if (const int rc = check_io("pbg_ppo_grad_host", uio, &io)) return rc;
  const int A = act_dim, Bm = io.mb_rows;
  if (io.idx)
    for (int i = 0; i < Bm; i++)
      if (io.idx[i] < 0 || io.idx[i] >= (int64_t)io.batch_rows)
        return pbg::capi_fail(PBG_E_ARG, "pbg_ppo_grad_host: an index is outside 0 .. batch_rows - 1");
  if (io.gate && io.gate[0] != 0) return PBG_OK;  // stopped: the outputs keep what they held
  const int Da = param_count(obs_dim, h1, h2, A), Dc = param_count(obs_dim, h1, h2, 1);
  double* acc = (double*)calloc((size_t)Da + Dc + A, sizeof(double));
  if (!acc) return pbg::capi_fail(PBG_E_NOMEM, "pbg_ppo_grad_host: out of host memory");
  const Weights P[2] = {weights_at(io.theta_actor, obs_dim, h1, h2, A), weights_at(io.theta_critic, obs_dim, h1, h2, 1)};
  double* base[2] = {acc, acc + Da};
  double* gls = acc + Da + Dc;
  double inv_sig[NA_MAX], sum_ls = 0.0;
  for (int j = 0; j < A; j++) {
    inv_sig[j] = exp(-(double)io.log_std[j]);
    sum_ls += (double)io.log_std[j];
  }
  const double inv_bm = 1.0 / (double)Bm;
  double st[4] = {0.0, 0.0, 0.0, 0.0};
  float x[PD], a1[PD], a2[PD], dy[PD], dls[NA_MAX], d2[PD], d1[PD];
  double x64[PD], a64[PD], b64[PD];
  for (int i = 0; i < Bm; i++) {
    const size_t r = io.idx ? (size_t)io.idx[i] : (size_t)i;
    const float* o = io.obs + r * obs_dim;
    for (int k = 0; k < obs_dim; k++) x[k] = io.mean ? normalise(o[k], io.mean[k], io.inv_std[k], io.clip) : o[k];
    for (int net = 0; net < 2; net++) {
      const Weights& W = P[net];
      const int NA = W.act_dim;
      host_layer(W.w1, W.b1, obs_dim, h1, true, x, a1);
      host_layer(W.w2, W.b2, h1, h2, true, a1, a2);
      host_layer(W.w3, W.b3, h2, NA, false, a2, dy);
      if (net == 0) {
        double ahat = (double)io.adv[r];
        if (io.adv_norm) ahat = (ahat - (double)io.adv_norm[0]) * (double)io.adv_norm[1];
        // the statistics' float64 forward
        for (int k = 0; k < obs_dim; k++)
          x64[k] = io.mean ? normalise64(o[k], io.mean[k], io.inv_std[k], io.clip) : (double)o[k];
        host_layer64(W.w1, W.b1, obs_dim, h1, true, x64, a64);
        host_layer64(W.w2, W.b2, h1, h2, true, a64, b64);
        host_layer64(W.w3, W.b3, h2, A, false, b64, x64);
        double s[3];
        ppo_stats_row(A, x64, 1, io.act + r * A, inv_sig, sum_ls, (double)io.logp_old[r], ahat, (double)io.clip_eps, s);
        const double logp = ppo_actor_row(A, dy, dls, 1, io.act + r * A, inv_sig, sum_ls, (double)io.logp_old[r], ahat,
                                          (double)io.clip_eps, inv_bm);
        st[0] += s[0];
        st[2] += s[1];
        st[3] += s[2];
        if (io.logp_out) io.logp_out[i] = (float)logp;
        for (int j = 0; j < A; j++) gls[j] += (double)dls[j];
      } else {
        double vf;
        const float v = dy[0];
        dy[0] = ppo_critic_row(v, io.ret[r], io.value_old ? io.value_old + r : nullptr, (double)io.vf_clip, (double)io.vf_coef,
                               inv_bm, &vf);
        st[1] += vf;
        if (io.v_out) io.v_out[i] = v;
      }
      // the flat layout's offsets inside this network's block of acc
      double* g1 = base[net];
      double* gb1 = g1 + (W.b1 - W.w1);
      double* g2 = g1 + (W.w2 - W.w1);
      double* gb2 = g1 + (W.b2 - W.w1);
      double* g3 = g1 + (W.w3 - W.w1);
      double* gb3 = g1 + (W.b3 - W.w1);
      for (int j = 0; j < NA; j++) gb3[j] += (double)dy[j];
      for (int k = 0; k < h2; k++) {
        float s = 0.f;
        for (int j = 0; j < NA; j++) {
          g3[(size_t)k * NA + j] += (double)a2[k] * (double)dy[j];
          s = __builtin_fmaf(dy[j], W.w3[(size_t)k * NA + j], s);
        }
        d2[k] = a2[k] > 0.f ? s : 0.f;
      }
      for (int j = 0; j < h2; j++) gb2[j] += (double)d2[j];
      for (int k = 0; k < h1; k++) {
        float s = 0.f;
        for (int j = 0; j < h2; j++) {
          g2[(size_t)k * h2 + j] += (double)a1[k] * (double)d2[j];
          s = __builtin_fmaf(d2[j], W.w2[(size_t)k * h2 + j], s);
        }
        d1[k] = a1[k] > 0.f ? s : 0.f;
      }
      for (int j = 0; j < h1; j++) gb1[j] += (double)d1[j];
      for (int k = 0; k < obs_dim; k++)
        for (int j = 0; j < h1; j++) g1[(size_t)k * h1 + j] += (double)x[k] * (double)d1[j];
    }
  }
  for (int d = 0; d < Da; d++) io.grad_actor[d] = (float)acc[d];
  for (int d = 0; d < Dc; d++) io.grad_critic[d] = (float)acc[Da + d];
  for (int j = 0; j < A; j++) io.grad_log_std[j] = (float)(gls[j] - (double)io.ent_coef);
  for (int t = 0; t < 4; t++) io.stats[t] = st[t] / (double)Bm;
  free(acc);
  return PBG_OK;
}

}  // extern "C"
