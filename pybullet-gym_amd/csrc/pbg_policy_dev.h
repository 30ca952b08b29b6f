// pbg_policy_dev.h -- what the actor translation units (pbg_policy.hip, pbg_population.hip, pbg_obsnorm.hip,
// pbg_actnoise.hip) and the PPO gradient (pbg_ppograd.hip: `layer`, `normalise`, host_layer and the per-row loss
// derivative and statistics ppo_actor_row / ppo_critic_row / ppo_stats_row) share: the description of an actor (Actor: a pbg_policy is one with
// a single member whose group is the whole batch, a pbg_population one with 2 n_pairs), the MLP tile that
// pbg_policy.hip's actor_kernel
// evaluates with the workgroup's member's weights, the rollout bookkeeping, the one actor launch and the
// rollout loop (pbg_rollout and pbg_rollout_population are the same 2 T + 1 launches), and the host helpers
// of the three objects.
//
// Numeric contract (pbg.h): out[j] = fmaf-chain over k ascending, started from b[j]; ReLU as
// `v < 0 ? 0 : v`.  One fma per (k, j, env), nothing split over k, nothing left for the compiler to
// contract.
//
// Geometry (DESIGN.md "Policy kernel"): a workgroup of 256 lanes owns a tile of 16 envs.  Inside a
// layer a lane owns one output column j and EL of the tile's envs: its weight reads W[k][j] are
// coalesced over the lanes (the reference's row-major [K, H] layout as is) and the activations
// x[k][e0 .. e0 + EL) are wave-uniform float4 LDS broadcasts.  A layer of H <= 64 columns splits the
// 16 envs over the four waves (EL = 4), H <= 128 over two wave pairs (EL = 8), wider layers give
// every lane all 16: no wave idles through a narrow layer.
//
// Observation normalisation and statistics (pbg.h "Running observation normalisation", DESIGN.md section
// 12): normalise() is the one spelling of the transform, host and device; stats_tile() the one spelling of
// the tile accumulation, used by the actor and by pbg_obsnorm.hip's stand-alone kernel.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include "pbg_es_noise.h"
#include "pbg_internal.h"

namespace pbg {
namespace policy {

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

struct Weights {
  const float *w1, *b1, *w2, *b2, *w3, *b3;
  int obs_dim, h1, h2, act_dim;
};

// pbg.h "Flat parameter layout": a weight set is the unpadded concatenation w1 b1 w2 b2 w3 b3 from `base`
// (layer_cols reads one float per lane, so no array needs an alignment), host or device
__host__ __device__ __forceinline__ Weights weights_at(const float* base, int obs_dim, int h1, int h2, int act_dim) {
  Weights W;
  W.obs_dim = obs_dim; W.h1 = h1; W.h2 = h2; W.act_dim = act_dim;
  W.w1 = base;
  W.b1 = W.w1 + obs_dim * h1;
  W.w2 = W.b1 + h1;
  W.b2 = W.w2 + h1 * h2;
  W.w3 = W.b2 + h2;
  W.b3 = W.w3 + h2 * act_dim;
  return W;
}

// D, the floats of one weight set: where weights_at's last array ends
inline int param_count(int obs_dim, int h1, int h2, int act_dim) {
  return obs_dim * h1 + h1 + h1 * h2 + h2 + h2 * act_dim + act_dim;
}

// an actor's normaliser: mean, inv_std [obs_dim] (device pointers in a kernel); mean NULL = none
struct Norm {
  const float* mean;
  const float* inv_std;
  float clip;
};

// pbg.h's transform: a subtraction and a multiply, one float32 rounding each (the subtraction feeds the
// multiply, so there is nothing to contract), then the clamp as two comparisons: a NaN passes through
__host__ __device__ __forceinline__ float normalise(float x, float mean, float inv_std, float clip) {
  const float d = x - mean;
  const float v = d * inv_std;
  return v < -clip ? -clip : (v > clip ? clip : v);
}

// one workgroup's slot of a pbg_obs_stats (sum NULL = nothing is collected)
struct Slot {
  int64_t* count;
  double* sum;    // [K]
  double* sumsq;  // [K]
};

// An actor: n_members weight sets of one MLP shape on one device, the normaliser they share and the
// statistics attached to them.  A launch over n rows cuts them into n_members groups of G = n / n_members
// consecutive rows, group m runs member m (a pbg_policy: one member, G = n).
struct Actor {
  int device;  // -1: host only (a pbg_policy), nothing below `D` is allocated
  int obs_dim, h1, h2, act_dim;
  int n_members;
  int D;          // parameters per member
  float* params;  // device [n_members, D], each row in the flat layout
  // the normaliser (pbg_*_set_obs_norm): device mean [obs_dim] then inv_std [obs_dim], allocated with the
  // parameters; norm_on 0 = none
  float* norm;
  float clip;
  int norm_on;
  pbg_obs_stats* stats;  // attached (pbg_*_attach_obs_stats), not owned
  pbg_action_noise* noise;  // attached (pbg_*_attach_action_noise), not owned
};

// The action noise of one actor launch (pbg.h "Stochastic Gaussian actions"); std NULL = the launch does
// not sample.  The lanes read the object's device step counter and add `step`, the launch's own.
struct Noise {
  const float* std;         // device [act_dim]
  const uint32_t* counter;  // device: the steps sampled before this rollout call
  double* eps2;             // device [n]: this step's row of eps2_traj, nullable
  uint32_t k0, k1;          // the seed
  uint32_t env_offset;      // global index of the launch's row 0
  uint32_t step;            // s, the step inside the call
};

// slot b of the object whose slot 0 is `base` (K = obs_dim)
__host__ __device__ __forceinline__ Slot slot_at(const Slot base, int K, unsigned b) {
  if (!base.sum) return base;
  return Slot{base.count + b, base.sum + (size_t)b * K, base.sumsq + (size_t)b * K};
}

// The flags of a tile while statistics are collected, PT ints each: [0] the row is active, [1 + w] wave w
// of the workgroup met a non-finite component of the row while loading it.  A flag plane per wave needs no
// zeroing barrier: a wave's LDS stores retire in program order, so its lanes 0 .. PT - 1 clear the wave's
// plane and the loads that follow in the same wave set it.  The flags live at the start of the
// workgroup's second LDS plane, which is idle until the first layer writes it.
constexpr int WAVE = 64;  // gfx950
constexpr int FLAG_WORDS = PT * (1 + PB / WAVE);
static_assert(FLAG_WORDS <= PD * PT, "the flags fit the idle plane");

__device__ __forceinline__ bool finite_bits(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

// The tile's observations (rows * K0 contiguous floats from row env0) -> xT [K0][PT], zero past `rows`,
// with a copy into obs_traj (nullable) of what was read.  nm.mean != NULL: the normalised value is stored.
// fl != NULL: the per-wave non-finite flags are written (the caller has written the active flags fl[0 .. PT)).
__device__ __forceinline__ void load_tile(int K0, int env0, int rows, const float* __restrict__ obs,
                                          float* __restrict__ obs_traj, const Norm nm, float* xT, int* fl) {
  const int tid = threadIdx.x;
  int* nf = fl ? fl + PT * (1 + tid / WAVE) : nullptr;
  if (nf && (tid & (WAVE - 1)) < PT) nf[tid & (WAVE - 1)] = 0;
  for (int i = tid; i < PT * K0; i += PB) {
    const int e = i / K0, k = i - e * K0;
    float v = 0.f;
    if (e < rows) {
      const size_t at = (size_t)env0 * K0 + i;
      v = obs[at];
      if (obs_traj) obs_traj[at] = v;
      if (nf && !finite_bits(v)) nf[e] = 1;
      if (nm.mean) v = normalise(v, nm.mean[k], nm.inv_std[k], nm.clip);
    }
    xT[k * PT + e] = v;
  }
}

// pbg.h's tile accumulation: lane k < K walks the PT rows of its column of the raw tile xT [K][PT] in
// ascending order and adds every counted (active and finite) row straight onto the slot's running values;
// lane 0 also adds the number of counted rows.  Call between the barrier after load_tile and the next one.
__device__ __forceinline__ void stats_tile(const Slot s, int K, const float* xT, const int* fl) {
  const int tid = threadIdx.x;
  if (tid >= K) return;
  unsigned counted = 0;
#pragma unroll
  for (int e = 0; e < PT; e++) {
    int bad = 0;
#pragma unroll
    for (int w = 0; w < PB / WAVE; w++) bad |= fl[PT * (1 + w) + e];
    counted |= (fl[e] != 0 && bad == 0 ? 1u : 0u) << e;
  }
  double a = s.sum[tid], q = s.sumsq[tid];
#pragma unroll
  for (int e = 0; e < PT; e++)
    if ((counted >> e) & 1u) {
      const double x = (double)xT[tid * PT + e];
      a += x;
      q += x * x;  // exact product: the same bits contracted or not
    }
  s.sum[tid] = a;
  s.sumsq[tid] = q;
  if (tid == 0) *s.count += (int64_t)__popc(counted);
}

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

// One workgroup's tile: envs env0 .. env0 + rows (1 <= rows <= PT) with the weights P.
// act[e] = pi(obs[e]), through the normaliser nm when it has one; optional copies of the raw observation
// and the action into the rollout's trajectories; the bookkeeping of the previous env step (bk.rew64 !=
// NULL) for the tile's envs comes first.  Rows past `rows` are zero-filled in LDS and neither read from nor
// written to memory.  bufA / bufB: the workgroup's two [PD][PT] LDS planes.
// MODE picks the instantiation, so that the plain path stays the code it was before normalisers existed:
// PLAIN: nm and st are ignored.  NORM (nm.mean != NULL): the transform is applied as the tile is stored.
// COLLECT (a rollout step with statistics attached, st.sum != NULL; nm.mean may be NULL): the tile is stored
// raw, lane k adds its column to the slot and then normalises that same column in place, which costs one
// more barrier than NORM.  NORM and COLLECT give the same bits.
enum Mode { PLAIN = 0, NORM = 1, COLLECT = 2 };

inline Mode mode_of(const Norm& nm, const Slot& st) { return st.sum ? COLLECT : (nm.mean ? NORM : PLAIN); }

// The four normals of action components 4 b .. 4 b + 3 of the global env `env` at step count `step`: the
// one spelling the sampling actor and pbg_actnoise.hip's fill kernel share (pbg.h's same-bits rule).
__device__ __forceinline__ void action_normals4(uint32_t k0, uint32_t k1, uint32_t b, uint32_t env, uint32_t step,
                                                float z[4]) {
  pbg::es::es_normals4(k0, k1, b, env, step, pbg::es::ACTION_TAG, z);
}

// SAMPLE (a rollout step with action noise attached, nz.std != NULL): after the third layer mu sits transposed
// in bufB and bufA is idle.  Lane (e = tid % PT, b = tid / PT) draws the block of components 4 b .. 4 b + 3 of
// row e into bufA [act_dim][PT]; after one more barrier lane e < rows sums its row's squares in ascending j and
// the output loop adds std[j] eps to mu in float64.  PT rows x 16 blocks = PB lanes: one pass.
static_assert((PB / PT) * 4 >= PBG_POLICY_MAX_ACT, "a lane per (row, block of 4 components)");

template <int MODE, bool SAMPLE>
__device__ __forceinline__ void act_tile(const Weights P, const Norm nm, const Slot st, const Noise nz, int env0, int rows,
                                         const float* __restrict__ obs, float* __restrict__ act,
                                         float* __restrict__ obs_traj, float* __restrict__ act_traj, const Book bk,
                                         float* bufA, float* bufB) {
  const int tid = threadIdx.x;
  if (bk.rew64 && tid < rows) book_env(bk, env0 + tid);

  const int K0 = P.obs_dim;
  if (MODE == COLLECT) {
    int* fl = reinterpret_cast<int*>(bufB);
    // active: the action computed from this row will be booked (this lane did the row's bookkeeping above)
    if (tid < PT) fl[tid] = tid < rows && (bk.autoreset || bk.done_episodes[env0 + tid] == 0) ? 1 : 0;
    load_tile(K0, env0, rows, obs, obs_traj, Norm{nullptr, nullptr, 0.f}, bufA, fl);
    __syncthreads();
    stats_tile(st, K0, bufA, fl);
    if (nm.mean && tid < K0) {
      const float mean = nm.mean[tid], inv_std = nm.inv_std[tid];
      for (int e = 0; e < rows; e++) bufA[tid * PT + e] = normalise(bufA[tid * PT + e], mean, inv_std, nm.clip);
    }
  } else {
    load_tile(K0, env0, rows, obs, obs_traj, MODE == NORM ? nm : Norm{nullptr, nullptr, 0.f}, bufA, nullptr);
  }
  __syncthreads();
  layer(P.w1, P.b1, K0, P.h1, true, bufA, bufB);
  __syncthreads();
  layer(P.w2, P.b2, P.h1, P.h2, true, bufB, bufA);
  __syncthreads();
  layer(P.w3, P.b3, P.h2, P.act_dim, false, bufA, bufB);
  __syncthreads();
  const int NA = P.act_dim;
  if (SAMPLE) {
    const int e = tid & (PT - 1), b = tid / PT;
    if (e < rows && 4 * b < NA) {
      float z[4];
      action_normals4(nz.k0, nz.k1, (uint32_t)b, nz.env_offset + (uint32_t)(env0 + e), *nz.counter + nz.step, z);
#pragma unroll
      for (int t = 0; t < 4; t++)
        if (4 * b + t < NA) bufA[(4 * b + t) * PT + e] = z[t];
    }
    __syncthreads();
    if (nz.eps2 && tid < rows) {
      double q = 0.0;
      for (int j = 0; j < NA; j++) {
        const double x = (double)bufA[j * PT + tid];
        q += x * x;  // exact product: the same bits contracted or not
      }
      nz.eps2[env0 + tid] = q;
    }
  }
  for (int i = tid; i < rows * NA; i += PB) {
    const int e = i / NA, j = i - e * NA;
    float v = bufB[j * PT + e];
    if (SAMPLE) v = (float)((double)v + (double)nz.std[j] * (double)bufA[j * PT + e]);  // exact product, one rounding
    const size_t at = (size_t)env0 * NA + i;
    act[at] = v;
    if (act_traj) act_traj[at] = v;
  }
}

// the contract's chain on the CPU (pbg_policy_act_host, pbg_ppo_grad_host): y[j] = fmaf chain over k ascending
// from the bias
inline void host_layer(const float* W, const float* b, int K, int H, bool relu, const float* x, float* y) {
  for (int j = 0; j < H; j++) y[j] = b[j];
  for (int k = 0; k < K; k++) {
    const float xk = x[k];
    const float* w = W + (size_t)k * H;
    for (int j = 0; j < H; j++) y[j] = __builtin_fmaf(xk, w[j], y[j]);
  }
  if (relu)
    for (int j = 0; j < H; j++) y[j] = y[j] < 0.f ? 0.f : y[j];
}

// pbg.h "PPO gradient": the per-row loss derivative and the row's terms of `stats`, host and device, float64.
// logp of a row from its means mu[j * stride] (float: the contract's forward; double: the statistics' forward):
// inv_sig[j] = exp(-log_std_j), sum_ls = sum_j log_std_j (j ascending)
template <typename T>
__host__ __device__ __forceinline__ double ppo_logp_row(int A, const T* mu, int stride, const float* __restrict__ act_row,
                                                        const double* inv_sig, double sum_ls) {
  double q = 0.0;
  for (int j = 0; j < A; j++) {
    const double z = ((double)act_row[j] - (double)mu[j * stride]) * inv_sig[j];
    q += z * z;
  }
  return -0.5 * q - sum_ls - 0.5 * (double)A * 1.8378770664093453;  // log 2 pi
}

// The actor's row: mu[j * stride] (j < A) holds the row's float32 means and takes dL/dmu_j in their place,
// dls[j * stride] takes the row's term of dL/dlog_std_j; ahat the (normalised) advantage, c = clip_eps,
// inv_bm = 1 / Bm.  Returns logp.
__host__ __device__ __forceinline__ double ppo_actor_row(int A, float* mu, float* dls, int stride,
                                                         const float* __restrict__ act_row, const double* inv_sig,
                                                         double sum_ls, double logp_old, double ahat, double c, double inv_bm) {
  const double logp = ppo_logp_row(A, mu, stride, act_row, inv_sig, sum_ls);
  const double ratio = exp(logp - logp_old);
  const double lo = 1.0 - c, hi = 1.0 + c;
  const double s1 = ratio * ahat, s2 = (ratio < lo ? lo : (ratio > hi ? hi : ratio)) * ahat;
  const double dlogp = s1 <= s2 ? -(ahat * ratio) * inv_bm : 0.0;
  for (int j = 0; j < A; j++) {
    const double z = ((double)act_row[j] - (double)mu[j * stride]) * inv_sig[j];
    mu[j * stride] = (float)(dlogp * z * inv_sig[j]);
    dls[j * stride] = (float)(dlogp * (z * z - 1.0));
  }
  return logp;
}

// The row's terms of (pg loss, clipped, logp_old - logp) from the float64 means mu64[j * stride]: the last is a
// mean of cancelling terms, which the float32 forward's rounding would leave with three digits.
__host__ __device__ __forceinline__ void ppo_stats_row(int A, const double* mu64, int stride, const float* __restrict__ act_row,
                                                       const double* inv_sig, double sum_ls, double logp_old, double ahat,
                                                       double c, double st[3]) {
  const double logp = ppo_logp_row(A, mu64, stride, act_row, inv_sig, sum_ls);
  const double ratio = exp(logp - logp_old);
  const double lo = 1.0 - c, hi = 1.0 + c;
  const double s1 = ratio * ahat, s2 = (ratio < lo ? lo : (ratio > hi ? hi : ratio)) * ahat;
  st[0] = -(s1 < s2 ? s1 : s2);
  st[1] = (ratio - 1.0 > c || 1.0 - ratio > c) ? 1.0 : 0.0;
  st[2] = logp_old - logp;
}

// The statistics' forward (pbg.h "PPO gradient"): the contract's transform and chain in float64, host and device.
__host__ __device__ __forceinline__ double normalise64(float x, float mean, float inv_std, float clip) {
  const double v = ((double)x - (double)mean) * (double)inv_std, c = (double)clip;
  return v < -c ? -c : (v > c ? c : v);
}

// y[j] = fma chain over k ascending from the bias, float64 from the float32 parameters
inline void host_layer64(const float* W, const float* b, int K, int H, bool relu, const double* x, double* y) {
  for (int j = 0; j < H; j++) y[j] = (double)b[j];
  for (int k = 0; k < K; k++) {
    const double xk = x[k];
    const float* w = W + (size_t)k * H;
    for (int j = 0; j < H; j++) y[j] = __builtin_fma(xk, (double)w[j], y[j]);
  }
  if (relu)
    for (int j = 0; j < H; j++) y[j] = y[j] < 0.0 ? 0.0 : y[j];
}

// The critic's row: dL/dv; *vf takes the row's term of the value loss.  value_old_r NULL: the plain squared error.
// Otherwise pbg.h "Value clipping" with e = vf_clip: the larger of the squared errors of v and of v clamped to
// *value_old_r +- e, and the derivative of the unclipped one where it is the larger or the two tie, else zero.
__host__ __device__ __forceinline__ float ppo_critic_row(float v, float ret, const float* value_old_r, double e, double vf_coef,
                                                         double inv_bm, double* vf) {
  const double d = (double)v - (double)ret;
  if (!value_old_r) {
    *vf = 0.5 * d * d;
    return (float)(vf_coef * d * inv_bm);
  }
  {
#pragma clang fp contract(off)
    const double vo = (double)*value_old_r;
    const double dv = (double)v - vo;
    const double vc = dv < -e ? vo - e : (dv > e ? vo + e : (double)v);  // inside the range v itself: u2 == u1 exactly
    const double dc = vc - (double)ret;
    const double u1 = d * d, u2 = dc * dc;
    const bool own = u1 >= u2;
    *vf = 0.5 * (own ? u1 : u2);
    return own ? (float)(vf_coef * d * inv_bm) : 0.f;
  }
}

// pbg.h's advantage scan for env e, host and device (pbg_actnoise.hip: pbg_gae; pbg_trunc.hip: pbg_gae_trunc): float64,
// nothing contracted; gl = gamma * lambda.  TRUNC: pbg_gae_trunc's lines (trunc, term_value: its arrays); without it
// neither is looked at, so pbg_gae's instantiation is the loop it was before truncations were recorded.
template <bool TRUNC>
__host__ __device__ __forceinline__ void gae_env(int T, int n, int e, const float* __restrict__ rew,
                                                 const uint8_t* __restrict__ done, const uint8_t* __restrict__ trunc,
                                                 const float* __restrict__ value, const float* __restrict__ term_value,
                                                 double gamma, double gl, float* __restrict__ adv, float* __restrict__ ret) {
#pragma clang fp contract(off)
  double A = 0.0;
  double vnext = (double)value[(size_t)T * n + e];
  for (int t = T - 1; t >= 0; t--) {
    const size_t at = (size_t)t * n + e;
    const double nd = done[at] ? 0.0 : 1.0;
    const double v = (double)value[at];
    double vn = vnext, nb = nd;
    if (TRUNC && trunc[at] != 0) {
      vn = (double)term_value[at];
      nb = 1.0;
    }
    const double delta = ((double)rew[at] + (gamma * vn) * nb) - v;
    A = delta + (gl * nd) * A;
    adv[at] = (float)A;
    ret[at] = (float)(A + v);
    vnext = v;
  }
}

// workgroups (= slots) of an actor launch over n rows in groups of G (n a multiple of G > 0)
inline long long tiles_of(int n, int G) { return (long long)(n / G) * ((G + PT - 1) / PT); }

// Workgroup b of such a launch, tpm = ceil(G / PT) tiles per group: tile t = b % tpm of group m = b / tpm owns
// rows row0 = m G + t PT .. row0 + rows; the last tile of a group whose G is no multiple of PT has fewer rows.
struct Tile {
  int m, row0, rows;
};

__device__ __forceinline__ Tile tile_of(unsigned b, int G, int tpm) {
  const int m = b / (unsigned)tpm, t = b - m * tpm;  // unsigned: no sign fix-up around the uniform division
  return Tile{m, m * G + t * PT, min(PT, G - t * PT)};
}

// The one actor launch (pbg_policy.hip): act = pi_m(obs) for n rows (n > 0, a multiple of a.n_members) after
// the bookkeeping `bk`, enqueued on `stream`; returns the hipError_t of the launch.
// `collect`: accumulate the actor's attached statistics (rollout steps only; the loop has validated them).
// `nz`: the launch's action noise (rollout steps only; std NULL, a Noise{}: none).
int launch_actor(const Actor& a, int n, const float* obs, float* act, float* obs_traj, float* act_traj, const Book& bk,
                 bool collect, const Noise& nz, hipStream_t stream);

// The closed loop of pbg_rollout / pbg_rollout_population (pbg_policy.hip): validates `io` against the
// handle and the actor's device and dims (the handle's n_envs a multiple of the actor's members; attached
// statistics on the actor's device, of its obs_dim and with a slot per workgroup; attached action noise on the
// actor's device and of its act_dim), then enqueues per step the actor and the handle's step, and one closing
// bookkeeping launch, which also advances the attached noise's step counter.  `who` names the entry point in
// error messages.
int rollout_loop(const char* who, pbg_handle* h, const pbg_rollout_io_t* io, void* stream, const Actor& a);

// ---------------------------------------------------------------- host helpers of the three objects
inline int hip_fail(int e, const char* what) {
  char msg[160];
  snprintf(msg, sizeof(msg), "%s: HIP error %d", what, e);
  return pbg::capi_fail(PBG_E_HIP, msg);
}

// PBG_OK when the launch just enqueued left no error behind; `what` names it in the message
inline int launched(const char* what) {
  const int e = (int)hipGetLastError();
  return e ? hip_fail(e, what) : PBG_OK;
}

// PBG_OK when HIP device `device` exists
inline int check_device(const char* who, int device) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) == hipSuccess && device < ndev) return PBG_OK;
  (void)hipGetLastError();
  char msg[96];
  snprintf(msg, sizeof(msg), "%s: no HIP device %d", who, device);
  return pbg::capi_fail(PBG_E_HIP, msg);
}

// PBG_OK when the four dims are inside pbg_policy_create's ranges
inline int check_dims(const char* who, int obs_dim, int h1, int h2, int act_dim) {
  if (obs_dim >= 1 && obs_dim <= PBG_POLICY_MAX_DIM && h1 >= 1 && h1 <= PBG_POLICY_MAX_DIM && h2 >= 1 &&
      h2 <= PBG_POLICY_MAX_DIM && act_dim >= 1 && act_dim <= PBG_POLICY_MAX_ACT)
    return PBG_OK;
  char msg[200];
  snprintf(msg, sizeof(msg), "%s: dims (%d, %d, %d, %d) outside 1..%d (obs_dim, h1, h2), 1..%d (act_dim)", who, obs_dim, h1,
           h2, act_dim, PBG_POLICY_MAX_DIM, PBG_POLICY_MAX_ACT);
  return pbg::capi_fail(PBG_E_ARG, msg);
}

// An actor's dims, member count and (zeroed) device storage; device < 0: the dims only.  PBG_OK, or the
// failure with nothing left allocated.
int actor_init(const char* who, Actor& a, int device, int obs_dim, int h1, int h2, int act_dim, int n_members);
void actor_free(Actor& a);

// What both pbg_*_set_obs_norm check before they copy: 1 = both arrays NULL, the normaliser is now off;
// 0 = go on: copy them, then set a.clip and a.norm_on; < 0 = refused
int norm_args(const char* who, Actor& a, const float* mean, const float* inv_std, float clip);

}  // namespace policy
}  // namespace pbg

// pbg.h pbg_obs_stats: one device allocation of 8-byte words, totals [1 + 2 K] | slot_sum [n_slots, K] |
// slot_sumsq [n_slots, K] | slot_count [n_slots] (pbg_obsnorm.hip owns it; the actors read the pointers)
struct pbg_obs_stats {
  int device, obs_dim, n_slots;
  double* totals;
  double* slot_sum;
  double* slot_sumsq;
  int64_t* slot_count;

  pbg::policy::Slot slot0() const { return pbg::policy::Slot{slot_count, slot_sum, slot_sumsq}; }
};

// pbg.h pbg_population: an Actor of 2 n_pairs members (a.params: member m's vector at m D) and the global index of
// its first pair (pbg_population.hip owns it; pbg_trunc.hip's masked launch reads the actor)
struct pbg_population {
  pbg::policy::Actor a;
  int n_pairs, pair0;
};

// pbg.h pbg_action_noise: one device allocation, std [act_dim] float32 then the uint32 step counter
// (pbg_actnoise.hip owns it; the rollout loop reads the pointers)
struct pbg_action_noise {
  int device, act_dim;
  uint64_t seed;
  float* std;
  uint32_t* counter;
  double* eps2_traj;  // device [T, n] of the next rollouts, nullable; not owned
};
