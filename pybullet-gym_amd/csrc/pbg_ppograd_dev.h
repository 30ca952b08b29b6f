// pbg_ppograd_dev.h -- what the two tile kernels of the PPO gradient share (pbg_ppograd.hip: the FMA path, the
// object, the reduction and the host twin; pbg_ppograd_mfma.hip: the matrix-core path): the object, the tile
// kernels' arguments, the gather of a tile's rows and the statistics' float64 forward of the actor.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "pbg_policy_dev.h"

struct pbg_ppo_grad {
  int device, obs_dim, h1, h2, act_dim, max_rows;
  int Da, Dc, Dtot;   // Dtot = Da + Dc + act_dim: a workgroup's float32 partial
  int n_wg;           // workgroups of the widest launch
  float* part;        // device [n_wg, Dtot]
  double* part_stats; // device [n_wg, 4], the same allocation
  int path;           // PBG_PPO_GRAD_FMA or PBG_PPO_GRAD_MFMA
};

namespace pbg {
namespace ppograd {

using namespace pbg::policy;

constexpr int NA_MAX = PBG_POLICY_MAX_ACT;

struct Args {
  const float *theta_a, *theta_c, *log_std;
  Norm nm;
  const float *obs, *act, *logp_old, *adv, *ret;
  const int64_t* idx;
  const float* adv_norm;
  float clip_eps, vf_coef;
  int Bm, obs_dim, h1, h2, A, Da, Dtot;
  int wg0, G;         // the launch's first workgroup and the workgroups of the whole gradient: block i is workgroup wg0 + i
  float* part;        // [gridDim.x, Dtot]: row i is block i's
  double* part_stats; // [gridDim.x, 4]
  float *logp_out, *v_out;
  const float* value_old;  // [B], nullable: value clipping with vf_clip
  const int32_t* gate;     // [2], nullable: gate[0] != 0 ends every workgroup at entry
  float vf_clip;
};

// The matrix-core path's tile kernel (pbg_ppograd_mfma.hip) for the `count` workgroups a.wg0 .. a.wg0 + count - 1 on
// `stream`: the hipError_t of the launch
int launch_tiles_mfma(const Args& a, int count, hipStream_t stream);
// its workgroup cap: one workgroup per CU
constexpr int MFMA_MAX_WG = 256;

// the tile's rows, gathered: row e is batch row idx[row0 + e] (idx NULL: row0 + e) -> xT [K0][PT], zero past `rows`
__device__ __forceinline__ void gather_tile(int K0, const int64_t* __restrict__ idx, int row0, int rows,
                                            const float* __restrict__ obs, const Norm nm, float* xT) {
  for (int i = threadIdx.x; i < PT * K0; i += PB) {
    const int e = i / K0, k = i - e * K0;
    float v = 0.f;
    if (e < rows) {
      const size_t r = idx ? (size_t)idx[row0 + e] : (size_t)(row0 + e);
      v = obs[r * K0 + k];
      if (nm.mean) v = normalise(v, nm.mean[k], nm.inv_std[k], nm.clip);
    }
    xT[k * PT + e] = v;
  }
}

// ---- the statistics' float64 forward of the actor, R rows of the tile at a time in [width][R] double planes laid
// over float [PD][PT] planes: the whole tile when obs_dim, h1, h2 <= PD / 2, half a tile otherwise
static_assert(PD * (PT / 2) * sizeof(double) == PD * PT * sizeof(float), "a double half-tile plane fits a float plane");

// one layer for this lane's column j and rows e0 .. e0 + EL of the pass: pbg_policy_dev.h's chain in float64;
// xT [K][R] -> yT [H][YS]
template <int EL, int R, int YS>
__device__ __forceinline__ void layer64_cols(const float* __restrict__ W, const float* __restrict__ bias, int K, int H, int j,
                                             int e0, bool relu, const double* xT, double* yT) {
  double acc[EL];
  const double bj = (double)bias[j];
#pragma unroll
  for (int e = 0; e < EL; e++) acc[e] = bj;
  const float* wp = W + j;
#pragma unroll 4
  for (int k = 0; k < K; k++) {
    const double w = (double)wp[(size_t)k * H];
#pragma unroll
    for (int e = 0; e < EL; e++) acc[e] = __builtin_fma(xT[k * R + e0 + e], w, acc[e]);
  }
#pragma unroll
  for (int e = 0; e < EL; e++) yT[j * YS + e0 + e] = relu && acc[e] < 0.0 ? 0.0 : acc[e];
}

// `layer`'s split of the columns over the lanes, for R rows.  WIDE false: the caller passes a whole tile (R = PT) only
// with H <= PD / 2, as actor_forward64 does, and the 16-row instance of the widest split, which no call reaches, is
// left out (the FMA path's kernels keep it: they are the code they were)
template <int R, int YS, bool WIDE>
__device__ __forceinline__ void layer64(const float* __restrict__ W, const float* __restrict__ bias, int K, int H, bool relu,
                                        const double* xT, double* yT) {
  const int tid = threadIdx.x;
  if (H <= 64) {
    const int j = tid & 63, g = tid >> 6;
    if (j < H) layer64_cols<R / 4, R, YS>(W, bias, K, H, j, (R / 4) * g, relu, xT, yT);
  } else if (H <= 128) {
    const int j = tid & 127, g = tid >> 7;
    if (j < H) layer64_cols<R / 2, R, YS>(W, bias, K, H, j, (R / 2) * g, relu, xT, yT);
  } else if (WIDE || R < PT) {
    if (tid < H) layer64_cols<R, R, YS>(W, bias, K, H, tid, 0, relu, xT, yT);
  }
}

// The float64 means of the tile's rows -> mu64 [A][PT].  x, h1, h2: three idle float planes.  Called behind a
// barrier; one barrier closes it.
template <int R, bool WIDE = true>
__device__ __forceinline__ void actor_forward64(const Weights& P, const Norm nm, const int64_t* __restrict__ idx, int row0,
                                                int rows, const float* __restrict__ obs, float* x, float* h1, float* h2,
                                                double* mu64) {
  double* dX = reinterpret_cast<double*>(x);
  double* dH1 = reinterpret_cast<double*>(h1);
  double* dH2 = reinterpret_cast<double*>(h2);
  const int K0 = P.obs_dim;
  for (int p = 0; p * R < rows; p++) {  // uniform over the workgroup
    for (int i = threadIdx.x; i < R * K0; i += PB) {
      const int e = i / K0, k = i - e * K0, row = p * R + e;
      double v = 0.0;
      if (row < rows) {
        const size_t r = idx ? (size_t)idx[row0 + row] : (size_t)(row0 + row);
        const float o = obs[r * K0 + k];
        v = nm.mean ? normalise64(o, nm.mean[k], nm.inv_std[k], nm.clip) : (double)o;
      }
      dX[k * R + e] = v;
    }
    __syncthreads();
    layer64<R, R, WIDE>(P.w1, P.b1, K0, P.h1, true, dX, dH1);
    __syncthreads();
    layer64<R, R, WIDE>(P.w2, P.b2, P.h1, P.h2, true, dH1, dH2);
    __syncthreads();
    layer64<R, PT, WIDE>(P.w3, P.b3, P.h2, P.act_dim, false, dH2, mu64 + p * R);
  }
  __syncthreads();
}

}  // namespace ppograd
}  // namespace pbg
