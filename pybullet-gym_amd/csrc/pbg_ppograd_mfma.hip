// pbg_ppograd_mfma.hip -- the matrix-core path of the PPO gradient (include/pbg.h "PPO gradient", "The matrix-core
// path"): the tile kernel of an object created with PBG_PPO_GRAD_MFMA.  The object, the
// reduction and the host twin are pbg_ppograd.hip's.
//
// Geometry.  The FMA path's tile (256 lanes, 16 rows, transposed [width][16] LDS planes) with every product on
// v_mfma_f32_16x16x4_f32, whose lane l = (i = l & 15, g = l >> 4) holds A[i][k = g], B[k = g][j = i] and, in register
// r, D[4 g + r][i].  The blocks of a product's output are dealt to the four waves round-robin.
//   forward   y[j][e] = b[j] + sum_k W[k][j] x[k][e]:  M = e, N = j, C = the bias.  A = xT[k0 + g][i] is 64 consecutive
//             floats of the plane, B = W[k0 + g][16 jb + i] four runs of 16 consecutive weights; a lane ends with
//             y[j][4 g .. 4 g + 3], one float4 store into the transposed plane.  k ascends: the contract's chain.
//   back      dx[k][e] = x[k][e] > 0 ? sum_j W[k][j] dy[j][e] : 0:  M = e, N = k, A = dyT[j0 + g][i],
//             B = W[16 kb + i][j0 + g].  j ascends from zero: the FMA path's chain.
//   gradient  dW[k][j] = sum_e x[k][e] dy[j][e]:  M = k, N = j, the sum over rows.  A lane reads x[16 kb + i][4 g .. 4 g + 3]
//             and dy[16 jb + i][4 g .. 4 g + 3] as one float4 each (the wave reads 1 KiB of each plane in a row) and
//             issues four instructions, component t of both: instruction t sums the rows e = t, 4 + t, 8 + t, 12 + t.
//             The C input is the patch's value after the previous tile: one chain over all the workgroup's rows.
// Ragged edges are zero operands, never branches: the planes' rows up to the next multiple of 16 are written (zeros)
// by the launch, operands past K or H are replaced by zero with a select, and every instruction runs with all 64
// lanes active under wave-uniform control flow only.
//
// A 16 x 16 patch of a weight gradient belongs to one wave.  On the on-chip route (on_chip(): obs_dim <= 80, h1 <= 256,
// h2 <= 128, act_dim <= 32, which holds every shipped shape) a wave's 56 accumulators (224 registers) live across the
// tile loop and are stored once; on the other route (any shape) the patches form one list (layer 1 first, row-major
// inside a layer), wave w owns the patches w, w + 4, ... and a patch's accumulator goes through the workgroup's partial
// once per tile.  A workgroup makes three passes over its tiles: the actor's gradient, the actor's float64 forward for
// `stats`, the critic's gradient; so one network's accumulators are live at a time and none during the float64 pass.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <type_traits>

#include "pbg_ppograd_dev.h"

namespace {

using namespace pbg::policy;
using namespace pbg::ppograd;

typedef float f32x4 __attribute__((ext_vector_type(4)));

// The kernel's Args where they lie, in the kernarg segment.  The tile loops read wg0 and G through it (the values of
// a.wg0 and a.G), as they once read gridDim.x through the implicit arguments behind the same segment: a loop that uses
// the segment's base keeps it in scalar registers, and with it there the compiler reads an argument again where it would
// otherwise spill it to a lane and read that back.  The cast holds
// because Args, passed by value, is the kernel's first and only explicit argument, so it lies at offset 0 of the segment
// in its own layout: the static_asserts behind the kernel pin the signature and the layout
__device__ __forceinline__ const __attribute__((address_space(4))) Args* karg() {
  return (const __attribute__((address_space(4))) Args*)__builtin_amdgcn_kernarg_segment_ptr();
}

constexpr int BE = 16;  // a block's edge

__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

__host__ __device__ __forceinline__ int nblk(int x) { return (x + BE - 1) / BE; }

// One layer's forward for the wave's blocks w, w + 4, ..., w + 4 (NQ - 1) of output columns: xT [K][PT] -> yT, whose
// rows up to 64 NQ are all written (columns at or past H: zeros).
template <int NQ>
__device__ __forceinline__ void fwd_blocks(const float* __restrict__ W, const float* __restrict__ bias, int K, int H, bool relu,
                                           int w, const float* xT, float* yT) {
  const int lane = threadIdx.x & 63, i = lane & 15, g = lane >> 4;
  f32x4 acc[NQ];
  int j[NQ];
#pragma unroll
  for (int q = 0; q < NQ; q++) {
    j[q] = (w + 4 * q) * BE + i;
    const bool in = j[q] < H;
    float b = bias[in ? j[q] : 0];
    b = in ? b : 0.f;
    acc[q] = f32x4{b, b, b, b};
  }
  // two steps per trip: the instruction is convergent, so a loop of run-time length is unrolled by hand; a step past K
  // has zero operands like the K tail
  for (int k8 = 0; k8 < K; k8 += 8)
#pragma unroll
  for (int k0 = k8; k0 < k8 + 8; k0 += 4) {
    const int k = k0 + g;
    const bool kin = k < K;
    float x = xT[k * PT + i];
    x = kin ? x : 0.f;
    const float* wr = W + (size_t)(kin ? k : 0) * H;
#pragma unroll
    for (int q = 0; q < NQ; q++) {
      const bool in = kin && j[q] < H;
      float wv = wr[in ? j[q] : 0];
      wv = in ? wv : 0.f;
      acc[q] = mfma4(x, wv, acc[q]);
    }
  }
#pragma unroll
  for (int q = 0; q < NQ; q++) {
    float4 y;
    y.x = acc[q][0]; y.y = acc[q][1]; y.z = acc[q][2]; y.w = acc[q][3];
    if (relu) {
      y.x = y.x < 0.f ? 0.f : y.x; y.y = y.y < 0.f ? 0.f : y.y;
      y.z = y.z < 0.f ? 0.f : y.z; y.w = y.w < 0.f ? 0.f : y.w;
    }
    *reinterpret_cast<float4*>(yT + j[q] * PT + 4 * g) = y;
  }
}

__device__ __forceinline__ void fwd_layer(const float* __restrict__ W, const float* __restrict__ bias, int K, int H, bool relu,
                                          int w, const float* xT, float* yT) {
  const int nq = (nblk(H) + 3) >> 2;  // uniform over the workgroup
  if (nq == 1) fwd_blocks<1>(W, bias, K, H, relu, w, xT, yT);
  else if (nq == 2) fwd_blocks<2>(W, bias, K, H, relu, w, xT, yT);
  else if (nq == 3) fwd_blocks<3>(W, bias, K, H, relu, w, xT, yT);
  else fwd_blocks<4>(W, bias, K, H, relu, w, xT, yT);
}

// The gradient of a layer's input activations (K rows, the wave's blocks w, w + 4, ...) from its outputs' (H rows):
// outT[k][e] = actT[k][e] > 0 ? sum_j W[k][j] dyT[j][e] : 0; rows at or past K: zeros
template <int NQ>
__device__ __forceinline__ void back_blocks(const float* __restrict__ W, int K, int H, int w, const float* dyT, const float* actT,
                                            float* outT) {
  const int lane = threadIdx.x & 63, i = lane & 15, g = lane >> 4;
  f32x4 acc[NQ];
  int k[NQ];
#pragma unroll
  for (int q = 0; q < NQ; q++) {
    k[q] = (w + 4 * q) * BE + i;
    acc[q] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  for (int j8 = 0; j8 < H; j8 += 8)  // two steps per trip, as in fwd_blocks
#pragma unroll
  for (int j0 = j8; j0 < j8 + 8; j0 += 4) {
    const int j = j0 + g;
    const bool jin = j < H;
    float d = dyT[j * PT + i];
    d = jin ? d : 0.f;
#pragma unroll
    for (int q = 0; q < NQ; q++) {
      const bool in = jin && k[q] < K;
      float wv = W[in ? (size_t)k[q] * H + j : 0];
      wv = in ? wv : 0.f;
      acc[q] = mfma4(d, wv, acc[q]);
    }
  }
#pragma unroll
  for (int q = 0; q < NQ; q++) {
    const float4 m = *reinterpret_cast<const float4*>(actT + k[q] * PT + 4 * g);
    const bool in = k[q] < K;
    float4 y;
    y.x = in && m.x > 0.f ? acc[q][0] : 0.f; y.y = in && m.y > 0.f ? acc[q][1] : 0.f;
    y.z = in && m.z > 0.f ? acc[q][2] : 0.f; y.w = in && m.w > 0.f ? acc[q][3] : 0.f;
    *reinterpret_cast<float4*>(outT + k[q] * PT + 4 * g) = y;
  }
}

__device__ __forceinline__ void back_layer(const float* __restrict__ W, int K, int H, int w, const float* dyT, const float* actT,
                                           float* outT) {
  const int nq = (nblk(K) + 3) >> 2;
  if (nq == 1) back_blocks<1>(W, K, H, w, dyT, actT, outT);
  else if (nq == 2) back_blocks<2>(W, K, H, w, dyT, actT, outT);
  else if (nq == 3) back_blocks<3>(W, K, H, w, dyT, actT, outT);
  else back_blocks<4>(W, K, H, w, dyT, actT, outT);
}

struct Planes {
  float *X, *H1, *H2, *E, *F, *D, *D2;
};

// a network's list of weight-gradient patches: layer 1's nb(obs_dim) x nb(h1), then layer 2's, then layer 3's
struct Patches {
  int e1, e2, ntot;     // where layer 1's and layer 2's patches end, and the list
  int nb1, nb2, nb3;    // a layer's blocks of columns
  int inv1, inv2, inv3; // ceil(2^16 / nb): p / nb == (p * inv) >> 16 for p < 2^16 / nb, and p < 256 here
};

__device__ __forceinline__ Patches patches_of(const Weights& P) {
  Patches s;
  s.nb1 = nblk(P.h1); s.nb2 = nblk(P.h2); s.nb3 = nblk(P.act_dim);
  s.e1 = nblk(P.obs_dim) * s.nb1;
  s.e2 = s.e1 + s.nb1 * s.nb2;
  s.ntot = s.e2 + s.nb2 * s.nb3;
  s.inv1 = (65536 + s.nb1 - 1) / s.nb1; s.inv2 = (65536 + s.nb2 - 1) / s.nb2; s.inv3 = (65536 + s.nb3 - 1) / s.nb3;
  return s;
}

// patch p of the list (wave-uniform): its planes, its weight block in G's layout and its place there
struct Patch {
  const float *xT, *dyT;
  float* gw;
  int K, H, kb, jb;
};

// by value: a conditional between two members is an lvalue, and the select of their addresses keeps the struct in memory
template <typename T>
__device__ __forceinline__ T pick(int layer, T a, T b, T c) {
  return layer == 0 ? a : (layer == 1 ? b : c);
}

__device__ __forceinline__ Patch patch_at(const Patches& s, int p, const Weights& P, const Weights& G, const Planes& L) {
  Patch t;
  const int layer = p < s.e1 ? 0 : (p < s.e2 ? 1 : 2);
  const int q = p - pick<int>(layer, 0, s.e1, s.e2);
  const int nb = pick<int>(layer, s.nb1, s.nb2, s.nb3);
  const int inv = pick<int>(layer, s.inv1, s.inv2, s.inv3);
  t.kb = (int)(((unsigned)q * (unsigned)inv) >> 16);
  t.jb = q - t.kb * nb;
  t.xT = pick<const float*>(layer, L.X, L.H1, L.H2);
  t.dyT = pick<const float*>(layer, L.F, L.E, L.D);
  t.gw = const_cast<float*>(pick<const float*>(layer, G.w1, G.w2, G.w3));
  t.K = pick<int>(layer, P.obs_dim, P.h1, P.h2);
  t.H = pick<int>(layer, P.h1, P.h2, P.act_dim);
  return t;
}

// the tile's 16 rows onto a patch's chain
__device__ __forceinline__ f32x4 patch_rows(const Patch& t, f32x4 c) {
  const int lane = threadIdx.x & 63, i = lane & 15, g = lane >> 4;
  const float4 x = *reinterpret_cast<const float4*>(t.xT + (t.kb * BE + i) * PT + 4 * g);
  const float4 d = *reinterpret_cast<const float4*>(t.dyT + (t.jb * BE + i) * PT + 4 * g);
  c = mfma4(x.x, d.x, c);
  c = mfma4(x.y, d.y, c);
  c = mfma4(x.z, d.z, c);
  c = mfma4(x.w, d.w, c);
  return c;
}

// a lane's four elements of a patch: column j = 16 jb + i, rows k = 16 kb + 4 g + r
__device__ __forceinline__ void patch_store(const Patch& t, f32x4 c) {
  const int lane = threadIdx.x & 63, i = lane & 15, g = lane >> 4;
  const int j = t.jb * BE + i, k = t.kb * BE + 4 * g;
  if (j < t.H) {
#pragma unroll
    for (int r = 0; r < 4; r++)
      if (k + r < t.K) t.gw[(size_t)(k + r) * t.H + j] = c[r];
  }
}

__device__ __forceinline__ f32x4 patch_load(const Patch& t) {
  const int lane = threadIdx.x & 63, i = lane & 15, g = lane >> 4;
  const int j = t.jb * BE + i, k = t.kb * BE + 4 * g;
  f32x4 c;
#pragma unroll
  for (int r = 0; r < 4; r++) {
    const bool in = j < t.H && k + r < t.K;
    const float v = t.gw[in ? (size_t)(k + r) * t.H + j : 0];
    c[r] = in ? v : 0.f;
  }
  return c;
}

// ---- the on-chip route: a wave's patches sit at compile-time places of its accumulator arrays, so that every LDS
// address is one of two per-plane lane addresses plus an immediate and nothing but wave-uniform conditions is left
// to compute.  Layers 1 and 2 deal the blocks of columns to the waves (wave w: jb = w, w + 4, ...; every kb), layer 3,
// which has few columns, the blocks of rows (wave w: kb = w, w + 4, ...; every jb).
constexpr int C_NK1 = 5, C_NQ1 = 4;   // obs_dim <= 80; h1 <= 256
constexpr int C_NK2 = 16, C_NQ2 = 2;  // h1 <= 256; h2 <= 128
constexpr int C_NK3 = 2, C_NJ3 = 2;   // h2 <= 128; act_dim <= 32

__host__ __device__ __forceinline__ bool on_chip(int obs_dim, int h1, int h2, int act_dim) {
  return nblk(obs_dim) <= C_NK1 && nblk(h1) <= 4 * C_NQ1 && nblk(h1) <= C_NK2 && nblk(h2) <= 4 * C_NQ2 &&
         nblk(h2) <= 4 * C_NK3 && nblk(act_dim) <= C_NJ3;
}

__device__ __forceinline__ f32x4 chain_rows(const float4 x, const float4 d, f32x4 c) {
  c = mfma4(x.x, d.x, c);
  c = mfma4(x.y, d.y, c);
  c = mfma4(x.z, d.z, c);
  c = mfma4(x.w, d.w, c);
  return c;
}

// BYCOL: acc[kk * NQ + q] is the patch (kb = kk, jb = w + 4 q); else acc[kk * NQ + q] is (kb = w + 4 kk, jb = q)
template <bool BYCOL, int NK, int NQ>
__device__ __forceinline__ void dw_chip(const float* xT, const float* dyT, int K, int H, int w, f32x4 (&acc)[NK * NQ]) {
  const int lane = threadIdx.x & 63, i = lane & 15, g = lane >> 4;
  const int nbK = nblk(K), nbH = nblk(H);
  const float* xp = xT + ((BYCOL ? 0 : w * BE) + i) * PT + 4 * g;
  const float* dp = dyT + ((BYCOL ? w * BE : 0) + i) * PT + 4 * g;
  float4 d[NQ];
#pragma unroll
  for (int q = 0; q < NQ; q++) d[q] = *reinterpret_cast<const float4*>(dp + q * (BYCOL ? 4 : 1) * BE * PT);
#pragma unroll
  for (int kk = 0; kk < NK; kk++) {
    if ((BYCOL ? kk : w + 4 * kk) < nbK) {
      const float4 x = *reinterpret_cast<const float4*>(xp + kk * (BYCOL ? 1 : 4) * BE * PT);
#pragma unroll
      for (int q = 0; q < NQ; q++)
        if ((BYCOL ? w + 4 * q : q) < nbH) acc[kk * NQ + q] = chain_rows(x, d[q], acc[kk * NQ + q]);
    }
  }
}

template <bool BYCOL, int NK, int NQ>
__device__ __forceinline__ void flush_chip(float* gw, int K, int H, int w, const f32x4 (&acc)[NK * NQ]) {
  const int nbK = nblk(K), nbH = nblk(H);
#pragma unroll
  for (int kk = 0; kk < NK; kk++)
#pragma unroll
    for (int q = 0; q < NQ; q++) {
      const int kb = BYCOL ? kk : w + 4 * kk, jb = BYCOL ? w + 4 * q : q;
      if (kb < nbK && jb < nbH) patch_store(Patch{nullptr, nullptr, gw, K, H, kb, jb}, acc[kk * NQ + q]);
    }
}

template <int N>
__device__ __forceinline__ void zero_acc(f32x4 (&acc)[N]) {
#pragma unroll
  for (int s = 0; s < N; s++) acc[s] = f32x4{0.f, 0.f, 0.f, 0.f};
}

// the tile's term of a bias gradient: lane j < H adds the sum over the tile's rows ascending from zero
__device__ __forceinline__ void bias_rows(int H, const float* dyT, float& ab) {
  const int tid = threadIdx.x;
  if (tid < H) {
    float s = 0.f;
#pragma unroll
    for (int e = 0; e < PT; e++) s += dyT[tid * PT + e];
    ab += s;
  }
}

// what the row lanes carry over both networks' passes
struct RowSums {
  double st0, st1, st2, st3;  // pg, vf, clipped, logp_old - logp
  float als;                  // lane j < A: log_std's sum
};

// One network over all the workgroup's tiles into its arrays G of the workgroup's partial.
template <bool CHIP, bool ACTOR>
__device__ __forceinline__ void net_pass(const Args& a, const Weights& P, const Weights& G, const Planes& L, const double* inv_sig,
                                         double sum_ls, RowSums& rs) {
  const int tid = threadIdx.x, A = a.A;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const Patches pl = patches_of(P);
  const double inv_bm = 1.0 / (double)a.Bm;
  f32x4 acc1[CHIP ? C_NK1 * C_NQ1 : 1], acc2[CHIP ? C_NK2 * C_NQ2 : 1], acc3[CHIP ? C_NK3 * C_NJ3 : 1];
  zero_acc(acc1);
  zero_acc(acc2);
  zero_acc(acc3);
  float ab1 = 0.f, ab2 = 0.f, ab3 = 0.f;
  const int K0 = P.obs_dim, K0pad = nblk(K0) * BE;

  const int ntiles = (a.Bm + PT - 1) / PT;
  bool first = true;
  for (int t = karg()->wg0 + (int)blockIdx.x; t < ntiles; t += karg()->G, first = false) {
    const int row0 = t * PT, rows = min(PT, a.Bm - row0);
    __syncthreads();  // the previous tile's (or network's) last readers of the planes
    gather_tile(K0, a.idx, row0, rows, a.obs, a.nm, L.X);
    for (int i = K0 * PT + tid; i < K0pad * PT; i += PB) L.X[i] = 0.f;  // the rows of the last block past K0
    __syncthreads();
    size_t r = 0;  // row lanes: the batch row
    if (tid < rows) r = a.idx ? (size_t)a.idx[row0 + tid] : (size_t)(row0 + tid);

    fwd_layer(P.w1, P.b1, K0, P.h1, true, w, L.X, L.H1);
    __syncthreads();
    fwd_layer(P.w2, P.b2, P.h1, P.h2, true, w, L.H1, L.H2);
    __syncthreads();
    fwd_layer(P.w3, P.b3, P.h2, P.act_dim, false, w, L.H2, L.D);
    __syncthreads();

    if (ACTOR) {
      if (tid < PT) {
        if (tid < rows) {
          double ahat = (double)a.adv[r];
          if (a.adv_norm) ahat = (ahat - (double)a.adv_norm[0]) * (double)a.adv_norm[1];
          const double logp = ppo_actor_row(A, L.D + tid, L.D2 + tid, PT, a.act + r * A, inv_sig, sum_ls, (double)a.logp_old[r],
                                            ahat, (double)a.clip_eps, inv_bm);
          if (a.logp_out) a.logp_out[row0 + tid] = (float)logp;
        } else {
          for (int j = 0; j < A; j++) L.D[j * PT + tid] = L.D2[j * PT + tid] = 0.f;
        }
      }
    } else {
      if (tid < PT) {
        float dv = 0.f;
        if (tid < rows) {
          const float v = L.D[tid];
          double vf;
          const float* vo = karg()->value_old;
          dv = ppo_critic_row(v, a.ret[r], vo ? vo + r : nullptr, (double)karg()->vf_clip, (double)a.vf_coef, inv_bm, &vf);
          rs.st1 += vf;
          if (a.v_out) a.v_out[row0 + tid] = v;
        }
        L.D[tid] = dv;
      }
    }
    __syncthreads();
    if (ACTOR && tid < A) {
      float s = 0.f;
#pragma unroll
      for (int e = 0; e < PT; e++) s += L.D2[tid * PT + e];
      rs.als += s;
    }

    back_layer(P.w3, P.h2, P.act_dim, w, L.D, L.H2, L.E);
    __syncthreads();
    back_layer(P.w2, P.h1, P.h2, w, L.E, L.H1, L.F);
    __syncthreads();

    // the weight gradients: every plane is read, none written
    bias_rows(P.act_dim, L.D, ab3);
    bias_rows(P.h2, L.E, ab2);
    bias_rows(P.h1, L.F, ab1);
    if (CHIP) {
      dw_chip<true, C_NK1, C_NQ1>(L.X, L.F, K0, P.h1, w, reinterpret_cast<f32x4(&)[C_NK1 * C_NQ1]>(acc1));
      dw_chip<true, C_NK2, C_NQ2>(L.H1, L.E, P.h1, P.h2, w, reinterpret_cast<f32x4(&)[C_NK2 * C_NQ2]>(acc2));
      dw_chip<false, C_NK3, C_NJ3>(L.H2, L.D, P.h2, P.act_dim, w, reinterpret_cast<f32x4(&)[C_NK3 * C_NJ3]>(acc3));
    } else {
      for (int p = w; p < pl.ntot; p += 4) {
        const Patch pt = patch_at(pl, p, P, G, L);
        f32x4 c = f32x4{0.f, 0.f, 0.f, 0.f};
        if (!first) c = patch_load(pt);
        c = patch_rows(pt, c);
        patch_store(pt, c);
      }
    }
  }

  if (CHIP) {
    flush_chip<true, C_NK1, C_NQ1>(const_cast<float*>(G.w1), K0, P.h1, w, reinterpret_cast<const f32x4(&)[C_NK1 * C_NQ1]>(acc1));
    flush_chip<true, C_NK2, C_NQ2>(const_cast<float*>(G.w2), P.h1, P.h2, w, reinterpret_cast<const f32x4(&)[C_NK2 * C_NQ2]>(acc2));
    flush_chip<false, C_NK3, C_NJ3>(const_cast<float*>(G.w3), P.h2, P.act_dim, w,
                                    reinterpret_cast<const f32x4(&)[C_NK3 * C_NJ3]>(acc3));
  }
  if (tid < P.h1) const_cast<float*>(G.b1)[tid] = ab1;
  if (tid < P.h2) const_cast<float*>(G.b2)[tid] = ab2;
  if (tid < P.act_dim) const_cast<float*>(G.b3)[tid] = ab3;
}

// The actor's statistics over all the workgroup's tiles from a float64 forward, a pass of its own between the two
// networks: no weight-gradient accumulator is live while it runs.  E, H1 and H2 are its planes, the means span D and D2.
__device__ __forceinline__ void stats_pass(const Args& a, const Weights& P, const Planes& L, const double* inv_sig, double sum_ls,
                                           RowSums& rs) {
  const int tid = threadIdx.x, A = a.A;
  const int ntiles = (a.Bm + PT - 1) / PT;
  double* mu64 = reinterpret_cast<double*>(L.D);
  for (int t = karg()->wg0 + (int)blockIdx.x; t < ntiles; t += karg()->G) {
    const int row0 = t * PT, rows = min(PT, a.Bm - row0);
    __syncthreads();  // the previous tile's rows read mu64; the actor's last tile read every plane
    if (a.obs_dim <= PD / 2 && a.h1 <= PD / 2 && a.h2 <= PD / 2)
      actor_forward64<PT, false>(P, a.nm, a.idx, row0, rows, a.obs, L.E, L.H1, L.H2, mu64);
    else
      actor_forward64<PT / 2, false>(P, a.nm, a.idx, row0, rows, a.obs, L.E, L.H1, L.H2, mu64);
    if (tid < rows) {
      const size_t r = a.idx ? (size_t)a.idx[row0 + tid] : (size_t)(row0 + tid);
      double ahat = (double)a.adv[r];
      if (a.adv_norm) ahat = (ahat - (double)a.adv_norm[0]) * (double)a.adv_norm[1];
      double st[3];
      ppo_stats_row(A, mu64 + tid, PT, a.act + r * A, inv_sig, sum_ls, (double)a.logp_old[r], ahat, (double)a.clip_eps, st);
      rs.st0 += st[0];
      rs.st2 += st[1];
      rs.st3 += st[2];
    }
  }
}

// Workgroup b = a.wg0 + blockIdx.x of a.G: the tiles b, b + a.G, ... of the minibatch into row blockIdx.x of a.part.  LDS: five [256][16] planes and two
// [64][16] ones, 88 KiB, plus the row lanes' doubles.
template <bool CHIP>
__global__ __launch_bounds__(PB) void ppograd_mfma_kernel(const Args a) {
  __shared__ __attribute__((aligned(16))) float plane[5 * PD * PT + 2 * NA_MAX * PT];
  __shared__ double inv_sig[NA_MAX];
  __shared__ double sstat[4 * PT];
  Planes L;
  L.X = plane; L.H1 = plane + PD * PT; L.H2 = plane + 2 * PD * PT; L.E = plane + 3 * PD * PT; L.F = plane + 4 * PD * PT;
  L.D = plane + 5 * PD * PT; L.D2 = L.D + NA_MAX * PT;
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
  RowSums rs{0.0, 0.0, 0.0, 0.0, 0.f};

  net_pass<CHIP, true>(a, Pa, Ga, L, inv_sig, sum_ls, rs);
  stats_pass(a, Pa, L, inv_sig, sum_ls, rs);
  net_pass<CHIP, false>(a, Pc, Gc, L, inv_sig, sum_ls, rs);

  if (tid < A) part[a.Dtot - A + tid] = rs.als;
  if (tid < PT) {
    sstat[0 * PT + tid] = rs.st0;
    sstat[1 * PT + tid] = rs.st1;
    sstat[2 * PT + tid] = rs.st2;
    sstat[3 * PT + tid] = rs.st3;
  }
  __syncthreads();
  if (tid < 4) {
    double s = 0.0;
    for (int e = 0; e < PT; e++) s += sstat[tid * PT + e];
    a.part_stats[(size_t)blockIdx.x * 4 + tid] = s;
  }
}

// what karg() relies on: one explicit argument, an Args by value (a function type drops the const), copied into the
// kernarg segment byte for byte
static_assert(std::is_same<decltype(&ppograd_mfma_kernel<true>), void (*)(Args)>::value &&
                  std::is_same<decltype(&ppograd_mfma_kernel<false>), void (*)(Args)>::value,
              "karg(): Args must be the kernel's only explicit argument");
static_assert(std::is_trivially_copyable<Args>::value && std::is_standard_layout<Args>::value,
              "karg(): Args must lie in the kernarg segment as it lies in memory");

}  // namespace

namespace pbg {
namespace ppograd {

int launch_tiles_mfma(const Args& a, int count, hipStream_t stream) {
  // the critic's third layer has one block of columns, so what holds the actor's patches holds the critic's
  if (on_chip(a.obs_dim, a.h1, a.h2, a.A))
    hipLaunchKernelGGL(ppograd_mfma_kernel<true>, dim3((unsigned)count), dim3(PB), 0, stream, a);
  else
    hipLaunchKernelGGL(ppograd_mfma_kernel<false>, dim3((unsigned)count), dim3(PB), 0, stream, a);
  return (int)hipGetLastError();
}

}  // namespace ppograd
}  // namespace pbg
