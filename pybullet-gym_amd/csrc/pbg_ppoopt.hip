// pbg_ppoopt.hip -- what is left of a PPO minibatch step once the gradient is there (include/pbg.h "PPO optimiser
// step"): the advantage normaliser's (shift, scale) pair as one launch (pbg_adv_norm, pbg_adv_norm_host) and Adam
// with global-norm gradient clipping over up to 8 flat float32 blocks as two launches with its moments, its step
// count and the running powers of the betas on the device (pbg_ppo_opt_*, pbg_ppo_opt_host), its learning rate
// optionally read from device memory (io.lr_ptr; pbg_perm.hip's pbg_ppo_lr_linear writes one).  Both launches of the
// step obey the KL gate (io.gate; include/pbg.h "Value clipping and the KL gate"), which pbg_ppogate.hip's launches write.
//
// Every sum is float64 in the order pbg.h states, every per-element expression one __host__ __device__ function
// compiled with contraction off, so the host twins give the device's bits.  (The optimiser's summed squares are
// squares of float32 values, exact in float64: a fused multiply-add there would round as the separate add does.)
#include <hip/hip_runtime.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <new>

#include "pbg_policy_dev.h"

namespace {

using namespace pbg::policy;
using pbg::DeviceGuard;

constexpr int AN_LANES = 1024;   // pbg_adv_norm's one workgroup
constexpr int OB = 256;          // the optimiser's workgroup
constexpr int OPT_MAX_WG = 64;   // workgroups per block at most (PBG_PPO_OPT_MAX_BLOCKS * 64 partials in all)
constexpr int NBLK = PBG_PPO_OPT_MAX_BLOCKS;

// what lives on the device between steps
struct OptState {
  double b1t, b2t;  // beta1^t, beta2^t, kept by multiplication
  uint32_t t;
  uint32_t pad[3];  // 32 bytes: what follows the word stays 16-byte aligned
};
static_assert(sizeof(OptState) == 32, "the state word is 32 bytes");

// ---------------------------------------------------------------------------- the shared arithmetic
// lanes[0] += lanes[1] + ... in pbg.h's tree: for s = n/2, n/4, ..., 1: lanes[l] += lanes[l + s] for l < s
inline void host_tree(double* lanes, int n) {
  for (int s = n / 2; s >= 1; s /= 2)
    for (int l = 0; l < s; l++) lanes[l] += lanes[l + s];
}

template <int N>
__device__ __forceinline__ double lds_tree(double* sh, double x) {
  const int l = (int)threadIdx.x;
  sh[l] = x;
  __syncthreads();
#pragma unroll
  for (int s = N / 2; s >= 1; s /= 2) {
    if (l < s) sh[l] += sh[l + s];
    __syncthreads();
  }
  const double r = sh[0];
  __syncthreads();  // sh is free again
  return r;
}

// one row onto a lane's sums: d = a - c0 with c0 the minibatch's first advantage, so constant advantages sum zeros.
// d * d is a float64 product like any other here (d need not be a float32): nothing may contract it into the add
__host__ __device__ __forceinline__ void adv_norm_add(float a, double c0, double& s1, double& s2) {
#pragma clang fp contract(off)
  const double d = (double)a - c0;
  s1 = s1 + d;
  s2 = s2 + d * d;
}

__host__ __device__ __forceinline__ void adv_norm_finish(double c0, double S1, double S2, int Bm, float* __restrict__ out) {
#pragma clang fp contract(off)
  const double ms = S1 / (double)Bm;  // the mean of the shifted values
  double var = (S2 - S1 * ms) / (double)(Bm - 1);
  var = var < 0.0 ? 0.0 : var;  // a NaN stays one
  out[0] = (float)(c0 + ms);
  out[1] = (float)(1.0 / (sqrt(var) + 1e-8));
}

__host__ __device__ __forceinline__ double opt_coef(double sumsq, double max_grad_norm, double* norm_out) {
#pragma clang fp contract(off)
  const double norm = sqrt(sumsq);
  *norm_out = norm;
  if (!(max_grad_norm > 0.0)) return 1.0;
  const double c = max_grad_norm / (norm + 1e-6);
  return c > 1.0 ? 1.0 : c;  // a NaN stays one
}

// the per-step factors every element shares
struct AdamK {
  double coef, b1, omb1, b2, omb2, c1, c2, eps;
};

__host__ __device__ __forceinline__ AdamK adam_factors(double coef, double lr, double beta1, double beta2, double eps, double b1t,
                                                       double b2t) {
#pragma clang fp contract(off)
  AdamK k;
  k.coef = coef;
  k.b1 = beta1;
  k.omb1 = 1.0 - beta1;
  k.b2 = beta2;
  k.omb2 = 1.0 - beta2;
  k.c1 = lr / (1.0 - b1t);
  k.c2 = sqrt(1.0 - b2t);
  k.eps = eps;
  return k;
}

// pbg.h's element update: the unrounded md and vd enter p
__host__ __device__ __forceinline__ void adam_elem(const AdamK& k, float g, float& p, float& m, float& v) {
#pragma clang fp contract(off)
  const double gd = (double)g * k.coef;
  const double md = k.b1 * (double)m + k.omb1 * gd;
  const double vd = k.b2 * (double)v + k.omb2 * (gd * gd);
  p = (float)((double)p - k.c1 * (md / (sqrt(vd) / k.c2 + k.eps)));
  m = (float)md;
  v = (float)vd;
}

// the geometry of one block: G workgroups of OB lanes, lane l of workgroup w owns the groups of four consecutive
// elements q = w * OB + l + k * (G * OB), k = 0, 1, ...
inline int block_wgs(int64_t size) {
  const int64_t groups = (size + 3) / 4;
  const int64_t g = (groups + OB - 1) / OB;
  return (int)(g < OPT_MAX_WG ? g : OPT_MAX_WG);
}

// ---------------------------------------------------------------------------- kernels
__global__ __launch_bounds__(AN_LANES) void adv_norm_kernel(int Bm, const float* __restrict__ adv, const int64_t* __restrict__ idx,
                                                            float* __restrict__ out) {
  __shared__ double sh[AN_LANES];
  const double c0 = (double)adv[idx ? (size_t)idx[0] : (size_t)0];
  double s1 = 0.0, s2 = 0.0;
  for (long long i = (long long)threadIdx.x; i < Bm; i += AN_LANES)
    adv_norm_add(adv[idx ? (size_t)idx[i] : (size_t)i], c0, s1, s2);
  const double S1 = lds_tree<AN_LANES>(sh, s1);
  const double S2 = lds_tree<AN_LANES>(sh, s2);
  if (threadIdx.x == 0) adv_norm_finish(c0, S1, S2, Bm, out);
}

struct OptArgs {
  float* param[NBLK];
  const float* grad[NBLK];
  float* m[NBLK];
  float* v[NBLK];
  unsigned long long size[NBLK];
  int wg0[NBLK + 1];  // block b owns the workgroups wg0[b] .. wg0[b + 1] - 1
  int vec[NBLK];      // param and grad of the block are 16-byte aligned: float4 access
  int n_blocks;
  OptState* state;
  double* partial;  // [wg0[n_blocks]]
  double lr, beta1, beta2, eps, max_grad_norm;
  double* info;     // [2], nullable
  const double* lr_ptr;  // nullable: launch 2 reads the learning rate here instead of lr
  const int32_t* gate;   // nullable: gate[0] != 0 makes both launches leave everything as it is
};

// the block of workgroup `wg` and its fields, by selects: no indexed access into the argument struct
struct Mine {
  float* param;
  const float* grad;
  float* m;
  float* v;
  size_t size;
  int w, G, vec;
};

__device__ __forceinline__ Mine mine(const OptArgs& a, int wg) {
  Mine r{a.param[0], a.grad[0], a.m[0], a.v[0], (size_t)a.size[0], wg, a.wg0[1], a.vec[0]};
#pragma unroll
  for (int b = 1; b < NBLK; b++)
    if (b < a.n_blocks && wg >= a.wg0[b]) r = Mine{a.param[b], a.grad[b], a.m[b], a.v[b], (size_t)a.size[b], wg - a.wg0[b],
                                                   a.wg0[b + 1] - a.wg0[b], a.vec[b]};
  return r;
}

// launch 1: workgroup `wg`'s float64 sum of squares; lane 0 of workgroup 0 advances the state word, which this
// launch reads nowhere else and the next launch reads advanced
__global__ __launch_bounds__(OB) void ppoopt_sumsq_kernel(OptArgs a) {
  __shared__ double sh[OB];
  if (a.gate && a.gate[0] != 0) return;  // stopped: uniform over the launch; the state word does not advance
  const Mine b = mine(a, (int)blockIdx.x);
  const size_t groups = (b.size + 3) / 4, stride = (size_t)b.G * OB;
  double s = 0.0;
  for (size_t q = (size_t)b.w * OB + threadIdx.x; q < groups; q += stride) {
    const size_t e = 4 * q;
    if (b.vec && e + 4 <= b.size) {
      const float4 g = *reinterpret_cast<const float4*>(b.grad + e);
      s += (double)g.x * (double)g.x;
      s += (double)g.y * (double)g.y;
      s += (double)g.z * (double)g.z;
      s += (double)g.w * (double)g.w;
    } else {
      for (size_t i = e; i < e + 4 && i < b.size; i++) {
        const double g = (double)b.grad[i];
        s += g * g;
      }
    }
  }
  const double S = lds_tree<OB>(sh, s);
  if (threadIdx.x == 0) {
    a.partial[blockIdx.x] = S;
    if (blockIdx.x == 0) {
#pragma clang fp contract(off)
      OptState st = *a.state;
      st.t += 1u;
      st.b1t *= a.beta1;
      st.b2t *= a.beta2;
      *a.state = st;
    }
  }
}

// launch 2: every lane re-adds the partials in ascending order, then updates its elements
__global__ __launch_bounds__(OB) void ppoopt_step_kernel(OptArgs a) {
  if (a.gate && a.gate[0] != 0) return;  // stopped: no parameter, no moment and not info
  const int P = a.wg0[a.n_blocks];
  double sumsq = 0.0;
  for (int i = 0; i < P; i++) sumsq += a.partial[i];
  double norm;
  const double coef = opt_coef(sumsq, a.max_grad_norm, &norm);
  if (a.info && blockIdx.x == 0 && threadIdx.x == 0) {
    a.info[0] = norm;
    a.info[1] = coef;
  }
  const double lr = a.lr_ptr ? *a.lr_ptr : a.lr;  // a uniform load: one value for the launch
  const AdamK k = adam_factors(coef, lr, a.beta1, a.beta2, a.eps, a.state->b1t, a.state->b2t);
  const Mine b = mine(a, (int)blockIdx.x);
  const size_t groups = (b.size + 3) / 4, stride = (size_t)b.G * OB;
  for (size_t q = (size_t)b.w * OB + threadIdx.x; q < groups; q += stride) {
    const size_t e = 4 * q;
    if (e + 4 <= b.size) {
      // m and v are the object's: every block of them is 16-byte aligned
      float4 m = *reinterpret_cast<const float4*>(b.m + e), v = *reinterpret_cast<const float4*>(b.v + e);
      if (b.vec) {
        const float4 g = *reinterpret_cast<const float4*>(b.grad + e);
        float4 p = *reinterpret_cast<const float4*>(b.param + e);
        adam_elem(k, g.x, p.x, m.x, v.x);
        adam_elem(k, g.y, p.y, m.y, v.y);
        adam_elem(k, g.z, p.z, m.z, v.z);
        adam_elem(k, g.w, p.w, m.w, v.w);
        *reinterpret_cast<float4*>(b.param + e) = p;
      } else {
        adam_elem(k, b.grad[e], b.param[e], m.x, v.x);
        adam_elem(k, b.grad[e + 1], b.param[e + 1], m.y, v.y);
        adam_elem(k, b.grad[e + 2], b.param[e + 2], m.z, v.z);
        adam_elem(k, b.grad[e + 3], b.param[e + 3], m.w, v.w);
      }
      *reinterpret_cast<float4*>(b.m + e) = m;
      *reinterpret_cast<float4*>(b.v + e) = v;
    } else {
      for (size_t i = e; i < b.size; i++) adam_elem(k, b.grad[i], b.param[i], b.m[i], b.v[i]);
    }
  }
}

__global__ void ppoopt_reset_kernel(OptState* st) {
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    st->b1t = 1.0;
    st->b2t = 1.0;
    st->t = 0u;
  }
}

int adv_norm_args(const char* who, int n_batch, int n_rows, const float* adv, const int64_t* idx, const float* out) {
  if (n_rows < 2 || n_batch < 1 || (!idx && n_rows > n_batch) || !adv || !out) {
    char msg[200];
    snprintf(msg, sizeof(msg), "%s: n_rows %d must be >= 2, n_batch %d >= 1 (>= n_rows without idx), adv and out not NULL", who,
             n_rows, n_batch);
    return pbg::capi_fail(PBG_E_ARG, msg);
  }
  return PBG_OK;
}

// the struct's version, then the fields step and host share; copies the caller's struct into `io`
int check_io(const char* who, const pbg_ppo_opt_io_t* uio, int n_blocks, pbg_ppo_opt_io_t* io) {
  char msg[200];
  if (!uio) {
    snprintf(msg, sizeof(msg), "%s: io is NULL", who);
    return pbg::capi_fail(PBG_E_ARG, msg);
  }
  constexpr uint32_t v1_size = (uint32_t)(offsetof(pbg_ppo_opt_io_t, bpow) + sizeof(double*));
  constexpr uint32_t v2_size = (uint32_t)(offsetof(pbg_ppo_opt_io_t, lr_ptr) + sizeof(double*));
  // the three versions: the one that ends with bpow, the one that appends lr_ptr and this library's, which appends gate
  // and a reserved word (NULL for what a version lacks); the size between the last two stays refused
  if (const int rc = pbg::read_versioned(who, "pbg_ppo_opt_io_t", uio, {v1_size, v2_size, (uint32_t)sizeof(pbg_ppo_opt_io_t)}, io))
    return rc;
  for (int b = 0; b < n_blocks; b++)
    if (!io->param[b] || !io->grad[b]) {
      snprintf(msg, sizeof(msg), "%s: param[%d] or grad[%d] is NULL", who, b, b);
      return pbg::capi_fail(PBG_E_ARG, msg);
    }
  if (!(io->beta1 >= 0.0 && io->beta1 < 1.0 && io->beta2 >= 0.0 && io->beta2 < 1.0) || !(io->eps > 0.0)) {
    snprintf(msg, sizeof(msg), "%s: beta1 %g and beta2 %g must lie in [0, 1) and eps %g be > 0", who, io->beta1, io->beta2, io->eps);
    return pbg::capi_fail(PBG_E_ARG, msg);
  }
  return PBG_OK;
}

int check_sizes(const char* who, int n_blocks, const int64_t* sizes) {
  char msg[160];
  if (n_blocks < 1 || n_blocks > NBLK || !sizes) {
    snprintf(msg, sizeof(msg), "%s: n_blocks %d outside 1..%d or sizes NULL", who, n_blocks, NBLK);
    return pbg::capi_fail(PBG_E_ARG, msg);
  }
  for (int b = 0; b < n_blocks; b++)
    if (sizes[b] < 1) {
      snprintf(msg, sizeof(msg), "%s: sizes[%d] = %lld < 1", who, b, (long long)sizes[b]);
      return pbg::capi_fail(PBG_E_ARG, msg);
    }
  return PBG_OK;
}

}  // namespace

struct pbg_ppo_opt {
  int device, n_blocks;
  int64_t size[NBLK];
  size_t off[NBLK];  // block b's first element in m and in v (a multiple of 4 floats)
  size_t padded;     // floats of m (and of v)
  int wg0[NBLK + 1];
  void* ws;          // one allocation: the state word, the partials, m, v
  OptState* state;
  double* partial;
  float *m, *v;
};

extern "C" {

int pbg_adv_norm(int n_batch, int n_rows, const float* adv, const int64_t* idx, float* out, void* stream) {
  if (const int rc = adv_norm_args("pbg_adv_norm", n_batch, n_rows, adv, idx, out)) return rc;
  hipLaunchKernelGGL(adv_norm_kernel, dim3(1), dim3(AN_LANES), 0, (hipStream_t)stream, n_rows, adv, idx, out);
  return launched("adv_norm_kernel launch");
}

int pbg_adv_norm_host(int n_batch, int n_rows, const float* adv, const int64_t* idx, float* out) {
  if (const int rc = adv_norm_args("pbg_adv_norm_host", n_batch, n_rows, adv, idx, out)) return rc;
  if (idx)
    for (int i = 0; i < n_rows; i++)
      if (idx[i] < 0 || idx[i] >= (int64_t)n_batch)
        return pbg::capi_fail(PBG_E_ARG, "pbg_adv_norm_host: an index is outside 0 .. n_batch - 1");
  double s1[AN_LANES], s2[AN_LANES];
  for (int l = 0; l < AN_LANES; l++) s1[l] = s2[l] = 0.0;
  const double c0 = (double)adv[idx ? (size_t)idx[0] : (size_t)0];
  for (int i = 0; i < n_rows; i++)  // i ascending visits every lane's rows ascending
    adv_norm_add(adv[idx ? (size_t)idx[i] : (size_t)i], c0, s1[i % AN_LANES], s2[i % AN_LANES]);
  host_tree(s1, AN_LANES);
  host_tree(s2, AN_LANES);
  adv_norm_finish(c0, s1[0], s2[0], n_rows, out);
  return PBG_OK;
}

int pbg_ppo_opt_create(int device, int n_blocks, const int64_t* sizes, pbg_ppo_opt** out) {
  if (!out) return pbg::capi_fail(PBG_E_ARG, "pbg_ppo_opt_create: out is NULL");
  *out = nullptr;
  if (const int rc = check_sizes("pbg_ppo_opt_create", n_blocks, sizes)) return rc;
  if (device < 0) return pbg::capi_fail(PBG_E_ARG, "pbg_ppo_opt_create: device < 0");
  if (const int rc = check_device("pbg_ppo_opt_create", device)) return rc;
  pbg_ppo_opt* o = new (std::nothrow) pbg_ppo_opt();
  if (!o) return pbg::capi_fail(PBG_E_NOMEM, "pbg_ppo_opt_create: out of host memory");
  o->device = device;
  o->n_blocks = n_blocks;
  o->wg0[0] = 0;
  size_t at = 0;
  for (int b = 0; b < NBLK; b++) {
    o->size[b] = b < n_blocks ? sizes[b] : 0;
    o->off[b] = at;
    o->wg0[b + 1] = o->wg0[b] + (b < n_blocks ? block_wgs(sizes[b]) : 0);
    at += (size_t)((o->size[b] + 3) / 4) * 4;
  }
  o->padded = at;
  const size_t head = sizeof(OptState) + (size_t)NBLK * OPT_MAX_WG * sizeof(double);  // a multiple of 16
  const size_t bytes = head + 2 * at * sizeof(float);
  DeviceGuard dg(device);
  int e = (int)hipMalloc(&o->ws, bytes);
  if (!e) e = (int)hipMemset(o->ws, 0, bytes);
  if (e) {
    if (o->ws) (void)hipFree(o->ws);
    delete o;
    return hip_fail(e, "pbg_ppo_opt_create: storage");
  }
  o->state = reinterpret_cast<OptState*>(o->ws);
  o->partial = reinterpret_cast<double*>(o->state + 1);
  o->m = reinterpret_cast<float*>(reinterpret_cast<char*>(o->ws) + head);
  o->v = o->m + at;
  // the state word by the reset kernel: this unit's code object is then loaded before a first step, which may be
  // one that a stream capture records
  hipLaunchKernelGGL(ppoopt_reset_kernel, dim3(1), dim3(64), 0, (hipStream_t) nullptr, o->state);
  e = (int)hipGetLastError();
  if (!e) e = (int)hipStreamSynchronize(nullptr);
  if (e) {
    pbg_ppo_opt_destroy(o);
    return hip_fail(e, "pbg_ppo_opt_create: state");
  }
  *out = o;
  return PBG_OK;
}

void pbg_ppo_opt_destroy(pbg_ppo_opt* o) {
  if (!o) return;
  if (o->ws) {
    DeviceGuard dg(o->device);
    (void)hipFree(o->ws);
  }
  delete o;
}

int pbg_ppo_opt_step(pbg_ppo_opt* o, const pbg_ppo_opt_io_t* uio, void* stream) {
  if (!o) return pbg::capi_fail(PBG_E_ARG, "pbg_ppo_opt_step: the object is NULL");
  pbg_ppo_opt_io_t io;
  if (const int rc = check_io("pbg_ppo_opt_step", uio, o->n_blocks, &io)) return rc;
  OptArgs a;
  memset(&a, 0, sizeof(a));
  for (int b = 0; b < o->n_blocks; b++) {
    a.param[b] = io.param[b];
    a.grad[b] = io.grad[b];
    a.m[b] = o->m + o->off[b];
    a.v[b] = o->v + o->off[b];
    a.size[b] = (unsigned long long)o->size[b];
    a.vec[b] = (((uintptr_t)io.param[b] | (uintptr_t)io.grad[b]) & 15u) == 0;
  }
  for (int b = 0; b <= NBLK; b++) a.wg0[b] = o->wg0[b];
  a.n_blocks = o->n_blocks;
  a.state = o->state;
  a.partial = o->partial;
  a.lr = io.lr; a.beta1 = io.beta1; a.beta2 = io.beta2; a.eps = io.eps; a.max_grad_norm = io.max_grad_norm;
  a.info = io.info;
  a.lr_ptr = io.lr_ptr;
  a.gate = io.gate;
  DeviceGuard dg(o->device);
  const unsigned G = (unsigned)o->wg0[o->n_blocks];
  hipLaunchKernelGGL(ppoopt_sumsq_kernel, dim3(G), dim3(OB), 0, (hipStream_t)stream, a);
  if (const int rc = launched("ppoopt_sumsq_kernel launch")) return rc;
  hipLaunchKernelGGL(ppoopt_step_kernel, dim3(G), dim3(OB), 0, (hipStream_t)stream, a);
  return launched("ppoopt_step_kernel launch");
}

int pbg_ppo_opt_reset(pbg_ppo_opt* o, void* stream) {
  if (!o) return pbg::capi_fail(PBG_E_ARG, "pbg_ppo_opt_reset: the object is NULL");
  DeviceGuard dg(o->device);
  const int e = (int)hipMemsetAsync(o->m, 0, 2 * o->padded * sizeof(float), (hipStream_t)stream);
  if (e) return hip_fail(e, "pbg_ppo_opt_reset: memset");
  hipLaunchKernelGGL(ppoopt_reset_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, o->state);
  return launched("ppoopt_reset_kernel launch");
}

int pbg_ppo_opt_get_state(const pbg_ppo_opt* o, float* m_out, float* v_out, uint32_t* t_out, void* stream) {
  if (!o) return pbg::capi_fail(PBG_E_ARG, "pbg_ppo_opt_get_state: the object is NULL");
  DeviceGuard dg(o->device);
  hipStream_t s = (hipStream_t)stream;
  size_t at = 0;
  int e = 0;
  for (int b = 0; b < o->n_blocks && !e; b++) {
    const size_t bytes = (size_t)o->size[b] * sizeof(float);
    if (m_out) e = (int)hipMemcpyAsync(m_out + at, o->m + o->off[b], bytes, hipMemcpyDeviceToDevice, s);
    if (v_out && !e) e = (int)hipMemcpyAsync(v_out + at, o->v + o->off[b], bytes, hipMemcpyDeviceToDevice, s);
    at += (size_t)o->size[b];
  }
  if (t_out && !e) e = (int)hipMemcpyAsync(t_out, &o->state->t, sizeof(uint32_t), hipMemcpyDeviceToDevice, s);
  return e ? hip_fail(e, "pbg_ppo_opt_get_state: copy") : PBG_OK;
}

int pbg_ppo_opt_host(int n_blocks, const int64_t* sizes, const pbg_ppo_opt_io_t* uio) {
  if (const int rc = check_sizes("pbg_ppo_opt_host", n_blocks, sizes)) return rc;
  pbg_ppo_opt_io_t io;
  if (const int rc = check_io("pbg_ppo_opt_host", uio, n_blocks, &io)) return rc;
  for (int b = 0; b < n_blocks; b++)
    if (!io.m[b] || !io.v[b]) return pbg::capi_fail(PBG_E_ARG, "pbg_ppo_opt_host: a block's m or v is NULL");
  if (!io.t || !io.bpow) return pbg::capi_fail(PBG_E_ARG, "pbg_ppo_opt_host: t or bpow is NULL");
  if (io.gate && io.gate[0] != 0) return PBG_OK;  // stopped: the parameters, the state and info keep what they held
  // launch 1: the partials in the device's geometry
  double sumsq = 0.0;
  double lanes[OB];
  for (int b = 0; b < n_blocks; b++) {
    const size_t size = (size_t)sizes[b], groups = (size + 3) / 4;
    const int G = block_wgs(sizes[b]);
    const size_t stride = (size_t)G * OB;
    for (int w = 0; w < G; w++) {
      for (int l = 0; l < OB; l++) {
        double s = 0.0;
        for (size_t q = (size_t)w * OB + l; q < groups; q += stride)
          for (size_t i = 4 * q; i < 4 * q + 4 && i < size; i++) {
            const double g = (double)io.grad[b][i];
            s += g * g;
          }
        lanes[l] = s;
      }
      host_tree(lanes, OB);
      sumsq += lanes[0];  // launch 2's ascending re-add
    }
  }
  {
#pragma clang fp contract(off)
    *io.t += 1u;
    io.bpow[0] *= io.beta1;
    io.bpow[1] *= io.beta2;
  }
  double norm;
  const double coef = opt_coef(sumsq, io.max_grad_norm, &norm);
  if (io.info) {
    io.info[0] = norm;
    io.info[1] = coef;
  }
  const AdamK k = adam_factors(coef, io.lr_ptr ? *io.lr_ptr : io.lr, io.beta1, io.beta2, io.eps, io.bpow[0], io.bpow[1]);
  for (int b = 0; b < n_blocks; b++)
    for (size_t i = 0; i < (size_t)sizes[b]; i++) adam_elem(k, io.grad[b][i], io.param[b][i], io.m[b][i], io.v[b][i]);
  return PBG_OK;
}

}  // extern "C"
