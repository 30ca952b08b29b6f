// pbg_ppogate.hip -- the KL gate of the PPO update (include/pbg.h "Value clipping and the KL gate"; DESIGN.md section
// 21): the two one-lane launches that alone write the gate's words (pbg_ppo_gate, pbg_ppo_gate_reset) and the host
// twin (pbg_ppo_gate_host).  Every other launch of the update only reads the words: the gradient's tile kernels and
// reduction (pbg_ppograd.hip, pbg_ppograd_mfma.hip) and the optimiser's two launches (pbg_ppoopt.hip).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pbg_policy_dev.h"

namespace {

using namespace pbg::policy;  // hip_fail

// the gate's step, host and device: plain loads and stores of one lane
__host__ __device__ __forceinline__ void gate_step(const double* stats, double kl_limit, int32_t* gate) {
  if (gate[0] != 0) return;
  if (stats[3] > kl_limit) gate[0] = 1;  // a NaN compares false: it does not stop
  else gate[1] += 1;
}

__global__ void ppo_gate_kernel(const double* stats, double kl_limit, int32_t* gate) {
  if (blockIdx.x == 0 && threadIdx.x == 0) gate_step(stats, kl_limit, gate);
}

__global__ void ppo_gate_reset_kernel(int32_t* gate) {
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    gate[0] = 0;
    gate[1] = 0;
  }
}

}  // namespace

extern "C" {

int pbg_ppo_gate_reset(int32_t* gate, void* stream) {
  if (!gate) return pbg::capi_fail(PBG_E_ARG, "pbg_ppo_gate_reset: gate is NULL");
  hipLaunchKernelGGL(ppo_gate_reset_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, gate);
  return launched("ppo_gate_reset_kernel launch");
}

int pbg_ppo_gate(const double* stats, double kl_limit, int32_t* gate, void* stream) {
  if (!stats || !gate) return pbg::capi_fail(PBG_E_ARG, "pbg_ppo_gate: stats or gate is NULL");
  hipLaunchKernelGGL(ppo_gate_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, stats, kl_limit, gate);
  return launched("ppo_gate_kernel launch");
}

int pbg_ppo_gate_host(const double* stats, double kl_limit, int32_t* gate) {
  if (!stats || !gate) return pbg::capi_fail(PBG_E_ARG, "pbg_ppo_gate_host: stats or gate is NULL");
  gate_step(stats, kl_limit, gate);
  return PBG_OK;
}

}  // extern "C"
