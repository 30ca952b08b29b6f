// The host-side interface of a robot's translation unit (pbg_robot.hip with -DPBG_ROBOT=<Name>, one unit per
// robot of models_gen.h's PBG_ROBOTS so the template instantiations build in parallel): the kernel plan and
// one accessor per robot that returns its launcher table.  pbg_capi.hip dispatches on the robot id.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "models_gen.h"

namespace pbg {
struct Buffers;
struct StepIO;
struct ResetIO;

// one CU's LDS (gfx950: 160 KiB), which all of its resident workgroups share
constexpr int CU_LDS_BYTES = 163840;

// what pbg_create_v2's options ask of the plan
struct PlanRequest {
  int mode;        // 0 = the lane kernel, 1 = default (quad for Ant, gang for the other walkers), 2 = gang
  int gang_dist;   // -1 = plan's choice, 0 / 1 = force Geometry::gang_dist
  int gang_lanes;  // -1 = plan's choice, 16 / 32 = gang width
};

// the plan: the step kernel selected for a handle and its launch geometry
struct Geometry {
  int team;          // lanes per env: 1 (step_kernel), 4 (team_step_kernel, pbg_team.hip) or
                     // 16 / 32 (gang_step_kernel, pbg_gang.hip)
  int block;         // lanes per step workgroup: 16, 32 or 64
  int lds_rows;      // contact-constraint rows (gang: contacts) resident in LDS per env
  int env_words;     // gang: LDS words per env
  int gang_dist;     // gang: distributed (1) or replicated (0) unconstrained dynamics
  size_t lds_bytes;  // dynamic LDS per step workgroup
  size_t scratch_words_per_env;
  int vgprs;          // the selected step kernel's registers per lane (hipFuncGetAttributes)
  int scratch_bytes;  // and its private segment per lane
  int word_bytes = 4; // bytes per constraint-row / workspace word: 4 (float32 kernels) or 8 (float64)
};

// a robot's launchers of one precision
struct Kern {
  int (*plan)(int n_envs, int cus, const PlanRequest& rq, Geometry* g);
  int (*step)(const Buffers& B, const StepIO& io, float* scratch, const Geometry& g, hipStream_t s);
  int (*reset)(const Buffers& B, const ResetIO& io, hipStream_t s);
  int (*get_state)(const Buffers& B, double* phys, double* aux, hipStream_t s);
  int (*set_state)(const Buffers& B, const double* phys, const double* aux, hipStream_t s);
};
struct RobotOps {
  Kern k32;                                                          // the float32 kernels
  int (*pack)(int n, const double* in, double* out, hipStream_t s);  // pbg_pack: the observation pack alone
  Kern k64;                                                          // the float64 (reference-precision) kernels
  int (*stamps)(unsigned long long* host_out);  // -DPBG_STAMPS builds: read and clear the phase stamps
};

#define PBG_DECLARE_ROBOT(NAME, ID, ENV, KEY) const RobotOps& robot_ops_##NAME();
PBG_ROBOTS(PBG_DECLARE_ROBOT)
#undef PBG_DECLARE_ROBOT
}  // namespace pbg
