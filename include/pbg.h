/* pbg.h -- C-ABI of the MI355X batched locomotion stepper (libpbg_amd.so).
 *
 * The reference (josiahls/pybullet-gym) has no native boundary of its own: its hot path
 * calls the pybullet C extension once per query, per env, through
 * pybullet_envs.bullet.bullet_client.BulletClient (pybulletgym/envs/roboschool/
 * env_bases.py:4,51-56).  This ABI replaces that whole per-env call sequence with one
 * batched call per env step.  Each entry point names the reference interface it replaces.
 *
 * Conventions
 *   - All array arguments are DEVICE pointers (HIP / PyTorch-ROCm tensors), row-major,
 *     except where marked "host".  The caller owns every I/O buffer; the handle owns its
 *     struct-of-arrays state.  Nothing allocates or synchronises inside step/reset.
 *   - `stream` is a hipStream_t (NULL = the legacy default stream); work is async on it.
 *   - Return 0 on success, a negative PBG_E_* code on failure; pbg_last_error() gives
 *     the message (thread-local).
 *   - One handle = the envs of one GPU.  Multi-GPU: one handle per rank, env_offset =
 *     global index of the rank's first env (reset RNG streams depend on the global id).
 */
#ifndef PBG_H
#define PBG_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PBG_OK 0
#define PBG_E_ARG (-1)
#define PBG_E_ENV (-2)
#define PBG_E_HIP (-3)
#define PBG_E_NOMEM (-4)

/* Layout version of the per-env state records of pbg_get_state / pbg_set_state (reported in
 * pbg_info_t.record_version).  1: round-1 aux record (no episode counter); 2: aux ends with
 * the episodes-started counter (the reset-noise Philox counter).  A checkpoint written under
 * another version must not be passed to pbg_set_state (the aux width differs). */
#define PBG_RECORD_VERSION 2

typedef struct pbg_handle pbg_handle;

typedef struct {
  int robot_id;          /* 0 pendulum, 1 hopper, 2 halfcheetah, 3 ant, 4 humanoid, 5 walker2d,
                            6 pendulum_swingup, 7 double_pendulum, 8 humanoid_flagrun,
                            9 hopper_mujoco, 10 walker2d_mujoco, 11 halfcheetah_mujoco,
                            12 ant_mujoco, 13 humanoid_mujoco, 14 double_pendulum_mujoco,
                            15 humanoid_flagrun_harder, 16 atlas */
  int n_envs;
  int action_dim;        /* action_space.shape[0]   (robot_bases.py:24-25) */
  int obs_dim;           /* observation_space.shape[0] (robot_bases.py:26-27) */
  int n_dof;             /* generalized velocities (6 floating-base + joint dofs) */
  int n_joints;          /* joint dofs incl. `ignore*` joints */
  int n_links;
  int n_feet;
  int state_words;       /* per-env physical state record (see pbg_get_state) */
  int aux_words;         /* per-env bookkeeping record (see pbg_get_state) */
  int substeps;          /* stepSimulation sub-steps per env step (the handle's frame_skip,
                            scene_bases.py:73 numSubSteps) */
  int max_episode_steps; /* gym TimeLimit (envs/__init__.py) */
  int reset_dofs;        /* joints randomised by reset (robot_locomotors.py:18-19) */
  int floating;
  int lanes_per_env;     /* step kernel geometry: 1 (lane per env), 4 (quad) or 16 (gang) */
  int block;             /* step kernel workgroup size (lanes) */
  int lds_bytes;         /* dynamic LDS per step workgroup */
  int vgprs;             /* step kernel registers per lane (hipFuncGetAttributes numRegs) */
  int scratch_bytes;     /* step kernel private segment per lane (0: no spills to memory) */
  int lds_rows;          /* contact rows (gang: contacts) resident in LDS per env */
  int record_version;    /* PBG_RECORD_VERSION of the state / aux records (appended in round 3) */
} pbg_info_t;

typedef struct {
  const float* act;   /* [n, action_dim] float32 */
  float* obs;         /* [n, obs_dim] float32: next observation (post-reset if auto-reset) */
  float* rew;         /* [n] float32 reward (computed in float64) */
  uint8_t* done;      /* [n] terminated | truncated */
  double* rew64;      /* nullable [n] float64 reward */
  uint8_t* trunc;     /* nullable [n] TimeLimit truncation flag */
  float* term_obs;    /* nullable [n, obs_dim] observation before an auto-reset */
  int32_t* ncontact;  /* nullable [n] contact points in the last sub-step */
  int autoreset;      /* reset envs that finished, inside the same launch */
  double* rew_terms;  /* nullable [n, 5] float64: the terms the reward sums, in the order of the
                         reference's self.rewards list, zero-padded -- walkers: alive, progress,
                         electricity, joints_at_limit, feet_collision (gym_locomotion_envs.py:99-105);
                         MuJoCo Ant/Humanoid: alive, progress, joints_at_limit, feet_collision
                         (mujoco/gym_locomotion_envs.py:98-103); MuJoCo planar: potential,
                         [alive,] power_cost; pendulums: their rewards list */
  uint32_t* csig;     /* nullable [n] contact-set signature of the env step: the sum mod 2^32 of
                         fmix32((substep << 16) + candidate + 0x9E3779B9) over every active collision
                         candidate (floor slots 0..NS-1, self pairs NS + p; HumanoidFlagrunHarder's
                         cube corners NS + NPAIR + k, cube vs robot geom NS + NPAIR + 8 + g) of every
                         sub-step (sim_params.h pbg_contact_hash; for parity tests) */
} pbg_step_io_t;

/* Test / diagnostic launch options (pbg_create_debug / pbg_create_ex).  -1 = the default everywhere.
 * ABI note: round 4 appended gang_lanes (3 -> 4 ints) without a size field; the struct is frozen at
 * these four ints.  Callers that need another option use pbg_create_v2 (pbg_create_opts_t is
 * versioned by its struct_size). */
typedef struct {
  int kernel;     /* 0: one-lane-per-env kernel for every robot (PBG_E_ARG for Atlas, whose 886
                     contact slots have no lane kernel, in either precision); 2: the 16-lane gang
                     kernel for every walker (Ant included); -1 / 1: default (quad for Ant, gang
                     otherwise) */
  int lds_rows;   /* k >= 0: at most k contact rows (gang: contacts) per env resident in LDS,
                     the rest in the device workspace (bitwise-equality tests of that path) */
  int gang_dist;  /* 0 / 1: force replicated / distributed gang dynamics (PBG_E_ARG when the planned
                     kernel is no gang kernel or has no such variant: 32-lane gangs and
                     HumanoidFlagrunHarder are distributed only) */
  int gang_lanes; /* 16 / 32: gang width (32: the Humanoid family only); PBG_E_ARG when the planned
                     kernel is not a gang kernel of that width (Ant's quad plan, kernel = 0) */
} pbg_debug_opts_t;

/* Scene / World parameters (scene_bases.py:8-18 Scene(gravity, timestep, frame_skip), 58-73
 * World: setGravity, numSolverIterations, numSubSteps).  pbg_default_sim_params fills the values
 * the reference's env constructs its scene with (gym_locomotion_envs.py:18-19 StadiumScene(9.8,
 * 0.0165/4, 4); Atlas StadiumScene(9.8, 0.0165/8, 8), gym_locomotion_envs.py:187;
 * gym_pendulum_envs.py:14 SingleRobotEmptyScene(9.8, 0.0165, 1); iterations 5,
 * scene_bases.py:65) plus the solver ERPs the kernels use; pbg_create_ex takes a modified copy.
 * An env step is frame_skip sub-steps of `timestep` seconds; the potential divides by
 * Scene.dt = timestep * frame_skip (scene_bases.py:17); HumanoidFlagrun's flag timeout is
 * 600 / frame_skip steps (robot_locomotors.py:218). */
typedef struct {
  double gravity;         /* m/s^2 along -z (World.gravity; 0 = weightless) */
  double timestep;        /* seconds per physics sub-step (Scene.timestep), in (0, 0.1] */
  int frame_skip;         /* sub-steps per env step (Scene.frame_skip = numSubSteps), 1..64 */
  int solver_iterations;  /* PGS sweeps per sub-step (World.numSolverIterations), 1..1000 */
  double contact_erp;     /* [0, 1]: share of a contact penetration corrected per sub-step */
  double joint_limit_erp; /* [0, 1]: share of a joint-limit violation corrected per sub-step */
} pbg_sim_params_t;

/* Options of pbg_create_v2, versioned: set struct_size = sizeof(pbg_create_opts_t) of the header the
 * caller was built with; the library reads only the fields that size covers (fields past it take
 * their defaults), so options appended later never read past an older caller's struct. */
typedef struct {
  uint32_t struct_size;  /* sizeof(pbg_create_opts_t) at the caller's build */
  int precision;         /* physics state and arithmetic: 64 = float64 (the default since round 6,
                            as for pbg_create / pbg_create_ex: the reference's precision, pybullet's
                            btScalar is double: stepSimulation, scene_bases.py:75-76) or 32 =
                            float32, the opt-in fast kernels.  The observation / reward pack is
                            float64 in both, as in the reference.  Every env id has both
                            (AtlasPyBulletEnv-v0: the gang kernel only) */
  int kernel;            /* as in pbg_debug_opts_t.  Precision 64: 1 (default) = the quad kernel for
                            Ant, the 16-lane gang kernel for the other walkers, the lane kernel for
                            the pendulums; 0 = the lane kernel for every robot; 2 = the gang kernel
                            for every walker (Ant included) */
  int lds_rows;
  int gang_dist;
  int gang_lanes;
} pbg_create_opts_t;

/* The reference's parameters for env_id (see pbg_sim_params_t). */
int pbg_default_sim_params(const char* env_id, pbg_sim_params_t* out);

/* gym.make(env_id) for n envs (envs/__init__.py:4-103 registry entries; the env's
 * physics client is created here instead of lazily in BaseBulletEnv._reset,
 * env_bases.py:46-56), with float64 physics (the reference's precision; pbg_create_v2 selects
 * float32).  env_id (robot_id order): "InvertedPendulumPyBulletEnv-v0",
 * "HopperPyBulletEnv-v0", "HalfCheetahPyBulletEnv-v0", "AntPyBulletEnv-v0",
 * "HumanoidPyBulletEnv-v0", "Walker2DPyBulletEnv-v0", "InvertedPendulumSwingupPyBulletEnv-v0",
 * "InvertedDoublePendulumPyBulletEnv-v0", "HumanoidFlagrunPyBulletEnv-v0", "HopperMuJoCoEnv-v0",
 * "Walker2DMuJoCoEnv-v0", "HalfCheetahMuJoCoEnv-v0", "AntMuJoCoEnv-v0", "HumanoidMuJoCoEnv-v0",
 * "InvertedDoublePendulumMuJoCoEnv-v0", "HumanoidFlagrunHarderPyBulletEnv-v0",
 * "AtlasPyBulletEnv-v0" (gym_locomotion_envs.py:181-188) (the short robot names are accepted
 * too). */
int pbg_create(const char* env_id, int n_envs, int device, uint64_t seed, int env_offset, pbg_handle** out);
/* pbg_create with test / diagnostic launch options (opts NULL = pbg_create). */
int pbg_create_debug(const char* env_id, int n_envs, int device, uint64_t seed, int env_offset,
                     const pbg_debug_opts_t* opts, pbg_handle** out);
/* pbg_create with the scene built from `params` (NULL = pbg_default_sim_params) and test /
 * diagnostic launch options (NULL = defaults).  PBG_E_ARG for parameters out of range. */
int pbg_create_ex(const char* env_id, int n_envs, int device, uint64_t seed, int env_offset,
                  const pbg_sim_params_t* params, const pbg_debug_opts_t* opts, pbg_handle** out);
/* pbg_create_ex with versioned options (opts NULL = defaults: float64, the default kernels).
 * PBG_E_ARG for a bad struct_size (not a multiple of 4 in [8, sizeof]) or precision, and for a
 * launch option the planned kernel cannot honour (in either precision); PBG_E_HIP when no kernel
 * plan fits the device.  *out is NULL after every failure. */
int pbg_create_v2(const char* env_id, int n_envs, int device, uint64_t seed, int env_offset,
                  const pbg_sim_params_t* params, const pbg_create_opts_t* opts, pbg_handle** out);
/* The handle's physics precision: 32 or 64 (PBG_E_ARG for NULL). */
int pbg_precision(const pbg_handle* h);
/* The parameters a handle was created with. */
int pbg_get_sim_params(const pbg_handle* h, pbg_sim_params_t* out);
/* BaseBulletEnv._close (env_bases.py:103-107) */
void pbg_destroy(pbg_handle* h);
/* action_space / observation_space / model sizes (robot_bases.py:24-27) */
int pbg_info(const pbg_handle* h, pbg_info_t* out);

/* WalkerBaseBulletEnv._reset (gym_locomotion_envs.py:22-39) + BaseBulletEnv._reset
 * (env_bases.py:46-71) + robot_specific_reset (robot_locomotors.py:16-24):
 * restoreState snapshot, resetJointState(U(-0.1,0.1)) on the ordered joints, calc_state.
 * mask: nullable [n] uint8 (NULL = all envs).  init_q: nullable [n, reset_dofs] float32
 * joint positions to use instead of the RNG (trace replay).  obs: [n, obs_dim]. */
int pbg_reset(pbg_handle* h, const uint8_t* mask, const float* init_q, float* obs, void* stream);

/* WalkerBaseBulletEnv._step (gym_locomotion_envs.py:54-114): apply_action
 * (robot_locomotors.py:26-29) -> stepSimulation x substeps (scene_bases.py:75-76) ->
 * calc_state / potential / alive / feet contacts / costs.  No auto-reset.
 * act: [n, action_dim] float32, clipped to [-1, 1] for the torques (+-inf -> +-1, NaN -> -1: IEEE
 * max); the electricity cost takes the unclipped value (a NaN action gives a NaN reward).  The
 * reference asserts finite actions (robot_locomotors.py:27); the per-env facade does too, the
 * batch API does not check them (that would cost a host sync per step). */
int pbg_step(pbg_handle* h, const float* act, float* obs, float* rew, uint8_t* done, void* stream);
/* pbg_step with optional outputs and in-launch auto-reset (gym TimeLimit + reset). */
int pbg_step_ex(pbg_handle* h, const pbg_step_io_t* io, void* stream);

/* pybullet saveState/restoreState (gym_locomotion_envs.py:25,36) generalised to trace
 * replay / teacher forcing / checkpoints.  phys: [n, state_words] float64 records
 *   [0..2] base COM pos, [3..6] base quat (x,y,z,w), [7..9] base COM lin vel (world),
 *   [10..12] base ang vel (world), then q[n_joints], qd[n_joints], (HumanoidFlagrunHarder: the
 *   cube's 13 words in the base's layout);
 * aux: [n, aux_words] float64 = [potential, initial_z, elapsed_steps, floor_in_parts,
 *   feet_contact[n_feet], (HumanoidFlagrun / Harder: walk target x, y, flag_timeout, flag draws),
 *   (HumanoidFlagrunHarder: frame, on_ground_frame_counter, crawl_start_potential (NaN = None),
 *   crawl_ignored_potential, cube launches), episodes started (the reset-noise RNG counter)],
 *   layout PBG_RECORD_VERSION (the Harder words are new robot-specific words, not a change of
 *   any existing robot's layout).
 * set_state with aux == NULL replaces the physical state only: the handle keeps its own
 * bookkeeping -- potential, initial_z, elapsed steps, feet flags and the episode counter --
 * so later resets continue that handle's reset-noise stream, not the checkpoint's. */
int pbg_get_state(pbg_handle* h, double* phys, double* aux, void* stream);
int pbg_set_state(pbg_handle* h, const double* phys, const double* aux, void* stream);

/* Test support: fill every CU's LDS (160 KB each) with the 32-bit pattern and, when h is not NULL,
 * h's device workspace (the contact / limit rows past the LDS capacity), stream-ordered before the
 * next launch.  The kernels write everything they read in a launch, so a step after a poison must
 * give the same bits whatever the pattern (tests/test_gpu.py test_uninitialised_memory_invariance).
 * h NULL: the current device's LDS only. */
int pbg_debug_poison(pbg_handle* h, uint32_t pattern, void* stream);

/* The observation/reward/done pack alone (calc_state + the reward half of _step) on
 * explicit inputs, for golden-vector parity; layouts in pbg_pack_record_sizes. */
int pbg_pack_record_sizes(const char* env_id, int* in_words, int* out_words);
int pbg_pack(const char* env_id, int n, const double* in_rec, double* out_rec, void* stream);

/* Batched action_space.sample() (robot_bases.py:24-25 Box(-1, 1)): out[s, e, i] = U(-1, 1)
 * float32 for s < n_steps, e < n_envs, i < action_dim; Philox4x32-10, key = seed, counter =
 * (step0 + s, env_offset + e, i / 4, 0xAC7) -- the bench's random-action protocol
 * (BASELINE.md section 2), independent of the sharding.  out: device [n_steps, n_envs, action_dim];
 * the kernel runs on the device that owns `out` (pbg_pack likewise on its records' device).
 * These two handle-less entry points take device (hipMalloc) or managed memory only: a host or
 * pinned-host (hipHostMalloc) pointer has no owning device and returns PBG_E_ARG. */
int pbg_sample_actions(int action_dim, int n_envs, int n_steps, uint64_t seed, uint32_t step0, int env_offset,
                       float* out, void* stream);

const char* pbg_last_error(void);

/* ---- The pretrained-policy closed loop (appended; nothing above changes) ----
 * The reference's enjoy scripts (examples/roboschool-weights/enjoy_TF_*.py) load a three-layer ReLU
 * MLP, SmallReactivePolicy (:21-31: relu(x w1 + b1) -> relu(. w2 + b2) -> . w3 + b3), and run
 * env.step(pi.act(obs)) until the episode ends.  A pbg_policy is that MLP; one kernel launch
 * evaluates all three layers for a batch of observations.
 *
 * Numeric contract (host and device give the same floats for every input): every output of a layer
 * is a k-ascending fused-multiply-add chain started from the bias,
 *   acc = b[j]; for k = 0..K-1: acc = fmaf(x[k], W[k][j], acc);
 * the hidden layers then apply  acc < 0 ? 0 : acc  (a NaN passes through, as np.maximum does). */
typedef struct pbg_policy pbg_policy;

#define PBG_POLICY_MAX_DIM 256 /* obs_dim, h1, h2 */
#define PBG_POLICY_MAX_ACT 64  /* act_dim */

/* weights: HOST float32, the reference's layout (enjoy_TF_*.py:21-31): w1[obs_dim,h1] b1[h1]
 * w2[h1,h2] b2[h2] w3[h2,act_dim] b3[act_dim], row-major; copied, the caller keeps its own.
 * 1 <= obs_dim, h1, h2 <= 256 and 1 <= act_dim <= 64, nothing need be a multiple of anything.
 * device >= 0: uploaded there.  device == -1: host-only policy (no HIP call at all).
 * PBG_E_ARG (before any HIP call) for dims out of range, a NULL array or device < -1; PBG_E_HIP
 * for a device that does not exist.  *out is NULL after every failure. */
int pbg_policy_create(int device, int obs_dim, int h1, int h2, int act_dim, const float* w1, const float* b1,
                      const float* w2, const float* b2, const float* w3, const float* b3, pbg_policy** out);
void pbg_policy_destroy(pbg_policy* p);
/* act[n, act_dim] = pi(obs[n, obs_dim]), device pointers on the policy's device, one launch, async
 * on `stream`; rows past n are neither read nor written.  PBG_E_ARG on a host-only policy. */
int pbg_policy_act(const pbg_policy* p, int n, const float* obs, float* act, void* stream);
/* The same floats on the CPU (host pointers; any policy, host-only or not). */
int pbg_policy_act_host(const pbg_policy* p, int n, const float* obs, float* act);

/* Buffers of a closed-loop rollout, all caller-owned DEVICE memory of the handle's GPU, n = the
 * handle's n_envs, T = n_steps.  Versioned by struct_size like pbg_create_opts_t: set it to
 * sizeof(pbg_rollout_io_t) of the header the caller was built with; the library reads only the
 * fields that size covers (fields appended after done_traj, the end of the first version, take zero),
 * so a caller built with an older header keeps working.  Two sizes exist: the first version's, which ends
 * with done_traj, and version 2's, which appends trunc_traj and term_obs_traj.  PBG_E_ARG for any other
 * size.
 *
 * Version 2, truncation records.  trunc_traj and term_obs_traj are given both or
 * neither, and only with autoreset != 0: any other combination is PBG_E_ARG before any launch.  In step t
 * the handle's step gets row t of the two arrays as pbg_step_io_t.trunc / .term_obs and writes them as it
 * does there: trunc_traj[t][e] for every env (truncated by the TimeLimit and not terminated), and row
 * (t, e) of term_obs_traj, the observation before env e's reset, ONLY where done_traj[t][e] (or done[e]
 * without trajectories) is set.  Every other row of term_obs_traj is never written and must never be
 * read.  The launches stay 2 T + 1 and nothing else the rollout produces changes. */
typedef struct {
  uint32_t struct_size;
  int n_steps;            /* T >= 1 */
  int autoreset;          /* as pbg_step_io_t.autoreset.  0: an env that has finished an episode
                             (done_episodes > 0) keeps stepping but stops accumulating: the
                             first-episode score of the enjoy scripts */
  int reserved;           /* 0 */
  float* obs;             /* [n, obs_dim] in: the current observation (of reset or of the last step);
                             out: the observation after the last step */
  float* act;             /* [n, act_dim] work: the last action */
  float* rew;             /* [n] work: the last float32 reward (unused when rew_traj is given) */
  double* rew64;          /* [n] work: the last float64 reward */
  uint8_t* done;          /* [n] work: the last done flags (unused when done_traj is given) */
  /* per-env episode accumulators: zeroed by the caller before the first call, continued by later ones.
   * Per env-step: cur_return += reward64, cur_length += 1; if done: done_return += cur_return,
   * done_length += cur_length, done_episodes += 1, cur_return = cur_length = 0 */
  double* cur_return;     /* [n] return of the running episode */
  int32_t* cur_length;    /* [n] its length */
  double* done_return;    /* [n] summed returns of the finished episodes */
  int32_t* done_length;   /* [n] their summed lengths */
  int32_t* done_episodes; /* [n] how many finished */
  /* nullable trajectories */
  float* obs_traj;        /* [T, n, obs_dim] the observation each action was computed from */
  float* act_traj;        /* [T, n, act_dim] */
  float* rew_traj;        /* [T, n] float32 reward */
  uint8_t* done_traj;     /* [T, n] */
  /* version 2: nullable, both or neither, autoreset != 0 only */
  uint8_t* trunc_traj;    /* [T, n] truncated and not terminated */
  float* term_obs_traj;   /* [T, n, obs_dim] the observation before the reset, rows where done is set */
} pbg_rollout_io_t;

/* T closed-loop steps: per step act = pi(obs), then the handle's step (pbg_step_ex) with `autoreset`,
 * then the bookkeeping above.  Enqueues 2 T + 1 kernels on `stream` only (per step the actor, which
 * also does the previous step's bookkeeping, and the step; one bookkeeping launch closes the call);
 * never synchronises, allocates or touches the host, so it captures into a HIP graph as a plain
 * chain.  PBG_E_ARG for a host-only policy, one on another device, or one whose obs_dim / act_dim
 * differ from the handle's. */
int pbg_rollout(pbg_handle* h, const pbg_policy* p, const pbg_rollout_io_t* io, void* stream);

/* ---- Policy populations and evolution strategies (appended; nothing above changes) ----
 * Evolution strategies with mirrored sampling (Salimans et al. 2017): a generation perturbs a centre
 * theta into n_pairs mirrored pairs theta +- sigma eps_i, scores every member by closed-loop episodes,
 * and moves theta along sum_i w_i eps_i.  The noise is counter-based (below), so it is regenerated where
 * it is needed and never stored, and a shard that holds pairs pair0 .. pair0 + n_pairs of a larger
 * population draws exactly the noise the whole population would: only one scalar per member (its
 * fitness) has to cross between shards.
 *
 * Flat parameter layout.  theta is [D] float32, D = obs*h1 + h1 + h1*h2 + h2 + h2*act + act: the
 * unpadded concatenation w1, b1, w2, b2, w3, b3, each row-major in pbg_policy_create's layout; the
 * dimension limits are pbg_policy_create's.
 *
 * A pbg_population is P = 2 n_pairs members (one theta each) of one MLP shape in the memory of one
 * device; members 2 i and 2 i + 1 are the mirrored pair i, whose global index is pair0 + i.
 *
 * Noise contract.  eps_i[4 b .. 4 b + 3] come from one Philox4x32-10 block, key = seed (low word k0,
 * high word k1), counter = (b, pair0 + i, generation, 0xE5); its words x0..x3 give four normals by two
 * Box-Muller pairs, (x0, x1) the first two and (x2, x3) the last two:
 *   u1 = fmaf((float)(x0 >> 9), 2^-23, 2^-24)   exact, in (0, 1)
 *   u2 = (float)(x1 >> 8) * 2^-24               exact, in [0, 1)
 *   r  = sqrtf(-2 logf(u1));  normals (r cospif(2 u2), r sinpif(2 u2))
 * The last block of a D that is no multiple of 4 drops its surplus normals.  The device computes this
 * in float32 with the device library's logf / cospif / sinpif, in ONE function that noise, perturb and
 * grad share: all three see the same bits.  The host counterpart computes in float64 and rounds once;
 * host and device agree within 1e-5 absolute (|r| <= sqrt(48 ln 2) = 5.77; log <= 3 ulp, sinpi / cospi
 * <= 4 ulp, correctly rounded sqrt and multiply: 5.77 (1.5 + 0.5 + 4 + 0.5) 2^-23 = 4.5e-6), not bitwise. */
typedef struct pbg_population pbg_population;

/* n_pairs >= 1 mirrored pairs on `device` (>= 0), members zeroed; pair0 >= 0: the global index of the
 * first pair.  PBG_E_ARG (before any HIP call) for dims out of pbg_policy_create's ranges, n_pairs < 1,
 * pair0 < 0 or device < 0; PBG_E_HIP for a device that does not exist.  *out is NULL after every failure. */
int pbg_population_create(int device, int obs_dim, int h1, int h2, int act_dim, int n_pairs, int pair0,
                          pbg_population** out);
void pbg_population_destroy(pbg_population* p);
/* eps_out: DEVICE [n_pairs, D] float32 = the noise of `generation`. */
int pbg_population_noise(const pbg_population* p, uint64_t seed, uint32_t generation, float* eps_out, void* stream);
/* The host counterpart (float64, rounded once; HOST eps_out [n_pairs, D]); needs no GPU. */
int pbg_population_noise_host(int obs_dim, int h1, int h2, int act_dim, uint64_t seed, uint32_t generation, int pair0,
                              int n_pairs, float* eps_out);
/* member[2 i][d]     = (float)((double)theta[d] + (double)sigma * (double)eps_i[d])
 * member[2 i + 1][d] = (float)((double)theta[d] - (double)sigma * (double)eps_i[d])
 * with the device's eps (pbg_population_noise's bits); theta: DEVICE [D].  The product of two float32
 * values is exact in float64, so each member is the correctly rounded theta +- sigma eps. */
int pbg_population_perturb(pbg_population* p, const float* theta, float sigma, uint64_t seed, uint32_t generation,
                           void* stream);
/* member m = theta (DEVICE [D]); m = -1 sets every member (the centre's evaluation).  get: DEVICE [D] out. */
int pbg_population_set_member(pbg_population* p, int m, const float* theta, void* stream);
int pbg_population_get_member(const pbg_population* p, int m, float* theta_out, void* stream);
/* act[n, act_dim] = pi_m(obs[n, obs_dim]): n must be a multiple of P (PBG_E_ARG otherwise); with
 * G = n / P env e uses member e / G.  The numeric contract is pbg_policy_act's, per member: row e equals
 * pbg_policy_act_host of a policy built from member e / G's weights, bit for bit.  One launch; rows past
 * n are neither read nor written.  Any G is correct; a G that is no multiple of 16 leaves lanes of each
 * member's last 16-env tile idle. */
int pbg_population_act(const pbg_population* p, int n, const float* obs, float* act, void* stream);
/* pbg_rollout with the population's actor: the same pbg_rollout_io_t, bookkeeping and 2 T + 1 launches,
 * nothing touches the host (capturable as a plain chain).  PBG_E_ARG when the handle's n_envs is no
 * multiple of P, for a population on another device, or for mismatched obs_dim / act_dim. */
int pbg_rollout_population(pbg_handle* h, const pbg_population* p, const pbg_rollout_io_t* io, void* stream);
/* fitness_out[m] (DEVICE [P] float64) = (sum over member m's G = n / P envs, env-ascending sequential
 * float64 adds, of (done_return[e] + cur_return[e])) / G: the mean return per env over everything the
 * rollout accumulators (pbg_rollout_io_t) hold.  n: a positive multiple of P. */
int pbg_population_fitness(const pbg_population* p, int n, const double* cur_return, const double* done_return,
                           double* fitness_out, void* stream);
/* g_out[d] (DEVICE [D] float32) = (float)(sum over i = 0 .. n_pairs - 1 ascending, in float64, of
 * (double)w[i] * (double)eps_i[d]): exact products, one float64 rounding per add, eps regenerated
 * (pbg_population_noise's bits).  w: DEVICE [n_pairs] float32. */
int pbg_population_grad(const pbg_population* p, const float* w, uint64_t seed, uint32_t generation, float* g_out,
                        void* stream);

/* ---- Running observation normalisation (appended; nothing above changes) ----
 * The evolution-strategy recipe (Salimans et al. 2017; Mania et al. 2018 "state normalisation") keeps the
 * running per-component mean and variance of every observation the population visits and feeds each policy
 *   clip((obs - mean) / std, -clip, clip)
 * instead of obs.  The observations of a rollout never leave the two-launch loop, so the statistics are
 * gathered inside the actor kernels, where the tile's observations already sit in LDS, and the
 * normalisation is applied there too.
 *
 * A pbg_obs_stats lives on one device and holds, for K = obs_dim,
 *   totals  float64 [1 + 2 K] = count, sum[K], sumsq[K]; initially OpenAI ES's RunningStat(eps = 1e-2):
 *           count = 1e-2, sum = 0, sumsq = 1e-2;
 *   n_slots partial accumulators: slot_count int64, slot_sum[K], slot_sumsq[K] float64, initially zero.
 * One slot belongs to one workgroup of a launch (a tile of at most 16 rows), so nothing is atomic and the
 * order of every sum is stated:
 *
 * Tile accumulation (one device function, shared by both actors and pbg_obs_stats_update).  A row of the
 * tile counts when it is active and finite (no NaN or inf component).  For component k the tile's counted
 * rows are added in ascending row order straight onto the slot's running values,
 *   slot_sum[k] += (double)x;  slot_sumsq[k] += (double)x * (double)x;
 * (the product of two float32 values is exact in float64, so a contraction into an fma changes no bit),
 * and slot_count grows by the number of counted rows.  Over several launches a slot therefore sums in the
 * order (launch ascending, row-in-tile ascending). */
typedef struct pbg_obs_stats pbg_obs_stats;

/* PBG_E_ARG (before any HIP call) for obs_dim outside pbg_policy_create's 1..256, n_slots < 1 or
 * device < 0; PBG_E_HIP for a device that does not exist.  *out is NULL after every failure. */
int pbg_obs_stats_create(int device, int obs_dim, int n_slots, pbg_obs_stats** out);
/* Detach it from every actor first (pbg_*_attach_obs_stats with NULL): the actors keep only the pointer. */
void pbg_obs_stats_destroy(pbg_obs_stats* s);
/* One launch over obs (DEVICE [n, K] float32); active: DEVICE [n] uint8 (0 = skip the row), NULL = every
 * row active.  group = G > 0: the rows are n / G groups of G consecutive rows and the tiles are cut per
 * group exactly as pbg_population_act cuts them, tile t of group m is workgroup (and slot)
 * m ceil(G / 16) + t; group = 0: one group of n rows, pbg_policy_act's tiling.  PBG_E_ARG when n is no
 * multiple of group or the launch needs more slots than the object has. */
int pbg_obs_stats_update(pbg_obs_stats* s, int n, int group, const float* obs, const uint8_t* active, void* stream);
/* Folds the slots into the totals and zeroes them: for each k sum[k] and sumsq[k] take the slots' values
 * by slot-ascending sequential float64 adds; the int64 slot counts are summed exactly and added to count
 * as one float64.  Then, into the nullable DEVICE float32 [K] outputs,
 *   mean[k]    = (float)(sum[k] / count)
 *   inv_std[k] = (float)(1 / sqrt(max(sumsq[k] / count - m m, 1e-2)))   with m = sum[k] / count,
 * all in float64 and nothing contracted; the variance floor bounds inv_std by 10. */
int pbg_obs_stats_finalize(pbg_obs_stats* s, float* mean_out, float* inv_std_out, void* stream);
/* The totals as DEVICE float64 [1 + 2 K] (count, sum, sumsq), copied on `stream`: to resume a run, or to
 * merge the statistics of several shards by adding their totals. */
int pbg_obs_stats_get_totals(const pbg_obs_stats* s, double* totals_out, void* stream);
int pbg_obs_stats_set_totals(pbg_obs_stats* s, const double* totals, void* stream);

/* The normaliser of an actor.  With one set, every path that evaluates the MLP (pbg_policy_act,
 * pbg_policy_act_host, pbg_population_act, pbg_rollout, pbg_rollout_population) feeds the first layer
 *   v = (x - mean[k]) * inv_std[k];  xn = v < -clip ? -clip : (v > clip ? clip : v)
 * instead of x: one float32 rounding for the subtraction, one for the multiply, a NaN passes through;
 * host and device agree bit for bit.  obs_traj keeps the raw observation.  With none set every path
 * computes exactly what it computed before normalisers existed.
 * pbg_policy_set_obs_norm: HOST float32 [obs_dim] arrays, copied (host-only policies too); for a device
 * policy it waits for the device first, so that no launch already enqueued sees half of the new arrays.
 * pbg_population_set_obs_norm: DEVICE float32 [obs_dim] arrays, copied on `stream` into the population's
 * own buffers (no host work: a training loop sets a new normaliser every generation).
 * Both arrays NULL: the normaliser is switched off.  PBG_E_ARG for one NULL array or a clip that is not > 0. */
int pbg_policy_set_obs_norm(pbg_policy* p, const float* mean, const float* inv_std, float clip);
int pbg_population_set_obs_norm(pbg_population* p, const float* mean, const float* inv_std, float clip, void* stream);

/* Attach statistics to an actor (NULL detaches).  While attached, every step of pbg_rollout /
 * pbg_rollout_population with that actor accumulates its tiles' raw observations, workgroup b into slot b,
 * inside the actor launch (a rollout stays 2 T + 1 launches).  A row is active when the action computed
 * from it will be booked: autoreset != 0, or done_episodes[e] == 0 after the previous step's bookkeeping.
 * The plain *_act calls never collect.  The rollout returns PBG_E_ARG when the attached object is on
 * another device, has another obs_dim, or has fewer slots than the actor launch has workgroups
 * (ceil(n / 16), for a population P ceil(G / 16)). */
int pbg_policy_attach_obs_stats(pbg_policy* p, pbg_obs_stats* s);
int pbg_population_attach_obs_stats(pbg_population* p, pbg_obs_stats* s);

/* ---- Stochastic Gaussian actions and advantage estimation (appended; nothing above changes) ----
 * A policy-gradient learner needs a = mu(obs) + std eps inside the rollout, the noise's squared norm for the
 * log-probability, and advantages from the reward / done trajectories.  A pbg_action_noise lives on one
 * device and holds act_dim, a uint64 seed, a DEVICE float32 std[act_dim] (initially zero), a DEVICE uint32
 * step counter (initially zero) and a nullable DEVICE pointer eps2_traj, float64 [T, n].
 *
 * Contract.  While one is attached to an actor (below), step s = 0 .. T - 1 of a pbg_rollout /
 * pbg_rollout_population call computes, for env e (row of the handle, whose global index is the handle's
 * env_offset + e) and component j,
 *   eps[e][j] : component j % 4 of the Noise contract's block (Philox4x32-10, key = seed, two Box-Muller
 *               pairs) at counter = (j / 4, env_offset + e, counter + s, 0xAC)
 *   a[e][j]   = (float)((double)mu[e][j] + (double)std[j] * (double)eps[e][j])
 *   eps2[e]   = sum over j ascending, sequential float64 adds, of (double)eps[e][j] * (double)eps[e][j]
 * mu is the third layer's output, exactly what the actor computes with nothing attached; a is what goes to
 * act, to act_traj and into the step; eps2[e] goes to eps2_traj[s][e] when that pointer is set.  The product
 * of two float32 values is exact in float64, so a and every partial sum are one rounding each (the same bits
 * contracted into an fma or not).  A NaN mu gives a NaN action, which the step turns into done.  std is not
 * validated (it lives on the device).  The fourth counter word 0xAC keeps the stream apart from the
 * evolution strategy's 0xE5; the device function is the one the populations' noise uses.
 * The step counter is read on the device by every actor launch, which adds its own s (a launch argument);
 * the call's closing bookkeeping launch adds T to it.  A rollout therefore stays 2 T + 1 launches with no
 * host work, and a captured graph draws fresh noise on every replay.  The noise depends on (seed, global
 * env index, step count, component) only: not on the batch or shard the env sits in, on the tile geometry,
 * or on whether the actor is a policy or a population.  obs_traj and attached statistics are unaffected;
 * the plain *_act calls never sample. */
typedef struct pbg_action_noise pbg_action_noise;

/* PBG_E_ARG (before any HIP call) for act_dim outside pbg_policy_create's 1..64, device < 0 or out NULL;
 * PBG_E_HIP for a device that does not exist.  *out is NULL after every failure. */
int pbg_action_noise_create(int device, int act_dim, uint64_t seed, pbg_action_noise** out);
/* Detach it from every actor first (pbg_*_attach_action_noise with NULL): the actors keep only the pointer. */
void pbg_action_noise_destroy(pbg_action_noise* z);
/* std: DEVICE float32 [act_dim], copied on `stream` (no host work: a training loop sets it every iteration). */
int pbg_action_noise_set_std(pbg_action_noise* z, const float* std, void* stream);
/* The step counter: set on `stream`; get copies it into a DEVICE uint32 on `stream`. */
int pbg_action_noise_set_counter(pbg_action_noise* z, uint32_t counter, void* stream);
int pbg_action_noise_get_counter(const pbg_action_noise* z, uint32_t* counter_out, void* stream);
/* Host-side: where the next rollouts write eps2 (DEVICE float64 [T, n] of that rollout; NULL: nowhere). */
int pbg_action_noise_set_eps2_traj(pbg_action_noise* z, double* eps2_traj);
/* eps_out (DEVICE [n, act_dim] float32) = the eps of envs env_offset .. env_offset + n at the absolute step
 * count `step` (the counter plus s of the rollout step it mirrors): one launch of the same device function. */
int pbg_action_noise_fill(const pbg_action_noise* z, int n, int env_offset, uint32_t step, float* eps_out, void* stream);
/* The host counterpart (float64, rounded once; HOST eps_out [n, act_dim]); needs no GPU.  Host and device
 * agree within the Noise contract's 1e-5 absolute, not bitwise. */
int pbg_action_noise_host(int act_dim, uint64_t seed, int n, int env_offset, uint32_t step, float* eps_out);
/* Attach the noise to an actor (NULL detaches).  The rollout returns PBG_E_ARG for an attached object on
 * another device or with another act_dim. */
int pbg_policy_attach_action_noise(pbg_policy* p, pbg_action_noise* z);
int pbg_population_attach_action_noise(pbg_population* p, pbg_action_noise* z);

/* Generalised advantage estimation (Schulman et al. 2016) as one launch, a lane per env, t descending from
 * T - 1, all DEVICE arrays: rew_traj float32 [T, n], done_traj uint8 [T, n], value float32 [T + 1, n] (row T:
 * the value of the observation after the last step), adv_out, ret_out float32 [T, n].  All arithmetic is
 * float64, nothing contracted, in this order (A = 0 before t = T - 1; gl = gamma * lambda, computed once on
 * the host):
 *   nd    = done[t][e] ? 0.0 : 1.0
 *   delta = (r + (gamma * v[t+1]) * nd) - v[t]
 *   A     = delta + (gl * nd) * A
 *   adv[t][e] = (float)A;  ret[t][e] = (float)(A + v[t])
 * done includes the TimeLimit truncation, and pbg_gae alone treats a truncated episode as terminal: nothing
 * bootstraps through it.  pbg_gae_trunc ("Truncation bootstrapping" below) takes the rollout's trunc_traj and
 * the values of the terminal observations and bootstraps through it.  PBG_E_ARG (before any HIP call) for
 * T < 1, n < 1 or a NULL array.  pbg_gae_host: the same loop on HOST pointers, the same bits; needs no GPU. */
int pbg_gae(int T, int n, const float* rew_traj, const uint8_t* done_traj, const float* value, double gamma,
            double lambda, float* adv_out, float* ret_out, void* stream);
int pbg_gae_host(int T, int n, const float* rew_traj, const uint8_t* done_traj, const float* value, double gamma,
                 double lambda, float* adv_out, float* ret_out);

/* ---- PPO gradient (appended; nothing above changes) ----
 * The gradient of the clipped-surrogate loss (Schulman et al. 2017) of one minibatch with respect to the actor's
 * and the critic's flat parameters and log_std, as at most two launches: the tiles, then the reduction.  Actor
 * (obs_dim -> h1 -> h2 -> act_dim) and critic (obs_dim -> h1 -> h2 -> 1) share obs_dim, h1, h2; A = act_dim,
 * Da, Dc = the two networks' D (Flat parameter layout), B = batch_rows, Bm = mb_rows.
 *
 * The function.  Row i of the minibatch is row r = idx[i] of the batch (idx NULL: r = i).  With c = clip_eps:
 *   mu = actor(obs_r), v = critic(obs_r)                  through the normaliser when mean / inv_std are set
 *   z_j = (act_rj - mu_j) exp(-log_std_j)
 *   logp = -1/2 sum_j z_j^2 - sum_j log_std_j - 1/2 A log 2 pi
 *   a^ = adv_norm ? (adv_r - adv_norm[0]) * adv_norm[1] : adv_r
 *   ratio = exp(logp - logp_old_r);  s1 = ratio a^;  s2 = clamp(ratio, 1 - c, 1 + c) a^
 *   L = mean_i(-min(s1, s2)) + vf_coef 1/2 mean_i((v - ret_r)^2) - ent_coef (sum_j log_std_j + const)
 * and the derivatives are
 *   dL/dlogp_i = -(s1 <= s2 ? a^ ratio : 0) / Bm     (inside the clip range s1 == s2: the gradient flows)
 *   dlogp/dmu_j = z_j exp(-log_std_j);  dlogp/dlog_std_j = z_j^2 - 1;  dL/dlog_std_j gets a further -ent_coef
 *   dL/dv_i = vf_coef (v - ret_r) / Bm
 *   ReLU passes the gradient where the stored activation is > 0.
 *
 * Forward numerics are the actor's: mu and v are the Numeric contract's k-ascending fmaf chains, after
 * pbg_policy_set_obs_norm's transform when a normaliser is given, so v_out equals pbg_population_act of the
 * critic's weights on the same rows bit for bit and the ReLU masks are the ones the rollout's network had.
 * Everything from z to the two derivatives dL/dmu_ij and dL/dv_i is float64 per row (one function, host and
 * device), rounded once to float32.  logp_out is that logp, the one the gradient used.
 *
 * The surrogate, the clipped fraction and mean(logp_old - logp) of `stats` come from a second, float64 evaluation
 * of the actor on the same rows (the same transform and the same k-ascending chain from the bias, as fma in
 * float64 on the float32 parameters; the same per-row expressions).  mean(logp_old - logp) is a mean of cancelling
 * terms, of which the float32 chain's rounding of mu would leave three digits at 64 action components.  The value
 * loss is taken from the float32 v.  A row whose ratio lies within the float32 forward's error of a clip edge can
 * count as clipped in `stats` and not in the gradient, or the reverse.
 *
 * Backward numerics and the order of every sum.  The minibatch is cut into tiles of 16 consecutive rows;
 * the launch has G = min(number of tiles, the object's workgroup count) workgroups, and workgroup b owns the
 * tiles b, b + G, b + 2 G, ...  Per tile every weight-gradient element is one float32 fmaf chain over the tile's
 * rows in ascending order started from zero (a bias or log_std element: the same chain with a factor 1), every
 * back-propagated activation one float32 fmaf chain over the layer's outputs j in ascending order started from
 * zero.  A workgroup adds its tiles' values in ascending tile order in float32 into a partial it alone owns;
 * the reduction adds the G partials in ascending b in float64 and rounds once (grad_log_std: after subtracting
 * ent_coef in float64).  The four stats are float64 throughout: per row-in-tile slot summed over the
 * workgroup's tiles ascending, then over the 16 slots ascending, then over b ascending, then divided by Bm.
 * The workgroup count is fixed at creation: min(ceil(max_rows / 16), 512, as many partials as fit 128 MiB),
 * at least 1.  There are no atomics: the result is a function of the inputs and of max_rows alone, the same
 * bits on every call, on every stream and inside a replayed graph.
 *
 * pbg_ppo_grad_host is the same function on HOST pointers with no GPU: the same forward chains and the same
 * per-row functions; its backward sums in float64 over rows ascending and rounds once, and its exp is the
 * host's, so it agrees with the device to rounding, not bitwise.  Its v_out is bitwise the device's. */
typedef struct pbg_ppo_grad pbg_ppo_grad;

/* All pointers DEVICE memory of the object's GPU (pbg_ppo_grad_run) or HOST memory (pbg_ppo_grad_host); nothing
 * is copied or kept, the parameters are read where they lie.  Versioned by struct_size like pbg_ppo_opt_io_t: the
 * library accepts exactly its versions' sizes, the first version's (which ends with v_out, 176 bytes) and the one
 * that appends value_old, gate, vf_clip and a pad (200 bytes); PBG_E_ARG for every other size: below the first
 * version's, above the library's, or between the two.  A caller that passes the first version's size gets NULL / 0
 * for the appended fields. */
typedef struct {
  uint32_t struct_size;
  int batch_rows;            /* B >= 1 */
  int mb_rows;               /* Bm: 1 <= Bm <= max_rows; with idx NULL also Bm <= B */
  int reserved;              /* 0 */
  const float* theta_actor;  /* [Da] */
  const float* theta_critic; /* [Dc] */
  const float* log_std;      /* [A] */
  const float* mean;         /* [obs_dim], nullable with inv_std: no normaliser */
  const float* inv_std;      /* [obs_dim] */
  float clip;                /* the normaliser's, > 0 when it is set */
  float clip_eps;            /* c >= 0 */
  float vf_coef;
  float ent_coef;
  const float* obs;          /* [B, obs_dim] */
  const float* act;          /* [B, A] */
  const float* logp_old;     /* [B] */
  const float* adv;          /* [B] */
  const float* ret;          /* [B] */
  const int64_t* idx;        /* [Bm] rows of the batch, nullable: rows 0 .. Bm - 1.  pbg_ppo_grad_run does NOT
                                validate the indices (they live on the device): every one must be in 0 .. B - 1.
                                pbg_ppo_grad_host does (PBG_E_ARG) */
  const float* adv_norm;     /* [2] (shift, scale), nullable */
  float* grad_actor;         /* [Da] out */
  float* grad_critic;        /* [Dc] out */
  float* grad_log_std;       /* [A] out */
  double* stats;             /* [4] out: mean_i(-min(s1, s2)), 1/2 mean_i((v - ret)^2), the fraction of rows with
                                |ratio - 1| > c, mean_i(logp_old - logp) */
  float* logp_out;           /* [Bm] out, nullable: logp in minibatch order */
  float* v_out;              /* [Bm] out, nullable: v in minibatch order */
  /* appended ("Value clipping and the KL gate" below) */
  const float* value_old;    /* [B], nullable: the values the batch was collected under, indexed by batch row like ret */
  const int32_t* gate;       /* [2], nullable: when set and gate[0] != 0 every launch returns at entry */
  float vf_clip;             /* e > 0 when value_old is set */
  int reserved2;             /* 0 */
} pbg_ppo_grad_io_t;

/* The object owns the reduction's device workspace for up to max_rows minibatch rows.  PBG_E_ARG (before any HIP
 * call) for dims out of pbg_policy_create's ranges, max_rows < 1, device < 0 or out NULL; PBG_E_HIP for a device
 * that does not exist.  *out is NULL after every failure. */
int pbg_ppo_grad_create(int device, int obs_dim, int h1, int h2, int act_dim, int max_rows, pbg_ppo_grad** out);
void pbg_ppo_grad_destroy(pbg_ppo_grad* g);
/* Two launches on `stream`, no host work, no synchronisation: captures as a plain chain.  PBG_E_ARG (before any
 * HIP call) for a NULL argument or required pointer, a bad struct_size, mb_rows outside 1 .. max_rows, batch_rows
 * < 1 (< mb_rows with idx NULL), one of mean / inv_std NULL, a normaliser clip that is not > 0 or a clip_eps that
 * is not >= 0.  Two calls with one object must not overlap on the device (they share the workspace). */
int pbg_ppo_grad_run(pbg_ppo_grad* g, const pbg_ppo_grad_io_t* io, void* stream);
int pbg_ppo_grad_host(int obs_dim, int h1, int h2, int act_dim, const pbg_ppo_grad_io_t* io);

/* The matrix-core path (appended to this block; nothing above changes).  An object created by
 * pbg_ppo_grad_create_ex with path = PBG_PPO_GRAD_MFMA computes the same function with the six products of each
 * network (three forward, two back-propagations, three weight gradients) on gfx950's exact float32 matrix instruction
 * v_mfma_f32_16x16x4_f32, whose result is bit for bit a k-ordered fmaf chain from its C input with one rounding per
 * product.  pbg_ppo_grad_run, pbg_ppo_grad_io_t, pbg_ppo_grad_destroy and pbg_ppo_grad_host serve both paths; the
 * host twin, whose backward is a float64 sum over rows, is the twin of both.
 *
 * Forward.  mu, v, v_out, logp_out and the ReLU masks are those of the Numeric contract's k-ascending chain from the
 * bias: the instruction takes the bias as C and four consecutive k per issue in ascending order.  They equal the FMA
 * path's and pbg_population_act's values.  A K that is no multiple of 4 is padded with zeros on both operands:
 * fmaf(0, 0, acc) returns acc, except that it turns an acc of -0 into +0.  An output is -0 only when its bias and
 * every one of its products are -0, and the two zeros compare equal; that sign is the one difference.
 *
 * Per-row part.  ppo_actor_row, ppo_critic_row and ppo_stats_row of the FMA path, unchanged: float64 per row,
 * rounded once.  `stats` keeps its second, float64 forward of the actor (on the vector unit) and its contract.
 *
 * Backward, the order of every sum.  The minibatch is cut into tiles of 16 consecutive rows; the launch has
 * G = min(number of tiles, the object's workgroup count) workgroups and workgroup b owns the tiles b, b + G, ...
 * The workgroup count is fixed at creation: min(ceil(max_rows / 16), 256, as many partials as fit 128 MiB), at least
 * 1.  A workgroup does the actor for all its tiles, then the critic for all its tiles.  A back-propagated activation
 * is one float32 fmaf chain over the layer's outputs j in ascending order started from zero (the FMA path's chain,
 * j padded to a multiple of 4 with zeros).  A weight-gradient element is ONE float32 fmaf chain started from zero
 * over all the rows of all the workgroup's tiles: tiles in ascending order, and inside a tile the rows in the order
 * e = 0, 4, 8, 12, 1, 5, 9, 13, 2, 6, 10, 14, 3, 7, 11, 15 (rows past the minibatch's end enter as zeros); there is
 * no per-tile value that is added afterwards.  A bias or log_std element is, as on the FMA path, the float32 sum over
 * the tile's rows ascending from zero, added in float32 onto the workgroup's running value in ascending tile order.
 * The float32 values of the G workgroups meet in the reduction, which adds them in ascending b in float64 and rounds
 * once (grad_log_std: after subtracting ent_coef in float64).  The four stats are summed as on the FMA path.
 *
 * Where the chain lives.  Every 16 x 16 patch of a weight gradient belongs to one wave of its workgroup.  For
 * obs_dim <= 80, h1 <= 256, h2 <= 128 and act_dim <= 32 (every network shape the project ships a policy for; at most
 * 224 patches a network) the chains stay in accumulator registers over all the workgroup's tiles and are stored
 * once; for every other shape (up to 576 patches at (256, 256, 256, 64); (44, 256, 256, 17) with 336 is one) a
 * chain's running value is stored to the workgroup's own partial after each tile and loaded back as the C input of
 * the next.  A float32 store and load is exact, so which route a shape takes does not enter its bits.
 *
 * Determinism.  There are no atomics.  The result is a function of the inputs, of max_rows and of the path alone:
 * the same bits on every call, on every stream and inside a replayed graph. */
#define PBG_PPO_GRAD_FMA 0
#define PBG_PPO_GRAD_MFMA 1

/* Versioned by struct_size like the other option structs. */
typedef struct {
  uint32_t struct_size;
  int path;  /* PBG_PPO_GRAD_FMA or PBG_PPO_GRAD_MFMA */
} pbg_ppo_grad_opts_t;

/* opts NULL or path PBG_PPO_GRAD_FMA: exactly pbg_ppo_grad_create.  PBG_E_ARG (before any HIP call) for an unknown
 * path, a struct_size that is not the struct's, and everything pbg_ppo_grad_create refuses; *out is NULL after every
 * failure.  The matrix-core path accepts every shape pbg_policy_create accepts and every mb_rows >= 1. */
int pbg_ppo_grad_create_ex(int device, int obs_dim, int h1, int h2, int act_dim, int max_rows,
                           const pbg_ppo_grad_opts_t* opts, pbg_ppo_grad** out);

/* ---- PPO optimiser step (appended; nothing above changes) ----
 * What a PPO minibatch step does besides the gradient: the advantage normaliser's (shift, scale) pair, and Adam
 * (Kingma & Ba 2015) with global-norm gradient clipping.  All arithmetic below is IEEE float64 add, multiply,
 * divide and square root in the stated order, nothing contracted, so each host twin gives its device function's
 * bits.  No atomics and no cooperative launch anywhere: every call is a function of its inputs and of the object's
 * state alone, the same bits on every stream and inside a replayed graph.
 *
 * pbg_adv_norm: out (DEVICE float32 [2]) = (shift, scale), the pair pbg_ppo_grad_io_t.adv_norm consumes, of the
 * Bm = n_rows advantages a_i = adv[idx[i]] (adv DEVICE float32 [B], B = n_batch; idx DEVICE int64 [Bm], nullable:
 * rows 0 .. Bm - 1; NOT validated on the device, every index must lie in 0 .. B - 1).  One launch of one workgroup
 * of 1,024 lanes, no workspace:
 *   c0 = a_0, the minibatch's first advantage;  d_i = a_i - c0   (both widened to float64 first; one subtraction)
 *   lane l:   s1_l = sum of d_i, s2_l = sum of d_i * d_i over i = l, l + 1024, l + 2048, ... ascending from 0.0
 *             (the product rounded, then the add: never fused)
 *   the tree: for s = 512, 256, ..., 1:  x_l += x_(l + s) for every l < s;  S1, S2 = lane 0's s1, s2
 *   ms   = S1 / Bm;  mean = c0 + ms
 *   var  = (S2 - S1 * ms) / (Bm - 1);  var < 0 becomes 0 (Bessel's correction, Tensor.std(); a NaN stays NaN)
 *   out  = ((float)mean, (float)(1 / (sqrt(var) + 1e-8)))
 * The sums are taken of the advantages less the first one because the unshifted S2 = sum a_i^2 outgrows 53 bits
 * from some 32 equal rows on and S2 - S1 * mean then keeps a rounding residue of a few ulp(S2): 1,537 rows of
 * 6836.862 gave a scale of 10,032 instead of 1e8.  Shifted, constant advantages have every d_i = 0, so S1 = S2 = 0,
 * mean = c0 and var = 0 exactly, scale = 1e8 and (a_i - shift) * scale = 0 for every row, whatever Bm and the value;
 * and in general the cancellation in S2 - S1 * ms is of the spread against the distance of the mean from a_0, not
 * against the mean itself.  PBG_E_ARG (before any HIP call) for
 * n_rows < 2, n_batch < 1, n_rows > n_batch with idx NULL, adv or out NULL.  pbg_adv_norm_host: the same on HOST
 * pointers with no GPU, the same bits; it validates the indices (PBG_E_ARG). */
int pbg_adv_norm(int n_batch, int n_rows, const float* adv, const int64_t* idx, float* out, void* stream);
int pbg_adv_norm_host(int n_batch, int n_rows, const float* adv, const int64_t* idx, float* out);

/* pbg_ppo_opt: Adam with global-norm clipping over n_blocks (1 .. 8) flat float32 blocks of sizes[b] >= 1 elements.
 * The object owns, on its device, the moments m and v (float32, zero at creation), the workspace of launch 1 and
 * one state word: the step count t (uint32, 0) and the float64 running products b1t = beta1^t and b2t = beta2^t
 * (1), advanced by one multiplication per step, never by pow.  Because the state lives on the device a captured
 * step replayed twice equals two eager steps.
 *
 * One step, with g, p, m, v a block's gradient, parameter and moments:
 *   t += 1;  b1t *= beta1;  b2t *= beta2
 *   norm = sqrt(sum of g * g over all blocks)                 (the order of the adds: below)
 *   coef = max_grad_norm > 0 ? min(1, max_grad_norm / (norm + 1e-6)) : 1        (clip_grad_norm_'s expression)
 *   c1 = lr / (1 - b1t);  c2 = sqrt(1 - b2t)                  (the products after this step's multiplication)
 *   per element:
 *     gd = g * coef
 *     md = beta1 * m + (1 - beta1) * gd
 *     vd = beta2 * v + (1 - beta2) * (gd * gd)
 *     p  = (float)(p - c1 * (md / (sqrt(vd) / c2 + eps)))     (the UNROUNDED md and vd enter p)
 *     m  = (float)md;  v = (float)vd
 * g, p, m, v are widened to float64 first; 1 - beta1 and 1 - beta2 are formed once in float64.  A non-finite norm
 * propagates as in torch.  With clipping (max_grad_norm > 0) a NaN norm makes coef NaN and with it every parameter, m
 * and v of every block; an infinite norm makes coef 0, every element whose gradient is infinite NaN (inf * 0) and
 * gd = 0 for the others, which then move by their old moments alone.  Without clipping coef is 1 and only the
 * elements whose own gradient is not finite become NaN.  A block whose gradient is all zero keeps its parameters.
 *
 * The order of the adds of the norm.  Block b has G_b = min(ceil(ceil(sizes[b] / 4) / 256), 64) workgroups of 256
 * lanes.  Lane l of the block's workgroup w owns the groups of four consecutive elements q = w * 256 + l + k *
 * (256 G_b), k = 0, 1, ..., that is the elements 4 q .. 4 q + 3 below sizes[b]; it adds their squares (exact in
 * float64) in ascending element order onto 0.0.  The workgroup's 256 lane sums are added by the tree of
 * pbg_adv_norm (s = 128, 64, ..., 1) into the workgroup's partial.  Launch 1 stores the partials in the order
 * (block ascending, w ascending); launch 2 adds them in that order onto 0.0 in every workgroup.
 *
 * pbg_ppo_opt_step is two launches on `stream`, no host work, no synchronisation: it captures as a plain chain.
 * Launch 1 writes the partials and one of its lanes advances the state word, which that launch reads nowhere
 * else; launch 2 reads the advanced word, re-adds the partials and updates its elements in the geometry above.  The
 * parameters are updated where they lie.  Blocks whose param and grad pointers are both 16-byte aligned are
 * accessed as float4, the others element by element; the arithmetic and its order are the same.  Two steps of one
 * object must not overlap on the device. */
#define PBG_PPO_OPT_MAX_BLOCKS 8
typedef struct pbg_ppo_opt pbg_ppo_opt;

/* Pointers: DEVICE memory of the object's GPU (pbg_ppo_opt_step) or HOST memory (pbg_ppo_opt_host); entries at and
 * after n_blocks are ignored.  Versioned by struct_size like pbg_ppo_grad_io_t: PBG_E_ARG for a size that is none of
 * the first version's (which ends with bpow, 328 bytes), the second's (which appends lr_ptr, 336) and the library's
 * (which appends gate and a reserved word, 352).  344, the second version's size plus one pointer, stays refused as the
 * second version's contract had it: the third version skips it. */
typedef struct {
  uint32_t struct_size;
  int reserved;                                /* 0 */
  float* param[PBG_PPO_OPT_MAX_BLOCKS];        /* [sizes[b]] in/out, updated in place */
  const float* grad[PBG_PPO_OPT_MAX_BLOCKS];   /* [sizes[b]] */
  double lr;
  double beta1, beta2;                         /* each in [0, 1) */
  double eps;                                  /* > 0 */
  double max_grad_norm;                        /* <= 0: no clipping (coef = 1) */
  double* info;                                /* [2] out, nullable: norm, coef */
  /* the state as HOST arrays, pbg_ppo_opt_host only (pbg_ppo_opt_step ignores them: the object holds its own) */
  float* m[PBG_PPO_OPT_MAX_BLOCKS];            /* [sizes[b]] in/out */
  float* v[PBG_PPO_OPT_MAX_BLOCKS];            /* [sizes[b]] in/out */
  uint32_t* t;                                 /* [1] in/out */
  double* bpow;                                /* [2] in/out: b1t, b2t (1, 1 before the first step) */
  /* appended ("Counter-based permutations and an on-device learning rate" below); a caller built with the struct
   * that ends with bpow passes its struct_size and gets NULL */
  const double* lr_ptr;                        /* [1], nullable: when set, the step uses *lr_ptr in place of lr */
  /* appended ("Value clipping and the KL gate" below); an older caller gets NULL */
  const int32_t* gate;                         /* [2], nullable: when set and gate[0] != 0 the step changes nothing */
  uint64_t reserved2;                          /* 0 */
} pbg_ppo_opt_io_t;

/* PBG_E_ARG (before any HIP call) for n_blocks outside 1 .. 8, a size < 1, sizes or out NULL, device < 0; PBG_E_HIP
 * for a device that does not exist.  *out is NULL after every failure. */
int pbg_ppo_opt_create(int device, int n_blocks, const int64_t* sizes, pbg_ppo_opt** out);
void pbg_ppo_opt_destroy(pbg_ppo_opt* opt);
/* PBG_E_ARG (before any HIP call) for a NULL object or io, a bad struct_size, a NULL param or grad of a block below
 * n_blocks, a beta outside [0, 1), eps <= 0 (NaNs included). */
int pbg_ppo_opt_step(pbg_ppo_opt* opt, const pbg_ppo_opt_io_t* io, void* stream);
/* m = v = 0, t = 0, b1t = b2t = 1, on `stream`. */
int pbg_ppo_opt_reset(pbg_ppo_opt* opt, void* stream);
/* Copies on `stream` to DEVICE arrays, each nullable: m_out, v_out float32 [sum of sizes], the blocks concatenated in
 * order; t_out uint32 [1]. */
int pbg_ppo_opt_get_state(const pbg_ppo_opt* opt, float* m_out, float* v_out, uint32_t* t_out, void* stream);
/* One step on HOST pointers with no GPU: the same sums in the same order and the same element function, the same
 * bits.  Further PBG_E_ARG: n_blocks or sizes as in create; a NULL m or v of a block; t or bpow NULL. */
int pbg_ppo_opt_host(int n_blocks, const int64_t* sizes, const pbg_ppo_opt_io_t* io);

/* ---- Counter-based permutations and an on-device learning rate (appended; nothing above changes) ----
 * What keeps a PPO iteration from being a function of the seed alone that runs with no host work: the minibatch
 * permutation and a learning rate that can change under a replayed graph.
 *
 * perm(seed, c, B)[i] for i in 0 .. B - 1, 1 <= B <= 2^31 - 1: a Feistel network on the smallest even number of
 * bits that holds B, cycle-walked into range.  All arithmetic is uint32.
 *   k    = max(2, bit_length(B - 1));  k += k & 1;  half = k / 2;  mask = (1 << half) - 1
 *   K[0..7] = the four words of Philox4x32-10(key = seed as (lo, hi), counter = (c, 0, 0, 0x9E)), then the four
 *             of counter (c, 1, 0, 0x9E)
 *   x = i
 *   do:  L = x >> half;  R = x & mask
 *        for r = 0 .. 7:  F = fmix32(R + K[r]) & mask;  (L, R) = (R, L ^ F)        (fmix32: murmur3's finaliser)
 *        x = (L << half) | R
 *   while x >= B
 *   perm[i] = x
 * The eight rounds are a bijection of [0, 2^k) and 2^k < 4 B.  The walk starts at i < B, which lies on its own
 * cycle, so it comes back below B: it ends for every input and the result is a bijection of [0, B).  The tag 0x9E
 * keeps the stream apart from 0xE5, 0xAC, 0xAC7 and 0x5EED.
 *
 * A pbg_perm lives on one device and owns one DEVICE uint32 counter (0 at creation).  pbg_perm_fill writes
 * out (DEVICE int64 [n_perms, n_rows]): row j = perm(seed, counter + j, n_rows), then counter += n_perms (uint32:
 * it wraps), all on `stream` with no host work: it captures as a plain chain, and because the counter lives on the
 * device a captured fill replayed twice leaves what two eager fills leave.  The arrangement is two launches: the
 * first (one lane per element, the permutation index the grid's second dimension) only reads the counter, the
 * second is one lane that advances it after every workgroup of the first has read it.  pbg_perm_host is the same
 * function on a HOST array with no GPU, the same bits. */
typedef struct pbg_perm pbg_perm;

/* PBG_E_ARG (before any HIP call) for device < 0 or out NULL; PBG_E_HIP for a device that does not exist.  *out
 * is NULL after every failure. */
int pbg_perm_create(int device, uint64_t seed, pbg_perm** out);
void pbg_perm_destroy(pbg_perm* p);
/* PBG_E_ARG (before any HIP call) for a NULL object or out, n_rows < 1, n_perms outside 1 .. 65535. */
int pbg_perm_fill(pbg_perm* p, int n_rows, int n_perms, int64_t* out, void* stream);
/* The counter: set on `stream`; get copies it into a DEVICE uint32 on `stream`. */
int pbg_perm_set_counter(pbg_perm* p, uint32_t c, void* stream);
int pbg_perm_get_counter(const pbg_perm* p, uint32_t* c_out, void* stream);
/* out: HOST int64 [n_perms, n_rows], rows at the counters counter, counter + 1, ... (wrapping).  PBG_E_ARG as
 * pbg_perm_fill. */
int pbg_perm_host(uint64_t seed, uint32_t counter, int n_rows, int n_perms, int64_t* out);

/* The optimiser's learning rate from device memory.  pbg_ppo_opt_io_t.lr_ptr (above), when not NULL, is a DEVICE
 * (pbg_ppo_opt_step) or HOST (pbg_ppo_opt_host) float64 [1] that launch 2 reads in place of io->lr: the bits are
 * those of passing the same value as lr, and a captured step follows what the memory holds at each replay.  The
 * value is not validated on the device.
 *
 * pbg_ppo_lr_linear: one launch of one lane on `stream`, float64, nothing contracted:
 *   q = (double)min(*it, n_total) / (double)n_total;   *lr_out = lr0 * (1.0 - q)
 * it: DEVICE uint32 [1] (an iteration count the caller advances on the stream), lr_out: DEVICE float64 [1].
 * PBG_E_ARG (before any HIP call) for n_total < 1 or a NULL pointer.  pbg_ppo_lr_linear_host: the same function on
 * HOST pointers, the same bits. */
int pbg_ppo_lr_linear(const uint32_t* it, uint32_t n_total, double lr0, double* lr_out, void* stream);
int pbg_ppo_lr_linear_host(const uint32_t* it, uint32_t n_total, double lr0, double* lr_out);

/* ---- The PPO gradient as parts, and the statistics' slots (appended; nothing above changes) ----
 * What a data-parallel learner needs to hold the one-device learner's bits.  A workgroup's partial of
 * pbg_ppo_grad_run depends on its global index b and on the global workgroup count G (workgroup b owns the tiles
 * b, b + G, ...), not on the launch it ran in or the device it ran on.  So a gradient can be cut into ranges of
 * workgroups, each range run by its own launch (on its own device, given the same inputs), the partials brought
 * into one [G, Dtot] buffer, and the unchanged reduction run over them.
 *
 * Contract.  For any cut of 0 .. G into consecutive ranges, pbg_ppo_grad_run_part for each range with part_out and
 * part_stats_out at the range's first row of one [G, Dtot] / [G, 4] buffer, then pbg_ppo_grad_reduce over that
 * buffer, leave in grad_actor, grad_critic, grad_log_std, stats, logp_out and v_out what pbg_ppo_grad_run leaves,
 * bit for bit: on either path, on any stream and inside a replayed graph.  The parts may come from objects on
 * several devices as long as the objects were created alike (dims, max_rows, path) and the inputs are equal.
 *
 * pbg_ppo_grad_geometry: host only, no HIP call.  *G_out = the G pbg_ppo_grad_run launches for mb_rows,
 * min(ceil(mb_rows / 16), the object's workgroup count); *dtot_out = Dtot = Da + Dc + A, the floats of a partial.
 * PBG_E_ARG for a NULL argument or mb_rows outside 1 .. max_rows. */
int pbg_ppo_grad_geometry(const pbg_ppo_grad* g, int mb_rows, int* G_out, int64_t* dtot_out);
/* One launch of wg_count workgroups on `stream`: the global workgroups wg_first .. wg_first + wg_count - 1 of the
 * G that io->mb_rows implies.  Workgroup wg_first + i writes row i of part_out (DEVICE float32 [wg_count, Dtot])
 * and of part_stats_out (DEVICE float64 [wg_count, 4]); the object's own workspace is not touched, so calls with
 * one object may overlap.  logp_out / v_out are written for the rows of the tiles these workgroups own, every other
 * row is left untouched.  io's grad_actor, grad_critic, grad_log_std and stats are not written and may be NULL.
 * wg_count == 0 is valid and launches nothing (the outputs may then be NULL).  PBG_E_ARG (before any HIP call)
 * for a range outside 0 .. G, a negative count, NULL outputs with wg_count > 0, and everything pbg_ppo_grad_run
 * refuses of the fields it reads. */
int pbg_ppo_grad_run_part(pbg_ppo_grad* g, const pbg_ppo_grad_io_t* io, int wg_first, int wg_count, float* part_out,
                          double* part_stats_out, void* stream);
/* pbg_ppo_grad_run's reduction, one launch on `stream`, over the caller's part (DEVICE float32 [G, Dtot]) and
 * part_stats (DEVICE float64 [G, 4]): the G partials in ascending order in float64 into io's grad_actor,
 * grad_critic, grad_log_std (less io->ent_coef) and stats (divided by io->mb_rows).  Of io only these, struct_size,
 * batch_rows and mb_rows are read.  PBG_E_ARG (before any HIP call) for a NULL argument or output, a bad
 * struct_size or mb_rows, and a G that is not pbg_ppo_grad_geometry's for io->mb_rows. */
int pbg_ppo_grad_reduce(pbg_ppo_grad* g, const pbg_ppo_grad_io_t* io, int G, const float* part, const double* part_stats,
                        void* stream);

/* The slots of a pbg_obs_stats, `count` of them from `first`: counts DEVICE int64 [count], sums DEVICE float64
 * [count, 2 K], per slot sum[K] | sumsq[K].  Each is one launch on `stream` (none for count == 0).  get copies
 * the slots out and zeroes nothing; set overwrites them.  PBG_E_ARG (before any HIP call) for a NULL pointer or a
 * range outside the object's slots.
 * pbg_obs_stats_finalize folds the slots in ascending order, and slot b is workgroup b of the actor's launch.  So
 * when every shard's tiles are tiles of the whole launch (equal shards whose rows per group are a multiple of 16),
 * each shard's slots set in shard order into one object and finalized there give the totals, mean and inv_std of
 * the object that saw the whole launch, bit for bit.  A slot that was never written adds +0.0 and 0. */
int pbg_obs_stats_get_slots(const pbg_obs_stats* s, int first, int count, int64_t* counts_out, double* sums_out, void* stream);
int pbg_obs_stats_set_slots(pbg_obs_stats* s, int first, int count, const int64_t* counts, const double* sums, void* stream);

/* ---- Truncation bootstrapping (appended; nothing above changes) ----
 * Every env sits under gym's TimeLimit, and a time limit is not a death: the return goes on past it.  A learner
 * that separates `terminated` from `truncated` bootstraps the value of the observation the episode was cut at,
 * V(terminal_obs), through a truncation.  The rollout records what that needs (pbg_rollout_io_t version 2:
 * trunc_traj, term_obs_traj), pbg_population_act_where values the flagged rows alone, and pbg_gae_trunc uses them.
 *
 * pbg_population_act_where: out[T, n, act_dim] from obs[T, n, obs_dim] under flags[T, n] (DEVICE arrays).  n is a
 * positive multiple of the P members; row (t, e) belongs to member e / (n / P), the rollout's mapping.  Where
 * flags[t][e] != 0, out's row is the row's output, through the population's normaliser when one is set: the bits
 * pbg_population_act gives for that row (the same k-ascending fmaf chain, which no other row enters).  Where the
 * flag is 0, out's row is +0.0f in every component and the obs row is NOT read from memory (it is zero-filled in
 * LDS, like the rows past a member's last).  Every element of out is written by the launch.  One launch of
 * T * P * ceil(n / P / 16) workgroups, tiles that never straddle a member or a time step; no atomics, no host
 * work, any stream, capturable.  A tile with no flag set writes its zeros and returns before it touches the
 * weights: the decision is one ballot over the tile's flag bytes, uniform over the workgroup.  Attached statistics
 * and action noise are ignored, as by pbg_population_act.  PBG_E_ARG (before any HIP call) for a NULL pointer,
 * T < 1, n < 1, n % P != 0, a host-only population, or T * tiles beyond the grid limit (2^31 - 1). */
int pbg_population_act_where(const pbg_population* p, int T, int n, const uint8_t* flags, const float* obs, float* out,
                             void* stream);

/* pbg_gae with a truncation flag: trunc_traj uint8 [T, n] and term_value float32 [T, n] (pbg_population_act_where's
 * output for the critic over term_obs_traj under trunc_traj) next to pbg_gae's arrays.  One launch, a lane per env,
 * t descending, float64, nothing contracted, in this order (A = 0 before t = T - 1; gl = gamma * lambda):
 *   tr    = trunc[t][e] != 0
 *   nd    = done[t][e] ? 0.0 : 1.0
 *   vn    = tr ? (double)term_value[t][e] : (double)value[t+1][e]
 *   nb    = tr ? 1.0 : nd
 *   delta = (r + (gamma * vn) * nb) - v[t]
 *   A     = delta + (gl * nd) * A
 *   adv[t][e] = (float)A;  ret[t][e] = (float)(A + v[t])
 * term_value is read only where trunc is set.  With trunc all zero this is pbg_gae's loop and gives its bits.  The
 * step kernels set trunc only together with done; a trunc flag without done is still defined by the lines above (the
 * step bootstraps term_value and the accumulation runs on through it).  PBG_E_ARG (before any HIP call) for T < 1,
 * n < 1 or a NULL array.  pbg_gae_trunc_host: the same loop on HOST pointers, the same bits; needs no GPU. */
int pbg_gae_trunc(int T, int n, const float* rew_traj, const uint8_t* done_traj, const uint8_t* trunc_traj, const float* value,
                  const float* term_value, double gamma, double lambda, float* adv_out, float* ret_out, void* stream);
int pbg_gae_trunc_host(int T, int n, const float* rew_traj, const uint8_t* done_traj, const uint8_t* trunc_traj,
                       const float* value, const float* term_value, double gamma, double lambda, float* adv_out,
                       float* ret_out);

/* ---- Return statistics: reward scaling by a running std of the discounted return (appended; nothing above changes) ----
 * What VecNormalize does to rewards, on the device: every env keeps a running discounted return
 * R <- gamma R + r, reset where the episode ends and carried from one rollout to the next; the rewards the critic
 * regresses are divided by the standard deviation of every R seen so far (no mean is subtracted) and clipped.
 *
 * A pbg_ret_stats lives on one device (device >= 0), or on the host (device == -1: the host twin, the same entry
 * points on HOST pointers, `stream` ignored, no HIP call, the same bits).  It owns
 *   carry   float64 [n_envs]      the running return of every env, +0.0 at creation
 *   slots   n_slots x (count int64, s1 float64, s2 float64): one per tile of 32 consecutive envs, the LAST walk's
 *           partials; n_slots >= ceil(n_envs / 32)
 *   totals  (count int64, s1, s2)  over every finalized batch so far, (0, +0.0, +0.0) at creation
 *   scale   float32 [1]            1.0f at creation
 * All float64 arithmetic below is IEEE add, multiply, divide and square root in the stated order, nothing contracted.
 * No launch uses atomics or reads anything back; each is a function of its inputs and of the object's state alone, the
 * same bits on every stream and inside a replayed graph, and because the state lives on the device a captured
 * walk -> finalize -> apply replayed twice leaves what two eager rounds leave.
 *
 * pbg_ret_stats_walk: rew_traj float32 [T, n], done_traj uint8 [T, n], n <= n_envs.  One launch of ceil(n / 64)
 * workgroups of 64 lanes, a lane per env e, t ascending from R = carry[e], (c, s1, s2) = (0, +0.0, +0.0):
 *   R = gamma * R + (double)r[t][e]                     (the product rounded, then the add)
 *   if isfinite(R):  c += 1;  s1 += R;  s2 += R * R     (the product rounded, then the add)
 *   if !isfinite(R) or done[t][e] != 0:  R = +0.0
 * then carry[e] = R.  A non-finite reward never reaches the sums and does not survive in the carry.  The 32 lanes of
 * tile b (envs 32 b .. 32 b + 31; a lane past n holds (0, +0.0, +0.0)) are added by the tree x[l] += x[l + s] for
 * every l < s, s = 16, 8, 4, 2, 1, and lane 0 OVERWRITES slot slot_offset + b.  Slots of no tile of this walk are left
 * as they are.  PBG_E_ARG (before any HIP call) for a NULL pointer, T < 1, n < 1, n > n_envs, slot_offset < 0 or
 * slot_offset + ceil(n / 32) > n_slots.
 *
 * pbg_ret_stats_finalize: one launch of one workgroup; one lane does, in this order,
 *   b = (0, +0.0, +0.0);  for g = 0 .. n_used_slots - 1 ascending:  b += slots[g]     (per field)
 *   totals += b                                                                          (per field)
 *   if totals.count == 0: scale is left as it is.  Otherwise
 *   m = s1 / count;  var = s2 / count - m * m  (the product rounded first);  var = var > var_floor ? var : var_floor
 *   scale = (float)(1.0 / sqrt(var))
 * with count converted to float64 once.  The slots are left as they are: a second finalize adds them a second time.
 * PBG_E_ARG (before any HIP call) for a NULL object, n_used_slots outside 0 .. n_slots or a var_floor that is not > 0.
 *
 * pbg_ret_stats_apply: rew_out[i] = clamp(rew_in[i] * scale) for i < count: v = r * scale in float32 (one rounding),
 * then v < -clip ? -clip : (v > clip ? clip : v), so a NaN passes.  One launch; float4 loads and stores where both
 * pointers are 16-byte aligned (the last count % 4 elements one by one), element by element otherwise: the same bits.
 * PBG_E_ARG (before any HIP call) for a NULL pointer, count < 1, a clip that is not > 0, or rew_out overlapping
 * rew_in.
 *
 * Slots compose like pbg_obs_stats': equal shards of a multiple of 32 envs, each walked at slot_offset = its first
 * global env / 32 (in any object with enough slots), their slots set into one object in shard order and finalized
 * there, give the totals and the scale of the object that walked all envs at once, bit for bit. */
typedef struct pbg_ret_stats pbg_ret_stats;

/* PBG_E_ARG (before any HIP call) for n_envs < 1, n_slots < ceil(n_envs / 32), gamma outside [0, 1] (a NaN included),
 * device < -1 or out NULL; PBG_E_HIP for a device that does not exist.  *out is NULL after every failure. */
int pbg_ret_stats_create(int device, int n_envs, int n_slots, double gamma, pbg_ret_stats** out);
void pbg_ret_stats_destroy(pbg_ret_stats* s);
int pbg_ret_stats_walk(pbg_ret_stats* s, int T, int n, int slot_offset, const float* rew_traj, const uint8_t* done_traj,
                       void* stream);
int pbg_ret_stats_finalize(pbg_ret_stats* s, int n_used_slots, double var_floor, void* stream);
int pbg_ret_stats_apply(const pbg_ret_stats* s, int count, float clip, const float* rew_in, float* rew_out, void* stream);
/* carry, slots and totals to zero, scale to 1: one launch on `stream`. */
int pbg_ret_stats_reset(pbg_ret_stats* s, void* stream);
/* The state as arrays on the object's side (DEVICE arrays of its GPU; HOST arrays for device -1), each a launch on
 * `stream` that copies the words as they are (two for slots and totals; none for count == 0).  Slots: `count` of them
 * from `first`, counts int64 [count], sums float64 [count, 2] (s1, s2 per slot).  Totals: count int64 [1], sums
 * float64 [2].  Carry: float64 [n_envs].  Scale: float32 [1].  PBG_E_ARG (before any HIP call) for a NULL pointer or a
 * range outside the object's slots. */
int pbg_ret_stats_get_slots(const pbg_ret_stats* s, int first, int count, int64_t* counts_out, double* sums_out, void* stream);
int pbg_ret_stats_set_slots(pbg_ret_stats* s, int first, int count, const int64_t* counts, const double* sums, void* stream);
int pbg_ret_stats_get_totals(const pbg_ret_stats* s, int64_t* count_out, double* sums_out, void* stream);
int pbg_ret_stats_set_totals(pbg_ret_stats* s, const int64_t* count, const double* sums, void* stream);
int pbg_ret_stats_get_carry(const pbg_ret_stats* s, double* carry_out, void* stream);
int pbg_ret_stats_set_carry(pbg_ret_stats* s, const double* carry, void* stream);
int pbg_ret_stats_get_scale(const pbg_ret_stats* s, float* scale_out, void* stream);
int pbg_ret_stats_set_scale(pbg_ret_stats* s, const float* scale, void* stream);

/* ---- Value clipping and the KL gate (appended; nothing above changes) ----
 * The two knobs of the PPO2 update the gradient and the optimiser step lacked.
 *
 * Value clipping.  pbg_ppo_grad_io_t.value_old (float32 [B], indexed by batch row like ret) and vf_clip = e > 0.
 * Per row, in float64 from the float32 v, ret_r and value_old_r:
 *   vc = value_old_r + clamp(v - value_old_r, -e, +e)
 *   u1 = (v - ret_r)^2;  u2 = (vc - ret_r)^2
 *   the row's value-loss term = 1/2 max(u1, u2)                       (stats[1] is its mean)
 *   dL/dv_i = vf_coef (u1 >= u2 ? (v - ret_r) : 0) / Bm               rounded once to float32
 * The clipped branch carries no gradient: it can only win when v is outside the clip range, where vc does not depend
 * on v.  Inside the range vc is taken as v itself, not as the rounded value_old_r + (v - value_old_r), so u2 == u1
 * there whatever the magnitudes and the row keeps its derivative.  An exact tie u1 == u2 with v clamped takes the unclipped derivative; torch's `maximum` halves it there.
 * With value_old NULL the function is the one above, the bits of stats[1] included.  v_out, the forward, every sum's
 * order and the workspace are as above on both paths and in pbg_ppo_grad_host.  PBG_E_ARG (before any work) for a
 * vf_clip that is not > 0 (a NaN included) when value_old is set.
 *
 * The KL gate.  `gate` is a caller-owned int32 [2] (DEVICE for the device entries, HOST for the host twins): gate[0] is
 * "stopped", gate[1] the number of minibatch steps applied since the last reset.
 *   pbg_ppo_gate_reset: both words to 0, one stream-ordered operation.
 *   pbg_ppo_gate: one launch of one lane.  If gate[0] == 0: if stats[3] > kl_limit then gate[0] = 1, else
 *     gate[1] += 1.  stats (DEVICE float64 [4]) is pbg_ppo_grad_run's, so stats[3] = mean(logp_old - logp) of the
 *     float64 forward (Spinning Up's criterion).  A NaN stats[3] does not stop: the comparison is false.  kl_limit is
 *     not validated.
 *   pbg_ppo_gate_host: the same on HOST pointers, no GPU.
 * PBG_E_ARG (before any HIP call) for a NULL pointer.
 *
 * What obeys it.  With pbg_ppo_grad_io_t.gate set and gate[0] != 0, the tile kernel of either path (pbg_ppo_grad_run
 * and pbg_ppo_grad_run_part) returns at entry in every workgroup, before it touches the weights, the batch or idx,
 * and the reduction returns at entry: grad_*, stats, logp_out, v_out, part_out and part_stats_out keep what they
 * held.  With pbg_ppo_opt_io_t.gate set and gate[0] != 0, pbg_ppo_opt_step's first launch does not advance t, b1t,
 * b2t and its second launch moves no parameter and no moment and leaves info.  pbg_ppo_grad_host and pbg_ppo_opt_host
 * honour the gate the same way (after their argument checks): PBG_OK, outputs and state untouched.
 *
 * The gate's words are only ever written by pbg_ppo_gate and pbg_ppo_gate_reset, in launches of their own; every
 * other launch only reads them, so no kernel reads a word its own launch writes, and there are no atomics.  A
 * minibatch with the gate is pbg_adv_norm, the tiles, the reduction, pbg_ppo_gate, and the optimiser's two launches: a
 * plain chain with no parallel branches and no conditional nodes, which captures as before.  The step whose
 * stats[3] trips the gate is not applied.  After a stop the parameters are those after the last applied step, stats
 * are the tripping minibatch's, and gate[1] says how many steps were applied. */
int pbg_ppo_gate_reset(int32_t* gate, void* stream);
int pbg_ppo_gate(const double* stats, double kl_limit, int32_t* gate, void* stream);
int pbg_ppo_gate_host(const double* stats, double kl_limit, int32_t* gate);

#ifdef __cplusplus
}
#endif
#endif /* PBG_H */
