/* cosim.h — C ABI of the MI355X batched rollout engine (libcosim_hip.so).
 *
 * Drop-in boundary.  The reference is pure Python: its hot path is
 *     env.step(action) -> StateBuildWrapper/TimeLimitWrapper/CommandWrapper -> <Robot>.step -> mj_step x frame_skip
 * (reference envs/wrappers.py:258-269,309-320,391-405; envs/flamingo_light_v1/flamingo_light_v1.py:131-164), where
 * the arithmetic is reached through pybind11 into libmujoco.  The entry points below are what a batched FFI for that
 * path binds; each comment names the reference interface it replaces.  Plain pointers and sizes only, no torch types.
 *
 * Conventions: every function returns 0 on success or a negative COSIM_E* code (cosim_last_error() has the text);
 * `*_dev` pointers are device (HBM) pointers owned by the caller; calls are ordered on `stream` (a hipStream_t passed
 * as void*, NULL = default stream) and are not re-entrant per handle.
 */
#ifndef COSIM_H
#define COSIM_H

#include <stdint.h>

#include "cosim_model.h"

#ifdef __cplusplus
extern "C" {
#endif

#define COSIM_OK 0
#define COSIM_EINVAL (-1)  /* bad argument / model the engine cannot run */
#define COSIM_EHIP (-2)    /* HIP runtime error */
#define COSIM_ENOGPU (-3)  /* no usable device */

#define CS_MAXFIELD 16
#define CS_MAXCMD 6

/* observation field ids: keys of obs_to_dim (reference flamingo_light_v1.py:68-77) */
#define CS_OBS_DOF_POS 0
#define CS_OBS_DOF_VEL 1
#define CS_OBS_ANG_VEL 2
#define CS_OBS_LIN_VEL 3
#define CS_OBS_PROJ_GRAVITY 4
#define CS_OBS_LAST_ACTION 5
#define CS_OBS_HEIGHT_MAP 6
#define CS_OBS_COMMAND 7

/* The wrapper-layer configuration: what StateBuildWrapper / TimeLimitWrapper / CommandWrapper and the robot env read
 * from config["observation"], config["env"], config["random"] (reference envs/wrappers.py:89-127,290-301,336-347;
 * flamingo_light_v1.py:36-42,56-77). */
typedef struct cosim_obs_config {
  int stack_size, command_dim;
  int n_stacked, n_non_stacked;                 /* entries used in the field lists below */
  int stacked_field[CS_MAXFIELD], non_stacked_field[CS_MAXFIELD]; /* CS_OBS_* in config order */
  int field_dim[8];                             /* obs_to_dim per CS_OBS_* id */
  int field_interval[8];                        /* max(1, round(control_freq / freq)) (wrappers.py:190) */
  float field_scale[8];                         /* config["observation"][name]["scale"] */
  float noise_mean[8], noise_std[8], noise_lower[8], noise_upper[8]; /* random_table sensor_noise level per field */
  int noise_enabled;                            /* 0: additive noise skipped (parity runs: level "none" == exactly 0) */
  int position_command;                         /* config["env"]["position_command"] */
  float command_scales[CS_MAXCMD];
  int max_sim_step;                             /* int(max_duration * control_freq) (wrappers.py:300) */
  float action_delay_prob, init_noise;          /* config["random"] */
  int auto_reset;                               /* engine extension: reset an env in the step that ends its episode */
  /* height map (config["observation"]["height_map"], reference utils/mujoco_utils.py:98-189) */
  int hm_res_x, hm_res_y;
  float hm_size_x, hm_size_y;
} cosim_obs_config_t;

typedef struct cosim_engine cosim_engine_t;

/* Replaces build_env(config) (reference envs/build.py:8-24): compiled model + wrapper config -> N env instances on
 * one GPU.  env_id0 is the global id of local env 0 (RNG streams are keyed by global env id, so results do not depend
 * on how envs are sharded over GPUs).  hull_* / hfield are host pointers (copied). */
int cosim_create(const cosim_model_t* model, const float* hull_vert, const int* hull_adr, const int* hull_nbr,
                 const float* hfield, const cosim_obs_config_t* obs, int n_envs, int device, uint64_t seed,
                 int64_t env_id0, cosim_engine_t** out);
int cosim_destroy(cosim_engine_t* e);

/* Sizes the caller needs to allocate buffers: "state_dim", "action_dim", "command_dim", "info_dim", "nq", "nv",
 * "n_envs", "state_stride", "param_stride", "lds_bytes", "vgprs" ... ; returns the value or a negative error. */
int cosim_query(const cosim_engine_t* e, const char* name);

/* Per-env parameters (domain randomisation; replaces the per-construction MJCF rewrite of XMLManager.get_model_path,
 * reference manager/xml_manager.py:43-87).  name: "body_mass"[N,nbody] "body_invweight0"[N,nbody] (translational)
 * "dof_invweight0"[N,nv] "meaninertia"[N] "dof_frictionloss"[N,nv] "geom_friction"[N,ngeom] (sliding, already
 * max-combined with the ground; robot-robot pairs use the model's geom friction) "kp"[N,nu] "kd"[N,nu].  `host` points to
 * host memory, float32, row-major.  Engine scalars (count 1): "solver_tolerance" (fp32 Newton tolerance), "max_newton",
 * "max_ls" (iteration caps below the model's iterations / ls_iterations, which still bound them; a negative value removes the
 * engine's cap.  Defaults: no Newton cap, so every precision level runs its own 50 / 75 / 100 iterations; a line-search cap of 24
 * against the reference models' 50, a deliberate deviation, DESIGN.md "Solver iteration caps"), "envs_per_wave" (1 | 2: kernel variant, 2 only for flat flamingo_light_v1 and
 * even env counts), "wave_priority" (count 4: s_setprio by solver lag -- Newton iterations taken as usual per substep, then the
 * lag thresholds of priority 1, 2, 3; a huge first threshold switches it off), "debug_substeps" (diagnostics: physics substeps
 * per control step, 0 = frame_skip), "boxbox_mode" (1, default: box-box geom pairs through the mjc_BoxBox routine, up to eight contacts
 * per pair; 0: through MPR like the other convex pairs, one contact), "pair_mode" (1, default: robot-robot pairs with a hull one at
 * a time with wave-cooperative vertex scans; 0: lane-parallel), "contact_twist" (flat flamingo_light_v1 only; 1: ground contacts in
 * twist space, 32 slots instead of the dense-row kernel's 14, at ~70 % of the speed; before the first step), "ls_tolerance_scale"
 * (multiplies the line-search tolerance; 1 = the model's), "ranges" (1..16: cosim_step issues the fleet as that many launches over
 * contiguous env ranges on engine-owned streams; default 1), "deferred_join" (see cosim_step / cosim_join), "inflight" (control steps cosim_step lets the host run ahead of each
 * range stream before it blocks, default 2, 0 = unbounded: deep queues step slower on this runtime), "split" (heightfield kernels that have the two-kernel pipeline -- humanoid_p_v0:
 * the prism walk in a kernel of its own, "narrow_waves" (default 6) waves per env, and the solver one substep per launch; 0 goes back
 * to the fused kernel), "fixup" (0 switches the
 * large-capacity fix-up launches off, the heightfield one included: contacts beyond the fleet kernel's slots are then left out and
 * counted), "hfield_fixup" (heightfield terrain, opt-in, default 0; COSIM_EINVAL on the plane and with "envs_per_wave" 2: 1 redoes what
 * does not fit the fleet kernel's ground-contact slots with 50 (mjMAXCONPAIR) slots per ground geom -- 650 flamingo_light_v1, 400
 * flamingo_p_v3, 850 w4_p_v2, 1100 humanoid_p_v0 -- the most the narrowphase can emit, so no ground contact is left out for want of a
 * slot; the fused kernel gives up and flags the control step, the split pipeline's solver launch the substep, and a fix-up launch on the
 * same stream redoes it from the untouched state; robot-robot pair slots are unchanged), "support_map" (1,
 * default: support queries on mesh geoms with 32 or more hull vertices go through the hull's support map -- the few vertices that can
 * win in the direction's cube-map cell, same arg max as the scan; 0: every query scans the whole hull, for A/B runs and tests),
 * "timing_stride" (default 1: with cosim_set_timing on, an event pair around every launch; n: around every n-th launch -- the
 * events cost ~4 % of a 20-step run at 1, choose n coprime with "ranges" so that every range is sampled),
 * "block_cull" (1, default: the narrowphase kernel of the split pipeline tests blocks of 8 prisms -- height and oriented box -- before
 * their prisms; 0: every block goes on to the per-prism tests; same contacts either way), "step_kernel" (1, default: cosim_step /
 * cosim_step_range / cosim_rollout launch the step-only instantiation of the fleet kernel where the fleet has one -- the dense plane
 * kernel of flamingo_light_v1 and its rollout kernel: the kernel mode compiled in, no reset branch, no debug dump; 0: the general
 * instantiation that reset, debug forward and replay always run; the same bits either way, kept as the A/B switch;
 * cosim_query "step_kernel" answers 1 while steps run the step-only instantiation, 0 otherwise).
 * cosim_query additionally answers "contact_slots" / "pair_slots" (capacity of the selected kernel variant: heightfields with cells
 * of 10 cm or more select the 48-slot variants of flamingo_light_v1 / w4_p_v2), "fixup_contact_slots" (capacity of the kernel that
 * redoes a control step -- on the split pipeline with "hfield_fixup", a substep -- whose contacts did not fit; 0: this model / terrain
 * has none, or it is switched off: on a heightfield it is non-zero only while "hfield_fixup" is 1), "ranges", "lds_bytes", "frame_skip" (physics
 * substeps per control step: the precision level's), "max_newton" / "max_ls" (the caps the solver runs with) and "spawn_rows" /
 * "spawn_mode" (cosim_spawn_set: rows of the spawn table, 0 = none; 0 = row by env id, 1 = drawn per episode).
 * Two of the kernel switches are one-way for the life of the engine: "contact_twist" 1 (a later 0 does nothing; it also ends
 * "envs_per_wave" 2, the plane fix-up, the step-only kernel and cosim_rollout) and "fixup" 0 (a later non-zero value does nothing, and
 * "hfield_fixup", either value, is refused from then on).  The others ("split", "step_kernel", "hfield_fixup", "envs_per_wave",
 * "narrow_occupancy") go back and forth; DESIGN.md section 4.17 has the rules in one table. */
int cosim_set_param(cosim_engine_t* e, const char* name, const float* host, int count);

/* Replaces env.reset() (reference envs/wrappers.py:245-256,303-307,385-389; flamingo_light_v1.py:209-232).
 * mask_dev: uint8[N] or NULL (= all).  commands_dev: float[N,command_dim] user commands (see cosim_step).
 * state_out_dev: float[N,state_dim] (rows of envs that are not reset are left untouched). */
int cosim_reset(cosim_engine_t* e, const uint8_t* mask_dev, const float* commands_dev, float* state_out_dev,
                void* stream);

/* Replaces receive_user_command() + env.step(action) (reference core/tester.py:68,90; envs/wrappers.py:349-405).
 * actions_dev float[N,nu]; commands_dev float[N,command_dim] raw user commands (scaling / position-mode transform is
 * applied in the kernel from the pre-step pose, as CommandWrapper.receive_user_command does before the step);
 * state_out_dev float[N,state_dim]; terminated_dev/truncated_dev uint8[N]; info_out_dev float[N,info_dim] or NULL:
 * [action_diff_RMSE, lin_vel_x, lin_vel_y, ang_vel_yaw, torque[nu], set_points[nu], state[k]]. */
int cosim_step(cosim_engine_t* e, const float* actions_dev, const float* commands_dev, float* state_out_dev,
               uint8_t* terminated_dev, uint8_t* truncated_dev, float* info_out_dev, void* stream);
/* With "ranges" > 1, cosim_step forks: the engine's range streams wait for `stream` (the step's inputs), each steps its range, and
 * `stream` then waits for all of them (join) -- unless "deferred_join" is 1: the join is then left to cosim_join, or to the next
 * cosim_reset / cosim_get / cosim_set / cosim_event_push (they join first).  A deferred join is what lets a range's next control
 * step start while the other ranges are still inside the current one (a launch ends with its slowest env): a caller whose next
 * actions do not depend on the whole fleet's last outputs (an action table, or a policy evaluated per range on the range's stream:
 * cosim_range) calls cosim_step back to back and joins when it reads results.  With a deferred join the INPUT buffers of a step (actions_dev,
 * commands_dev) must stay untouched until that step has run: at most "inflight" (default 2) steps are in flight, so rotating three
 * action buffers, or an action table, is enough; the output buffers hold the newest step's results after the join.
 * (The reference steps one env: core/tester.py:90.) */
/* The reference's loop itself (core/tester.py:66-97: command -> policy -> step -> reporter, until done) with the policy replaced by an
 * action table: `steps` control steps in ONE launch per range.  actions_dev is [steps][N][nu]; state_out_dev [steps][N][state_dim],
 * terminated_dev / truncated_dev [steps][N], info_out_dev [steps][N][info_dim] or NULL: row k holds what cosim_step would have been
 * given / would have returned at step k (auto-reset included); commands_dev [N][command_dim] holds for the whole rollout.  A wave
 * stays on its env for all the steps, so no env waits at every step for the slowest env of its launch.  Envs that a dense fleet
 * kernel abandons at step k (more contacts than slots) finish the rollout in the large-capacity kernel.  Available where
 * cosim_query "rollout" is 1; the caller's stream waits for the whole rollout on return. */
int cosim_rollout(cosim_engine_t* e, int steps, const float* actions_dev, const float* commands_dev, float* state_out_dev, uint8_t* terminated_dev,
                  uint8_t* truncated_dev, float* info_out_dev, void* stream);
/* Test hook, host only (no GPU call): the support map the engine builds for a mesh geom's convex hull (csrc/cosim_hullmap.h: per cell
 * of a cube map of directions, the vertices that can be the support point somewhere in the cell) against the full scan over the hull
 * that the reference's support function performs (mjc_support -> arg max of dir . vertex).  verts [n][3]; adr [n + 1] / nbr: CSR
 * neighbour graph of the hull, ids local to the hull; dirs [ndir][3] in the hull's frame.  out_map_idx / out_scan_idx [ndir]: the
 * arg-max vertex through the map / by scanning; out_stats[3] (may be NULL): candidates in the table, largest cell, cells. */
int cosim_hull_support_check(const float* verts, int n, const int* adr, const int* nbr, const float* dirs, int ndir, int* out_map_idx,
                             int* out_scan_idx, int* out_stats);
/* Test hook (GPU): the device's own support routines on mesh geom `geom` at identity pose, for n_dirs directions (host float[n][3]):
 * out_host [n_dirs][6] = support point from the lane-parallel routine, then from the wave-cooperative one.  use_map 0: full scans. */
int cosim_debug_support(cosim_engine_t* e, int geom, const float* dirs_host, int n_dirs, float* out_host, int use_map);
int cosim_join(cosim_engine_t* e, void* stream);
/* Range i of "ranges": its first env, env count and stream (hipStream_t; NULL when ranges == 1).  Work enqueued on that stream from
 * outside (a per-range policy, a reporter reduction) is ordered with the range's steps; cosim_range_mark(i) re-arms the range's
 * "done" event afterwards so that the next join waits for that work too. */
int cosim_range(const cosim_engine_t* e, int i, int* first, int* count, void** stream);
int cosim_range_mark(cosim_engine_t* e, int i);

/* The same control step for envs [first, first + count) only; every pointer still addresses the WHOLE fleet's buffers ([N, ...]).
 * Lets a caller step one fleet as several independent shards on streams of its own (a shard's next control step fills the tail
 * of the others' launches: a launch ends with its slowest env) without one handle per shard.  Envs never interact and every
 * random stream is keyed by the global env id, so results do not depend on the split.  (No reference counterpart: the
 * reference steps one env, core/tester.py:90.) */
int cosim_step_range(cosim_engine_t* e, int first, int count, const float* actions_dev, const float* commands_dev, float* state_out_dev,
                     uint8_t* terminated_dev, uint8_t* truncated_dev, float* info_out_dev, void* stream);

/* Replaces env.get_data() reads (reference flamingo_light_v1.py:247-248; wrappers.py:360-367): copies
 * "qpos"[N,nq] / "qvel"[N,nv] / "qacc_warmstart"[N,nv] / "sim_step"[N] (as float) to a device buffer.  "meta"[N,16] (int32 bits):
 * per-env counters, among them [8] contacts left out, [10] most contacts in one substep, [12] fix-up passes -- control steps redone
 * by a large-capacity kernel; on the split pipeline with "hfield_fixup", substeps (the unit that pipeline redoes) -- and [13] prism
 * walks cut at their bound (solver_stats() in cosim_amd/batched_env.py sums them), [14] the spawn-table row the env's last reset
 * took its base pose from (cosim_spawn_set; written only while a table is set), [15] the cause of the env's latest episode end
 * (cosim_fall_set; written only while a fall rule is set). */
int cosim_get(cosim_engine_t* e, const char* name, float* out_dev, void* stream);
/* Test / checkpoint hook: overwrite "qpos"/"qvel"/"qacc_warmstart" from a device buffer. */
int cosim_set(cosim_engine_t* e, const char* name, const float* in_dev, void* stream);

/* Full-state snapshots (no reference counterpart: the reference has one env and no checkpoint).  A snapshot row is opaque and
 * self-contained: cosim_query "snapshot_floats" float32 words = the env's whole state record ("state_stride": qpos, qvel, warm start,
 * action-delay line, last action, the 16 meta words -- sim_step and the Philox step counter that keys every later noise, delay and
 * spawn draw among them --, the per-field frequency cache, the observation stack) followed by its parameter record ("param_stride":
 * masses, inverse weights, friction, gains); both are padded to 32 floats, so is the row.  Nothing else survives a control step: the
 * split pipeline's per-step record ("xstate") is rewritten by the first launch of every control step before it is read, and the
 * overflow flags are cleared by the fix-up launch that follows the launch that set them, so neither is part of the row.  A row does
 * NOT carry the model, the terrain or the spawn table: restore rows only into an engine built like the one they came from (the rows
 * cannot tell; cosim_amd/snapshot.py checks metadata).  The diagnostic counters in the meta words travel with the row: after a restore
 * they describe the restored history.
 * cosim_snapshot: joins the range streams, flushes a pending parameter upload (the row holds what the next step would run with; the
 * only host-blocking part, and only after a cosim_set_param), then packs every env's row into out_dev [N][snapshot_floats] in one
 * launch on `stream`; asynchronous, capturable.
 * cosim_restore: joins, then env d takes row src_index_dev[d] of snap_dev [snap_rows][snapshot_floats] (NULL: row d, and snap_rows
 * must equal N); envs with mask_dev[d] == 0 are left untouched; with_params 0 leaves every env's parameter record as it is (the robot
 * in slot d keeps its masses and gains), 1 restores it too (the host mirror cosim_set_param edits is read back from the device before
 * the next per-env cosim_set_param, which rewrites the whole table from it).  One launch of a gather kernel (csrc/cosim_snapshot.hip);
 * the source is the caller's buffer, never the live state, so a permutation cannot alias.  An index outside [0, snap_rows) is refused
 * by the kernel: it never reads the row, leaves that env untouched (the other envs are restored) and counts it in a device error
 * word; with a source index the call then waits for `stream` and returns COSIM_EINVAL naming the first such env.  With src_index_dev
 * NULL nothing can be out of range and the call is asynchronous; while `stream` is being captured the wait is skipped (refused envs
 * are still skipped by the kernel).  A restored env in slot d draws from slot d's random streams (they are keyed by the global env
 * id), so envs forked from one row share no random stream with their source or with each other.  snap_dev / out_dev: 16-byte aligned. */
int cosim_snapshot(cosim_engine_t* e, float* out_dev, void* stream);
int cosim_restore(cosim_engine_t* e, const float* snap_dev, int snap_rows, const int32_t* src_index_dev, const uint8_t* mask_dev,
                  int with_params, void* stream);
/* History ring: snapshots taken by cosim_step itself, without the join a caller's cosim_snapshot needs (which would undo the
 * deferred join of the range chains).  cosim_history_set(slots, every): slots 0 switches it off and frees it; otherwise cosim_step
 * counts its calls from here on, and after every `every`-th call packs each range's rows into ring slot (capture number) mod slots on
 * that range's own stream, behind the range's last launch of the step (fix-up launches included): no join, no extra event, nothing on
 * the other steps.  Blocks until the device is idle (it frees / allocates slots x N rows).  cosim_reset, cosim_step_range and
 * cosim_rollout neither capture nor count.  While `stream` is being captured into a graph and a history is set, cosim_step returns
 * COSIM_EINVAL (a replayed graph would repeat whatever step parity was captured).  cosim_query answers "history_slots" /
 * "history_every".  cosim_history_get: joins and copies capture `age` (0 = newest) to out_dev [N][snapshot_floats]; *steps_ago =
 * cosim_step calls since it was taken; COSIM_EINVAL if age >= slots or that capture does not exist yet. */
int cosim_history_set(cosim_engine_t* e, int slots, int every);
int cosim_history_get(cosim_engine_t* e, int age, float* out_dev, int* steps_ago, void* stream);

/* Episode ledger (no reference counterpart: the reference tests one robot and reads its flags on the host every step).  Per-episode
 * outcomes of every env, kept on the device without a host read per step.  cosim_ledger_set(slots): 0 switches it off and frees its
 * buffers (no launch then differs from an engine that never had one); 1..4096 allocates a ring of `slots` records per env and every
 * env starts an open episode at length 0 -- with flag 8 if the engine has been stepped since its last whole-fleet cosim_reset.
 * Blocks until the device is idle.  From then on cosim_step_range (so cosim_step, on every range's own stream, deferred join or not)
 * and cosim_rollout launch ledger_step_kernel (csrc/cosim_ledger.hip) behind the range's last launch -- fix-up launches and the split
 * pipeline's last substep included -- over the rows they were given (1 / `steps`): plain device work on persistent buffers, so a
 * captured step carries it.  Both calls then need info_out_dev (COSIM_EINVAL without).  Per env and row, in this order: length and
 * steps_seen + 1; six double sums += (double) of the fp32 values info[0] (action_diff_RMSE), info[1] (lin_vel_x),
 * fabsf(cmd[i] - info[1 + i]) for i < min(command_dim, 3) (fp32 subtraction; raw user command, cosim_fleet_stats' convention) and
 * (sum over j ascending of fabsf(info[4 + j])) / nu (fp32 sum, one fp32 divide); two fp32 peaks by fmaxf (NaN is ignored):
 * max_j |torque_j| and |cmd[0] - info[1]|.  If terminated | truncated of the row is non-zero, one record goes to slot
 * (episode mod slots) of the env's ring and the next episode begins: sums, peaks and length zero, flags clear, spawn row = meta
 * word 14 (the auto-reset has written the new episode's row), nan_resets base = meta word 4.  Record, 16 int32 words:
 *   [0] episode ordinal of this env since cosim_ledger_set (0-based)   [1] length in control steps
 *   [2] flags: 1 terminated, 2 truncated, 4 meta word 4 advanced during the episode (a non-finite state reset the env), 8 the episode
 *       did not begin at a reset (cosim_restore / cosim_set / a ledger set on a stepped fleet), 16 still open (open_dev rows only),
 *       32 / 64 / 128 a fall rule ended it: tilt / height / body contact = (meta word 15 & 7) << 5, read while a rule is set
 *       (cosim_fall_set) behind the step that closed the record; 0 with no rule
 *   [3] spawn-table row the episode started from (-1 with no table)    [4] steps_seen: rows of this env since cosim_ledger_set
 *   float32 bits: [5] mean action_diff_RMSE  [6..8] mean tracking error i (0 beyond command_dim)  [9] mean abs torque
 *   [10] peak abs torque  [11] mean lin_vel_x  [12] peak tracking error 0;   [13] scenario row + 1 (0: no scenario table)   [14..15] 0.   Means are (float)(sum / (double)length).
 * A rollout's kernel sees the meta words as the launch left them: with several episodes of an env ending inside one cosim_rollout,
 * flag 4, the spawn row and the fall cause (flags 32 / 64 / 128) are exact per launch, not per row.
 * cosim_reset begins a new episode for its mask's envs and discards what they had open (an episode the host cut is no outcome);
 * cosim_restore does so for the envs it restored, cosim_set for all envs, both with flag 8.  An episode "ends" whenever a step
 * returns a flag: without auto-reset a termination that persists yields one-step episodes.  cosim_profile_step does not feed the
 * ledger, and the ledger is not part of a snapshot row.
 * cosim_ledger_get: joins the range streams, then copies the rings to records_dev int32[N][slots][16], the per-env count of ended
 * episodes to counts_dev int32[N] (the ring holds the last min(count, slots) of them; count - slots were overwritten) and, unless
 * NULL, the open episodes formatted as records (flag 16; means 0 at length 0) to open_dev int32[N][16] (16-byte aligned).
 * cosim_query answers "ledger_slots". */
int cosim_ledger_set(cosim_engine_t* e, int slots);
int cosim_ledger_get(cosim_engine_t* e, int32_t* records_dev, int32_t* counts_dev, int32_t* open_dev, void* stream);

/* Failure traces (no reference counterpart): a per-env flight recorder on the device.  The ledger says that an episode failed, how and
 * after how many steps; a trace holds what the robot did in its last `frames` control steps before that.  cosim_ftrace_set(frames,
 * keep, on_mask): frames 0 switches the feature off and frees its buffers (no launch then differs from an engine that never had
 * it); otherwise frames is 1..1024, keep 1..64 and on_mask a non-empty subset of 1|2|4|32|64|128 (the ledger's flags: the causes
 * that freeze a window).  Every env gets keep + 1 buffers of 16 + frames * F int32 words -- a header, then a ring of frames -- and
 * starts an open episode in an empty window, with flag 8 if the engine has been stepped since its last whole-fleet cosim_reset.
 * Blocks until the device is idle; an allocation failure returns COSIM_EHIP with the byte count in the message.
 * Frame, F = "ftrace_frame_words" 32-bit words (a multiple of 4; every word a plain copy, NaN stays NaN):
 *   [0] 1-based step of the episode   [1] 1 terminated | 2 truncated   [2..3] 0
 *   qpos[nq], qvel[nv]: the state record as the previous step, or the reset, left it -- the state the step started from
 *   action[nu]: the caller's raw action row   command[command_dim]: the applied command (cmd_out_dev while a scenario table is set)
 *   info[info_dim]: the step's info row (on a done step: written before the auto-reset, it describes the step that ended)
 *   zero padding up to F.
 * From then on cosim_step_range (so cosim_step, on every range's own stream, deferred join or not, captured or not) launches
 * ftrace_step_kernel (csrc/cosim_ftrace.hip) behind the range's last launch of the step, behind the ledger's.  Per env, in this
 * order: the outcome part (words 0..3, action, command, info) of the frame at the ring cursor; if terminated | truncated is set,
 * flags as the ledger builds them, and if flags & on_mask != 0 the header below is written, the working index moves to the next
 * buffer modulo keep + 1 (nothing is copied: the keep buffers behind the working one are the latest keep traces, an older one is
 * overwritten and counted as lost) -- otherwise the window is emptied in place -- and the next episode begins at ring position 0
 * (spawn row = meta word 14, nan_resets base = meta word 4); with no flag the cursor advances modulo frames; last, the state part
 * (qpos, qvel) of the frame at the new cursor is copied from the live state record: after a done step under auto-reset that is the
 * new episode's reset pose.  Header, 16 int32 words:
 *   [0] episode ordinal of this env since cosim_ftrace_set (the ledger's, if both were set together)   [1] length in control steps
 *   [2] flags, the ledger's meanings and values: 1 terminated, 2 truncated, 4 meta word 4 advanced, 8 did not begin at a reset,
 *       16 open (open_dev rows only), 32 / 64 / 128 = (meta word 15 & 7) << 5, read only while a fall rule is set
 *   [3] valid frames = min(length, frames)   [4] ring position of the oldest valid frame (time order: oldest, oldest + 1, ... modulo
 *       frames)   [5] spawn-table row the episode started from (-1 with no table)   [6] scenario row + 1 (0: no table)
 *   [7] steps_seen: steps of this env since cosim_ftrace_set   [8..15] 0.
 * The kernel reads actions_dev, info_out_dev, the flags and the command buffer of the step: like the ledger's command buffer, the
 * ACTION BUFFER MUST OUTLIVE THE STEP (stay untouched until the range's stream has run it).  cosim_step* then needs info_out_dev
 * (COSIM_EINVAL without).  cosim_rollout returns COSIM_EINVAL while traces are set: one launch leaves one state record for K steps,
 * the per-step state is not there to copy.  cosim_profile_step does not feed the recorder.  cosim_reset begins a new episode for its
 * mask's envs and discards their open window (flag 0); cosim_restore does so for the envs it restored, cosim_set for all envs, both
 * with flag 8: nothing is kept for an episode the host cut.  Limits: a scenario push applied ahead of the step is not in the frame's
 * state part (it shows in the next frame and in the info row); the pose a terminal step ends in is reset inside the step kernel and
 * is not captured (the last frame holds the pose one control step earlier and the terminal info row); traces are not part of a
 * snapshot row.
 * cosim_ftrace_get: joins the range streams, then copies every buffer to buffers_dev int32[N][keep + 1][16 + frames * F], per env
 * the working buffer index, the count of traces triggered and of traces lost to counts_dev int32[N][3] (the kept traces are the
 * min(triggered, keep) buffers behind the working one) and, unless NULL, the headers of the open windows (flag 16) to open_dev
 * int32[N][16]; an open window's cursor frame already holds the next step's starting state, so its [3] is min(length, frames - 1).
 * COSIM_EINVAL with nothing set.  cosim_query answers "ftrace_frames", "ftrace_keep", "ftrace_frame_words" and "ftrace_mask". */
int cosim_ftrace_set(cosim_engine_t* e, int frames, int keep, int on_mask);
int cosim_ftrace_get(cosim_engine_t* e, int32_t* buffers_dev, int32_t* counts_dev, int32_t* open_dev, void* stream);

/* Scenario table (the reference's tester changes the command and holds the push button of its ONE robot while it runs,
 * core/tester.py:41-53,68,80-81): per-env command and push schedules, kept and applied on the device.  S = n_scn scenarios in CSR
 * form, host arrays: scenario s owns command keyframes [key_adr[s], key_adr[s + 1]) -- times key_t int32, strictly increasing, rows
 * key_cmd float[.][command_dim] -- and push windows [push_adr[s], push_adr[s + 1]) -- push_t int32[.][2] = (t0, t1) with t1 > t0,
 * world velocities push_v float[.][3], in listed order, possibly overlapping.  At most 64 keyframes and 64 windows per scenario,
 * either list may be empty; times are control steps of the episode, 0 <= t < 2^30; 1 <= S <= 65536.
 * From then on cosim_step_range (so cosim_step, on every range's own stream, deferred join or not) launches scenario_step_kernel
 * (csrc/cosim_scenario.hip) AHEAD of the range's first launch of the control step -- on the split pipeline once per control step,
 * ahead of the first narrowphase launch.  Per env: t = meta word 0 (steps of the running episode, 0 right after any reset, the
 * auto-reset inside the previous step included), ep = meta word 11 (episodes ended), gid = env_id0 + env;
 *   row = gid mod S (mode 0, "env")  or  (gid mod S + ep mod S) mod S with ep as uint32 (mode 1, "cycle": one scenario per episode);
 *   command: cmd_out_dev[env][:] = the last keyframe of the row with key_t <= t, whole row; none: commands_dev[env][:] of the call;
 *   push: the last LISTED window of the row with t0 <= t < t1, if any, sets qvel[0:3] of the record with cosim_event_push's bits, from
 *   the pre-step quaternion, before every step of the window;   row_out_dev[env] = row.
 * The step kernels, the fix-up kernels, the ledger and (through cmd_out_dev) the caller's reporter read cmd_out_dev as the command.
 * cosim_reset runs the same kernel ahead of the reset launch for the envs under its mask with t = 0 and no push: the reset's state
 * vector carries the scenario's first command.  Nothing is kept per env -- the rule is a function of words of the state record -- so a
 * restored snapshot continues its schedule, a fork follows its slot's global id, and shards that set the same table give one
 * fleet's results.  Plain device work on persistent buffers: a captured step carries it.  The table is not part of a snapshot row.
 * A host command or cosim_event_push still works; a scenario keyframe / push due in the same step overrides it.
 * cmd_out_dev float[N][command_dim] and row_out_dev int32[N] are caller-owned and must outlive the table.  n_scn = 0 clears the
 * table (no launch then differs from an engine that never had one).  A table of the sizes (S, keyframes, windows) of the one that is
 * set is rewritten in place: the device pointers stay, captured graphs keep working and pick up the new values.  The call joins the
 * ranges and blocks until the device is idle and the table uploaded.  Validated on the host before anything is launched or changed,
 * the message names the scenario and the row (COSIM_EINVAL): non-finite values, keyframe times that do not increase, t1 <= t0, more
 * than 64 keyframes / windows, S out of range, mode 1 without auto_reset (meta word 11 would advance on every flagged step).
 * cosim_rollout returns COSIM_EINVAL while a table is set (one launch reads one command row); cosim_profile_step ignores the table.
 * While a table is set, word 13 of a ledger record is the scenario row of its episode + 1 (0 with no table) and the ledger's
 * tracking errors are against cmd_out_dev.  cosim_query answers "scenario_rows" and "scenario_mode". */
int cosim_scenario_set(cosim_engine_t* e, int n_scn, const int32_t* key_adr, const int32_t* key_t, const float* key_cmd,
                       const int32_t* push_adr, const int32_t* push_t, const float* push_v, int mode,
                       float* cmd_out_dev /*[N][command_dim]*/, int32_t* row_out_dev /*[N]*/, void* stream);

/* Fall rules (the reference ends an episode early only through a robot's own _is_done, which is an empty body list for
 * flamingo_light_v1 and False for w4_p_v2 and humanoid_p_v0): the step kernels end an episode on the posture of the state a control
 * step ends in, per cause.  Evaluated once per control step (every step of a rollout launch, the last substep launch of the split
 * pipeline, the fix-up kernels), before the info row, the auto-reset and the reset observation, so a fall is an episode end like any
 * other: terminated = 1, the info row of the fallen step, the reset state vector, meta word 11, the ledger, scenario mode "cycle".
 *   tilt (cause bit 1):   up = 1 - 2 (qx^2 + qy^2) of qpos[3:7] as stored (the world-z component of the base's z axis) < min_up, so
 *                         min_up = cos(max tilt); min_up <= -1 switches the rule off;
 *   height (cause bit 2): qpos[2] - ground < min_height; ground = the plane's z, or the heightfield's elevation under the base (the
 *                         height-map observation's lookup; off the field the rule does not fire); min_height <= 0 switches it off;
 *   body contact (bit 4): the robot's _is_done rule (cfrc_ext of the listed bodies, any signed component > 1.0).  n_bodies < 0 leaves
 *                         the model's own list alone; n_bodies >= 0 replaces it by body_ids (0 bodies: no body rule) in the device
 *                         model, which is uploaded again (the call blocks until the device is idle).
 * Tilt and height hold only while the episode clock (meta word 0, 1 on the first step after a reset) is > grace_steps; the body rule
 * is the model's block unchanged and knows no grace.  NaN compares false: a non-finite state is the non-finite check's case.  While
 * any rule is set, every episode end writes its cause into meta word 15 (the OR of the bits; 0 for a time limit, a non-finite state
 * or no rule firing), and bit 4 is recorded for the model's own list too.  min_up <= -1, min_height <= 0 and n_bodies < 0 together
 * switch everything off: the model's own list is restored and meta word 15 is no longer written (no launch then differs from an
 * engine that never had a rule).  COSIM_EINVAL, naming the value: body id 0 (the world) or >= nbody, grace_steps < 0, a non-finite
 * threshold.  cosim_query "fall" answers the mask of rules in force (1 | 2 | 4, 0 for none).
 * The thresholds travel as kernel arguments: a captured graph keeps the values it was captured with.  Set the rule before capturing.
 * The rule is not part of a snapshot row (the cause word is, like every meta word). */
int cosim_fall_set(cosim_engine_t* e, float min_up, float min_height, int grace_steps, const int32_t* body_ids, int n_bodies);

/* Spawn table (no reference counterpart: the reference resets its one robot to the model's init_qpos).  M = `rows` base poses
 * spread over the terrain; every reset -- cosim_reset, the auto-reset inside every step / rollout / fix-up kernel, the reset after a
 * non-finite state -- takes qpos[0:7] from a row instead of init_qpos[0:7]; joint angles, init noise and velocities are unchanged.
 * xyyaw_host float[rows][3]: x, y, yaw per row.  A HIP kernel places each row on the heightfield: footprint_host float[n_foot][4] =
 * (ox, oy, r, free) per ground geom -- horizontal offset of its bounding-sphere centre from the base, radius, and height of the
 * sphere's lowest point above z = 0, all at init_qpos (cosim_amd/spawn.py footprint()) --, g_xy = (x, y) + R(yaw) (ox, oy), hmax_g =
 * the highest heightfield sample among the vertices cmin..cmax x rmin..rmax with cmin = floor((lx - r + sx) / dx), cmax =
 * ceil((lx + r + sx) / dx), lx = g_x - ground_pos.x, dx = 2 sx / (ncol - 1) (rows alike), and
 *     z = init_qpos[2] + max(0, max_g(sz hmax_g - free_g)) + clearance,    quat = (cos yaw/2, 0, 0, sin yaw/2) (x) init_qpos[3:7]:
 * no geom ends lower over the terrain than it was over z = 0 at init_qpos.  On plane ground z = init_qpos[2] + clearance.
 * A yaw does not turn gravity in the body frame, so the state vector a reset returns takes projected gravity from init_qpos[3:7]:
 * on plane ground it is, bit for bit, the state vector of a reset without a table.
 * COSIM_EINVAL, with the row in the message, if a row is not finite or puts a footprint sphere off the field (|l| + r > s).
 * rows = 0 clears the table; the same `rows` again rewrites it in place (the device pointer stays, captured graphs keep working);
 * a new table takes effect at each env's next reset.  per_episode 0: row = global env id mod rows; 1: row = min(rows - 1,
 * floor(u01(philox(seed, gid, step_count, purpose 5, index 0)) * rows)) with the step counter (meta word 1) of the launch that resets,
 * the one its init-noise draw uses.  Both depend on the global env id and the seed only: shards that set the same table give the
 * results of one fleet.  Joins the range streams and blocks until the table is placed.  With no table (the default) nothing changes. */
int cosim_spawn_set(cosim_engine_t* e, const float* xyyaw_host, int rows, const float* footprint_host, int n_foot, float clearance,
                    int per_episode, void* stream);
/* The placed poses, float[rows][7] = x, y, z, qw, qx, qy, qz, to host memory (at most `capacity` rows); returns the table's row count. */
int cosim_spawn_get(cosim_engine_t* e, float* poses_host, int capacity);

/* Replaces env.event("push", v) (reference flamingo_light_v1.py:234-245): v_dev float[N,3] world-frame velocity,
 * mask_dev uint8[N] or NULL. */
int cosim_event_push(cosim_engine_t* e, const float* v_dev, const uint8_t* mask_dev, void* stream);

/* Debug hook for the parity tests: runs ONE mj_forward-equivalent on env `env` in a diagnostic kernel and copies the
 * named intermediate to host doubles-as-float: "xpos" "xquat" "M" "cdof" "contacts" "J" "efc" "qacc" ... */
int cosim_debug_forward(cosim_engine_t* e, int env, const char* name, float* host_out, int capacity);

/* Average duration (ms) of the step kernel since the last call, measured with HIP events on the launch stream, and
 * the number of launches averaged; resets the accumulator. */
/* Diagnostics: the 32 64-bit counters diagnostic kernel builds accumulate (cosim_set_param "narrow_occupancy" 0: the narrowphase
 * kernel of the split pipeline -- [0] sum, [1] max, [2] number of wave lifetimes in shader-clock cycles, [3] work items, [8..15]
 * the walk's phases; see tools/gpu_narrow_prof.py); clear != 0 zeroes them afterwards. */
int cosim_debug_counters(cosim_engine_t* e, unsigned long long* out32, int clear);
int cosim_kernel_time(cosim_engine_t* e, float* avg_ms, int* launches);
int cosim_set_timing(cosim_engine_t* e, int enabled);
/* Diagnostic build of the step kernel with s_memtime stamps at phase boundaries (one variant per bench workload): one control
 * step; cycles_out16 must hold 32 doubles: [i < 16] = mean shader-clock cycles per env spent in phase i, [16..23] = the heightfield
 * narrowphase's split (flat kernels: robot-robot pairs, contact-matrix accumulation, tree pass), [24..28] = hull pairs: MPR runs,
 * hits, refinement iterations, cycles, pairs past the bounding spheres; see tools/gpu_phases.py.  Never timed. */
int cosim_profile_step(cosim_engine_t* e, const float* actions_dev, const float* commands_dev, float* state_out_dev,
                       uint8_t* terminated_dev, uint8_t* truncated_dev, double* cycles_out16);

/* Policy side of the loop (reference core/policy.py:11-21, one state per call on the CPU): the actor MLP of an ONNX policy for
 * all N envs in one launch on the matrix pipe, out = clip(act_L(... act_1(x W_1^T + b_1) ...)).  All pointers are device
 * pointers; dims[n_layers + 1] (each 1..512); w_dev[l] is [dims[l+1], dims[l]] row-major (Gemm with transB = 1), b_dev[l] may
 * be NULL; act[l]: 0 none, 1 relu, 2 tanh, 3 elu, 4 sigmoid, 5 leaky relu (act_alpha[l]); clip > 0 clamps to [-clip, clip]. */
int cosim_mlp_forward(const float* x_dev, int n, int n_layers, const int* dims, const float* const* w_dev, const float* const* b_dev,
                      const int* act, const float* act_alpha, float clip, float* out_dev, void* stream);

/* The recurrent policy's cell (reference core/policy.py:24-47: an ONNX LSTM node fed one step at a time with h_in / c_in kept by the
 * caller): one LSTM step for all N envs in one launch.  Gate order and layouts are ONNX's: w_dev [4H, I], r_dev [4H, H], b_dev [8H]
 * (Wb then Rb) or NULL, gates i, o, f, c; default activations.  h_out_dev / c_out_dev may alias h_dev / c_dev (in-place state). */
int cosim_lstm_cell(const float* x_dev, const float* h_dev, const float* c_dev, int n, int in_dim, int hidden, const float* w_dev,
                    const float* r_dev, const float* b_dev, float* h_out_dev, float* c_out_dev, void* stream);

/* Reporter side (reference core/reporter.py:210-218 write_info, :429-442, :506-508): fleet statistics of one step's info in one
 * launch.  acc_dev is double[3][K], K = 4 + nu + ncmd <= 32: count, sum, sum of squares of info[:, 0:4], |info[:, 4:4+nu]| (torque)
 * and |cmd[:, i] - info[:, 1 + i]| for i < ncmd <= 3 (command tracking); cmd_dev is [N, cmd_stride]. */
int cosim_fleet_stats(const float* info_dev, int n, int info_dim, int nu, const float* cmd_dev, int cmd_stride, int ncmd, double* acc_dev,
                      void* stream);

/* Percentiles for the same columns (reference core/reporter.py:429-442, 506-530 keeps and plots every sample of one env; a fleet
 * keeps a mergeable sketch): adds this step's rows to hist_dev, double[K][nbins], bin b of column c = magnitudes in
 * [b, b + 1) * hi_dev[c] / nbins (the last bin also takes what lies above hi_dev[c]).  Sums over steps and ranks are percentiles'
 * sufficient statistic; cosim_amd/reporter.py turns them into p5 / p50 / p95. */
int cosim_fleet_hist(const float* info_dev, int n, int info_dim, int nu, const float* cmd_dev, int cmd_stride, int ncmd, const float* hi_dev,
                     int nbins, double* hist_dev, void* stream);

const char* cosim_last_error(void);
int cosim_model_sizeof(void);
int cosim_obs_config_sizeof(void);

#ifdef __cplusplus
}
#endif
#endif /* COSIM_H */
