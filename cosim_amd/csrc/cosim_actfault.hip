// cosim_actfault.hip — action faults of a scenario table (cosim_set_param "action_faults", include/cosim.h): timed actuator-command
// bias, noise, hold and loss per env, on the device.
//
// actfault_step_kernel runs behind scenario_step_kernel and scnparams_step_kernel, AHEAD of a range's first launch of a control step
// on that range's own stream.  One wave per env, lane = actuator (nu <= 64): it reads the env's pre-step clock (meta[0]), step counter
// (meta[1]) and episode count (meta[11]), looks its row up (scenario_row, cosim_scenario.h), loads the caller's action row
// (coalesced), walks the row's 16-byte item records once (cosim_actfault.h and cosim_fault.h have the rule) and stores the env's rows of the two
// engine-owned buffers: actions_raw, the caller's bits, and actions_eff, what every step kernel of the control step is handed as its
// action while faults are set.  EVERY env of the range is written: one under no holding item gets a plain copy.
// One wave per env, not several: the row, the clock and so every item record and every branch on "does this item hold" are the same
// for the whole wave, so the records come through scalar loads and the walk does not diverge; with several envs in a wave the item
// loop would run to the longest row of the wave under a per-lane mask and every record would be a vector load.  The launch is far
// from filling the machine either way (N waves of a few hundred cycles); the arithmetic per word does not depend on the choice.
//
// actfault_obs_kernel runs BEHIND the last launch of the step that writes the state record or state_out (the redo included), ahead
// of obsfault_step_kernel, and only if the observation has last_action elements.  The step kernel built last_action from the action
// it was given, the effective one; a policy on a real robot sees its own output.  One wave per env, lane = frame element in passes
// of 64: for an env whose post-step clock is not 0, each last_action element that is due (clock % el_interval == 0) is rewritten
// with actions_raw[idx] * el_scale -- the frequency cache, stack row 0 and the newest frame of state_out: what the step kernel would
// have written had it been handed the raw action.  An env that was just reset keeps the zeros the step kernel wrote.
// No LDS, no atomics, no cross-env traffic, no host read, no join: a captured step carries both.
#include "cosim_dev.h"
#include "cosim_actfault.h"

namespace cosim {

struct ActFaultArgs {
  ScnTable tab;            // the scenario table (row rule)
  FaultTable flt;
  const float* state;      // [N][s_stride] live state records
  const float* actions;    // [N][nu] the caller's actions
  float* eff;              // [N][nu] effective actions
  float* raw;              // [N][nu] the caller's actions, kept for actfault_obs_kernel
  int n_envs, first, count;
  int s_stride, s_meta, s_lastact, nu;
  unsigned seed_lo, seed_hi;
  long long env_id0;
};

struct ActObsArgs {
  const DevObs* ob;
  float* state;            // [N][s_stride] live state records
  float* state_out;        // [N][state_dim] the step's observation rows
  const float* raw;        // [N][nu]
  int n_envs, first, count;
  int s_stride, s_meta, s_cache, s_stack, nu;
};

constexpr int ACF_PASSES = MAXFRAME / 64;    // every frame fits
static_assert(ACF_PASSES * 64 == MAXFRAME, "passes of 64 lanes");

__global__ __launch_bounds__(64 * FLT_WAVES) void actfault_step_kernel(ActFaultArgs a) {
  const int lane = (int)threadIdx.x & 63;
  const int i = __builtin_amdgcn_readfirstlane((int)blockIdx.x * FLT_WAVES + ((int)threadIdx.x >> 6));   // one value per wave
  if (i >= a.count) return;   // the last block's tail
  const int env = a.first + i;
  if (env >= a.n_envs) return;
  if (lane >= a.nu) return;
  const float* rec = a.state + (size_t)env * a.s_stride;
  int t, row;
  ActFaultEnv E = {fault_wave_key(a.tab, reinterpret_cast<const int*>(rec + a.s_meta), env, a.seed_lo, a.seed_hi, a.env_id0, &t, &row), rec + a.s_lastact};
  const size_t w = (size_t)env * a.nu + lane;
  const float x = a.actions[w];
  a.raw[w] = x;
  a.eff[w] = actfault_apply(a.flt, row, t, E, lane, x);
}

// actfault_step_kernel while a limit search whose targets name the action faults is armed (cosim_search.h): the same wave = env
// shape at the same site, with the env's level -- word 0 of its search record, one scalar per wave -- multiplied into the values of
// the row's marked items.  It runs behind the scenario kernel, ahead of the step, so the level is the one the open episode runs at.
struct ActFaultSearchArgs {
  ActFaultArgs flt;
  const int* srch_rec;     // [N][srch_ncnt] the search's records: word 0 is the level this step runs at
  int srch_ncnt;
};

__global__ __launch_bounds__(64 * FLT_WAVES) void actfault_search_step_kernel(ActFaultSearchArgs sa) {
  const ActFaultArgs& a = sa.flt;
  const int lane = (int)threadIdx.x & 63;
  const int i = __builtin_amdgcn_readfirstlane((int)blockIdx.x * FLT_WAVES + ((int)threadIdx.x >> 6));   // one value per wave
  if (i >= a.count) return;   // the last block's tail
  const int env = a.first + i;
  if (env >= a.n_envs) return;
  if (lane >= a.nu) return;
  const float* rec = a.state + (size_t)env * a.s_stride;
  int t, row;
  ActFaultEnv E = {fault_wave_key(a.tab, reinterpret_cast<const int*>(rec + a.s_meta), env, a.seed_lo, a.seed_hi, a.env_id0, &t, &row), rec + a.s_lastact};
  const float level = __int_as_float(__builtin_amdgcn_readfirstlane(sa.srch_rec[(size_t)env * sa.srch_ncnt]));
  const size_t w = (size_t)env * a.nu + lane;
  const float x = a.actions[w];
  a.raw[w] = x;
  a.eff[w] = actfault_apply_scaled(a.flt, row, t, E, lane, x, level);
}

__global__ __launch_bounds__(64 * FLT_WAVES) void actfault_obs_kernel(ActObsArgs a) {
  const int lane = (int)threadIdx.x & 63;
  const int i = __builtin_amdgcn_readfirstlane((int)blockIdx.x * FLT_WAVES + ((int)threadIdx.x >> 6));   // one value per wave
  if (i >= a.count) return;   // the last block's tail
  const int env = a.first + i;
  if (env >= a.n_envs) return;
  float* rec = a.state + (size_t)env * a.s_stride;
  const int t = __builtin_amdgcn_readfirstlane(reinterpret_cast<const int*>(rec + a.s_meta)[0]);   // post-step: 0 after a reset
  if (t == 0) return;
  const DevObs& ob = *a.ob;
  const int fd = ob.frame_dim, sd = ob.stacked_dim, S = ob.stack_size;
  float* out = a.state_out + (size_t)env * ob.state_dim;
#pragma unroll
  for (int p = 0; p < ACF_PASSES; p++) {
    const int e = lane + 64 * p;
    if (e >= fd) break;
    if (ob.el_field[e] != CS_OBS_LAST_ACTION) continue;
    const int idx = ob.el_index[e], interval = ob.el_interval[e];
    if (idx >= a.nu || interval < 1 || (t % interval) != 0) continue;   // not due: the cached word stands
    actfault_restore(a.raw[(size_t)env * a.nu + idx], ob.el_scale[e], e, sd, S, rec + a.s_cache, rec + a.s_stack, out);
  }
}

}  // namespace cosim
