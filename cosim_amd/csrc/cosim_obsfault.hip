// cosim_obsfault.hip — observation faults of a scenario table (cosim_set_param "obs_faults", include/cosim.h): timed sensor bias, noise,
// freeze and loss per env, on the device.
//
// obsfault_step_kernel runs BEHIND the last launch of a control step that writes the state record or state_out (the fix-up kernel,
// on the split pipeline the last substep's solver and fix-up) on that stream group's own stream, and behind a reset's launch for
// the envs under its mask; ahead of the observers and the history pack.  One wave per env, lane = frame element in passes of 64:
// it reads the env's post-step clock (meta[0]), step counter (meta[1]) and episode count (meta[11]), looks its row up (scenario_row,
// cosim_scenario.h) and walks the row's 16-byte item records once (cosim_obsfault.h and cosim_fault.h have the rule; the row is the same for the whole
// wave, so the item loads are scalar).  An env whose row has no item that holds leaves after its meta words and the row's records,
// with nothing of its frame loaded.  The faulted values go to row 0 of the record's observation stack, so the next step's roll
// carries them on as a sensor history would, and to state_out.
// No LDS, no atomics, no cross-env traffic, no host read, no join: a captured step carries it.
#include "cosim_dev.h"
#include "cosim_obsfault.h"

namespace cosim {

struct ObsFaultArgs {
  ScnTable tab;            // the scenario table (row rule)
  FaultTable flt;
  float* state;            // [N][s_stride] live state records
  float* state_out;        // [N][state_dim] the step's / reset's observation rows
  const uint8_t* mask;     // reset: uint8[N] or null
  int n_envs, first, count;
  int s_stride, s_meta, s_stack;
  int sd, S, frame_dim, state_dim;
  unsigned seed_lo, seed_hi;
  long long env_id0;
};

constexpr int OBF_PASSES = MAXFRAME / 64;    // every frame fits
static_assert(OBF_PASSES * 64 == MAXFRAME, "passes of 64 lanes");

__global__ __launch_bounds__(64 * FLT_WAVES) void obsfault_step_kernel(ObsFaultArgs a) {
  const int lane = (int)threadIdx.x & 63;
  const int i = __builtin_amdgcn_readfirstlane((int)blockIdx.x * FLT_WAVES + ((int)threadIdx.x >> 6));   // one value per wave
  if (i >= a.count) return;   // the last block's tail
  const int env = a.first + i;
  if (env >= a.n_envs) return;
  if (a.mask != nullptr && a.mask[env] == 0) return;
  float* rec = a.state + (size_t)env * a.s_stride;
  int t, row;
  ObsFaultEnv E = {fault_wave_key(a.tab, reinterpret_cast<const int*>(rec + a.s_meta), env, a.seed_lo, a.seed_hi, a.env_id0, &t, &row),
                   rec + a.s_stack, a.state_out + (size_t)env * a.state_dim, a.sd, a.S, a.frame_dim};
  obsfault_apply<OBF_PASSES>(a.flt, row, t, E, lane, 64, 0);
}

// obsfault_step_kernel while a limit search whose targets name the observation faults is armed.  An observation is scaled by the
// level of the episode it belongs to: on the step that ends episode e the returned observation is clock 0 of episode e + 1, so at the
// step site the engine issues this launch BEHIND search_step_kernel, which has moved the level by then (neither the observers nor the
// search read the words written here: stack row 0 and state_out).  The reset site needs no change: the level does not move there.
struct ObsFaultSearchArgs {
  ObsFaultArgs flt;
  const int* srch_rec;     // [N][srch_ncnt]
  int srch_ncnt;
};

__global__ __launch_bounds__(64 * FLT_WAVES) void obsfault_search_step_kernel(ObsFaultSearchArgs sa) {
  const ObsFaultArgs& a = sa.flt;
  const int lane = (int)threadIdx.x & 63;
  const int i = __builtin_amdgcn_readfirstlane((int)blockIdx.x * FLT_WAVES + ((int)threadIdx.x >> 6));   // one value per wave
  if (i >= a.count) return;   // the last block's tail
  const int env = a.first + i;
  if (env >= a.n_envs) return;
  if (a.mask != nullptr && a.mask[env] == 0) return;
  float* rec = a.state + (size_t)env * a.s_stride;
  int t, row;
  ObsFaultEnv E = {fault_wave_key(a.tab, reinterpret_cast<const int*>(rec + a.s_meta), env, a.seed_lo, a.seed_hi, a.env_id0, &t, &row),
                   rec + a.s_stack, a.state_out + (size_t)env * a.state_dim, a.sd, a.S, a.frame_dim};
  const float level = __int_as_float(__builtin_amdgcn_readfirstlane(sa.srch_rec[(size_t)env * sa.srch_ncnt]));
  obsfault_apply<OBF_PASSES, true>(a.flt, row, t, E, lane, 64, 0, level);
}

}  // namespace cosim
