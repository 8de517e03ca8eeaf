// cosim_scnparams.hip — parameter windows of a scenario table (cosim_scenario_params_set, include/cosim.h): timed gain and friction
// changes per env, on the device.
//
// scnparams_step_kernel runs directly behind scenario_step_kernel, AHEAD of a range's first launch of a control step on that range's
// own stream (and ahead of a reset's launch for the envs under its mask, with t = 0).  One wave per env, lane = word of the parameter
// record: it reads the env's episode clock (meta[0]) and episode count (meta[11]), looks its row up (scenario_row, cosim_scenario.h),
// loads the BASE record (d_params, coalesced), applies the row's items (cosim_scnparams.h has the rule; the row is the same for the
// whole wave, so the item loads are scalar) and stores the EFFECTIVE record, which is what every step kernel is handed as its
// parameter record while windows are set.  The whole record is rewritten every step: a row change in mode cycle or a base changed
// by cosim_set_param needs no bookkeeping.  No LDS, no atomics, no cross-env traffic, no host read, no join: a captured step carries it.
#include "cosim_scnparams.h"

namespace cosim {

struct ScnParArgs {
  ScnTable tab;            // the scenario table (row rule)
  ScnParTable par;
  const float* state;      // [N][s_stride] live state records
  const float* base;       // [N][p_stride] base parameter records (d_params)
  float* eff;              // [N][p_stride] effective parameter records
  const uint8_t* mask;     // reset: uint8[N] or null
  int n_envs, first, count;
  int s_stride, s_meta, p_stride;
  int reset;               // 1: ahead of a reset -- t = 0, masked envs only
};

constexpr int SCNPAR_WAVES = 4;   // envs per block

__global__ __launch_bounds__(64 * SCNPAR_WAVES) void scnparams_step_kernel(ScnParArgs a) {
  const int lane = (int)threadIdx.x & 63;
  const int i = __builtin_amdgcn_readfirstlane((int)blockIdx.x * SCNPAR_WAVES + ((int)threadIdx.x >> 6));   // one value per wave
  if (i >= a.count) return;   // the last block's tail
  const int env = a.first + i;
  if (env >= a.n_envs) return;
  if (a.reset && a.mask != nullptr && a.mask[env] == 0) return;
  const int* meta = reinterpret_cast<const int*>(a.state + (size_t)env * a.s_stride + a.s_meta);
  const int t = a.reset ? 0 : __builtin_amdgcn_readfirstlane(meta[0]);
  const int row = scenario_row(a.tab, env, __builtin_amdgcn_readfirstlane(meta[11]));
  const size_t p0 = (size_t)env * a.p_stride;
  scnparams_apply(a.par, row, t, a.base + p0, a.eff + p0, a.p_stride, lane, 64);
}

// scnparams_step_kernel while a limit search whose targets name the parameter windows is armed: the same wave = env shape at the same
// sites, with the env's level -- word 0 of its search record, one scalar per wave -- multiplied into the values of the row's marked
// items.  It runs behind the scenario kernel, ahead of the step: the level is the one the open episode runs at (a reset does not move it).
struct ScnParSearchArgs {
  ScnParArgs par;
  const int* srch_rec;     // [N][srch_ncnt]
  int srch_ncnt;
};

__global__ __launch_bounds__(64 * SCNPAR_WAVES) void scnparams_search_step_kernel(ScnParSearchArgs sa) {
  const ScnParArgs& a = sa.par;
  const int lane = (int)threadIdx.x & 63;
  const int i = __builtin_amdgcn_readfirstlane((int)blockIdx.x * SCNPAR_WAVES + ((int)threadIdx.x >> 6));   // one value per wave
  if (i >= a.count) return;   // the last block's tail
  const int env = a.first + i;
  if (env >= a.n_envs) return;
  if (a.reset && a.mask != nullptr && a.mask[env] == 0) return;
  const int* meta = reinterpret_cast<const int*>(a.state + (size_t)env * a.s_stride + a.s_meta);
  const int t = a.reset ? 0 : __builtin_amdgcn_readfirstlane(meta[0]);
  const int row = scenario_row(a.tab, env, __builtin_amdgcn_readfirstlane(meta[11]));
  const float level = __int_as_float(__builtin_amdgcn_readfirstlane(sa.srch_rec[(size_t)env * sa.srch_ncnt]));
  const size_t p0 = (size_t)env * a.p_stride;
  scnparams_apply(a.par, row, t, a.base + p0, a.eff + p0, a.p_stride, lane, 64, true, level);
}

}  // namespace cosim
