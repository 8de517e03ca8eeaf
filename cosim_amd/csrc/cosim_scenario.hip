// cosim_scenario.hip — scenario tables (cosim_scenario_set, include/cosim.h): per-env command and push schedules on the device.
//
// scenario_step_kernel runs AHEAD of a range's first launch of a control step, on that range's own stream (and ahead of a reset's
// launch for the envs under its mask).  Lane = env: it reads the env's episode clock (meta[0]) and episode count (meta[11]) from the
// state record, looks its row up in the table (cosim_scenario.h has the rule, shared with the host twin's test program), writes the
// env's command into cmd_out -- which the step kernel, the ledger and the reporter read instead of the caller's buffer -- and, if a
// push window is due, sets qvel[0:3] of the record the way cosim_event_push does.  No LDS, no atomics, no cross-lane traffic, no host
// read, no join: a captured step carries it, and a step that is abandoned and redone by a fix-up kernel sees the pushed record.
#include "cosim_scenario.h"

namespace cosim {

struct ScnArgs {
  ScnTable tab;
  float* state;            // [N][s_stride] live state records
  const float* cmd_in;     // [N][cd] the caller's commands (null with cd 0)
  float* cmd_out;          // [N][cd]
  int32_t* row_out;        // [N]
  const uint8_t* mask;     // reset: uint8[N] or null
  int n_envs, first, count;
  int s_stride, s_meta, s_qpos, s_qvel;
  int reset;               // 1: ahead of a reset -- t = 0, no push, masked envs only
};

__global__ __launch_bounds__(64) void scenario_step_kernel(ScnArgs a) {
  const int i = (int)blockIdx.x * 64 + (int)threadIdx.x;
  if (i >= a.count) return;   // the last wave's tail
  const int env = a.first + i;
  if (env >= a.n_envs) return;
  if (a.reset && a.mask != nullptr && a.mask[env] == 0) return;
  float* rec = a.state + (size_t)env * a.s_stride;
  const int* meta = reinterpret_cast<const int*>(rec + a.s_meta);
  const int t = a.reset ? 0 : meta[0];
  const int row = scenario_row(a.tab, env, meta[11]);
  const size_t c0 = (size_t)env * a.tab.cd;
  scenario_apply(a.tab, row, t, a.cmd_in + c0, a.cmd_out + c0, rec + a.s_qpos + 3, rec + a.s_qvel, !a.reset);
  a.row_out[env] = row;
}

}  // namespace cosim
