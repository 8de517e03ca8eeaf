// cosim_ftrace.hip — failure traces (cosim_ftrace_set / cosim_ftrace_get, include/cosim.h): every env's last control steps before an
// episode ends, kept on the device.
//
// The step kernels hand back one control step's flags and info row and leave the state record one step further; the next step
// overwrites all of it.  ftrace_step_kernel runs behind a range's last launch of a control step on that range's own stream, behind
// the ledger's launch, and copies the step into the env's window as one (s, a, outcome) frame; the rules are in cosim_ftrace.h,
// which a host program compiles too.  One wave per env: the 64 lanes stride over the words of a frame (70 for flamingo_light_v1,
// more than one pass for humanoid_p_v0), the loads from the state record are the coalesced rec[l] of the step kernels, the frame
// store is contiguous, and the env's counters are wave-uniform loads.  No atomics and no cross-env traffic: the traces are a pure
// function of the step's inputs and outputs, whatever the ranges and the launch order.
#include "cosim_ftrace.h"
#include "cosim_scenario.h"
namespace cosim {

__global__ __launch_bounds__(64) void ftrace_step_kernel(FtArgs a) {
  const int i = (int)blockIdx.x;
  if (i >= a.count) return;
  const int env = a.first + i;
  if (env >= a.n_envs) return;
  int* cnt = a.cnt + (size_t)env * FT_NCNT;
  FtCnt c = ftrace_load(cnt);   // every lane reads the counters ahead of lane 0's store below (one instruction stream per wave)
  ftrace_step_lane(a, env, (int)threadIdx.x, 64, c);
  if (threadIdx.x == 0) ftrace_store(cnt, c);
}

// the masked envs begin an episode; what they had open is discarded (an episode the host cut short is not a failure)
__global__ __launch_bounds__(64) void ftrace_begin_kernel(FtArgs a) {
  const int env = (int)blockIdx.x;
  if (env >= a.n_envs) return;
  if (!ftrace_begin_applies(a, env)) return;
  int* cnt = a.cnt + (size_t)env * FT_NCNT;
  FtCnt c = ftrace_load(cnt);
  ftrace_begin_lane(a, env, (int)threadIdx.x, 64, c);
  if (threadIdx.x == 0) ftrace_store(cnt, c);
}

// the open windows' headers (flag 16) into open_out [N][16]; lane = env
__global__ __launch_bounds__(64) void ftrace_open_kernel(FtArgs a) {
  const int env = (int)blockIdx.x * 64 + (int)threadIdx.x;
  if (env >= a.n_envs) return;
  const FtCnt c = ftrace_load(a.cnt + (size_t)env * FT_NCNT);
  int scn = 0;
  if (a.scn_rows > 0) {
    const int* meta = reinterpret_cast<const int*>(a.state + (size_t)env * a.s_stride + a.s_meta);
    ScnTable T = {};
    T.n_scn = a.scn_rows; T.mode = a.scn_mode; T.gid_off = a.scn_off;
    scn = scenario_row(T, env, meta[11]) + 1;
  }
  int* out = a.open_out + (size_t)env * FT_HDR;
  for (int w = 0; w < FT_HDR; w++) out[w] = ftrace_open_word(a, env, w, c, scn);
}

}  // namespace cosim
