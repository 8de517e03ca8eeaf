// cosim_latency.hip — latency lines of a scenario table (cosim_set_param "latency", include/cosim.h): timed k-step delays of the
// command channel and of observation elements per env, on the device.  cosim_latency.h has the rule.
//
// latency_act_kernel runs behind scenario_step_kernel and scnparams_step_kernel, AHEAD of actfault_step_kernel and of a range's
// first launch of a control step, on that range's own stream.  One wave per env, lane = actuator (nu <= 64): it reads the env's
// pre-step clock (meta[0]), step counter (meta[1]) and episode count (meta[11]), looks its row up, loads the caller's action row
// (coalesced), writes it to the env's line, walks the row's 16-byte item records once and stores the env's rows of two engine-owned
// buffers: `raw`, the caller's bits (what last_action is rebuilt from), and `eff`, the delivered action.  EVERY env of the range is
// written: one whose row lists no action item gets a plain copy and touches neither its line nor its header.
//
// latency_obs_kernel runs BEHIND the last launch of the step that writes the state record or state_out and behind
// actfault_obs_kernel, AHEAD of obsfault_step_kernel, and behind a reset's launch for the envs under its mask.  One wave per env,
// lane = frame element in passes of 64: the newest frame as the step left it goes to the env's line, and an element under an item
// that holds is rewritten -- row 0 of the record's observation stack and the newest frame of state_out (a non-stacked element: its
// one word behind the stack rows) -- with the line's word of k clocks ago.  An env whose row lists no observation item leaves after
// its meta words and the two row addresses.
//
// One wave per env, as the fault kernels (cosim_actfault.hip has the reasons): the row, the clock, the item records, the jitter draw
// and the slots are the same for the whole wave, so the records come through scalar loads and a line row is one coalesced access.
// latency_cut_kernel invalidates the headers of the envs a host cut touched.
// No LDS, no atomics, no cross-env traffic, no host read, no join: a captured step carries all of it.
#include "cosim_dev.h"
#include "cosim_latency.h"

namespace cosim {

struct LatActArgs {
  ScnTable tab;            // the scenario table (row rule)
  LatTable lat;
  const float* state;      // [N][s_stride] live state records
  const float* actions;    // [N][nu] the caller's actions
  float* eff;              // [N][nu] delivered actions
  float* raw;              // [N][nu] the caller's actions, kept for actfault_obs_kernel
  float* line;             // [N][D][nu]
  int* from;               // [N]
  int n_envs, first, count;
  int s_stride, s_meta, nu;
  unsigned seed_lo, seed_hi;
  long long env_id0;
};

struct LatObsArgs {
  ScnTable tab;
  LatTable lat;
  float* state;            // [N][s_stride] live state records
  float* state_out;        // [N][state_dim] the step's / reset's observation rows
  const uint8_t* mask;     // reset: uint8[N] or null
  float* line;             // [N][D][frame_dim]
  int* from;               // [N]
  int n_envs, first, count;
  int s_stride, s_meta, s_stack;
  int sd, S, frame_dim, state_dim;
  unsigned seed_lo, seed_hi;
  long long env_id0;
};

struct LatCutArgs {
  int* from_act;           // [N] or null
  int* from_obs;           // [N] or null
  const uint8_t* mask;     // uint8[N] or null: all
  const int* src;          // a restore's source index [N] or null: rows outside [0, n_rows) were refused
  int n_rows, n_envs;
};

constexpr int LAT_PASSES = MAXFRAME / 64;    // every frame fits
static_assert(LAT_PASSES * 64 == MAXFRAME, "passes of 64 lanes");

__global__ __launch_bounds__(64 * FLT_WAVES) void latency_act_kernel(LatActArgs a) {
  const int lane = (int)threadIdx.x & 63;
  const int i = __builtin_amdgcn_readfirstlane((int)blockIdx.x * FLT_WAVES + ((int)threadIdx.x >> 6));   // one value per wave
  if (i >= a.count) return;   // the last block's tail
  const int env = a.first + i;
  if (env >= a.n_envs) return;
  if (lane >= a.nu) return;
  const float* rec = a.state + (size_t)env * a.s_stride;
  int t, row;
  const FaultKey K = fault_wave_key(a.tab, reinterpret_cast<const int*>(rec + a.s_meta), env, a.seed_lo, a.seed_hi, a.env_id0, &t, &row);
  const size_t w = (size_t)env * a.nu + lane;
  const float x = a.actions[w];
  a.raw[w] = x;
  const int D = a.lat.depth;
  int k[1];
  float y = x;
  if (latency_walk<1>(a.lat.act_adr, a.lat.act_item, row, t, D, K, lane, 64, k)) {
    const int from = __builtin_amdgcn_readfirstlane(a.from[env]);
    const int f = latency_from(from, t);
    if (f != from && lane == 0) a.from[env] = f;
    y = latency_act_word(a.line + (size_t)env * D * a.nu, D, a.nu, lane, t, f, k[0], x);
  }
  a.eff[w] = y;
}

__global__ __launch_bounds__(64 * FLT_WAVES) void latency_obs_kernel(LatObsArgs a) {
  const int lane = (int)threadIdx.x & 63;
  const int i = __builtin_amdgcn_readfirstlane((int)blockIdx.x * FLT_WAVES + ((int)threadIdx.x >> 6));   // one value per wave
  if (i >= a.count) return;   // the last block's tail
  const int env = a.first + i;
  if (env >= a.n_envs) return;
  if (a.mask != nullptr && a.mask[env] == 0) return;
  float* rec = a.state + (size_t)env * a.s_stride;
  int t, row;
  const FaultKey K = fault_wave_key(a.tab, reinterpret_cast<const int*>(rec + a.s_meta), env, a.seed_lo, a.seed_hi, a.env_id0, &t, &row);
  const int D = a.lat.depth, fd = a.frame_dim, sd = a.sd;
  int k[LAT_PASSES];
  if (!latency_walk<LAT_PASSES>(a.lat.obs_adr, a.lat.obs_item, row, t, D, K, lane, 64, k)) return;
  const int from = __builtin_amdgcn_readfirstlane(a.from[env]);
  const int f = latency_from(from, t);
  if (f != from && lane == 0) a.from[env] = f;
  float* stack = rec + a.s_stack;
  float* out = a.state_out + (size_t)env * a.state_dim;
  float* line = a.line + (size_t)env * D * fd;
#pragma unroll
  for (int p = 0; p < LAT_PASSES; p++) {
    const int e = lane + 64 * p;
    if (e >= fd) break;
    float* word = e < sd ? stack + e : out + (a.S * sd + (e - sd));
    const float v = latency_obs_word(line, D, fd, e, t, f, k[p], *word);
    if (k[p] == 0) continue;
    *word = v;
    if (e < sd) out[e] = v;
  }
}

__global__ __launch_bounds__(64) void latency_cut_kernel(LatCutArgs a) {
  const int env = (int)blockIdx.x * 64 + (int)threadIdx.x;
  if (env >= a.n_envs) return;
  if (a.mask != nullptr && a.mask[env] == 0) return;
  if (a.src != nullptr && (a.src[env] < 0 || a.src[env] >= a.n_rows)) return;
  if (a.from_act != nullptr) a.from_act[env] = -1;
  if (a.from_obs != nullptr) a.from_obs[env] = -1;
}

}  // namespace cosim
