// cosim_curves.hip — response curves (cosim_scenario_curves_set / cosim_scenario_curves_get, include/cosim.h): per-scenario ensemble
// time series of a signal over the episode clock, split by outcome, kept on the device.
//
// cosim_curves.h has the rule, which a host program compiles too.  curves_step_kernel runs behind a range's last launch of a control
// step on that range's own stream, behind the checks' launch.  One wave per env, four per block; env, row, clock and flags are
// wave-uniform (readfirstlane; the items are read through the constant address space).  Sampling phase: lane = item, one plain
// store into the env's stage.  Fold phase, only on a row with a done flag: for each item the lanes stride over the time bins, so the
// stage read is coalesced and each atomic wave-instruction covers 256 contiguous bytes of a cell array (the bin is the innermost
// index of every array); the same lanes write "no sample" back.  Every cell update is an integer atomic whose result is discarded:
// the cells are a function of the set of ended episodes, whatever the ranges, the streams and the arrival order.  No LDS, no host
// read, no join; a captured step carries the launch.  The kernels only read what the step wrote.
// With groups set (cosim_scenario_curves_groups) the host launches the siblings curves_step_grouped_kernel / curves_clear_grouped_kernel
// instead: the cells are G planes and the fold goes into the plane the env's group word names; curves_step_kernel's own code is
// what it was.
#include "cosim_curves.h"

namespace cosim {

constexpr int CUR_WAVES = 4;   // envs per block

// the cell updates as device-wide atomics that discard their result (the no-return forms)
struct CurAtomics {
  __device__ __forceinline__ void add(unsigned* p, unsigned v) { (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
  __device__ __forceinline__ void add64(unsigned long long* p, unsigned long long v) {
    (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __device__ __forceinline__ void min(unsigned* p, unsigned v) { (void)__hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
  __device__ __forceinline__ void max(unsigned* p, unsigned v) { (void)__hip_atomic_fetch_max(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
};

// one value per wave: the env of this wave, or -1 past the range
__device__ __forceinline__ int curves_wave_env(const CurArgs& a, bool ranged) {
  const int i = __builtin_amdgcn_readfirstlane((int)blockIdx.x * CUR_WAVES + ((int)threadIdx.x >> 6));
  if (ranged && i >= a.count) return -1;   // the last block's tail
  const int env = (ranged ? a.first : 0) + i;
  return env < a.n_envs ? env : -1;
}

__global__ __launch_bounds__(64 * CUR_WAVES) void curves_step_kernel(CurArgs a) {
  const int lane = (int)threadIdx.x & 63;
  const int env = curves_wave_env(a, true);
  if (env < 0) return;
  const int t = __builtin_amdgcn_readfirstlane(a.clk[env]);   // every lane reads the clock ahead of lane 0's store below
  const int te = __builtin_amdgcn_readfirstlane((int)a.term[env]) != 0, tr = __builtin_amdgcn_readfirstlane((int)a.trunc[env]) != 0;
  const int row = __builtin_amdgcn_readfirstlane(a.scn_row[env]);
  // the clock as the step left it: what the next scenario launch will read
  const int meta0 = __builtin_amdgcn_readfirstlane(reinterpret_cast<const int*>(a.state + (size_t)env * a.s_stride + a.s_meta)[0]);
  curves_sample_lane(a, env, lane, 64, t, row, (te | tr) != 0);
  if (te | tr) {
    __threadfence_block();   // this step's samples were stored by other lanes of the wave
    CurAtomics at;
    curves_fold_lane(a, env, lane, 64, row, te, at);
  }
  if (lane == 0) a.clk[env] = meta0;
}

// curves_step_kernel with groups set (cosim_scenario_curves_groups): the same sampling and clock; the fold reads the env's group word
// once, wave-uniform, and folds into that plane of the cells (curves_fold_group_lane).  The word is read on a row with a done flag
// only, behind the step that ended the episode on this range's stream.
__global__ __launch_bounds__(64 * CUR_WAVES) void curves_step_grouped_kernel(CurArgs a) {
  const int lane = (int)threadIdx.x & 63;
  const int env = curves_wave_env(a, true);
  if (env < 0) return;
  const int t = __builtin_amdgcn_readfirstlane(a.clk[env]);   // every lane reads the clock ahead of lane 0's store below
  const int te = __builtin_amdgcn_readfirstlane((int)a.term[env]) != 0, tr = __builtin_amdgcn_readfirstlane((int)a.trunc[env]) != 0;
  const int row = __builtin_amdgcn_readfirstlane(a.scn_row[env]);
  const int meta0 = __builtin_amdgcn_readfirstlane(reinterpret_cast<const int*>(a.state + (size_t)env * a.s_stride + a.s_meta)[0]);
  curves_sample_lane(a, env, lane, 64, t, row, (te | tr) != 0);
  if (te | tr) {
    const int g = __builtin_amdgcn_readfirstlane(a.group[env]);
    __threadfence_block();   // this step's samples were stored by other lanes of the wave
    CurAtomics at;
    curves_fold_group_lane(a, env, lane, 64, row, te, g, at);
  }
  if (lane == 0) a.clk[env] = meta0;
}

// the masked envs begin an episode; what they had staged is discarded (an episode the host cut short is in no cell)
__global__ __launch_bounds__(64 * CUR_WAVES) void curves_begin_kernel(CurArgs a) {
  const int lane = (int)threadIdx.x & 63;
  const int env = curves_wave_env(a, false);
  if (env < 0) return;
  if (!curves_begin_applies(a, env)) return;
  const int meta0 = reinterpret_cast<const int*>(a.state + (size_t)env * a.s_stride + a.s_meta)[0];
  curves_begin_lane(a, env, lane, 64);
  if (lane == 0) a.clk[env] = meta0;
}

// the cells of (item, class) = block back to empty: zeros, the min keys all ones
__global__ __launch_bounds__(256) void curves_clear_kernel(CurArgs a) {
  SCN_TAB(int32_t) nt = SCN_TAB_CAST(int32_t, a.tab.nt);
  SCN_TAB(int32_t) coff = SCN_TAB_CAST(int32_t, a.tab.coff);
  SCN_TAB(int32_t) cw = SCN_TAB_CAST(int32_t, a.tab.cw);
  const int i = (int)blockIdx.x >> 1, cls = (int)blockIdx.x & 1;
  if (i >= a.tab.n_items) return;
  const int n = nt[i], words = cw[i];
  unsigned* cell = a.cells + (size_t)coff[i] + (size_t)cls * (size_t)words;
  for (int w = (int)threadIdx.x; w < words; w += (int)blockDim.x) cell[w] = curves_clear_word(w, n);
}

// with groups: block = (plane, item, class), every plane back to empty, and the `ungrouped` word to zero
__global__ __launch_bounds__(256) void curves_clear_grouped_kernel(CurArgs a) {
  SCN_TAB(int32_t) nt = SCN_TAB_CAST(int32_t, a.tab.nt);
  SCN_TAB(int32_t) coff = SCN_TAB_CAST(int32_t, a.tab.coff);
  SCN_TAB(int32_t) cw = SCN_TAB_CAST(int32_t, a.tab.cw);
  const int per = 2 * a.tab.n_items;
  const int g = (int)blockIdx.x / per, r = (int)blockIdx.x - g * per;
  if (blockIdx.x == 0 && threadIdx.x == 0) *a.ungrouped = 0u;
  if (g >= a.n_groups) return;
  const int i = r >> 1, cls = r & 1;
  const int n = nt[i], words = cw[i];
  unsigned* cell = a.cells + (size_t)g * a.plane_words + (size_t)coff[i] + (size_t)cls * (size_t)words;
  for (int w = (int)threadIdx.x; w < words; w += (int)blockDim.x) cell[w] = curves_clear_word(w, n);
}

}  // namespace cosim
