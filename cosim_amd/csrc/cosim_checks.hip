// cosim_checks.hip — scenario checks (cosim_scenario_checks_set / cosim_scenario_checks_get, include/cosim.h): per-scenario pass /
// fail criteria judged on the device.
//
// A check is a timed criterion on a signal of the step (cosim_checks.h has the rule, which a host program compiles too).
// checks_step_kernel runs behind a range's last launch of a control step on that range's own stream, behind the ledger's launch:
// it samples every item of the env's scenario row whose window holds at the step's pre-step clock and, when the row carries a done
// flag, closes the items into one verdict record in the env's ring and begins the next episode with clean accumulators.  One wave
// per env, lane = item: the accumulators are [N][I], so a wave's loads and stores are contiguous; the row, the clock and the flags
// are wave-uniform (scalar loads; the table is read through the constant address space); the two masks of a record come from a
// ballot; lane 0 stores the header and the counters.  No atomics, no LDS, no cross-env traffic, no host read, no join: the verdicts
// are a pure function of the step's outputs, whatever the ranges, the streams and the launch order, and a captured step carries
// the launch.  The kernels only read what the step wrote.
#include "cosim_checks.h"

namespace cosim {

constexpr int CHK_WAVES = 4;   // envs per block

// one value per wave: the env of this wave, or -1 past the range
__device__ __forceinline__ int checks_wave_env(const ChkArgs& a, bool ranged) {
  const int i = __builtin_amdgcn_readfirstlane((int)blockIdx.x * CHK_WAVES + ((int)threadIdx.x >> 6));
  if (ranged && i >= a.count) return -1;   // the last block's tail
  const int env = (ranged ? a.first : 0) + i;
  return env < a.n_envs ? env : -1;
}

__global__ __launch_bounds__(64 * CHK_WAVES) void checks_step_kernel(ChkArgs a) {
  const int lane = (int)threadIdx.x & 63;
  const int env = checks_wave_env(a, true);
  if (env < 0) return;
  int* cnt = a.cnt + (size_t)env * CHK_NCNT;
  ChkCnt c = checks_load(cnt);   // every lane reads the counters ahead of lane 0's store below (one instruction stream per wave)
  c.episode = __builtin_amdgcn_readfirstlane(c.episode); c.length = __builtin_amdgcn_readfirstlane(c.length);
  c.oflags = __builtin_amdgcn_readfirstlane(c.oflags); c.clock = __builtin_amdgcn_readfirstlane(c.clock);
  const int te = __builtin_amdgcn_readfirstlane((int)a.term[env]) != 0, tr = __builtin_amdgcn_readfirstlane((int)a.trunc[env]) != 0;
  const int row = __builtin_amdgcn_readfirstlane(a.scn_row[env]);
  // the clock as the step left it: what the next scenario launch will read
  const int meta0 = __builtin_amdgcn_readfirstlane(reinterpret_cast<const int*>(a.state + (size_t)env * a.s_stride + a.s_meta)[0]);
  int* rec = (te | tr) ? a.rec + ((size_t)env * a.slots + (size_t)((unsigned)c.episode % (unsigned)a.slots)) * checks_words(a.tab.I) : nullptr;
  unsigned long long f = 0ull, n = 0ull;
  checks_step_lane(a, env, lane, 64, c, row, rec, &f, &n);
  const ChkCnt c0 = c;
  const int flags = checks_advance(c, te, tr, meta0);
  if (rec != nullptr) {
    const unsigned long long fm = __ballot(f != 0ull), nm = __ballot(n != 0ull);   // 64 lanes: lane k holds item k's bit alone
    if (lane == 0)
      for (int w = 0; w < CHK_HDR; w++) rec[w] = checks_header_word(w, c0.episode, c0.length + 1, flags, row + 1, fm, nm);
  }
  if (lane == 0) checks_store(cnt, c);
}

// the masked envs begin an episode; what they had open is discarded (an episode the host cut short gets no verdict)
__global__ __launch_bounds__(64 * CHK_WAVES) void checks_begin_kernel(ChkArgs a) {
  const int lane = (int)threadIdx.x & 63;
  const int env = checks_wave_env(a, false);
  if (env < 0) return;
  if (!checks_begin_applies(a, env)) return;
  int* cnt = a.cnt + (size_t)env * CHK_NCNT;
  ChkCnt c = checks_load(cnt);
  const int meta0 = reinterpret_cast<const int*>(a.state + (size_t)env * a.s_stride + a.s_meta)[0];
  checks_begin_lane(a, env, lane, 64, c, meta0);
  if (lane == 0) checks_store(cnt, c);
}

// the open episodes as records (flag 16) into rec [N][8 + 2 I]
__global__ __launch_bounds__(64 * CHK_WAVES) void checks_open_kernel(ChkArgs a) {
  const int lane = (int)threadIdx.x & 63;
  const int env = checks_wave_env(a, false);
  if (env < 0) return;
  const ChkCnt c = checks_load(a.cnt + (size_t)env * CHK_NCNT);
  const int* meta = reinterpret_cast<const int*>(a.state + (size_t)env * a.s_stride + a.s_meta);
  ScnTable T = {};
  T.n_scn = a.tab.n_scn; T.mode = a.scn_mode; T.gid_off = a.scn_off;
  const int row = __builtin_amdgcn_readfirstlane(scenario_row(T, env, meta[11]));
  int* out = a.rec + (size_t)env * checks_words(a.tab.I);
  unsigned long long f = 0ull, n = 0ull;
  checks_open_lane(a, env, lane, 64, row, out, &f, &n);
  const unsigned long long fm = __ballot(f != 0ull), nm = __ballot(n != 0ull);
  if (lane == 0)
    for (int w = 0; w < CHK_HDR; w++) out[w] = checks_header_word(w, c.episode, c.length, CHK_OPEN | c.oflags, row + 1, fm, nm);
}

}  // namespace cosim
