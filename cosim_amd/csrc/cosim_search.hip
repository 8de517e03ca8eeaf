// cosim_search.hip — limit search (cosim_set_param "search", include/cosim.h): a per-env staircase on the push and command scale of
// a scenario, kept on the device.
//
// Every env whose scenario row has a search item keeps one float32 word, its level (cosim_search.h has the rule, which a host program
// compiles too).  While a search is armed scenario_search_step_kernel runs INSTEAD OF scenario_step_kernel (cosim_scenario.hip, which
// this file is included behind): the same lane = env shape at the same sites, with the level multiplied into the row's pushes and / or
// keyframes.  search_step_kernel runs behind a range's last launch of a control step on that range's own stream, behind the curves'
// launch: it counts the open episode's length and, when the row carries a done flag, builds the ledger's flags, moves the level by
// the item's rule and writes one trial record into the env's ring.  Lane = env, 64-lane blocks, no LDS, no cross-lane traffic, no
// host read, no join: a captured step carries the launches.  The kernels write only the search's own buffers (the scenario kernel:
// what scenario_step_kernel writes); the one atomic is the decrement of the engine's "remaining" word when an env spends its budget.
// search_step_checks_kernel is search_step_kernel for a search with an item that fails on a check: it also reads the verdict record
// checks_step_kernel closed behind the same step.  The level's third reader, actfault_search_step_kernel, is in cosim_actfault.hip.
#include "cosim_search.h"

namespace cosim {

struct ScnSearchArgs {
  ScnArgs scn;
  SrchTable srch;
  const int* rec;          // [N][SRCH_NCNT]: word 0 is the level this step runs at
};

__global__ __launch_bounds__(64) void scenario_search_step_kernel(ScnSearchArgs s) {
  const ScnArgs& a = s.scn;
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
  const int targets = search_targets(s.srch, row);
  const float level = targets ? __int_as_float(s.rec[(size_t)env * SRCH_NCNT + SRCH_LEVEL]) : 1.f;
  scenario_apply_scaled(a.tab, row, t, a.cmd_in + c0, a.cmd_out + c0, rec + a.s_qpos + 3, rec + a.s_qvel, !a.reset, targets, level);
  a.row_out[env] = row;
}

__global__ __launch_bounds__(64) void search_step_kernel(SrchArgs a) {
  const int i = (int)blockIdx.x * 64 + (int)threadIdx.x;
  if (i >= a.count) return;   // the last wave's tail
  const int env = a.first + i;
  if (env >= a.n_envs) return;
  const int te = a.term[env] != 0, tr = a.trunc[env] != 0;
  const int* meta = reinterpret_cast<const int*>(a.state + (size_t)env * a.s_stride + a.s_meta);
  // the usual step moves one word of the record (length); the table is read only on a step that ends the episode
  const SrchItem it = (te | tr) ? search_item(a.tab, a.scn_row[env]) : SrchItem();
  const int became_done = search_step_lane(a.rec + (size_t)env * SRCH_NCNT, a.ring + (size_t)env * a.slots * SRCH_TRIAL_WORDS, a.slots, it, te, tr, meta, a.fall);
  if (became_done) atomicSub(a.remaining, 1);
}

// where the verdict records of the scenario checks lie (cosim_checks.h): counters [N][ncnt] (word 0: episodes ended), rings
// [N][slots][words]
struct SrchVerdicts {
  const int* cnt;
  const int* rec;
  int ncnt, slots, words;
};

// search_step_kernel of a search with an item that selects a check.  checks_step_kernel ran behind this same step ahead of this
// launch on the same stream: on a step with a done flag it closed the ended episode's record and moved its own ordinal on, so the
// record is the one of ordinal cnt[0] - 1 (the checks' own count: the two ordinals need not agree).
struct SrchChkArgs {
  SrchArgs srch;
  SrchVerdicts v;
};

__global__ __launch_bounds__(64) void search_step_checks_kernel(SrchChkArgs s) {
  const SrchArgs& a = s.srch;
  const SrchVerdicts& v = s.v;
  const int i = (int)blockIdx.x * 64 + (int)threadIdx.x;
  if (i >= a.count) return;   // the last wave's tail
  const int env = a.first + i;
  if (env >= a.n_envs) return;
  const int te = a.term[env] != 0, tr = a.trunc[env] != 0;
  const int* meta = reinterpret_cast<const int*>(a.state + (size_t)env * a.s_stride + a.s_meta);
  const SrchItem it = (te | tr) ? search_item(a.tab, a.scn_row[env]) : SrchItem();
  const int* verdict = nullptr;
  if ((te | tr) && it.has && (it.chk_lo | it.chk_hi) != 0) {
    const unsigned closed = (unsigned)v.cnt[(size_t)env * v.ncnt] - 1u;
    verdict = v.rec + ((size_t)env * v.slots + (size_t)(closed % (unsigned)v.slots)) * v.words;
  }
  const int became_done = search_step_lane(a.rec + (size_t)env * SRCH_NCNT, a.ring + (size_t)env * a.slots * SRCH_TRIAL_WORDS, a.slots, it, te, tr, meta, a.fall, verdict);
  if (became_done) atomicSub(a.remaining, 1);
}

// the masked envs begin an episode; what they had open is discarded (an episode the host cut short is no trial), the level stays
__global__ __launch_bounds__(64) void search_begin_kernel(SrchArgs a) {
  const int env = (int)blockIdx.x * 64 + (int)threadIdx.x;
  if (env >= a.n_envs) return;
  if (!search_begin_applies(a, env)) return;
  const int* meta = reinterpret_cast<const int*>(a.state + (size_t)env * a.s_stride + a.s_meta);
  search_begin_lane(a.rec + (size_t)env * SRCH_NCNT, a.flag, meta[4]);
}

// a table is armed: every env's record from its row's item, its ring emptied, `remaining` at the envs that have an item
__global__ __launch_bounds__(64) void search_init_kernel(SrchArgs a) {
  const int env = (int)blockIdx.x * 64 + (int)threadIdx.x;
  if (env == 0) *a.remaining = a.n_armed;
  if (env >= a.n_envs) return;
  ScnTable T = {};
  T.n_scn = a.tab.n_scn; T.mode = SCN_MODE_ENV; T.gid_off = a.scn_off;
  const int* meta = reinterpret_cast<const int*>(a.state + (size_t)env * a.s_stride + a.s_meta);
  int rec[SRCH_NCNT];
  search_init(rec, search_item(a.tab, scenario_row(T, env, 0)), meta[4], a.flag);
  int4* rp = reinterpret_cast<int4*>(a.rec + (size_t)env * SRCH_NCNT);
#pragma unroll
  for (int q = 0; q < 4; q++) rp[q] = make_int4(rec[4 * q], rec[4 * q + 1], rec[4 * q + 2], rec[4 * q + 3]);
  int4* ring = reinterpret_cast<int4*>(a.ring + (size_t)env * a.slots * SRCH_TRIAL_WORDS);
  for (int k = 0; k < a.slots; k++) ring[k] = make_int4(0, 0, 0, 0);
}

}  // namespace cosim
