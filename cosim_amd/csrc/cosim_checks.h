// cosim_checks.h — the per-item rule of a scenario table's checks (cosim_scenario_checks_set / cosim_scenario_checks_get,
// include/cosim.h), as inline functions that the device kernels (cosim_checks.hip) and a plain host C++ program
// (tests/checks_lanes.cpp) both compile.
//
// Scenario s owns the items [adr[s], adr[s + 1]) (at most 64).  Item i = (t0, t1, signal, index, mode, cmp, bound) takes one sample
// per control step whose PRE-STEP episode clock t holds t0 <= t < t1 -- the clock the scenario kernel keyed this step's keyframes and
// pushes on.  The clock is not recomputed: a per-env clock word is set to meta word 0 by the begin rule and again behind every step,
// which is what the next scenario launch reads; a step's t is the word the previous invocation stored.
//   signal v (float32)  0 info[index]  1 |info[index]|  2 |cmd[index] - info[1 + index]| (fp32 subtraction first)
//                       3 max_j |info[4 + j]| (fmaxf from 0.f, j ascending)  4 up = 1 - 2 (qx^2 + qy^2), contraction off
//                       5 qpos[index]  6 qvel[index]  7 |qvel[index]|
//     4 .. 7 read the live state record behind the step (the pose the step ended in) and take NO sample on a row with a done flag:
//     the auto-reset has already replaced the pose.  0 .. 3 are sampled on done rows (the info row is written before the reset).
//   cmp    0: ok = v < bound   1: ok = v > bound   (NaN is not ok)
//   mode   0 always  every sample must be ok.        aux = t of the FIRST sample not ok (-1: none); fails iff aux >= 0
//          1 settle  ok from some step on to t1 - 1. aux = t of the LAST sample not ok (-1: none);  fails iff complete and aux == t1 - 1
//          2 mean    sum += (double)v; at close m = (float)(sum / (double)n); fails iff n > 0 and !cmp(m, bound); value m, aux n
//     always / settle: the value word is the sample furthest on the failing side (the largest for <, the smallest for >; a NaN
//     sample never replaces it, ties keep the earlier sample).  A value with no sample behind it, and a NaN mean, is the word CHK_NONE.
//   incomplete iff n < t1 - t0 when the record is written.  passed = complete and not failed (derived on the host).
// Per (env, item) accumulator: ext float, aux int, n int, sum double, as arrays [N][I] (I: the largest item count of any scenario,
// rounded up to even), so a wave's loads and stores are contiguous.  Per env CHK_NCNT counters: 0 episodes ended (the ordinal of the
// open one), 1 length, 2 open flags (bit 8), 3 clock.
// Record, 8 + 2 I int32 words: 0 episode ordinal  1 length  2 flags (1 terminated | 2 truncated | 8 did not begin at a reset | 16
// open)  3 scenario row + 1  4..5 fail mask (low, high)  6..7 incomplete mask  then per item: value bits, aux (0, 0 past the row's
// items).  Episode o of an env lies in slot o mod slots of its ring.
//
// The bodies are written per lane: lane `lane` of `nl` handles the items lane, lane + nl, ... and returns the mask bits of its own
// items; the caller combines the lanes' bits (the kernel: one item per lane, a ballot) and stores the header and the counters once.
#pragma once
#include <stddef.h>
#include <string.h>

#include "cosim_scenario.h"

namespace cosim {

enum { CHK_INFO = 0, CHK_ABS_INFO = 1, CHK_TRACKING_ERROR = 2, CHK_TORQUE_MAX = 3, CHK_UP = 4, CHK_QPOS = 5, CHK_QVEL = 6, CHK_ABS_QVEL = 7,
       CHK_NSIGNAL = 8 };
enum { CHK_ALWAYS = 0, CHK_SETTLE = 1, CHK_MEAN = 2, CHK_NMODE = 3 };
enum { CHK_LT = 0, CHK_GT = 1 };
// the ledger's flag values (cosim_ledger.hip)
enum { CHK_TERMINATED = 1, CHK_TRUNCATED = 2, CHK_NO_RESET = 8, CHK_OPEN = 16 };
constexpr int CHK_MAX_ITEMS = 64, CHK_MAX_SLOTS = 64, CHK_HDR = 8, CHK_NCNT = 4;
constexpr int CHK_NONE = 0x7fc00000;   // value word with no sample behind it

struct ChkTable {
  const int32_t* adr;      // [S + 1]
  const int32_t* t;        // [n][2]
  const int32_t* signal;   // [n]
  const int32_t* index;    // [n]
  const int32_t* mode;     // [n]
  const int32_t* cmp;      // [n]
  const float* bound;      // [n]
  int n_scn, n_items, I;   // I: items per env the accumulators and a record hold
};

struct ChkArgs {
  ChkTable tab;
  const float* info;       // [N][info_dim] the caller's info rows of this step
  const uint8_t* term;     // [N]
  const uint8_t* trunc;    // [N]
  const float* cmd;        // [N][cmd_stride] the applied command (scenario_cmd), or null with command_dim 0
  const float* state;      // [N][s_stride] live state records
  const int32_t* scn_row;  // [N] rows the scenario kernel wrote ahead of this step
  float* ext;              // [N][I]
  int* aux;                // [N][I]
  int* n;                  // [N][I]
  double* sum;             // [N][I]
  int* cnt;                // [N][CHK_NCNT]
  int* rec;                // step: the rings [N][slots][8 + 2 I]; open: [N][8 + 2 I] output rows
  const uint8_t* mask;     // begin: uint8[N] or null
  const int* src;          // begin: the restore's source index or null; envs it refused (outside [0, n_rows)) are left alone
  int n_rows;
  int n_envs, first, count;
  int info_dim, nu, cmd_stride;
  int s_stride, s_qpos, s_qvel, s_meta, slots;
  int flag;                // begin: open flags of the new episode
  int scn_mode;            // open: the table's rule at the live meta words
  unsigned scn_off;
};

struct ChkCnt { int episode, length, oflags, clock; };
struct ChkAcc { float ext; int aux, n; double sum; };

SCN_HD int checks_words(int I) { return CHK_HDR + 2 * I; }
SCN_HD int checks_bits(float f) { int u; memcpy(&u, &f, 4); return u; }
SCN_HD float checks_float(int u) { float f; memcpy(&f, &u, 4); return f; }
SCN_HD bool checks_state_signal(int signal) { return signal >= CHK_UP; }
SCN_HD bool checks_cmp(int cmp, float v, float bound) { return cmp == CHK_LT ? v < bound : v > bound; }

SCN_HD ChkCnt checks_load(const int* c) { ChkCnt k; k.episode = c[0]; k.length = c[1]; k.oflags = c[2]; k.clock = c[3]; return k; }
SCN_HD void checks_store(int* c, const ChkCnt& k) { c[0] = k.episode; c[1] = k.length; c[2] = k.oflags; c[3] = k.clock; }
SCN_HD ChkAcc checks_clean() { ChkAcc x; x.ext = checks_float(CHK_NONE); x.aux = -1; x.n = 0; x.sum = 0.0; return x; }
SCN_HD ChkAcc checks_acc_load(const ChkArgs& a, size_t k) { ChkAcc x; x.ext = a.ext[k]; x.aux = a.aux[k]; x.n = a.n[k]; x.sum = a.sum[k]; return x; }
SCN_HD void checks_acc_store(const ChkArgs& a, size_t k, const ChkAcc& x) { a.ext[k] = x.ext; a.aux[k] = x.aux; a.n[k] = x.n; a.sum[k] = x.sum; }

// the items [i0, i0 + ni) of a row; a row outside the table is clamped into it
SCN_HD void checks_row_items(const ChkTable& T, int row, int* i0, int* ni) {
  SCN_TAB(int32_t) adr = SCN_TAB_CAST(int32_t, T.adr);
  row = row < 0 ? 0 : (row >= T.n_scn ? T.n_scn - 1 : row);
  *i0 = adr[row];
  const int n = adr[row + 1] - adr[row];
  *ni = n < 0 ? 0 : (n > T.I ? T.I : n);
}

// The signal of env `env` behind its step.
SCN_HD float checks_signal(const ChkArgs& a, int env, int signal, int index) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float* info = a.info + (size_t)env * a.info_dim;
  const float* rec = a.state + (size_t)env * a.s_stride;
  switch (signal) {
    case CHK_INFO: return info[index];
    case CHK_ABS_INFO: return fabsf(info[index]);
    case CHK_TRACKING_ERROR: return fabsf(a.cmd[(size_t)env * a.cmd_stride + index] - info[1 + index]);
    case CHK_TORQUE_MAX: {
      float m = 0.f;
      for (int j = 0; j < a.nu; j++) m = fmaxf(m, fabsf(info[4 + j]));   // fmaxf ignores NaN
      return m;
    }
    case CHK_UP: {
      const float qx = rec[a.s_qpos + 4], qy = rec[a.s_qpos + 5];
      const float xx = qx * qx, yy = qy * qy;
      const float s = xx + yy;
      const float d = 2.f * s;
      return 1.f - d;
    }
    case CHK_QPOS: return rec[a.s_qpos + index];
    case CHK_QVEL: return rec[a.s_qvel + index];
    default: return fabsf(rec[a.s_qvel + index]);
  }
}

// one sample v at clock t into an item's accumulator
SCN_HD void checks_sample(ChkAcc& x, int mode, int cmp, float bound, float v, int t) {
  x.n++;
  if (mode == CHK_MEAN) { x.sum += (double)v; return; }
  if (v == v) {
    const bool unset = !(x.ext == x.ext);
    if (unset || (cmp == CHK_LT ? v > x.ext : v < x.ext)) x.ext = v;
  }
  if (!checks_cmp(cmp, v, bound)) {
    if (mode == CHK_SETTLE || x.aux < 0) x.aux = t;
  }
}

// an item's two record words and its verdict from its accumulator
SCN_HD void checks_verdict(const ChkAcc& x, int t0, int t1, int mode, int cmp, float bound, int* value, int* aux, bool* failed, bool* incomplete) {
  *incomplete = x.n < t1 - t0;
  if (mode == CHK_MEAN) {
    const float m = x.n > 0 ? (float)(x.sum / (double)x.n) : checks_float(CHK_NONE);
    *value = m == m ? checks_bits(m) : CHK_NONE;
    *aux = x.n;
    *failed = x.n > 0 && !checks_cmp(cmp, m, bound);
    return;
  }
  *value = x.ext == x.ext ? checks_bits(x.ext) : CHK_NONE;
  *aux = x.aux;
  *failed = mode == CHK_ALWAYS ? x.aux >= 0 : (!*incomplete && x.aux == t1 - 1);
}

// One env behind one control step, lane `lane` of `nl`.  `c`: the env's counters as loaded before any lane ran (c.clock is this
// step's t); `row`: the row the scenario kernel wrote ahead of the step; `rec`: the record's slot if the row carries a done flag,
// else null.  Adds the bits of this lane's items to *fail / *inc.
SCN_HD void checks_step_lane(const ChkArgs& a, int env, int lane, int nl, const ChkCnt& c, int row, int* rec, unsigned long long* fail,
                             unsigned long long* inc) {
  const ChkTable& T = a.tab;
  SCN_TAB(int32_t) tt = SCN_TAB_CAST(int32_t, T.t);
  SCN_TAB(int32_t) sig = SCN_TAB_CAST(int32_t, T.signal);
  SCN_TAB(int32_t) idx = SCN_TAB_CAST(int32_t, T.index);
  SCN_TAB(int32_t) mode = SCN_TAB_CAST(int32_t, T.mode);
  SCN_TAB(int32_t) cmp = SCN_TAB_CAST(int32_t, T.cmp);
  SCN_TAB(float) bound = SCN_TAB_CAST(float, T.bound);
  int i0, ni;
  checks_row_items(T, row, &i0, &ni);
  const bool done = rec != nullptr;
  const int t = c.clock;
  for (int k = lane; k < T.I; k += nl) {
    const size_t ak = (size_t)env * T.I + k;
    int value = 0, aux = 0;
    if (k < ni) {
      const int i = i0 + k;
      const int t0 = tt[2 * i], t1 = tt[2 * i + 1], sg = sig[i], md = mode[i], cp = cmp[i];
      const float bd = bound[i];
      ChkAcc x = checks_acc_load(a, ak);
      if (t0 <= t && t < t1 && !(done && checks_state_signal(sg))) checks_sample(x, md, cp, bd, checks_signal(a, env, sg, idx[i]), t);
      if (!done) { checks_acc_store(a, ak, x); continue; }
      bool f, n;
      checks_verdict(x, t0, t1, md, cp, bd, &value, &aux, &f, &n);
      if (f) *fail |= 1ull << k;
      if (n) *inc |= 1ull << k;
    }
    if (done) {   // the record's item words, then the next episode starts clean
      rec[CHK_HDR + 2 * k] = value;
      rec[CHK_HDR + 2 * k + 1] = aux;
      checks_acc_store(a, ak, checks_clean());
    }
  }
}

// header word w of a record
SCN_HD int checks_header_word(int w, int episode, int length, int flags, int scn, unsigned long long fail, unsigned long long inc) {
  switch (w) {
    case 0: return episode;
    case 1: return length;
    case 2: return flags;
    case 3: return scn;
    case 4: return (int)(unsigned)(fail & 0xffffffffull);
    case 5: return (int)(unsigned)(fail >> 32);
    case 6: return (int)(unsigned)(inc & 0xffffffffull);
    default: return (int)(unsigned)(inc >> 32);
  }
}

// The counters behind a step, once per env after all lanes have run.  Returns the closed record's flags (0: the episode goes on).
SCN_HD int checks_advance(ChkCnt& c, int te, int tr, int meta0) {
  c.length++;
  int flags = 0;
  if (te | tr) {
    flags = (te ? CHK_TERMINATED : 0) | (tr ? CHK_TRUNCATED : 0) | c.oflags;
    c.episode++; c.length = 0; c.oflags = 0;
  }
  c.clock = meta0;   // what the next scenario launch reads
  return flags;
}

// whether the begin rule applies to env (mask and restore source, as ledger_begin_kernel reads them)
SCN_HD bool checks_begin_applies(const ChkArgs& a, int env) {
  if (a.mask != nullptr && a.mask[env] == 0) return false;
  if (a.src != nullptr && (a.src[env] < 0 || a.src[env] >= a.n_rows)) return false;
  return true;
}

// One env behind a reset / restore / set: what it had open is discarded, an episode begins with clean accumulators.
SCN_HD void checks_begin_lane(const ChkArgs& a, int env, int lane, int nl, ChkCnt& c, int meta0) {
  for (int k = lane; k < a.tab.I; k += nl) checks_acc_store(a, (size_t)env * a.tab.I + k, checks_clean());
  c.length = 0; c.oflags = a.flag; c.clock = meta0;
}

// The open episode of an env as a record's item words into `out` (nothing is changed); `row`: the table's rule at the live meta words.
SCN_HD void checks_open_lane(const ChkArgs& a, int env, int lane, int nl, int row, int* out, unsigned long long* fail, unsigned long long* inc) {
  const ChkTable& T = a.tab;
  SCN_TAB(int32_t) tt = SCN_TAB_CAST(int32_t, T.t);
  SCN_TAB(int32_t) mode = SCN_TAB_CAST(int32_t, T.mode);
  SCN_TAB(int32_t) cmp = SCN_TAB_CAST(int32_t, T.cmp);
  SCN_TAB(float) bound = SCN_TAB_CAST(float, T.bound);
  int i0, ni;
  checks_row_items(T, row, &i0, &ni);
  for (int k = lane; k < T.I; k += nl) {
    int value = 0, aux = 0;
    if (k < ni) {
      const int i = i0 + k;
      bool f, n;
      checks_verdict(checks_acc_load(a, (size_t)env * T.I + k), tt[2 * i], tt[2 * i + 1], mode[i], cmp[i], bound[i], &value, &aux, &f, &n);
      if (f) *fail |= 1ull << k;
      if (n) *inc |= 1ull << k;
    }
    out[CHK_HDR + 2 * k] = value;
    out[CHK_HDR + 2 * k + 1] = aux;
  }
}

}  // namespace cosim
