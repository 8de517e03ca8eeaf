// cosim_curves.h — the rule of a scenario table's response curves (cosim_scenario_curves_set / cosim_scenario_curves_get,
// include/cosim.h), as inline functions that the device kernels (cosim_curves.hip) and a plain host C++ program
// (tests/curves_lanes.cpp) both compile.
//
// Scenario s owns the items [adr[s], adr[s + 1]) (at most 8).  Item i = (t0, t1, every, signal, index, lo, hi, bins) takes one sample
// at every control step whose PRE-STEP episode clock t holds t0 <= t < t1 and (t - t0) % every == 0, into time bin j = (t - t0) /
// every of T = ceil((t1 - t0) / every) <= 1024.  The clock is the checks' (cosim_checks.h): a per-env word set to meta word 0 by the
// begin rule and again behind every step; a step's t is the word the previous invocation stored.  The value is checks_signal():
// signals 4 .. 7 read the live state record and take NO sample on a row with a done flag, 0 .. 3 do.
// Stage, int32 [N][SW] (SW: the largest sum of T over a scenario's items): word soff[i] + j of the env's row holds the sample's float
// bits, written with a plain store; CUR_NONE = no sample; a NaN or +-inf sample is stored as CUR_NONFINITE.
// Fold, on a row with a done flag: every bin of the episode's row that holds a sample goes into the cells of (item, class), class 1
// if `terminated` is set, else 0, and the stage word becomes CUR_NONE again.  The cells of (item, class) are cw[i] 32-bit words at
// coff[i] + class * cw[i], time bin innermost:  count[T] | nan[T] | min[T] | max[T] | sum[T] (int64, 8-byte aligned) | hist[B + 2][T]
//   non-finite sample: nan[j] += 1 and nothing else
//   finite v:          count[j] += 1;  sum[j] += llrint((double)clamp(v, -2^20, 2^20) * 2^20) (round to nearest even);
//                      min[j] / max[j]: unsigned min / max of key(v) = bits ^ (bits >> 31 ? 0xffffffff : 0x80000000);
//                      B > 0: hist[r][j] += 1, r = 0 if v < lo, B + 1 if v >= hi, else 1 + min((int)((v - lo) * inv_w), B - 1) in fp32,
//                      one rounded operation at a time, contraction off (inv_w = float32(B / (double(hi) - double(lo))), from the host)
// Every cell update is an integer operation that commutes, handed to the caller's `At` (the kernel: atomics that discard their
// result; the host program: plain operations), so the cells are a function of the set of ended episodes alone.
//
// Groups (cosim_scenario_curves_groups): with G groups the cells are G planes, each a whole cell image of the layout above (the same
// coff / cw, W words), plane g at word g * W.  Sampling, staging and the clock do not change.  The fold reads the env's group word
// once, as it stands then, and folds the episode into that plane; a word outside [0, G) touches no cell, the stage still goes back to
// "no sample", and the episode is counted in one device word, `ungrouped`.  Each plane being a whole image, the planes merged word
// kind by word kind (counts, sums and histograms add, extremes merge on their keys) are the cells without groups.
//
// The bodies are written per lane: in the sampling phase lane `lane` of `nl` handles the items lane, lane + nl, ...; in the fold
// phase the items are walked by every lane and the lanes stride over an item's time bins.
#pragma once
#include <stddef.h>
#include <string.h>

#include "cosim_checks.h"

namespace cosim {

constexpr int CUR_MAX_ITEMS = 8, CUR_MAX_T = 1024, CUR_MAX_BINS = 64, CUR_MAX_GROUPS = 64;
constexpr int CUR_NONE = 0x7fc00000;        // stage word: no sample
constexpr int CUR_NONFINITE = 0x7fc00001;   // stage word: a NaN or +-inf sample
constexpr size_t CUR_MAX_BYTES = (size_t)256 << 20;   // of the cells and of the stage, each (a design limit)

struct CurTable {
  const int32_t* adr;      // [S + 1]
  const int32_t* t;        // [n][3] t0, t1, every
  const int32_t* signal;   // [n]
  const int32_t* index;    // [n]
  const int32_t* bins;     // [n] B
  const int32_t* nt;       // [n] T
  const int32_t* soff;     // [n] first stage word of the item in an env's row
  const int32_t* coff;     // [n] first cell word of (item, class 0)
  const int32_t* cw;       // [n] cell words of one class: (B + 8) T rounded up to even
  const float* lo;         // [n]
  const float* hi;         // [n]
  const float* inv_w;      // [n]
  int n_scn, n_items, SW;
};

struct CurArgs {
  CurTable tab;
  const float* info;       // [N][info_dim] the caller's info rows of this step
  const uint8_t* term;     // [N]
  const uint8_t* trunc;    // [N]
  const float* cmd;        // [N][cmd_stride] the applied command (scenario_cmd), or null with command_dim 0
  const float* state;      // [N][s_stride] live state records
  const int32_t* scn_row;  // [N] rows the scenario kernel wrote ahead of this step
  int* stage;              // [N][SW]
  int* clk;                // [N] the clock word
  unsigned* cells;         // the cells of every (item, class)
  const uint8_t* mask;     // begin: uint8[N] or null
  const int* src;          // begin: the restore's source index or null; envs it refused (outside [0, n_rows)) are left alone
  int n_rows;
  int n_envs, first, count;
  int info_dim, nu, cmd_stride;
  int s_stride, s_qpos, s_qvel, s_meta;
  // groups (cosim_scenario_curves_groups); all zero: no groups, one plane
  const int32_t* group;    // [N] the caller's group word of every env, read on a row with a done flag only
  int n_groups;            // G: the cells are G planes, each a whole cell image; plane g starts at word g * plane_words
  size_t plane_words;      // W: the cell words of one plane
  unsigned* ungrouped;     // one word: the ended episodes whose group word was outside [0, G)
};

SCN_HD int curves_nt(int t0, int t1, int every) { return (int)(((long long)t1 - t0 + every - 1) / every); }
SCN_HD int curves_cell_words(int T, int B) { return ((B + 8) * T + 1) & ~1; }
SCN_HD unsigned curves_key(int bits) { return (unsigned)bits ^ (((unsigned)bits >> 31) ? 0xffffffffu : 0x80000000u); }
SCN_HD bool curves_finite(int bits) { return (bits & 0x7f800000) != 0x7f800000; }

// the fields of ChkArgs that checks_signal() reads
SCN_HD ChkArgs curves_signal_args(const CurArgs& a) {
  ChkArgs c = {};
  c.info = a.info; c.state = a.state; c.cmd = a.cmd;
  c.info_dim = a.info_dim; c.nu = a.nu; c.cmd_stride = a.cmd_stride; c.s_stride = a.s_stride; c.s_qpos = a.s_qpos; c.s_qvel = a.s_qvel;
  return c;
}

// the items [i0, i0 + ni) of a row; a row outside the table is clamped into it
SCN_HD void curves_row_items(const CurTable& T, int row, int* i0, int* ni) {
  SCN_TAB(int32_t) adr = SCN_TAB_CAST(int32_t, T.adr);
  row = row < 0 ? 0 : (row >= T.n_scn ? T.n_scn - 1 : row);
  *i0 = adr[row];
  const int n = adr[row + 1] - adr[row];
  *ni = n < 0 ? 0 : (n > CUR_MAX_ITEMS ? CUR_MAX_ITEMS : n);
}

// the histogram row of a finite sample
SCN_HD int curves_hist_row(float v, float lo, float hi, float inv_w, int B) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  if (v < lo) return 0;
  if (v >= hi) return B + 1;
  const float d = v - lo;
  const float x = d * inv_w;
  return 1 + (x < (float)B ? (int)x : B - 1);   // min((int)x, B - 1), also where x is past what an int holds
}

// the fixed-point addend of a finite sample
SCN_HD long long curves_fixed(float v) {
  const float c = v > 1048576.f ? 1048576.f : (v < -1048576.f ? -1048576.f : v);
  return llrint((double)c * 1048576.0);
}

// Sampling phase of one env behind one control step at clock t, lane `lane` of `nl`: one plain store per item that is due.
SCN_HD void curves_sample_lane(const CurArgs& a, int env, int lane, int nl, int t, int row, bool done) {
  const CurTable& T = a.tab;
  SCN_TAB(int32_t) tt = SCN_TAB_CAST(int32_t, T.t);
  SCN_TAB(int32_t) sig = SCN_TAB_CAST(int32_t, T.signal);
  SCN_TAB(int32_t) idx = SCN_TAB_CAST(int32_t, T.index);
  SCN_TAB(int32_t) soff = SCN_TAB_CAST(int32_t, T.soff);
  int i0, ni;
  curves_row_items(T, row, &i0, &ni);
  for (int k = lane; k < ni; k += nl) {
    const int i = i0 + k;
    const int t0 = tt[3 * i], t1 = tt[3 * i + 1], every = tt[3 * i + 2], sg = sig[i];
    if (t < t0 || t >= t1 || (done && checks_state_signal(sg))) continue;
    const int d = t - t0, j = d / every;
    if (d - j * every != 0) continue;
    const ChkArgs c = curves_signal_args(a);
    const int bits = checks_bits(checks_signal(c, env, sg, idx[i]));
    a.stage[(size_t)env * T.SW + soff[i] + j] = curves_finite(bits) ? bits : CUR_NONFINITE;
  }
}

// Fold phase of one env on a row with a done flag, lane `lane` of `nl`: the staged bins of the episode's row into the cells of class
// `cls`, and the stage back to "no sample".  The lanes stride over the time bins of one item after the other.
template <class At>
SCN_HD void curves_fold_lane(const CurArgs& a, int env, int lane, int nl, int row, int cls, At& at) {
  const CurTable& T = a.tab;
  SCN_TAB(int32_t) bins = SCN_TAB_CAST(int32_t, T.bins);
  SCN_TAB(int32_t) nt = SCN_TAB_CAST(int32_t, T.nt);
  SCN_TAB(int32_t) soff = SCN_TAB_CAST(int32_t, T.soff);
  SCN_TAB(int32_t) coff = SCN_TAB_CAST(int32_t, T.coff);
  SCN_TAB(int32_t) cw = SCN_TAB_CAST(int32_t, T.cw);
  SCN_TAB(float) lo = SCN_TAB_CAST(float, T.lo);
  SCN_TAB(float) hi = SCN_TAB_CAST(float, T.hi);
  SCN_TAB(float) inv_w = SCN_TAB_CAST(float, T.inv_w);
  int i0, ni;
  curves_row_items(T, row, &i0, &ni);
  for (int k = 0; k < ni; k++) {
    const int i = i0 + k;
    const int n = nt[i], B = bins[i];
    const float l = lo[i], h = hi[i], w = inv_w[i];
    int* st = a.stage + (size_t)env * T.SW + soff[i];
    unsigned* cell = a.cells + (size_t)coff[i] + (size_t)cls * (size_t)cw[i];
    unsigned long long* sum = reinterpret_cast<unsigned long long*>(cell + 4 * (size_t)n);
    for (int j = lane; j < n; j += nl) {
      const int bits = st[j];
      if (bits == CUR_NONE) continue;
      st[j] = CUR_NONE;
      if (!curves_finite(bits)) { at.add(cell + n + j, 1u); continue; }
      const float v = checks_float(bits);
      at.add(cell + j, 1u);
      at.add64(sum + j, (unsigned long long)curves_fixed(v));
      const unsigned key = curves_key(bits);
      at.min(cell + 2 * (size_t)n + j, key);
      at.max(cell + 3 * (size_t)n + j, key);
      if (B > 0) at.add(cell + (size_t)(6 + curves_hist_row(v, l, h, w, B)) * n + j, 1u);
    }
  }
}

// Fold phase with groups: the episode goes into plane `g` (the env's group word as the fold read it, the same value in every lane) by
// curves_fold_lane's arithmetic.  A word outside [0, G) touches no cell: the episode's staged bins go back to "no sample" and lane 0
// counts the episode in `ungrouped`.
template <class At>
SCN_HD void curves_fold_group_lane(const CurArgs& a, int env, int lane, int nl, int row, int cls, int g, At& at) {
  if (g >= 0 && g < a.n_groups) {
    CurArgs p = a;
    p.cells = a.cells + (size_t)g * a.plane_words;
    curves_fold_lane(p, env, lane, nl, row, cls, at);
    return;
  }
  const CurTable& T = a.tab;
  SCN_TAB(int32_t) nt = SCN_TAB_CAST(int32_t, T.nt);
  SCN_TAB(int32_t) soff = SCN_TAB_CAST(int32_t, T.soff);
  int i0, ni;
  curves_row_items(T, row, &i0, &ni);
  for (int k = 0; k < ni; k++) {
    int* st = a.stage + (size_t)env * T.SW + soff[i0 + k];
    const int n = nt[i0 + k];
    for (int j = lane; j < n; j += nl) st[j] = CUR_NONE;
  }
  if (lane == 0) at.add(a.ungrouped, 1u);
}

// whether the begin rule applies to env (mask and restore source, as checks_begin_applies reads them)
SCN_HD bool curves_begin_applies(const CurArgs& a, int env) {
  if (a.mask != nullptr && a.mask[env] == 0) return false;
  if (a.src != nullptr && (a.src[env] < 0 || a.src[env] >= a.n_rows)) return false;
  return true;
}

// One env behind a reset / restore / set: what it had staged is discarded.
SCN_HD void curves_begin_lane(const CurArgs& a, int env, int lane, int nl) {
  int* st = a.stage + (size_t)env * a.tab.SW;
  for (int j = lane; j < a.tab.SW; j += nl) st[j] = CUR_NONE;
}

// word w of the cleared cells of one (item, class): zeros, the min keys all ones
SCN_HD unsigned curves_clear_word(int w, int T) { return (w >= 2 * T && w < 3 * T) ? 0xffffffffu : 0u; }

}  // namespace cosim
