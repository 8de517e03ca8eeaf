// cosim_search.h — the per-env rule of a scenario table's limit search (cosim_set_param "search", include/cosim.h), as inline
// functions that the device kernels (cosim_search.hip) and a plain host C++ program (tests/search_lanes.cpp) both compile.
//
// A scenario carries at most one search item (lo, hi, x0, d0, d_min, rule, trials, targets, fail_mask, rev_skip, harder, check mask).
// Every env whose row has one keeps a LEVEL, a float32 word inside [lo, hi] that the scenario kernel multiplies into the row's push
// vectors (targets bit 1) and / or command keyframes (bit 2), and the parameter-window, observation-fault and action-fault kernels
// into the values of the row's MARKED items of their kind (bits 4, 8, 16; cosim_scnparams.h, cosim_fault.h).  When an episode of the env ends, its outcome moves the level:
//   flags = 1 terminated | 2 truncated | 4 meta[4] moved | 8 the episode did not begin at a reset | (meta[15] & 7) << 5 with a fall
//           rule set -- the ledger's flags (cosim_ledger.hip), restated here
//   the episode is a COUNTED TRIAL iff the row has an item, the env is not done and the episode began at a reset (one that began
//   at a restore / set_state may have missed its push window)
//   fail = (flags & fail_mask) != 0 || a selected check of the ended episode is not passed: (fail mask | incomplete mask) of the
//     verdict record the checks kernel closed behind this same step (cosim_checks.h, record words 4..7) & the item's check mask
//   harder up (0):   dir = fail ? -1 : +1, x = level:
//     fail ? lo_fail = has_fail ? fminf(lo_fail, x) : x : hi_pass = has_pass ? fmaxf(hi_pass, x) : x
//   harder down (1): dir = fail ? +1 : -1 (a LOWER level is harder: friction, a gain scale); the two bracket words then hold the
//     highest failure and the lowest pass: fail ? lo_fail = has_fail ? fmaxf(lo_fail, x) : x : hi_pass = has_pass ? fminf(hi_pass, x) : x
//     rev = last_dir != 0 && dir != last_dir;  a reversal beyond the first rev_skip adds x to rev_sum (rev_n++)
//     staircase: on a reversal step = fmaxf(step * 0.5f, d_min), then x' = x + dir * step
//     bisect:    x' = x + dir * step, then step = fmaxf(step * 0.5f, d_min)
//     level = fminf(fmaxf(x', lo), hi);  after `trials` counted trials the env is done and its level frozen
// All floats are float32, one operation per statement, contraction off: the numpy twin (cosim_amd/search.py reference_search)
// repeats them bit for bit.
// Per env SRCH_NCNT int32 words: 0 level  1 step  2 trials  3 fails  4 last_dir  5 reversals  6 rev_sum  7 rev_n  8 hi_pass
// 9 lo_fail  10 status (1 the open episode began at a reset | 2 done | 4 has a pass | 8 has a fail | 16 the row has an item)
// 11 episodes ended since arming (the ledger's ordinal)  12 length of the open episode  13 meta[4] at its start  14 ended episodes
// that were not trials  15 zero.
// Trial record, 4 words, in slot (episode mod slots) of the env's ring: episode, the level the episode RAN at (bits),
// flags | 256 counted | 512 fail | 1024 reversal | 2048 failed by a check, length.
#pragma once
#include <stddef.h>
#include <string.h>

#include "cosim_scenario.h"

namespace cosim {

enum { SRCH_BISECT = 0, SRCH_STAIRCASE = 1 };
enum { SRCH_PUSHES = 1, SRCH_COMMANDS = 2, SRCH_PARAMS = 4, SRCH_OBS_FAULTS = 8, SRCH_ACT_FAULTS = 16 };
enum { SRCH_HARDER_UP = 0, SRCH_HARDER_DOWN = 1 };
enum { SRCH_AT_RESET = 1, SRCH_DONE = 2, SRCH_HAS_PASS = 4, SRCH_HAS_FAIL = 8, SRCH_HAS_ITEM = 16 };
// the ledger's flag values (cosim_ledger.hip) and the three a trial record adds
enum { SRCH_TERMINATED = 1, SRCH_TRUNCATED = 2, SRCH_NONFINITE = 4, SRCH_NO_RESET = 8, SRCH_COUNTED = 256, SRCH_FAILED = 512, SRCH_REVERSAL = 1024,
       SRCH_BY_CHECK = 2048 };
constexpr int SRCH_NCNT = 16, SRCH_TRIAL_WORDS = 4, SRCH_MAX_SLOTS = 64, SRCH_MAX_TRIALS = 1 << 20, SRCH_MAX_REV_SKIP = 255;
constexpr int SRCH_FAIL_BITS = 1 | 4 | 32 | 64 | 128;   // what a fail_mask may select: terminated, non-finite, tilt, height, contact
enum { SRCH_LEVEL = 0, SRCH_STEP, SRCH_TRIALS, SRCH_FAILS, SRCH_LAST_DIR, SRCH_REVERSALS, SRCH_REV_SUM, SRCH_REV_N, SRCH_HI_PASS, SRCH_LO_FAIL,
       SRCH_STATUS, SRCH_EPISODE, SRCH_LENGTH, SRCH_NAN0, SRCH_UNCOUNTED };

struct SrchTable {
  const int32_t* has;        // [S] 1: the scenario has an item
  const float* lo;           // [S]
  const float* hi;
  const float* x0;
  const float* d0;
  const float* d_min;
  const int32_t* rule;
  const int32_t* trials;
  const int32_t* targets;
  const int32_t* fail_mask;
  const int32_t* rev_skip;
  int n_scn, n_items;        // n_items: scenarios that have one
  // the long form's columns; null (the short form): harder up, no check
  const int32_t* harder;     // [S] SRCH_HARDER_*
  const int32_t* chk_lo;     // [S] the selected checks of the row, bit i = check item i (low, high word)
  const int32_t* chk_hi;
};

struct SrchItem { float lo, hi, x0, d0, d_min; int has, rule, trials, targets, fail_mask, rev_skip, harder, chk_lo, chk_hi; };

struct SrchArgs {
  SrchTable tab;
  const uint8_t* term;     // [N]
  const uint8_t* trunc;    // [N]
  const float* state;      // [N][s_stride] live state records (meta words 4 and 15 are read)
  const int32_t* scn_row;  // [N] rows the scenario kernel wrote ahead of this step
  int* rec;                // [N][SRCH_NCNT]
  int* ring;               // [N][slots][SRCH_TRIAL_WORDS]
  int* remaining;          // one word: envs with an item that are not done
  const uint8_t* mask;     // begin: uint8[N] or null
  const int* src;          // begin: the restore's source index or null; envs it refused (outside [0, n_rows)) are left alone
  int n_rows;
  int n_envs, first, count;
  int s_stride, s_meta, slots;
  int flag;                // begin: open flags of the new episode
  int fall;                // a fall rule is set: meta word 15 holds the cause of the env's latest episode end
  int n_armed;             // init: what `remaining` starts at
  unsigned scn_off;        // init: the table's gid_off (mode env: the row never changes)
};

SCN_HD int search_bits(float f) { int u; memcpy(&u, &f, 4); return u; }
SCN_HD float search_float(int u) { float f; memcpy(&f, &u, 4); return f; }

// the item of a row; a row outside the table is clamped into it
SCN_HD SrchItem search_item(const SrchTable& T, int row) {
  row = row < 0 ? 0 : (row >= T.n_scn ? T.n_scn - 1 : row);
  SrchItem it;
  it.has = SCN_TAB_CAST(int32_t, T.has)[row];
  it.lo = SCN_TAB_CAST(float, T.lo)[row]; it.hi = SCN_TAB_CAST(float, T.hi)[row]; it.x0 = SCN_TAB_CAST(float, T.x0)[row];
  it.d0 = SCN_TAB_CAST(float, T.d0)[row]; it.d_min = SCN_TAB_CAST(float, T.d_min)[row];
  it.rule = SCN_TAB_CAST(int32_t, T.rule)[row]; it.trials = SCN_TAB_CAST(int32_t, T.trials)[row];
  it.targets = SCN_TAB_CAST(int32_t, T.targets)[row]; it.fail_mask = SCN_TAB_CAST(int32_t, T.fail_mask)[row];
  it.rev_skip = SCN_TAB_CAST(int32_t, T.rev_skip)[row];
  it.harder = 0; it.chk_lo = 0; it.chk_hi = 0;
  if (T.harder != nullptr) {
    it.harder = SCN_TAB_CAST(int32_t, T.harder)[row]; it.chk_lo = SCN_TAB_CAST(int32_t, T.chk_lo)[row]; it.chk_hi = SCN_TAB_CAST(int32_t, T.chk_hi)[row];
  }
  return it;
}

// what the level of an env scales: the item's targets, 0 for a row without an item
SCN_HD int search_targets(const SrchTable& T, int row) {
  row = row < 0 ? 0 : (row >= T.n_scn ? T.n_scn - 1 : row);
  return SCN_TAB_CAST(int32_t, T.has)[row] != 0 ? SCN_TAB_CAST(int32_t, T.targets)[row] : 0;
}

// an ended episode's flags, as ledger_step_kernel builds them
SCN_HD int search_flags(int te, int tr, int nan_now, int nan0, int status, int fall, int meta15) {
  return (te ? SRCH_TERMINATED : 0) | (tr ? SRCH_TRUNCATED : 0) | (nan_now != nan0 ? SRCH_NONFINITE : 0) | ((status & SRCH_AT_RESET) ? 0 : SRCH_NO_RESET) |
         (fall ? (meta15 & 7) << 5 : 0);
}

// a fresh record of an env whose row holds item `it`
SCN_HD void search_init(int* rec, const SrchItem& it, int meta4, int flag) {
  for (int w = 0; w < SRCH_NCNT; w++) rec[w] = 0;
  if (it.has) { rec[SRCH_LEVEL] = search_bits(it.x0); rec[SRCH_STEP] = search_bits(it.d0); }
  rec[SRCH_STATUS] = (it.has ? SRCH_HAS_ITEM : 0) | (flag == 0 ? SRCH_AT_RESET : 0);
  rec[SRCH_NAN0] = meta4;
}

// One counted trial at level x: the update of the record's words 0 .. 10.  Returns the trial record's extra flags.
SCN_HD int search_trial(int* rec, const SrchItem& it, bool fail) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float x = search_float(rec[SRCH_LEVEL]);
  float step = search_float(rec[SRCH_STEP]);
  int status = rec[SRCH_STATUS];
  const bool down = it.harder == SRCH_HARDER_DOWN;
  const int dir = (fail != down) ? -1 : 1, last = rec[SRCH_LAST_DIR];
  if (fail) {
    const float old = search_float(rec[SRCH_LO_FAIL]);
    rec[SRCH_LO_FAIL] = search_bits((status & SRCH_HAS_FAIL) ? (down ? fmaxf(old, x) : fminf(old, x)) : x);
    status |= SRCH_HAS_FAIL;
  } else {
    const float old = search_float(rec[SRCH_HI_PASS]);
    rec[SRCH_HI_PASS] = search_bits((status & SRCH_HAS_PASS) ? (down ? fminf(old, x) : fmaxf(old, x)) : x);
    status |= SRCH_HAS_PASS;
  }
  const bool rev = last != 0 && dir != last;
  if (rev) {
    rec[SRCH_REVERSALS]++;
    if (rec[SRCH_REVERSALS] > it.rev_skip) {
      const float sum = search_float(rec[SRCH_REV_SUM]) + x;
      rec[SRCH_REV_SUM] = search_bits(sum);
      rec[SRCH_REV_N]++;
    }
  }
  float xn;
  if (it.rule == SRCH_STAIRCASE) {
    if (rev) { const float h = step * 0.5f; step = fmaxf(h, it.d_min); }
    const float d = dir > 0 ? step : -step;
    xn = x + d;
  } else {
    const float d = dir > 0 ? step : -step;
    xn = x + d;
    const float h = step * 0.5f;
    step = fmaxf(h, it.d_min);
  }
  rec[SRCH_LEVEL] = search_bits(fminf(fmaxf(xn, it.lo), it.hi));
  rec[SRCH_STEP] = search_bits(step);
  rec[SRCH_LAST_DIR] = dir;
  rec[SRCH_TRIALS]++;
  rec[SRCH_FAILS] += fail ? 1 : 0;
  if (rec[SRCH_TRIALS] >= it.trials) status |= SRCH_DONE;
  rec[SRCH_STATUS] = status;
  return SRCH_COUNTED | (fail ? SRCH_FAILED : 0) | (rev ? SRCH_REVERSAL : 0);
}

// One env behind one control step.  `rec`: its SRCH_NCNT words; `ring`: its slots * 4 trial words; `meta`: the env's meta words as
// the step left them; `verdict`: the verdict record the checks kernel closed for the episode this step ended (read only on a step
// with a done flag and an item that selects a check), or null.  Returns 1 if the env became done on this step (the caller takes 1
// off the engine's "remaining" word).
SCN_HD int search_step_lane(int* rec, int* ring, int slots, const SrchItem& it, int te, int tr, const int* meta, int fall, const int* verdict = nullptr) {
  const int length = rec[SRCH_LENGTH] + 1;
  if (!(te | tr)) { rec[SRCH_LENGTH] = length; return 0; }
  const int status = rec[SRCH_STATUS], nan_now = meta[4];
  const int flags = search_flags(te, tr, nan_now, rec[SRCH_NAN0], status, fall, meta[15]);
  const int level = rec[SRCH_LEVEL], episode = rec[SRCH_EPISODE];
  int extra = 0;
  if (it.has && !(status & SRCH_DONE) && (status & SRCH_AT_RESET)) {
    const bool by_check = verdict != nullptr && ((((verdict[4] | verdict[6]) & it.chk_lo) | ((verdict[5] | verdict[7]) & it.chk_hi)) != 0);
    extra = search_trial(rec, it, (flags & it.fail_mask) != 0 || by_check) | (by_check ? SRCH_BY_CHECK : 0);
  } else rec[SRCH_UNCOUNTED]++;
  int* t = ring + (size_t)((unsigned)episode % (unsigned)slots) * SRCH_TRIAL_WORDS;
  t[0] = episode; t[1] = level; t[2] = flags | extra; t[3] = length;
  rec[SRCH_EPISODE] = episode + 1;
  rec[SRCH_LENGTH] = 0;
  rec[SRCH_NAN0] = nan_now;
  rec[SRCH_STATUS] |= SRCH_AT_RESET;   // the auto-reset began the next episode
  return (rec[SRCH_STATUS] & SRCH_DONE) && !(status & SRCH_DONE);
}

// whether the begin rule applies to env (mask and restore source, as ledger_begin_kernel reads them)
SCN_HD bool search_begin_applies(const SrchArgs& a, int env) {
  if (a.mask != nullptr && a.mask[env] == 0) return false;
  if (a.src != nullptr && (a.src[env] < 0 || a.src[env] >= a.n_rows)) return false;
  return true;
}

// One env behind a reset / restore / set_state: what it had open is discarded, the level does not move.
SCN_HD void search_begin_lane(int* rec, int flag, int meta4) {
  rec[SRCH_STATUS] = (rec[SRCH_STATUS] & ~SRCH_AT_RESET) | (flag == 0 ? SRCH_AT_RESET : 0);
  rec[SRCH_LENGTH] = 0;
  rec[SRCH_NAN0] = meta4;
}

// scenario_apply with the env's level multiplied into what `targets` names (0: nothing, the unscaled expressions): the selected
// keyframe row is key_cmd[c] * level (SRCH_COMMANDS; a pass-through caller's command is never scaled), the hit push is (v0 * level,
// v1 * level, v2 * level) into scenario_push (SRCH_PUSHES).  Returns 1 if a push was applied.
SCN_HD int scenario_apply_scaled(const ScnTable& T, int row, int t, const float* cmd_in, float* cmd_out, const float* quat, float* qvel, bool push,
                                 int targets, float level) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  SCN_TAB(int32_t) key_adr = SCN_TAB_CAST(int32_t, T.key_adr);
  SCN_TAB(int32_t) key_t = SCN_TAB_CAST(int32_t, T.key_t);
  SCN_TAB(float) key_cmd = SCN_TAB_CAST(float, T.key_cmd);
  const int k0 = key_adr[row], k1 = key_adr[row + 1];
  int sel = -1;
  for (int k = k0; k < k1; k++) {   // sorted: stop at the first keyframe still ahead
    if (key_t[k] > t) break;
    sel = k;
  }
  for (int c = 0; c < T.cd; c++) {
    float v;
    if (sel >= 0) {
      v = key_cmd[(size_t)sel * T.cd + c];
      if (targets & SRCH_COMMANDS) v = v * level;
    } else v = cmd_in[c];
    cmd_out[c] = v;
  }
  if (!push) return 0;
  SCN_TAB(int32_t) push_adr = SCN_TAB_CAST(int32_t, T.push_adr);
  SCN_TAB(int32_t) push_t = SCN_TAB_CAST(int32_t, T.push_t);
  SCN_TAB(float) push_v = SCN_TAB_CAST(float, T.push_v);
  const int p0 = push_adr[row], p1 = push_adr[row + 1];
  int hit = -1;
  for (int p = p0; p < p1; p++)
    if (push_t[2 * p] <= t && t < push_t[2 * p + 1]) hit = p;   // the last listed window wins
  if (hit < 0) return 0;
  float v0 = push_v[3 * hit], v1 = push_v[3 * hit + 1], v2 = push_v[3 * hit + 2];
  if (targets & SRCH_PUSHES) { v0 = v0 * level; v1 = v1 * level; v2 = v2 * level; }
  scenario_push(quat, v0, v1, v2, qvel);
  return 1;
}

}  // namespace cosim
