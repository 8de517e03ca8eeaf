// cosim_actfault.h — the per-env rule of a scenario table's action faults (cosim_set_param "action_faults", include/cosim.h), as
// inline functions that the device kernels (cosim_actfault.hip) and a plain host C++ program (tests/actfault_lanes.cpp) both compile.
//
// Scenario s owns the items [adr[s], adr[s + 1]).  An item is ONE 16-byte record of four 32-bit words
//   (t0, t1, j | op << 16 | ord << 24, value)
// (the array of records ends in ACF_CHUNK - 1 all-zero ones, so that a reader may fetch ACF_CHUNK records from any item on)
// and covers the PRE-STEP episode clocks t0 <= t < t1: t = meta[0] as the step finds it, the clock keyframes, pushes and parameter
// windows use.  j is an actuator (j < nu <= 64), ord the ordinal of the listed item it was expanded from (0..255: all actuators of
// one listed item share it).  The row is that of cosim_scenario.h on the pre-step meta words.
//
// Per actuator under at least one item that holds: start from x, the caller's action word (the policy's raw output, before a_scale),
// and apply the holding items that name the actuator IN LISTED ORDER, composing, every operation with contraction off:
//   0 scale  x * value                         4 hold   rec[s_lastact + j]: the action the step kernel was given one step earlier,
//   1 bias   x + value                                  the EFFECTIVE one, so a held channel stays frozen through the window
//   2 set    value                             5 drop   as hold if (w' >> 8) * 2^-24 < value, one word w' per (env, step, item)
//   3 noise  x + value * u, u in [-1, 1)       6 clip   x > value ? value : (x < -value ? -value : x); NaN stays NaN
// Philox4x32-10, first output word, key (seed_lo, seed_hi), counter (meta[1] pre-step, 8 | index << 8, gid_lo, gid_hi): purpose 8;
// noise: index = j, mapped by obsfault_noise_u; drop: index = 0x10000 + ord, mapped by obsfault_drop_u.
// At t == 0 the record holds no previous action: hold and drop are the identity there.  An actuator under no holding item gets the
// caller's bits.  Nothing is kept per env: the effective action is a function of (state record, table, caller's action).
#pragma once
#include "cosim_obsfault.h"

namespace cosim {

enum { ACF_SCALE = 0, ACF_BIAS = 1, ACF_SET = 2, ACF_NOISE = 3, ACF_HOLD = 4, ACF_DROP = 5, ACF_CLIP = 6, ACF_NOP = 7 };
#define ACF_SETTER "cosim_set_param \"action_faults\""   /* how the messages name the setter */
constexpr int ACF_MAX_ITEMS = 256;          // per scenario, expanded
constexpr unsigned ACF_PURPOSE = 8u;        // of the Philox counter (cosim_amd/rng.py lists the others)
constexpr unsigned ACF_DROP_INDEX = 0x10000u;
constexpr int ACF_CHUNK = 4;                // item records fetched at a time; the item array is padded by ACF_CHUNK - 1 records

struct ActFaultTable {
  const int32_t* adr;    // [S + 1]
  const int32_t* item;   // [n + ACF_CHUNK - 1][4]: t0, t1, j | op << 16 | ord << 24, value (float bits); the padding is zeros
  int n_scn, n_items;
};

// what the rule reads of one env besides the caller's action
struct ActFaultEnv {
  const float* lastact;          // rec + s_lastact: [nu], the previous step's effective action (zeros after a reset)
  unsigned k0, k1, c0, g0, g1;   // Philox key, counter word 0 (meta[1] pre-step) and the global env id
};

// Actuator j of one env in row `row` at pre-step clock t: the effective action word from the caller's word x.  The row's items are
// walked once; the previous action is loaded at the first item that holds, so an env under no holding item reads nothing of its
// record here and returns x's bits.  The walk does not depend on j but in the compare that selects an item: every lane of a wave
// that serves one env makes the same loads and takes the same branches up to that compare.
SCN_HD float actfault_apply(const ActFaultTable& F, int row, int t, const ActFaultEnv& E, int j, float x) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  SCN_TAB(int32_t) adr = SCN_TAB_CAST(int32_t, F.adr);
  SCN_TAB(int32_t) item = SCN_TAB_CAST(int32_t, F.item);
  const int i0 = adr[row], i1 = adr[row + 1];
  const bool first = t == 0;
  float prev = 0.f;
  bool loaded = false;
  // the row is the same for every lane of an env: these loads do not depend on the lane.  ACF_CHUNK records, one 64-byte line, are
  // fetched at a time, unconditionally (the array ends in ACF_CHUNK - 1 records that never hold)
  for (int c = i0; c < i1; c += ACF_CHUNK) {
    int32_t w[4 * ACF_CHUNK];
#pragma unroll
    for (int k = 0; k < 4 * ACF_CHUNK; k++) w[k] = item[4 * c + k];
#pragma unroll
    for (int i = 0; i < ACF_CHUNK; i++) {
      if (c + i >= i1) break;
      const int t0 = w[4 * i], t1 = w[4 * i + 1];
      if (!(t0 <= t && t < t1)) continue;
      const unsigned key = (unsigned)w[4 * i + 2];
      const float value = obsfault_bits(w[4 * i + 3]);
      const int el = (int)(key & 0xffffu), ord = (int)(key >> 24);
      int op = (int)((key >> 16) & 0xffu);
      if (!loaded) {
        loaded = true;
        if (!first) prev = E.lastact[j];
      }
      if (op == ACF_DROP) {   // one draw for the item: its actuators are lost together
        const unsigned draw = obsfault_philox(E.k0, E.k1, E.c0, ACF_PURPOSE | ((ACF_DROP_INDEX + (unsigned)ord) << 8), E.g0, E.g1);
        op = obsfault_drop_u(draw) < value ? ACF_HOLD : ACF_NOP;
      }
      if (op == ACF_HOLD && first) op = ACF_NOP;
      if (el != j) continue;
      if (op == ACF_SCALE) x = x * value;
      else if (op == ACF_BIAS) x = x + value;
      else if (op == ACF_SET) x = value;
      else if (op == ACF_NOISE) {
        const float u = obsfault_noise_u(obsfault_philox(E.k0, E.k1, E.c0, ACF_PURPOSE | ((unsigned)j << 8), E.g0, E.g1));
        const float d = value * u;
        x = x + d;
      } else if (op == ACF_HOLD) x = prev;
      else if (op == ACF_CLIP) x = x > value ? value : (x < -value ? -value : x);
    }
  }
  return x;
}

// The words of last_action element e (actuator idx, scale el_scale) that the step kernel wrote from the action it was given, rewritten
// from the policy's own output `raw`: the frequency cache, row 0 of the record's observation stack and the newest frame of state_out
// (a non-stacked element: its one word behind the stack rows).  One float32 multiply, the step kernel's own.
SCN_HD void actfault_restore(float raw, float scale, int e, int sd, int S, float* cache, float* stack, float* out) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float v = raw * scale;
  cache[e] = v;
  if (e < sd) { stack[e] = v; out[e] = v; }
  else out[S * sd + (e - sd)] = v;
}

}  // namespace cosim
