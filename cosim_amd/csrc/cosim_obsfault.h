// cosim_obsfault.h — the per-env rule of a scenario table's observation faults (cosim_set_param "obs_faults", include/cosim.h), as
// inline functions that the device kernel (cosim_obsfault.hip) and a plain host C++ program (tests/obsfault_lanes.cpp) both compile.
//
// Scenario s owns the items [adr[s], adr[s + 1]).  An item is ONE 16-byte record of four 32-bit words
//   (t0, t1, e | op << 16 | ord << 24, value)
// (the array of records ends in OBF_CHUNK - 1 all-zero ones, so that a reader may fetch OBF_CHUNK records from any item on)
// and covers the observation clocks t0 <= t_obs < t1: t_obs = meta[0] as the step (or reset) that produced the observation left it,
// 0 for a reset's observation (a fill), k after the k-th step of the episode.  e is a frame element (the index space of el_field /
// el_index: e < stacked_dim is stacked), ord the ordinal of the listed item it was expanded from (0..255: all elements of one listed
// item share it).  The row is that of cosim_scenario.h on the post-step meta words.
//
// Per element under at least one item that holds: start from x, the value the step kernel wrote for the newest frame, and apply the
// holding items that name the element IN LISTED ORDER, composing, every operation with contraction off:
//   0 scale  x * value                         3 noise  x + value * u,  u = (w >> 8) * 2^-23 - 1 in [-1, 1), w one Philox word
//   1 bias   x + value                         4 hold   the element in the previous frame (stack row 1 after the roll)
//   2 set    value                             5 drop   as hold if (w' >> 8) * 2^-24 < value, one word w' per (env, step, item)
// Philox4x32-10, first output word, key (seed_lo, seed_hi), counter (meta[1] post-step, 7 | index << 8, gid_lo, gid_hi): purpose 7;
// noise: index = e; drop: index = 0x10000 + ord (frame elements are below 256, so the ranges are disjoint).
// At t_obs == 0 every stack row holds the first frame: hold and drop are the identity there and the result goes to EVERY row; at
// t_obs > 0 it goes to row 0 of the record's stack and to the newest frame of state_out.  An element under no holding item is
// neither read nor written.  Nothing is kept per env: the faulted observation is a function of (state record, table).
#pragma once
#include "cosim_scenario.h"

namespace cosim {

enum { OBF_SCALE = 0, OBF_BIAS = 1, OBF_SET = 2, OBF_NOISE = 3, OBF_HOLD = 4, OBF_DROP = 5, OBF_NOP = 6 };
#define OBF_SETTER "cosim_set_param \"obs_faults\""   /* how the messages name the setter */
constexpr int OBF_MAX_ITEMS = 256;          // per scenario, expanded
constexpr unsigned OBF_PURPOSE = 7u;        // of the Philox counter (cosim_amd/rng.py lists the others)
constexpr unsigned OBF_DROP_INDEX = 0x10000u;
constexpr int OBF_CHUNK = 4;                // item records fetched at a time; the item array is padded by OBF_CHUNK - 1 records

struct ObsFaultTable {
  const int32_t* adr;    // [S + 1]
  const int32_t* item;   // [n + OBF_CHUNK - 1][4]: t0, t1, e | op << 16 | ord << 24, value (float bits); the padding is zeros
  int n_scn, n_items;
};

// what the rule touches of one env
struct ObsFaultEnv {
  float* stack;   // the record's observation stack [stack_size][stacked_dim], newest row first
  float* out;     // the env's state_out row [stack_size * stacked_dim + non_stacked_dim]
  int sd, S, frame_dim;
  unsigned k0, k1, c0, g0, g1;   // Philox key, counter word 0 (meta[1] post-step) and the global env id
};

SCN_HD unsigned obsfault_philox(unsigned k0, unsigned k1, unsigned c0, unsigned c1, unsigned c2, unsigned c3) {
  for (int r = 0; r < 10; r++) {
    const unsigned long long p0 = 0xD2511F53ull * c0, p1 = 0xCD9E8D57ull * c2;
    const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n1 = (unsigned)p1, n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1, n3 = (unsigned)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  return c0;
}
SCN_HD float obsfault_bits(int32_t w) {
  float f;
  __builtin_memcpy(&f, &w, 4);
  return f;
}
// the two maps of a Philox word: both exact in fp32 (a 24-bit integer times a power of two, minus 1)
SCN_HD float obsfault_noise_u(unsigned w) { return (float)(w >> 8) * (1.0f / 8388608.0f) - 1.0f; }   // [-1, 1)
SCN_HD float obsfault_drop_u(unsigned w) { return (float)(w >> 8) * (1.0f / 16777216.0f); }          // [0, 1)

// One env in row `row` at observation clock t, lane `lane` of `lanes`: the elements lane + lanes * (pass0 + p), p < NP, below
// frame_dim.  The row's items are walked ONCE with the NP words of the lane held in registers; nothing of the env is loaded before
// the first item that holds.  (The kernel: lanes 64, pass0 0, NP = MAXFRAME / 64.)
template <int NP>
SCN_HD void obsfault_apply(const ObsFaultTable& F, int row, int t, const ObsFaultEnv& E, int lane, int lanes, int pass0) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  SCN_TAB(int32_t) adr = SCN_TAB_CAST(int32_t, F.adr);
  SCN_TAB(int32_t) item = SCN_TAB_CAST(int32_t, F.item);
  const int i0 = adr[row], i1 = adr[row + 1];
  const bool fill = t == 0;
  float x[NP], prev[NP];
  bool hit[NP];
#pragma unroll
  for (int p = 0; p < NP; p++) { x[p] = 0.f; prev[p] = 0.f; hit[p] = false; }
  bool loaded = false;
  // the row is the same for every lane of an env: these loads do not depend on the lane.  OBF_CHUNK records, one 64-byte line, are
  // fetched at a time, unconditionally (the array ends in OBF_CHUNK - 1 records that never hold), so a row of n items costs
  // ceil(n / OBF_CHUNK) trips to memory, not one per word read
  for (int c = i0; c < i1; c += OBF_CHUNK) {
    int32_t w[4 * OBF_CHUNK];
#pragma unroll
    for (int k = 0; k < 4 * OBF_CHUNK; k++) w[k] = item[4 * c + k];
#pragma unroll
    for (int j = 0; j < OBF_CHUNK; j++) {
      if (c + j >= i1) break;
      const int t0 = w[4 * j], t1 = w[4 * j + 1];
      if (!(t0 <= t && t < t1)) continue;
      const unsigned key = (unsigned)w[4 * j + 2];
      const float value = obsfault_bits(w[4 * j + 3]);
      const int el = (int)(key & 0xffffu), ord = (int)(key >> 24);
      int op = (int)((key >> 16) & 0xffu);
      if (!loaded) {
        loaded = true;
#pragma unroll
        for (int p = 0; p < NP; p++) {
          const int e = lane + lanes * (pass0 + p);
          if (e >= E.frame_dim) continue;
          x[p] = e < E.sd ? E.stack[e] : E.out[E.S * E.sd + (e - E.sd)];
          if (e < E.sd && E.S >= 2 && !fill) prev[p] = E.stack[E.sd + e];
        }
      }
      if (op == OBF_DROP) {   // one draw for the item: its elements are lost together
        const unsigned draw = obsfault_philox(E.k0, E.k1, E.c0, OBF_PURPOSE | ((OBF_DROP_INDEX + (unsigned)ord) << 8), E.g0, E.g1);
        op = obsfault_drop_u(draw) < value ? OBF_HOLD : OBF_NOP;
      }
      if (op == OBF_HOLD && fill) op = OBF_NOP;
#pragma unroll
      for (int p = 0; p < NP; p++) {
        const int e = lane + lanes * (pass0 + p);
        if (e != el || e >= E.frame_dim) continue;
        hit[p] = true;
        if (op == OBF_SCALE) x[p] = x[p] * value;
        else if (op == OBF_BIAS) x[p] = x[p] + value;
        else if (op == OBF_SET) x[p] = value;
        else if (op == OBF_NOISE) {
          const float u = obsfault_noise_u(obsfault_philox(E.k0, E.k1, E.c0, OBF_PURPOSE | ((unsigned)e << 8), E.g0, E.g1));
          const float d = value * u;
          x[p] = x[p] + d;
        } else if (op == OBF_HOLD) x[p] = prev[p];
      }
    }
  }
  if (!loaded) return;
#pragma unroll
  for (int p = 0; p < NP; p++) {
    if (!hit[p]) continue;
    const int e = lane + lanes * (pass0 + p);
    if (e >= E.sd) { E.out[E.S * E.sd + (e - E.sd)] = x[p]; continue; }
    const int rows = fill ? E.S : 1;   // a fill left the first frame in every row
    for (int k = 0; k < rows; k++) { E.stack[k * E.sd + e] = x[p]; E.out[k * E.sd + e] = x[p]; }
  }
}

}  // namespace cosim
