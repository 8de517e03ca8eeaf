// cosim_fault.h — what the fault tables of a scenario table share (cosim_set_param "obs_faults" / "action_faults", include/cosim.h):
// the item record, the operations and the walk of a row's items, as inline functions that the device kernels (cosim_obsfault.hip,
// cosim_actfault.hip) and plain host C++ programs (tests/obsfault_lanes.cpp, tests/actfault_lanes.cpp) both compile.  What a kind
// adds -- which clock, which words an element is, where they are loaded from and stored to -- is in cosim_obsfault.h / cosim_actfault.h.
//
// Scenario s owns the items [adr[s], adr[s + 1]).  An item is ONE 16-byte record of four 32-bit words
//   (t0, t1, el | op << 16 | ord << 24, value)
// (the array of records ends in FLT_CHUNK - 1 all-zero ones, so that a reader may fetch FLT_CHUNK records from any item on)
// and covers the episode clocks t0 <= t < t1.  el is an element of the kind (a frame element, an actuator), ord the ordinal of the
// listed item it was expanded from (0..255: all elements of one listed item share it).  The row is that of cosim_scenario.h.
//
// Per element under at least one item that holds: start from x, the word the kind hands in, and apply the holding items that name
// the element IN LISTED ORDER, composing, every operation with contraction off:
//   0 scale  x * value                         4 hold   the kind's previous word of the element
//   1 bias   x + value                         5 drop   as hold if (w' >> 8) * 2^-24 < value, one word w' per (env, step, item)
//   2 set    value                             6 clip   x > value ? value : (x < -value ? -value : x); NaN stays NaN (actions only)
//   3 noise  x + value * u,  u = (w >> 8) * 2^-23 - 1 in [-1, 1), w one Philox word
// Philox4x32-10, first output word, key (seed_lo, seed_hi), counter (c0, purpose | index << 8, gid_lo, gid_hi): purpose 7 for
// observations, 8 for actions; noise: index = el; drop: index = 0x10000 + ord (elements are below 256, so the ranges are disjoint).
// At clock 0 there is no previous word: hold and drop are the identity there.
//
// A MARKED item (bit FLT_MARK of el; elements are below 256) is one a limit search scales (cosim_search.h): the walk a search's
// kernel runs (fault_walk<true>) uses v = value * level for it, one float32 multiply, contraction off, done first, in the place of
// value -- drop compares its draw against v -- and the item's own rule runs next.  hold has no value and is never marked.  The
// unmarked items of the same row, and every item under fault_walk<false>, take the expressions above bit for bit.
#pragma once
#include "cosim_scenario.h"

namespace cosim {

enum { FLT_SCALE = 0, FLT_BIAS = 1, FLT_SET = 2, FLT_NOISE = 3, FLT_HOLD = 4, FLT_DROP = 5, FLT_CLIP = 6, FLT_NOP = 7 };
constexpr int FLT_MAX_ITEMS = 256;          // per scenario, expanded
constexpr unsigned FLT_DROP_INDEX = 0x10000u;
constexpr unsigned FLT_MARK = 0x8000u;      // of the el field: a limit search scales the item's value
constexpr int FLT_CHUNK = 4;                // item records fetched at a time; the item array is padded by FLT_CHUNK - 1 records

struct FaultTable {
  const int32_t* adr;    // [S + 1]
  const int32_t* item;   // [n + FLT_CHUNK - 1][4]: t0, t1, el | op << 16 | ord << 24, value (float bits); the padding is zeros
  int n_scn, n_items;
};

// the words of one env's draws
struct FaultKey {
  unsigned k0, k1, c0, g0, g1;   // Philox key, counter word 0 (meta[1] as the kind's kernel finds it) and the global env id
};

SCN_HD unsigned fault_philox(unsigned k0, unsigned k1, unsigned c0, unsigned c1, unsigned c2, unsigned c3) {
  for (int r = 0; r < 10; r++) {
    const unsigned long long p0 = 0xD2511F53ull * c0, p1 = 0xCD9E8D57ull * c2;
    const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n1 = (unsigned)p1, n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1, n3 = (unsigned)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  return c0;
}
SCN_HD unsigned fault_draw(const FaultKey& K, unsigned purpose, unsigned index) { return fault_philox(K.k0, K.k1, K.c0, purpose | (index << 8), K.g0, K.g1); }
SCN_HD float fault_bits(int32_t w) {
  float f;
  __builtin_memcpy(&f, &w, 4);
  return f;
}
// the two maps of a Philox word: both exact in fp32 (a 24-bit integer times a power of two, minus 1)
SCN_HD float fault_noise_u(unsigned w) { return (float)(w >> 8) * (1.0f / 8388608.0f) - 1.0f; }   // [-1, 1)
SCN_HD float fault_drop_u(unsigned w) { return (float)(w >> 8) * (1.0f / 16777216.0f); }          // [0, 1)

// One holding item on the word x of element el: `op` as fault_walk resolved it (never drop), prev the kind's previous word.  A kind
// whose validator admits no op above MAX_OP compiles no branch for one.
template <int MAX_OP>
SCN_HD float fault_op(float x, int op, float value, float prev, int el, unsigned purpose, const FaultKey& K) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  if (op == FLT_SCALE) return x * value;
  if (op == FLT_BIAS) return x + value;
  if (op == FLT_SET) return value;
  if (op == FLT_NOISE) {
    const float u = fault_noise_u(fault_draw(K, purpose, (unsigned)el));
    const float d = value * u;
    return x + d;
  }
  if (op == FLT_HOLD) return prev;
  if (MAX_OP >= FLT_CLIP && op == FLT_CLIP) return x > value ? value : (x < -value ? -value : x);
  return x;
}

// The items of row `row` at clock t, walked ONCE for the lane state L: L.load(first) at the first item that holds -- nothing of the
// env is loaded before it --, then L.item(el, op, value) per holding item in listed order, drop resolved to hold or nop with one
// draw for the item (its elements are lost together) and hold to nop at clock 0.  Returns whether any item held.
// Nothing here depends on the lane: the row is the same for every lane of an env, so on the device the records come through scalar
// loads and every branch up to L.item's compare of el is taken by the whole wave.
// MARKED: the walk of a search's kernel; `level` is the env's level, the same for the whole wave.
template <bool MARKED = false, class Lane>
SCN_HD bool fault_walk(const FaultTable& F, int row, int t, unsigned purpose, const FaultKey& K, Lane& L, float level = 1.f) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  SCN_TAB(int32_t) adr = SCN_TAB_CAST(int32_t, F.adr);
  SCN_TAB(int32_t) item = SCN_TAB_CAST(int32_t, F.item);
  const int i0 = adr[row], i1 = adr[row + 1];
  const bool first = t == 0;
  bool loaded = false;
  // FLT_CHUNK records, one 64-byte line, are fetched at a time, unconditionally (the array ends in FLT_CHUNK - 1 records that never
  // hold), so a row of n items costs ceil(n / FLT_CHUNK) trips to memory, not one per word read
  for (int c = i0; c < i1; c += FLT_CHUNK) {
    int32_t w[4 * FLT_CHUNK];
#pragma unroll
    for (int k = 0; k < 4 * FLT_CHUNK; k++) w[k] = item[4 * c + k];
#pragma unroll
    for (int j = 0; j < FLT_CHUNK; j++) {
      if (c + j >= i1) break;
      const int t0 = w[4 * j], t1 = w[4 * j + 1];
      if (!(t0 <= t && t < t1)) continue;
      const unsigned key = (unsigned)w[4 * j + 2];
      float value = fault_bits(w[4 * j + 3]);
      if (MARKED && (key & FLT_MARK)) value = value * level;
      const int el = (int)(key & (MARKED ? 0xffffu & ~FLT_MARK : 0xffffu)), ord = (int)(key >> 24);
      int op = (int)((key >> 16) & 0xffu);
      if (!loaded) {
        loaded = true;
        L.load(first);
      }
      if (op == FLT_DROP) op = fault_drop_u(fault_draw(K, purpose, FLT_DROP_INDEX + (unsigned)ord)) < value ? FLT_HOLD : FLT_NOP;
      if (op == FLT_HOLD && first) op = FLT_NOP;
      L.item(el, op, value);
    }
  }
  return loaded;
}

#if defined(__HIPCC__)
constexpr int FLT_WAVES = 4;   // envs per block of the fault kernels: one wave per env
// the env's clock (meta[0]), row (by meta[11]) and draw words (meta[1], the global env id) from the meta words of its record
__device__ __forceinline__ FaultKey fault_wave_key(const ScnTable& tab, const int* meta, int env, unsigned seed_lo, unsigned seed_hi, long long env_id0,
                                                   int* t, int* row) {
  *t = __builtin_amdgcn_readfirstlane(meta[0]);
  *row = scenario_row(tab, env, __builtin_amdgcn_readfirstlane(meta[11]));
  const unsigned long long gid = (unsigned long long)(env_id0 + env);
  return {seed_lo, seed_hi, (unsigned)__builtin_amdgcn_readfirstlane(meta[1]), (unsigned)gid, (unsigned)(gid >> 32)};
}
#endif

}  // namespace cosim
