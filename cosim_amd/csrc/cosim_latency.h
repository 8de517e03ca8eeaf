// cosim_latency.h — the per-env rule of a scenario table's latency lines (cosim_set_param "latency", include/cosim.h): timed k-step
// delays of the command channel (policy -> drives) and of observation elements (sensor -> policy), as inline functions that the
// device kernels (cosim_latency.hip) and a plain host C++ program (tests/latency_lanes.cpp) both compile.
//
// Unlike a fault, a delay keeps something per env: a LINE of the channel's clean words of the last D clocks, [D][width] floats
// (width = nu for actions, frame_dim for observations), slot = clock mod D, and one header word `from`, the clock the line is valid
// from (below 0: invalid).  D is the table's largest steps + jitter, plus 1, so a word of clock t - k, k < D, is still in its slot
// when clock t is written.
//
// Scenario s owns the items [adr[s], adr[s + 1]) of a kind.  An item is ONE 16-byte record of four 32-bit words
//   (t0, t1, el | ord << 16, steps | jitter << 8)
// and covers the clocks t0 <= t < t1: the pre-step episode clock for actions (el an actuator), the observation's own clock for
// observations (el a frame element), as for the faults (cosim_actfault.h, cosim_obsfault.h).  ord is the ordinal of the listed item
// it was expanded from; all elements of a listed item share one jitter draw.
//
// Per env whose row lists at least one item of the kind, at every clock t, inside and outside the windows:
//   from  = t if t == 0 or from is invalid (a host cut invalidated it), else from
//   line[t mod D][el] = the element's CLEAN word, every element
//   per element, the LAST listed item that holds gives k = steps + j, j = ((w >> 8) * (jitter + 1)) >> 24 in 0..jitter, w the first
//   Philox word of purpose 9, index ord, counter word 0 and env id as the fault kernels take them at the same site (jitter 0: no
//   draw); k == 0 or no item: the element's own bits; else with c = t - k
//     c >= from                 line[c mod D][el]
//     c <  from, observations   line[from mod D][el]: the channel is full of its first reading
//     c <  from, actions        0.0f if from == 0 (nothing has arrived yet: what s_lastact holds after a reset), else line[from mod D][el]
// An env whose row lists no item of the kind neither reads nor writes its line or header.
#pragma once
#include "cosim_fault.h"

namespace cosim {

#define LAT_SETTER "cosim_set_param \"latency\""   /* how the messages name the setter */
constexpr unsigned LAT_PURPOSE = 9u;        // of the Philox counter (cosim_amd/rng.py lists the others)
constexpr int LAT_MAX_ITEMS = 256;          // per scenario and kind, expanded
constexpr int LAT_MAX_DELAY = 63;           // steps + jitter: the line depth stays <= 64 and the jitter map inside 32 bits
constexpr int LAT_MAX_ORD = 65535;

struct LatTable {
  const int32_t* act_adr;    // [S + 1]
  const int32_t* obs_adr;    // [S + 1]
  const int32_t* act_item;   // [n_act][4]: t0, t1, actuator | ord << 16, steps | jitter << 8
  const int32_t* obs_item;   // [n_obs][4]: the same with a frame element
  int n_scn, n_act, n_obs;
  int depth;                 // D of both kinds' lines
};

// 0..jitter from a Philox word: a 24-bit integer times at most 64, shifted back: exact
SCN_HD int latency_jitter(unsigned w, int jitter) { return (int)(((w >> 8) * (unsigned)(jitter + 1)) >> 24); }
// the slot of a clock (>= 0; the kernels hand in nothing else) in a line of depth D >= 1
SCN_HD int latency_slot(int clock, int depth) { return (int)((unsigned)(clock < 0 ? 0 : clock) % (unsigned)depth); }
// the clock the line is valid from once clock t is written
SCN_HD int latency_from(int from, int t) { return (t == 0 || from < 0 || from > t) ? t : from; }

// The items of row `row` of one kind at clock t, walked ONCE for the NP elements lane + lanes * p of a lane: k[p] becomes the delay
// of that element, 0 where no item holds.  Returns whether the row lists any item of the kind (holding or not): the env keeps a line.
// Nothing but the compare of el depends on the lane: on the device the records come through scalar loads and the draw is the wave's.
template <int NP>
SCN_HD bool latency_walk(const int32_t* adr_, const int32_t* item_, int row, int t, int depth, const FaultKey& K, int lane, int lanes, int (&k)[NP]) {
  SCN_TAB(int32_t) adr = SCN_TAB_CAST(int32_t, adr_);
  SCN_TAB(int32_t) item = SCN_TAB_CAST(int32_t, item_);
  const int i0 = adr[row], i1 = adr[row + 1];
#pragma unroll
  for (int p = 0; p < NP; p++) k[p] = 0;
  int last_ord = -1, kk = 0;   // the elements of one listed item lie one behind the other and share the delay
  for (int i = i0; i < i1; i++) {
    const int t0 = item[4 * i], t1 = item[4 * i + 1];
    if (!(t0 <= t && t < t1)) continue;
    const unsigned key = (unsigned)item[4 * i + 2], d = (unsigned)item[4 * i + 3];
    const int el = (int)(key & 0xffffu), ord = (int)(key >> 16);
    if (ord != last_ord) {
      const int steps = (int)(d & 0xffu), jitter = (int)((d >> 8) & 0xffu);
      kk = steps + (jitter > 0 ? latency_jitter(fault_draw(K, LAT_PURPOSE, (unsigned)ord), jitter) : 0);
      kk = kk > depth - 1 ? depth - 1 : kk;   // (the validator guarantees it)
      last_ord = ord;
    }
#pragma unroll
    for (int p = 0; p < NP; p++)
      if (lane + lanes * p == el) k[p] = kk;
  }
  return i1 > i0;
}

// Actuator j of one env at pre-step clock t: writes the caller's word x to the line and returns the delivered word.  `line` is the
// env's [D][nu], `from` the header as latency_from left it.
SCN_HD float latency_act_word(float* line, int depth, int nu, int j, int t, int from, int k, float x) {
  line[(size_t)latency_slot(t, depth) * nu + j] = x;
  if (k == 0) return x;
  const int c = t - k;
  if (c >= from) return line[(size_t)latency_slot(c, depth) * nu + j];
  if (from == 0) return 0.0f;
  return line[(size_t)latency_slot(from, depth) * nu + j];
}

// Frame element e of one env at observation clock t: writes the clean word x to the line and returns the delivered word.  `line` is
// the env's [D][frame_dim].
SCN_HD float latency_obs_word(float* line, int depth, int frame_dim, int e, int t, int from, int k, float x) {
  line[(size_t)latency_slot(t, depth) * frame_dim + e] = x;
  if (k == 0) return x;
  const int c = t - k;
  return line[(size_t)latency_slot(c >= from ? c : from, depth) * frame_dim + e];
}

}  // namespace cosim
