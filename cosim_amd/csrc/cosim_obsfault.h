// cosim_obsfault.h — the per-env rule of a scenario table's observation faults (cosim_set_param "obs_faults", include/cosim.h), as
// inline functions that the device kernel (cosim_obsfault.hip) and a plain host C++ program (tests/obsfault_lanes.cpp) both compile.
// cosim_fault.h has the item record, the operations (0 scale .. 5 drop here) and the walk; this is what observations add.
//
// An item covers the observation clocks t0 <= t_obs < t1: t_obs = meta[0] as the step (or reset) that produced the observation left
// it, 0 for a reset's observation (a fill), k after the k-th step of the episode; the row is that of cosim_scenario.h on the
// post-step meta words, counter word 0 of the draws is meta[1] post-step, their purpose 7.  el is a frame element (the index space
// of el_field / el_index: e < stacked_dim is stacked).  x is the value the step kernel wrote for the newest frame, the previous word
// the element in the previous frame (stack row 1 after the roll).
// At t_obs == 0 every stack row holds the first frame: hold and drop are the identity there and the result goes to EVERY row; at
// t_obs > 0 it goes to row 0 of the record's stack and to the newest frame of state_out.  An element under no holding item is
// neither read nor written.  Nothing is kept per env: the faulted observation is a function of (state record, table).
#pragma once
#include "cosim_fault.h"

namespace cosim {

#define OBF_SETTER "cosim_set_param \"obs_faults\""   /* how the messages name the setter */
constexpr unsigned OBF_PURPOSE = 7u;        // of the Philox counter (cosim_amd/rng.py lists the others)
using ObsFaultTable = FaultTable;           // the names a caller that knows this kind alone uses (tests/obsfault_lanes.cpp)
constexpr int OBF_CHUNK = FLT_CHUNK;

// what the rule touches of one env
struct ObsFaultEnv : FaultKey {
  float* stack;   // the record's observation stack [stack_size][stacked_dim], newest row first
  float* out;     // the env's state_out row [stack_size * stacked_dim + non_stacked_dim]
  int sd, S, frame_dim;
};

// the NP words of a lane, held in registers through the walk: the elements lane + lanes * (pass0 + p), p < NP, below frame_dim
template <int NP>
struct ObsFaultLane {
  const ObsFaultEnv& E;
  int lane, lanes, pass0;
  float x[NP], prev[NP];
  bool hit[NP];

  SCN_HD void load(bool fill) {
#pragma unroll
    for (int p = 0; p < NP; p++) {
      const int e = lane + lanes * (pass0 + p);
      if (e >= E.frame_dim) continue;
      x[p] = e < E.sd ? E.stack[e] : E.out[E.S * E.sd + (e - E.sd)];
      if (e < E.sd && E.S >= 2 && !fill) prev[p] = E.stack[E.sd + e];
    }
  }
  SCN_HD void item(int el, int op, float value) {
#pragma unroll
    for (int p = 0; p < NP; p++) {
      const int e = lane + lanes * (pass0 + p);
      if (e != el || e >= E.frame_dim) continue;
      hit[p] = true;
      x[p] = fault_op<FLT_DROP>(x[p], op, value, prev[p], e, OBF_PURPOSE, E);
    }
  }
  SCN_HD void store(bool fill) const {
#pragma unroll
    for (int p = 0; p < NP; p++) {
      if (!hit[p]) continue;
      const int e = lane + lanes * (pass0 + p);
      if (e >= E.sd) { E.out[E.S * E.sd + (e - E.sd)] = x[p]; continue; }
      const int rows = fill ? E.S : 1;   // a fill left the first frame in every row
      for (int k = 0; k < rows; k++) { E.stack[k * E.sd + e] = x[p]; E.out[k * E.sd + e] = x[p]; }
    }
  }
};

// One env in row `row` at observation clock t, lane `lane` of `lanes`, NP passes from pass0 on.  (The kernel: lanes 64, pass0 0,
// NP = MAXFRAME / 64.)
// MARKED: under a limit search whose targets name the observation faults, the row's marked items (FLT_MARK, cosim_fault.h) use
// value * level; `level` is that of the episode the observation belongs to.
template <int NP, bool MARKED = false>
SCN_HD void obsfault_apply(const FaultTable& F, int row, int t, const ObsFaultEnv& E, int lane, int lanes, int pass0, float level = 1.f) {
  ObsFaultLane<NP> L = {E, lane, lanes, pass0, {}, {}, {}};
  if (fault_walk<MARKED>(F, row, t, OBF_PURPOSE, E, L, level)) L.store(t == 0);
}

}  // namespace cosim
