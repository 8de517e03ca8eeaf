// cosim_actfault.h — the per-env rule of a scenario table's action faults (cosim_set_param "action_faults", include/cosim.h), as
// inline functions that the device kernels (cosim_actfault.hip) and a plain host C++ program (tests/actfault_lanes.cpp) both compile.
// cosim_fault.h has the item record, the operations (0 scale .. 6 clip here) and the walk; this is what actions add.
//
// An item covers the PRE-STEP episode clocks t0 <= t < t1: t = meta[0] as the step finds it, the clock keyframes, pushes and
// parameter windows use; the row is that of cosim_scenario.h on the pre-step meta words, counter word 0 of the draws is meta[1]
// pre-step, their purpose 8.  el is an actuator (j < nu <= 64).  x is the caller's action word (the policy's raw output, before
// a_scale), the previous word rec[s_lastact + j]: the action the step kernel was given one step earlier, the EFFECTIVE one, so a
// held channel stays frozen through the window.
// At t == 0 the record holds no previous action: hold and drop are the identity there.  An actuator under no holding item gets the
// caller's bits.  Nothing is kept per env: the effective action is a function of (state record, table, caller's action).
#pragma once
#include "cosim_fault.h"

namespace cosim {

#define ACF_SETTER "cosim_set_param \"action_faults\""   /* how the messages name the setter */
constexpr unsigned ACF_PURPOSE = 8u;        // of the Philox counter (cosim_amd/rng.py lists the others)
using ActFaultTable = FaultTable;           // the names a caller that knows this kind alone uses (tests/actfault_lanes.cpp)
constexpr int ACF_CHUNK = FLT_CHUNK;

// what the rule reads of one env besides the caller's action
struct ActFaultEnv : FaultKey {
  const float* lastact;          // rec + s_lastact: [nu], the previous step's effective action (zeros after a reset)
};

// the one word of a lane: actuator j
struct ActFaultLane {
  const ActFaultEnv& E;
  int j;
  float x, prev;

  SCN_HD void load(bool first) {
    if (!first) prev = E.lastact[j];
  }
  SCN_HD void item(int el, int op, float value) {
    if (el == j) x = fault_op<FLT_CLIP>(x, op, value, prev, j, ACF_PURPOSE, E);
  }
};

// Actuator j of one env in row `row` at pre-step clock t: the effective action word from the caller's word x.  An env under no
// holding item reads nothing of its record here and returns x's bits.
SCN_HD float actfault_apply(const FaultTable& F, int row, int t, const ActFaultEnv& E, int j, float x) {
  ActFaultLane L = {E, j, x, 0.f};
  fault_walk(F, row, t, ACF_PURPOSE, E, L);
  return L.x;
}

// actfault_apply under a limit search whose targets name the action faults: the row's marked items (FLT_MARK, cosim_fault.h) use
// value * level, `level` being the level the env's open episode runs at (the search's record word 0); the others are as above.
SCN_HD float actfault_apply_scaled(const FaultTable& F, int row, int t, const ActFaultEnv& E, int j, float x, float level) {
  ActFaultLane L = {E, j, x, 0.f};
  fault_walk<true>(F, row, t, ACF_PURPOSE, E, L, level);
  return L.x;
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
