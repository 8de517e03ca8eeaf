// cosim_scnparams.h — the per-env rule of a scenario table's parameter windows (cosim_scenario_params_set, include/cosim.h), as
// inline functions that the device kernel (cosim_scnparams.hip) and a plain host C++ program (tests/scnparams_lanes.cpp) both compile.
//
// Scenario s owns the items [adr[s], adr[s + 1]): item i covers the episode steps t[2i] <= t < t[2i + 1] and names ONE 32-bit word
// word[i] of the env's parameter record (field offset + index, resolved on the host), an op[i] and a value[i].  Per env and control
// step, with the clock t and the row of cosim_scenario.h:
//   eff[w] = base[w] * value (op 0, "scale": one fp32 multiply)  |  value (op 1, "set")
// for the last LISTED item of the row that names w and holds at t; a word no item holds is the base word, bit for bit.  The whole
// record is written every time: nothing is kept per env, the effective record is a function of (base record, state record, table).
//
// A MARKED item (bit SCNPAR_MARK of its op word, above the op values) is one a limit search scales (cosim_search.h): the form a
// search's kernel runs (marked = true) uses v = value * level for it, one float32 multiply, contraction off, done first, so scale
// becomes base * v and set becomes v.  Unmarked items of the same row, and every item with marked = false, take the expressions above.
#pragma once
#include "cosim_scenario.h"

namespace cosim {

enum { SCNPAR_SCALE = 0, SCNPAR_SET = 1 };
constexpr int SCNPAR_MARK = 0x100, SCNPAR_OP_MASK = 0xff;
// fields of an item as the C ABI numbers them; 4 .. 7 are named only to be refused with a reason
enum { SCNPAR_KP = 0, SCNPAR_KD = 1, SCNPAR_GEOM_FRICTION = 2, SCNPAR_DOF_FRICTIONLOSS = 3, SCNPAR_BODY_MASS = 4, SCNPAR_BODY_INVWEIGHT0 = 5,
       SCNPAR_DOF_INVWEIGHT0 = 6, SCNPAR_MEANINERTIA = 7 };
constexpr int SCNPAR_MAX_ITEMS = 256;

struct ScnParTable {
  const int32_t* adr;     // [S + 1]
  const int32_t* t;       // [n][2]
  const int32_t* word;    // [n] word of the parameter record
  const int32_t* op;      // [n]
  const float* value;     // [n]
  int n_scn, n_items;
};

// Word w of the effective record of an env in row `row` at episode step t.
SCN_HD float scnparams_word(const ScnParTable& P, int row, int t, int w, float base, bool marked = false, float level = 1.f) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  SCN_TAB(int32_t) adr = SCN_TAB_CAST(int32_t, P.adr);
  SCN_TAB(int32_t) tt = SCN_TAB_CAST(int32_t, P.t);
  SCN_TAB(int32_t) word = SCN_TAB_CAST(int32_t, P.word);
  SCN_TAB(int32_t) op = SCN_TAB_CAST(int32_t, P.op);
  SCN_TAB(float) value = SCN_TAB_CAST(float, P.value);
  const int i0 = adr[row], i1 = adr[row + 1];
  float out = base;
  for (int i = i0; i < i1; i++) {   // the row is the same for every lane of an env: these loads do not depend on w
    const bool holds = tt[2 * i] <= t && t < tt[2 * i + 1];
    if (!(holds && word[i] == w)) continue;
    if (!marked) { out = op[i] == SCNPAR_SET ? value[i] : base * value[i]; continue; }   // the last listed item wins
    const int o = op[i];
    float v = value[i];
    if (o & SCNPAR_MARK) v = v * level;
    out = (o & SCNPAR_OP_MASK) == SCNPAR_SET ? v : base * v;
  }
  return out;
}

// One env, one control step, lane `lane` of `lanes`: words lane, lane + lanes, ... < p_stride of eff (the last pass is a tail).
SCN_HD void scnparams_apply(const ScnParTable& P, int row, int t, const float* base, float* eff, int p_stride, int lane, int lanes, bool marked = false,
                            float level = 1.f) {
  for (int w = lane; w < p_stride; w += lanes) eff[w] = scnparams_word(P, row, t, w, base[w], marked, level);
}

}  // namespace cosim
