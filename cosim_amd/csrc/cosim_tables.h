// cosim_tables.h — what the host does with a table of the scenario family before it reaches the device (cosim_scenario_set,
// cosim_scenario_params_set, cosim_set_param "obs_faults" / "action_faults" / "search", cosim_scenario_checks_set, cosim_scenario_curves_set, include/cosim.h): the rules every such table is
// held to, one validator per setter, and the packer that lays a table's arrays into one allocation.  Plain C++ with no HIP in it:
// cosim_engine.hip and a host program (tests/tables_host.cpp) both compile it.
//
// A validator takes the caller's raw arrays and what it needs to know of the engine (TableDims); it returns the refusal as
// cosim_last_error words it (empty: the table is good) and the values the setter derives from the table.  Where a table has several
// faults the first one in the order of the code below is reported: a row's addresses, then its items, one row after the other.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <string>
#include <vector>

#include "cosim_actfault.h"
#include "cosim_curves.h"
#include "cosim_latency.h"
#include "cosim_obsfault.h"
#include "cosim_scnparams.h"
#include "cosim_search.h"

namespace cosim {

struct TableDims {
  int nq, nv, nu, ngeom, info_dim, command_dim;
  int p_kp, p_kd, p_gmu, p_floss;   // offsets in the parameter record
};

// ---- the shared rules; each returns the refusal, empty if there is none
// what an id selects: the name the messages use, how many entries it has, and (parameter fields) where they lie in the record
struct TabEntry { const char* name; int width, off; };
// "0 info, 1 abs_info, ..."
inline std::string tab_id_list(const TabEntry* e, int n) {
  std::string s;
  for (int k = 0; k < n; k++) s += (k ? ", " : "") + std::to_string(k) + " " + e[k].name;
  return s;
}
inline std::string index_rule(const std::string& row, int index, const TabEntry& e) {
  if (index >= 0 && index < e.width) return "";
  return row + ": index " + std::to_string(index) + " out of range: " + e.name + " has " + std::to_string(e.width) + " entries";
}

// One CSR row-address array and the items it addresses.
struct RowAdr {
  const char* name;     // of the array in the messages
  const int32_t* adr;   // [S + 1]
  const char* noun;     // of its items in the messages
  int cap;              // most items a row may hold
  bool arrays;          // the item arrays are all there
};
// the address arrays as a whole: all there, each beginning at 0
template <size_t NR>
inline std::string row_heads(const std::string& fn, const RowAdr (&rows)[NR]) {
  std::string names;
  bool zero = true;
  for (const RowAdr& r : rows) {
    if (!r.adr) return fn + ": null argument";
    zero = zero && r.adr[0] == 0;
    names += (names.empty() ? "" : " and ") + std::string(r.name) + "[0]";
  }
  return zero ? "" : fn + ": " + names + " must be 0";
}
// row s of them (who: "<function>: scenario <s>"): non-decreasing, within the cap, and no items without their arrays
template <size_t NR>
inline std::string row_rule(const std::string& who, const RowAdr (&rows)[NR], int s) {
  for (const RowAdr& r : rows)
    if (r.adr[s + 1] < r.adr[s]) return who + ": row addresses must not decrease";
  for (const RowAdr& r : rows) {
    const long long ni = (long long)r.adr[s + 1] - r.adr[s];
    if (ni > r.cap) return who + ": " + std::to_string(ni) + " " + r.noun + ", at most " + std::to_string(r.cap);
  }
  for (const RowAdr& r : rows)
    if (r.adr[s + 1] > r.adr[s] && !r.arrays) return who + ": null table array";
  return "";
}

// a window [t0, t1) of episode steps
inline std::string window_rule(const std::string& row, int t0, int t1) {
  if (t0 < 0 || t0 >= SCN_MAX_TIME || t1 < 0 || t1 > SCN_MAX_TIME) return row + ": times outside [0, 2^30)";
  if (t1 <= t0) return row + ": t1 " + std::to_string(t1) + " is not after t0 " + std::to_string(t0);
  return "";
}

// the signals of checks and curves (checks_signal, cosim_checks.h)
inline std::string signal_rule(const std::string& row, const TableDims& d, int signal, int index) {
  const int ncmd = d.command_dim < 3 ? d.command_dim : 3;
  const TabEntry sig[CHK_NSIGNAL] = {{"info", d.info_dim, 0}, {"abs_info", d.info_dim, 0}, {"tracking_error", ncmd, 0}, {"torque_max", 1, 0},
                                     {"up", d.nq >= 7 ? 1 : 0, 0}, {"qpos", d.nq, 0}, {"qvel", d.nv, 0}, {"abs_qvel", d.nv, 0}};
  if (signal < 0 || signal >= CHK_NSIGNAL) return row + ": unknown signal " + std::to_string(signal) + " (" + tab_id_list(sig, CHK_NSIGNAL) + ")";
  return index_rule(row, index, sig[signal]);
}

// the fields of a parameter window; *word: the word of the parameter record that field + index name
inline std::string field_rule(const std::string& row, const TableDims& d, int field, int index, int32_t* word) {
  const TabEntry fld[4] = {{"kp", d.nu, d.p_kp}, {"kd", d.nu, d.p_kd}, {"geom_friction", d.ngeom, d.p_gmu}, {"dof_frictionloss", d.nv, d.p_floss}};
  if (field >= SCNPAR_BODY_MASS && field <= SCNPAR_MEANINERTIA)
    return row + ": field " + std::to_string(field) + " (body_mass, body_invweight0, dof_invweight0, meaninertia) is refused: the mass "
           "fields are consistent only as a set computed on the host in fp64; a payload change in mid-episode is out of scope";
  if (field < 0 || field >= 4) return row + ": unknown field " + std::to_string(field) + " (" + tab_id_list(fld, 4) + ")";
  *word = fld[field].off + index;
  return index_rule(row, index, fld[field]);
}

// ---- the packer: the 4-byte arrays of a table, one behind the other in one allocation
class WordPacker {
 public:
  // the next array of the image: n words from src; patch() will point *slot at them
  template <class T>
  void add(const T** slot, const T* src, size_t n) {
    static_assert(sizeof(T) == 4, "arrays of 4-byte words");
    arr_.push_back({slot, img_.size(), n});
    img_.resize(img_.size() + n, 0);
    if (n > 0) memcpy(&img_[arr_.back().off], src, n * 4);
  }
  const int32_t* data() const { return img_.data(); }
  size_t words() const { return img_.size(); }
  size_t bytes() const { return img_.size() * 4; }
  // the table's pointers, once the address the image lies at (or will be copied to) is known
  void patch(const void* base) const {
    for (const Arr& a : arr_) {
      const int32_t* p = static_cast<const int32_t*>(base) + a.off;
      memcpy(a.slot, &p, sizeof p);
    }
  }
  // whether the array behind `slot` holds the words it holds in `old`, an image of the same arrays with the same sizes
  bool same(const void* slot, const int32_t* old) const {
    for (const Arr& a : arr_)
      if (a.slot == slot) return a.n == 0 || memcmp(&img_[a.off], old + a.off, a.n * 4) == 0;
    return false;
  }

 private:
  struct Arr { void* slot; size_t off, n; };
  std::vector<Arr> arr_;
  std::vector<int32_t> img_;
};

#define TAB_TRY(expr) do { v.err = (expr); if (!v.err.empty()) return v; } while (0)

// ---- cosim_scenario_set.  Image: key_adr | push_adr | key_t | push_t | key_cmd | push_v
struct ScnRaw {
  int n_scn;   // 1 .. SCN_MAX_ROWS (the setter has checked)
  const int32_t *key_adr, *key_t; const float* key_cmd;
  const int32_t *push_adr, *push_t; const float* push_v;
};
struct ScnShape { std::string err; int nkey = 0, npush = 0; };

inline ScnShape validate_scenario(const TableDims& d, const ScnRaw& r) {
  const std::string fn = "cosim_scenario_set";
  const int cd = d.command_dim;
  ScnShape v;
  const RowAdr rows[2] = {{"key_adr", r.key_adr, "keyframes", SCN_MAX_ITEMS, r.key_t && (cd == 0 || r.key_cmd)},
                          {"push_adr", r.push_adr, "push windows", SCN_MAX_ITEMS, r.push_t && r.push_v}};
  TAB_TRY(row_heads(fn, rows));
  for (int s = 0; s < r.n_scn; s++) {
    const std::string who = fn + ": scenario " + std::to_string(s);
    TAB_TRY(row_rule(who, rows, s));
    for (int k = r.key_adr[s]; k < r.key_adr[s + 1]; k++) {
      const std::string row = who + ", keyframe " + std::to_string(k - r.key_adr[s]);
      const int t = r.key_t[k];
      if (t < 0 || t >= SCN_MAX_TIME) TAB_TRY(row + ": time " + std::to_string(t) + " outside [0, 2^30)");
      if (k > r.key_adr[s] && t <= r.key_t[k - 1])
        TAB_TRY(row + ": time " + std::to_string(t) + " does not increase (previous " + std::to_string(r.key_t[k - 1]) + ")");
      for (int c = 0; c < cd; c++)
        if (!std::isfinite(r.key_cmd[(size_t)k * cd + c])) TAB_TRY(row + ": command " + std::to_string(c) + " is not finite");
    }
    for (int p = r.push_adr[s]; p < r.push_adr[s + 1]; p++) {
      const std::string row = who + ", push window " + std::to_string(p - r.push_adr[s]);
      TAB_TRY(window_rule(row, r.push_t[2 * p], r.push_t[2 * p + 1]));
      for (int c = 0; c < 3; c++)
        if (!std::isfinite(r.push_v[3 * (size_t)p + c])) TAB_TRY(row + ": velocity " + std::to_string(c) + " is not finite");
    }
  }
  v.nkey = r.key_adr[r.n_scn]; v.npush = r.push_adr[r.n_scn];
  return v;
}

inline void pack_scenario(WordPacker& pk, ScnTable& tab, int cd, const ScnRaw& r, const ScnShape& v) {
  const size_t S1 = (size_t)r.n_scn + 1, nk = (size_t)v.nkey, np = (size_t)v.npush;
  pk.add(&tab.key_adr, r.key_adr, S1); pk.add(&tab.push_adr, r.push_adr, S1); pk.add(&tab.key_t, r.key_t, nk); pk.add(&tab.push_t, r.push_t, 2 * np);
  pk.add(&tab.key_cmd, r.key_cmd, nk * cd); pk.add(&tab.push_v, r.push_v, 3 * np);
  tab.n_scn = r.n_scn; tab.cd = cd;
}

// ---- cosim_scenario_params_set.  Image: adr | t | word | op | value
struct ParRaw {
  int n_scn;   // that of the scenario table that is set
  const int32_t *adr, *t, *field, *index, *op; const float* value;
};
struct ParShape { std::string err; int n = 0, marked = 0; std::vector<int32_t> word; };   // marked: items a limit search scales
// The limit search that is armed, as a marked item (SCNPAR_MARK of an op word, FLT_MARK of a fault's elem) is held against it: `bit` is
// the kind's SRCH_* target.  Null where no search is armed: a marked item is refused then.
struct FltMarks { int bit; const int32_t *has, *targets; const float *lo, *hi; };

inline ParShape validate_params(const TableDims& d, const ParRaw& r, const FltMarks* marks = nullptr) {
  const std::string fn = "cosim_scenario_params_set";
  ParShape v;
  const RowAdr rows[1] = {{"adr", r.adr, "parameter items", SCNPAR_MAX_ITEMS, r.t && r.field && r.index && r.op && r.value}};
  TAB_TRY(row_heads(fn, rows));
  for (int s = 0; s < r.n_scn; s++) {
    const std::string who = fn + ": scenario " + std::to_string(s);
    TAB_TRY(row_rule(who, rows, s));
    for (int i = r.adr[s]; i < r.adr[s + 1]; i++) {
      const std::string row = who + ", parameter item " + std::to_string(i - r.adr[s]);
      int32_t word = 0;
      TAB_TRY(window_rule(row, r.t[2 * i], r.t[2 * i + 1]));
      TAB_TRY(field_rule(row, d, r.field[i], r.index[i], &word));
      const bool mark = r.op[i] >= 0 && (r.op[i] & SCNPAR_MARK) != 0;
      const int op = mark ? (r.op[i] & ~SCNPAR_MARK) : r.op[i];
      if (op != SCNPAR_SCALE && op != SCNPAR_SET) TAB_TRY(row + ": unknown op " + std::to_string(r.op[i]) + " (0 scale, 1 set)");
      if (!std::isfinite(r.value[i])) TAB_TRY(row + ": value is not finite");
      if (mark) {
        if (!marks || !marks->has[s] || !(marks->targets[s] & marks->bit))
          TAB_TRY(row + ": the item is marked for a limit search and no search whose targets name the parameter windows is armed on the scenario (cosim_set_param \"search\" first)");
        if (!std::isfinite(r.value[i] * marks->lo[s]) || !std::isfinite(r.value[i] * marks->hi[s])) TAB_TRY(row + ": value * level is not finite at an end of the search's range");
        v.marked++;
      }
      v.word.push_back(word);
    }
  }
  v.n = r.adr[r.n_scn];
  if (v.n == 0) TAB_TRY(fn + ": the table holds no parameter item (n_scn = 0 clears the windows)");
  return v;
}

inline void pack_params(WordPacker& pk, ScnParTable& tab, const ParRaw& r, const ParShape& v) {
  const size_t n = (size_t)v.n;
  pk.add(&tab.adr, r.adr, (size_t)r.n_scn + 1); pk.add(&tab.t, r.t, 2 * n); pk.add(&tab.word, v.word.data(), n); pk.add(&tab.op, r.op, n);
  pk.add(&tab.value, r.value, n);
  tab.n_scn = r.n_scn; tab.n_items = v.n;
}

// ---- cosim_set_param "obs_faults" / "action_faults".  Image: adr | item ([n + FLT_CHUNK - 1][4]: t0, t1, el | op << 16 | ord << 24, value: cosim_fault.h)
struct FltRaw {
  int n_scn;   // that of the scenario table that is set
  const int32_t *adr, *t, *elem, *op, *ord; const float* value;
};
struct FltShape { std::string err; int n = 0, marked = 0; std::vector<int32_t> item; };   // marked: items a limit search scales
// what the two kinds differ in besides their rules: how the messages name the setter and an item, the highest op and the list an unknown one is answered with
struct FltKind { const char *setter, *noun; int max_op; const char* ops; };

// The rules of both kinds, in the order they are reported in.  elem_rule(row, el) is the kind's word on an element, ahead of the op;
// op_rule(row, el, op, value) its word on an op the shared rules have passed, behind them.
template <class ElemRule, class OpRule>
inline FltShape validate_fault_items(const FltKind& kind, const FltRaw& r, ElemRule elem_rule, OpRule op_rule, const FltMarks* marks = nullptr) {
  const std::string fn = kind.setter, noun = kind.noun, nouns = noun + "s";
  FltShape v;
  const RowAdr rows[1] = {{"adr", r.adr, nouns.c_str(), FLT_MAX_ITEMS, r.t && r.elem && r.op && r.ord && r.value}};
  TAB_TRY(row_heads(fn, rows));
  // all rows first: the item arrays hold adr[S] items (the setter sized them so), and 0 = adr[0] <= ... <= adr[S] keeps every row inside
  for (int s = 0; s < r.n_scn; s++) TAB_TRY(row_rule(fn + ": scenario " + std::to_string(s), rows, s));
  for (int s = 0; s < r.n_scn; s++) {
    const std::string who = fn + ": scenario " + std::to_string(s);
    for (int i = r.adr[s]; i < r.adr[s + 1]; i++) {
      const std::string row = who + ", " + noun + " " + std::to_string(i - r.adr[s]);
      const bool mark = r.elem[i] >= 0 && ((unsigned)r.elem[i] & FLT_MARK) != 0;
      const int el = mark ? (int)((unsigned)r.elem[i] & ~FLT_MARK) : r.elem[i], op = r.op[i];
      TAB_TRY(window_rule(row, r.t[2 * i], r.t[2 * i + 1]));
      if (mark && (!marks || !marks->has[s] || !(marks->targets[s] & marks->bit)))
        TAB_TRY(row + ": the item is marked for a limit search and no search whose targets name these items is armed on the scenario (cosim_set_param \"search\" first)");
      TAB_TRY(elem_rule(row, el));
      if (op < FLT_SCALE || op > kind.max_op) TAB_TRY(row + ": unknown op " + std::to_string(op) + " " + kind.ops);
      if (!std::isfinite(r.value[i])) TAB_TRY(row + ": value is not finite");
      if (op == FLT_NOISE && r.value[i] < 0.f) TAB_TRY(row + ": a noise amplitude must be >= 0");
      if (op == FLT_DROP && !(r.value[i] >= 0.f && r.value[i] <= 1.f)) TAB_TRY(row + ": a drop probability must lie in [0, 1]");
      TAB_TRY(op_rule(row, el, op, r.value[i]));
      if (mark) {   // the kind's value rule at both ends of the search's range, as the kernel computes them
        if (op == FLT_HOLD) TAB_TRY(row + ": a hold has no value and cannot be marked for a limit search");
        const float ends[2] = {r.value[i] * marks->lo[s], r.value[i] * marks->hi[s]};
        for (const float x : ends) {
          if (!std::isfinite(x)) TAB_TRY(row + ": value * level is not finite at an end of the search's range");
          if (op == FLT_NOISE && x < 0.f) TAB_TRY(row + ": a noise amplitude must be >= 0 at both ends of the search's range");
          if (op == FLT_DROP && !(x >= 0.f && x <= 1.f)) TAB_TRY(row + ": a drop probability must lie in [0, 1] at both ends of the search's range");
          TAB_TRY(op_rule(row, el, op, x));
        }
        v.marked++;
      }
      if (r.ord[i] < 0 || r.ord[i] >= FLT_MAX_ITEMS) TAB_TRY(row + ": ordinal " + std::to_string(r.ord[i]) + " outside 0..255");
      int32_t vb;
      memcpy(&vb, &r.value[i], 4);
      v.item.push_back(r.t[2 * i]); v.item.push_back(r.t[2 * i + 1]);
      v.item.push_back((int32_t)((unsigned)el | (mark ? FLT_MARK : 0u) | (unsigned)op << 16 | (unsigned)r.ord[i] << 24)); v.item.push_back(vb);
    }
  }
  v.n = r.adr[r.n_scn];
  if (v.n == 0) TAB_TRY(fn + ": the table holds no " + noun + " (n_scn = 0 clears the faults)");
  v.item.resize(v.item.size() + 4 * (FLT_CHUNK - 1), 0);   // records that never hold: the kernels fetch FLT_CHUNK at a time
  return v;
}

inline void pack_faults(WordPacker& pk, FaultTable& tab, const FltRaw& r, const FltShape& v) {
  pk.add(&tab.adr, r.adr, (size_t)r.n_scn + 1); pk.add(&tab.item, v.item.data(), v.item.size());
  tab.n_scn = r.n_scn; tab.n_items = v.n;
}

// observations: what a fault item is held against of the observation frame
struct ObsDims {
  int frame_dim, stacked_dim, stack_size;
  const unsigned char* el_field;   // [frame_dim] CS_OBS_* of every frame element
  int command_field;               // CS_OBS_COMMAND
};
inline FltShape validate_faults(const ObsDims& d, const FltRaw& r, const FltMarks* marks = nullptr) {
  const auto elem_rule = [&d](const std::string& row, int e) {
    if (e < 0 || e >= d.frame_dim) return row + ": element " + std::to_string(e) + " out of range: the frame has " + std::to_string(d.frame_dim) + " elements";
    if (d.el_field[e] != d.command_field) return std::string();
    return row + ": element " + std::to_string(e) + " is a command word and is refused: the command words are the scenario's keyframes";
  };
  const auto op_rule = [&d](const std::string& row, int e, int op, float) {
    if ((op != FLT_HOLD && op != FLT_DROP) || (e < d.stacked_dim && d.stack_size >= 2)) return std::string();
    return row + ": hold / drop needs a stacked element and stack_size >= 2: there is no previous frame in the record";
  };
  return validate_fault_items({OBF_SETTER, "fault item", FLT_DROP, "(0 scale, 1 bias, 2 set, 3 noise, 4 hold, 5 drop)"}, r, elem_rule, op_rule, marks);
}

// actions: `elem` is an actuator index
inline FltShape validate_action_faults(int nu, const FltRaw& r, const FltMarks* marks = nullptr) {
  const auto elem_rule = [nu](const std::string& row, int j) {
    return j >= 0 && j < nu ? std::string() : row + ": actuator " + std::to_string(j) + " out of range: the model has " + std::to_string(nu) + " actuators";
  };
  const auto op_rule = [](const std::string& row, int, int op, float value) { return op == FLT_CLIP && value < 0.f ? row + ": a clip bound must be >= 0" : std::string(); };
  return validate_fault_items({ACF_SETTER, "action-fault item", FLT_CLIP, "(0 scale, 1 bias, 2 set, 3 noise, 4 hold, 5 drop, 6 clip)"}, r, elem_rule, op_rule, marks);
}

// ---- cosim_set_param "latency".  Image: act_adr | obs_adr | act_item | obs_item ([n][4]: t0, t1, el | ord << 16, steps | jitter << 8: cosim_latency.h)
struct LatRaw {
  int n_scn;   // that of the scenario table that is set
  const int32_t *act_adr, *obs_adr;
  const int32_t *act, *obs;   // [n][6]: t0, t1, el, ord, steps, jitter
};
struct LatShape { std::string err; int n_act = 0, n_obs = 0, max_delay = 0; std::vector<int32_t> act_item, obs_item; };

inline LatShape validate_latency(int nu, const ObsDims& d, const LatRaw& r) {
  const std::string fn = LAT_SETTER;
  LatShape v;
  const RowAdr rows[2] = {{"act_adr", r.act_adr, "action latency items", LAT_MAX_ITEMS, r.act != nullptr},
                          {"obs_adr", r.obs_adr, "observation latency items", LAT_MAX_ITEMS, r.obs != nullptr}};
  TAB_TRY(row_heads(fn, rows));
  for (int s = 0; s < r.n_scn; s++) TAB_TRY(row_rule(fn + ": scenario " + std::to_string(s), rows, s));
  for (int kind = 0; kind < 2; kind++) {
    const int32_t* adr = kind ? r.obs_adr : r.act_adr;
    const int32_t* it = kind ? r.obs : r.act;
    std::vector<int32_t>& out = kind ? v.obs_item : v.act_item;
    for (int s = 0; s < r.n_scn; s++) {
      for (int i = adr[s]; i < adr[s + 1]; i++) {
        const std::string row = fn + ": scenario " + std::to_string(s) + (kind ? ", observation latency item " : ", action latency item ") + std::to_string(i - adr[s]);
        const int32_t* w = it + 6 * (size_t)i;
        const int el = w[2], ord = w[3], steps = w[4], jitter = w[5];
        TAB_TRY(window_rule(row, w[0], w[1]));
        if (!kind && (el < 0 || el >= nu)) TAB_TRY(row + ": actuator " + std::to_string(el) + " out of range: the model has " + std::to_string(nu) + " actuators");
        if (kind && (el < 0 || el >= d.frame_dim)) TAB_TRY(row + ": element " + std::to_string(el) + " out of range: the frame has " + std::to_string(d.frame_dim) + " elements");
        if (kind && d.el_field[el] == d.command_field)
          TAB_TRY(row + ": element " + std::to_string(el) + " is a command word and is refused: the command words are the scenario's keyframes");
        if (steps < 0) TAB_TRY(row + ": steps " + std::to_string(steps) + " is negative");
        if (jitter < 0) TAB_TRY(row + ": jitter " + std::to_string(jitter) + " is negative");
        if ((long long)steps + jitter > LAT_MAX_DELAY)
          TAB_TRY(row + ": steps " + std::to_string(steps) + " + jitter " + std::to_string(jitter) + " is more than " + std::to_string(LAT_MAX_DELAY));
        if (ord < 0 || ord > LAT_MAX_ORD) TAB_TRY(row + ": ordinal " + std::to_string(ord) + " outside 0..65535");
        if (steps + jitter > v.max_delay) v.max_delay = steps + jitter;
        out.push_back(w[0]); out.push_back(w[1]);
        out.push_back((int32_t)((unsigned)el | (unsigned)ord << 16)); out.push_back((int32_t)((unsigned)steps | (unsigned)jitter << 8));
      }
    }
  }
  v.n_act = r.act_adr[r.n_scn]; v.n_obs = r.obs_adr[r.n_scn];
  if (v.n_act + v.n_obs == 0) TAB_TRY(fn + ": the table holds no latency item (n_scn = 0 clears the latency)");
  return v;
}

inline void pack_latency(WordPacker& pk, LatTable& tab, const LatRaw& r, const LatShape& v) {
  const size_t S1 = (size_t)r.n_scn + 1;
  pk.add(&tab.act_adr, r.act_adr, S1); pk.add(&tab.obs_adr, r.obs_adr, S1);
  pk.add(&tab.act_item, v.act_item.data(), v.act_item.size()); pk.add(&tab.obs_item, v.obs_item.data(), v.obs_item.size());
  tab.n_scn = r.n_scn; tab.n_act = v.n_act; tab.n_obs = v.n_obs;
}
// whether the image holds the row addresses of `old`, an image of the same counts: every env keeps the kinds it had a line for
inline bool latency_same_rows(const WordPacker& pk, const LatTable& tab, const int32_t* old) { return pk.same(&tab.act_adr, old) && pk.same(&tab.obs_adr, old); }

// ---- cosim_scenario_checks_set.  Image: adr | t | signal | index | mode | cmp | bound
struct ChkRaw {
  int n_scn;   // that of the scenario table that is set
  const int32_t *adr, *t, *signal, *index, *mode, *cmp; const float* bound;
  int slots;
};
struct ChkShape { std::string err; int n = 0, I = 0; };   // I: the largest row, rounded up to even

inline ChkShape validate_checks(const TableDims& d, const ChkRaw& r) {
  const std::string fn = "cosim_scenario_checks_set";
  ChkShape v;
  if (r.slots < 1 || r.slots > CHK_MAX_SLOTS) TAB_TRY(fn + ": slots " + std::to_string(r.slots) + " outside 1..64");
  const RowAdr rows[1] = {{"adr", r.adr, "check items", CHK_MAX_ITEMS, r.t && r.signal && r.index && r.mode && r.cmp && r.bound}};
  TAB_TRY(row_heads(fn, rows));
  int most = 0;
  for (int s = 0; s < r.n_scn; s++) {
    const std::string who = fn + ": scenario " + std::to_string(s);
    TAB_TRY(row_rule(who, rows, s));
    if (r.adr[s + 1] - r.adr[s] > most) most = r.adr[s + 1] - r.adr[s];
    for (int i = r.adr[s]; i < r.adr[s + 1]; i++) {
      const std::string row = who + ", check item " + std::to_string(i - r.adr[s]);
      TAB_TRY(window_rule(row, r.t[2 * i], r.t[2 * i + 1]));
      TAB_TRY(signal_rule(row, d, r.signal[i], r.index[i]));
      if (r.mode[i] < 0 || r.mode[i] >= CHK_NMODE) TAB_TRY(row + ": unknown mode " + std::to_string(r.mode[i]) + " (0 always, 1 settle, 2 mean)");
      if (r.cmp[i] != CHK_LT && r.cmp[i] != CHK_GT) TAB_TRY(row + ": unknown cmp " + std::to_string(r.cmp[i]) + " (0 <, 1 >)");
      if (!std::isfinite(r.bound[i])) TAB_TRY(row + ": bound is not finite");
    }
  }
  v.n = r.adr[r.n_scn];
  if (v.n == 0) TAB_TRY(fn + ": the table holds no check item (n_scn = 0 clears the checks)");
  v.I = (most + 1) & ~1;
  return v;
}

inline void pack_checks(WordPacker& pk, ChkTable& tab, const ChkRaw& r, const ChkShape& v) {
  const size_t n = (size_t)v.n;
  pk.add(&tab.adr, r.adr, (size_t)r.n_scn + 1); pk.add(&tab.t, r.t, 2 * n); pk.add(&tab.signal, r.signal, n); pk.add(&tab.index, r.index, n);
  pk.add(&tab.mode, r.mode, n); pk.add(&tab.cmp, r.cmp, n); pk.add(&tab.bound, r.bound, n);
  tab.n_scn = r.n_scn; tab.n_items = v.n; tab.I = v.I;
}

// A table of the S, n and I of the one whose image `old` is may be written over it (the counters and the verdict records keep their
// meaning) if every row holds as many items as before.
inline bool checks_same_rows(const WordPacker& pk, const ChkTable& tab, const int32_t* old) { return pk.same(&tab.adr, old); }

// ---- cosim_scenario_curves_set.  Image: adr | t | signal | index | bins | nt | soff | coff | cw | lo | hi | inv_w
struct CurRaw {
  int n_scn;   // that of the scenario table that is set
  const int32_t *adr, *t, *signal, *index; const float *lo, *hi; const int32_t* bins;
};
struct CurShape {
  std::string err;
  int n = 0;
  std::vector<int32_t> nt, soff, coff, cw;   // per item: T, first stage word, first cell word, cell words of one class
  std::vector<float> inv_w;
  size_t cells = 0, SW = 0;   // 32-bit words of all cells; stage words per env: the largest sum of T over a row
};

inline CurShape validate_curves(const TableDims& d, int n_envs, const CurRaw& r) {
  const std::string fn = "cosim_scenario_curves_set";
  CurShape v;
  const RowAdr rows[1] = {{"adr", r.adr, "curve items", CUR_MAX_ITEMS, r.t && r.signal && r.index && r.lo && r.hi && r.bins}};
  TAB_TRY(row_heads(fn, rows));
  for (int s = 0; s < r.n_scn; s++) TAB_TRY(row_rule(fn + ": scenario " + std::to_string(s), rows, s));   // all rows first: n sizes the arrays below
  v.n = r.adr[r.n_scn];
  if (v.n == 0) TAB_TRY(fn + ": the table holds no curve item (n_scn = 0 clears the curves)");
  v.nt.resize(v.n); v.soff.resize(v.n); v.coff.resize(v.n); v.cw.resize(v.n); v.inv_w.assign(v.n, 0.f);
  for (int s = 0; s < r.n_scn; s++) {
    size_t row_words = 0;
    for (int i = r.adr[s]; i < r.adr[s + 1]; i++) {
      const std::string row = fn + ": scenario " + std::to_string(s) + ", curve item " + std::to_string(i - r.adr[s]);
      const int t0 = r.t[3 * i], t1 = r.t[3 * i + 1], every = r.t[3 * i + 2], B = r.bins[i];
      TAB_TRY(window_rule(row, t0, t1));
      if (every < 1) TAB_TRY(row + ": every " + std::to_string(every) + " is below 1");
      const int T = curves_nt(t0, t1, every);
      if (T > CUR_MAX_T) TAB_TRY(row + ": " + std::to_string(T) + " time bins, at most 1024");
      if (B < 0 || B > CUR_MAX_BINS) TAB_TRY(row + ": bins " + std::to_string(B) + " outside 0..64");
      if (!std::isfinite(r.lo[i]) || !std::isfinite(r.hi[i])) TAB_TRY(row + ": lo / hi is not finite");
      if (B > 0 && !(r.hi[i] > r.lo[i])) TAB_TRY(row + ": hi is not above lo");
      TAB_TRY(signal_rule(row, d, r.signal[i], r.index[i]));
      v.nt[i] = T; v.soff[i] = (int32_t)row_words; v.cw[i] = curves_cell_words(T, B);
      if (v.cells + 2 * (size_t)v.cw[i] > CUR_MAX_BYTES / 4) TAB_TRY(row + ": the cells would exceed 256 MiB (a design limit)");
      v.coff[i] = (int32_t)v.cells;
      v.cells += 2 * (size_t)v.cw[i];
      row_words += (size_t)T;
      if (B > 0) v.inv_w[i] = (float)((double)B / ((double)r.hi[i] - (double)r.lo[i]));
    }
    if (row_words > v.SW) v.SW = row_words;
  }
  if ((size_t)n_envs * v.SW > CUR_MAX_BYTES / 4)
    TAB_TRY(fn + ": the stage, " + std::to_string((long long)v.SW) + " words for each of " + std::to_string(n_envs) + " envs, would exceed 256 MiB (a design limit)");
  return v;
}

inline void pack_curves(WordPacker& pk, CurTable& tab, const CurRaw& r, const CurShape& v) {
  const size_t n = (size_t)v.n;
  pk.add(&tab.adr, r.adr, (size_t)r.n_scn + 1); pk.add(&tab.t, r.t, 3 * n); pk.add(&tab.signal, r.signal, n); pk.add(&tab.index, r.index, n);
  pk.add(&tab.bins, r.bins, n); pk.add(&tab.nt, v.nt.data(), n); pk.add(&tab.soff, v.soff.data(), n); pk.add(&tab.coff, v.coff.data(), n);
  pk.add(&tab.cw, v.cw.data(), n); pk.add(&tab.lo, r.lo, n); pk.add(&tab.hi, r.hi, n); pk.add(&tab.inv_w, v.inv_w.data(), n);
  tab.n_scn = r.n_scn; tab.n_items = v.n; tab.SW = (int)v.SW;
}

// A table of the S, n, SW and cell words of the one whose image `old` is may be written over it (the stage and the cells keep their
// layout) if every row holds as many items as before and every item has the T and B it had.
inline bool curves_same_sizes(const WordPacker& pk, const CurTable& tab, const int32_t* old) {
  return pk.same(&tab.adr, old) && pk.same(&tab.bins, old) && pk.same(&tab.nt, old) && pk.same(&tab.soff, old) && pk.same(&tab.coff, old) &&
         pk.same(&tab.cw, old);
}

// ---- cosim_set_param "search".  Image: has | lo | hi | x0 | d0 | d_min | rule | trials | targets | fail_mask | rev_skip, [S] each; the
// long form adds harder | chk_lo | chk_hi
struct SrchRaw {
  int n_scn;   // the table's first word
  int slots;
  const int32_t* has; const float *lo, *hi, *x0, *d0, *d_min; const int32_t *rule, *trials, *targets, *fail_mask, *rev_skip;
  const int32_t *harder = nullptr, *chk_lo = nullptr, *chk_hi = nullptr;   // the long form's columns (null: the short form)
};
// what the validator needs to know of the scenario table that is set; key_adr / push_adr: its row addresses [S + 1] (read only once S
// matches); chk_adr: those of the checks that are armed (null: none are)
// par_adr / obs_adr / act_adr: the row addresses of the parameter windows, observation faults and action faults that are set (null: none)
struct SrchDims {
  int n_scn, mode, auto_reset; const int32_t *key_adr, *push_adr; const int32_t* chk_adr = nullptr;
  const int32_t *par_adr = nullptr, *obs_adr = nullptr, *act_adr = nullptr;
};
constexpr int SRCH_TARGET_BITS = SRCH_PUSHES | SRCH_COMMANDS | SRCH_PARAMS | SRCH_OBS_FAULTS | SRCH_ACT_FAULTS;
struct SrchShape { std::string err; int n = 0; };   // n: scenarios that have an item

// A fall bit in fail_mask while no fall rule is set is NOT refused: the bit never fires (the rule may be set later).
inline SrchShape validate_search(const SrchDims& d, const SrchRaw& r) {
  const std::string fn = "cosim_set_param \"search\"";
  SrchShape v;
  if (d.n_scn == 0) TAB_TRY(fn + ": no scenario table is set (cosim_scenario_set): a search item is a row of a table; set the table first");
  if (r.n_scn != d.n_scn) TAB_TRY(fn + ": " + std::to_string(r.n_scn) + " scenarios, the table that is set has " + std::to_string(d.n_scn));
  if (d.mode == SCN_MODE_CYCLE) TAB_TRY(fn + ": the scenario mode is cycle: the search keeps one record per env, which needs the env's row to stay (mode env)");
  if (!d.auto_reset) TAB_TRY(fn + ": the search needs auto_reset: without it no episode follows the one that ended");
  if (r.slots < 1 || r.slots > SRCH_MAX_SLOTS) TAB_TRY(fn + ": slots " + std::to_string(r.slots) + " outside 1..64");
  for (int s = 0; s < r.n_scn; s++) {
    const std::string who = fn + ": scenario " + std::to_string(s);
    if (r.has[s] != 0 && r.has[s] != 1) TAB_TRY(who + ": has " + std::to_string(r.has[s]) + " is neither 0 nor 1");
    if (!r.has[s]) continue;
    v.n++;
    if (!std::isfinite(r.lo[s]) || !std::isfinite(r.hi[s])) TAB_TRY(who + ": lo / hi is not finite");
    if (!(r.lo[s] < r.hi[s])) TAB_TRY(who + ": hi is not above lo");
    if (!(r.x0[s] >= r.lo[s] && r.x0[s] <= r.hi[s])) TAB_TRY(who + ": the start level lies outside [lo, hi]");
    if (!std::isfinite(r.d0[s]) || !(r.d_min[s] > 0.f) || !(r.d_min[s] <= r.d0[s])) TAB_TRY(who + ": the steps must hold 0 < d_min <= d0");
    if (r.rule[s] != SRCH_BISECT && r.rule[s] != SRCH_STAIRCASE) TAB_TRY(who + ": unknown rule " + std::to_string(r.rule[s]) + " (0 bisect, 1 staircase)");
    if (r.trials[s] < 1 || r.trials[s] > SRCH_MAX_TRIALS) TAB_TRY(who + ": trials " + std::to_string(r.trials[s]) + " outside 1..2^20");
    if (r.targets[s] < 1 || (r.targets[s] & ~SRCH_TARGET_BITS))
      TAB_TRY(who + ": targets " + std::to_string(r.targets[s]) + " names nothing (1 pushes | 2 commands | 4 parameter windows | 8 observation faults | 16 action faults)");
    {   // an item kind (4, 8, 16) names the items of a table that is set; with no such table the word names nothing a search knew before them
      const struct { int bit; const int32_t* adr; const char* what; } kinds[3] = {{SRCH_PARAMS, d.par_adr, "parameter windows and the scenario has no parameter item"},
          {SRCH_OBS_FAULTS, d.obs_adr, "observation faults and the scenario has no fault item"}, {SRCH_ACT_FAULTS, d.act_adr, "action faults and the scenario has no action-fault item"}};
      for (const auto& k : kinds) {
        if (!(r.targets[s] & k.bit)) continue;
        if (!k.adr) TAB_TRY(who + ": targets " + std::to_string(r.targets[s]) + " names nothing (1 pushes | 2 commands)");
        if (k.adr[s + 1] == k.adr[s]) TAB_TRY(who + ": the target is the " + k.what);
      }
    }
    const unsigned long long chk = r.harder ? (unsigned long long)(uint32_t)r.chk_lo[s] | (unsigned long long)(uint32_t)r.chk_hi[s] << 32 : 0ull;
    if ((r.fail_mask[s] == 0 && chk == 0ull) || (r.fail_mask[s] & ~SRCH_FAIL_BITS))
      TAB_TRY(who + ": fail_mask " + std::to_string(r.fail_mask[s]) + " must be a non-empty set of 1 terminated | 4 non-finite | 32 tilt | 64 height | 128 contact (empty only with a check selected)");
    if (r.harder && r.harder[s] != SRCH_HARDER_UP && r.harder[s] != SRCH_HARDER_DOWN) TAB_TRY(who + ": harder " + std::to_string(r.harder[s]) + " is neither 0 (up) nor 1 (down)");
    if (chk != 0ull) {
      if (!d.chk_adr) TAB_TRY(who + ": the item fails on a check and no checks are armed (cosim_scenario_checks_set): arm the checks first");
      const int nc = d.chk_adr[s + 1] - d.chk_adr[s];
      if (nc < 64 && (chk >> nc) != 0ull) TAB_TRY(who + ": the item fails on a check the scenario does not have: it has " + std::to_string(nc) + " check items");
    }
    if (r.rev_skip[s] < 0 || r.rev_skip[s] > SRCH_MAX_REV_SKIP) TAB_TRY(who + ": rev_skip " + std::to_string(r.rev_skip[s]) + " outside 0..255");
    if ((r.targets[s] & SRCH_PUSHES) && d.push_adr[s + 1] == d.push_adr[s]) TAB_TRY(who + ": the target is the pushes and the scenario has no push window");
    if ((r.targets[s] & SRCH_COMMANDS) && d.key_adr[s + 1] == d.key_adr[s]) TAB_TRY(who + ": the target is the commands and the scenario has no keyframe");
  }
  if (v.n == 0) TAB_TRY(fn + ": the table holds no search item (the one word 0 clears the search)");
  return v;
}

inline void pack_search(WordPacker& pk, SrchTable& tab, const SrchRaw& r, const SrchShape& v) {
  const size_t S = (size_t)r.n_scn;
  pk.add(&tab.has, r.has, S); pk.add(&tab.lo, r.lo, S); pk.add(&tab.hi, r.hi, S); pk.add(&tab.x0, r.x0, S); pk.add(&tab.d0, r.d0, S);
  pk.add(&tab.d_min, r.d_min, S); pk.add(&tab.rule, r.rule, S); pk.add(&tab.trials, r.trials, S); pk.add(&tab.targets, r.targets, S);
  pk.add(&tab.fail_mask, r.fail_mask, S); pk.add(&tab.rev_skip, r.rev_skip, S);
  if (r.harder) { pk.add(&tab.harder, r.harder, S); pk.add(&tab.chk_lo, r.chk_lo, S); pk.add(&tab.chk_hi, r.chk_hi, S); }
  tab.n_scn = r.n_scn; tab.n_items = v.n;
}

// A table of the S of the one whose image `old` is may be written over it, the records kept, if the same scenarios have an item.
inline bool search_same_rows(const WordPacker& pk, const SrchTable& tab, const int32_t* old) { return pk.same(&tab.has, old); }

#undef TAB_TRY

}  // namespace cosim
