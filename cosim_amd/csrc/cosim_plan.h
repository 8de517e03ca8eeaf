// cosim_plan.h -- which kernel runs when.  Plain C++17, no HIP: FN is the launcher type (a function pointer in cosim_engine.hip, an
// int id in tests/kernel_plan.cpp); a value-initialised FN means "no such kernel".  KernelSet: what the model and terrain have, filled
// once by cosim_create.  Switches: what cosim_set_param asked for, changed only by switch_set.  Plan = make_plan(set, switches): the
// kernels the launch sites run and the answers of cosim_query, recomputed after every accepted switch and only read everywhere else.
#pragma once
#include <string>

namespace cosim {

template <class FN>
struct Kernel {
  FN launch{};
  // LDS per env; ground-contact / robot-robot contact capacity; plane kernels: geom lanes that can stage their contacts
  int lds_bytes = 0, contact_slots = 0, pair_slots = 0, geom_stage = 64;
};
template <class FN> bool has(const Kernel<FN>& k) { return !(k.launch == FN{}); }

template <class FN>
struct KernelSet {
  // fleet kernel (reset, step, debug forward), its step-only instantiation (no reset branch, no debug dump) and its diagnostic build
  Kernel<FN> fleet, fleet_step, fleet_prof;
  Kernel<FN> epw2, epw2_prof;            // two environments per wave
  Kernel<FN> ct, ct_prof;                // contact-twist variant of a dense-row fleet kernel (more ground-contact slots)
  Kernel<FN> fix;                        // plane: redoes the control step of envs whose contacts did not fit the fleet kernel
  Kernel<FN> roll, roll_step, roll_fix;  // K control steps per launch; roll_fix takes over the envs roll gave up
  // heightfield fix-up (opt-in, 50 slots per ground geom): behind the fused kernel (a control step), behind each solver launch of the
  // split pipeline (a substep), and the fleet kernel at that capacity for cosim_debug_forward
  Kernel<FN> hfix, stepfix, dbg_hfix;
  Kernel<FN> narrow[4];                  // split pipeline's narrowphase: diagnostic build, then 2, 3, 4 waves per SIMD
  Kernel<FN> solver;                     // split pipeline's solver: one substep per launch, and the reset
};

struct Switches {
  bool contact_twist = false, fixup_off = false;   // one-way: set by "contact_twist" 1 / "fixup" 0, never cleared
  bool hfield_fixup = false;
  bool split = true;            // these two take effect where the set has a solver / a step-only kernel
  bool step_kernel = true;
  int epw = 1;                  // environments per wave
  int narrow_occ = 2;           // waves per SIMD of the narrowphase kernel (0: diagnostic build)
};

template <class FN>
struct Plan {
  Kernel<FN> reset;                 // always a general instantiation; the solver kernel when split
  Kernel<FN> narrow, step;          // a control step: step alone, or per substep narrow (narrow_waves blocks per env) then step
  Kernel<FN> fixup;                 // behind every step launch (split: behind every substep's), if any
  Kernel<FN> rollout, rollout_fix;  // none: cosim_rollout is refused
  Kernel<FN> prof;                  // cosim_profile_step; none: refused
  Kernel<FN> debug;                 // cosim_debug_forward, behind narrow when split
  bool narrow_diag = false;         // narrow accumulates its counters in the debug buffer
  int lds_bytes = 0, contact_slots = 0, pair_slots = 0, fixup_contact_slots = 0;   // these and the next two: answers of cosim_query
  bool step_kernel = false, split = false;
};

template <class FN>
Plan<FN> make_plan(const KernelSet<FN>& k, const Switches& s) {
  Plan<FN> p;
  const Kernel<FN> none{};
  const bool ct = s.contact_twist, one = s.epw == 1;
  const Kernel<FN>& fleet = ct ? k.ct : k.fleet;
  const Kernel<FN>& general = one ? fleet : k.epw2;
  p.split = s.split && has(k.solver);
  p.step_kernel = s.step_kernel && one && !ct && has(k.fleet_step);   // (the contact-twist kernels have no step-only instantiation)
  p.reset = p.split ? k.solver : general;
  p.step = p.split ? k.solver : p.step_kernel ? k.fleet_step : general;
  if (p.split) {
    p.narrow = k.narrow[s.narrow_occ >= 4 ? 3 : s.narrow_occ == 3 ? 2 : s.narrow_occ == 2 ? 1 : 0];
    p.narrow_diag = s.narrow_occ == 0;
  }
  const Kernel<FN>& fix = p.split ? (s.hfield_fixup ? k.stepfix : none) : s.hfield_fixup ? k.hfix : (ct || s.fixup_off) ? none : k.fix;
  p.fixup = one ? fix : none;
  // the contact-twist kernel redoes nothing and hands nothing over; without fix-ups a rollout that needs roll_fix is gone too
  const bool roll = one && !ct && has(k.roll) && !(s.fixup_off && has(k.roll_fix));
  p.rollout = !roll ? none : (s.step_kernel && has(k.roll_step)) ? k.roll_step : k.roll;
  p.rollout_fix = roll ? k.roll_fix : none;
  p.prof = ct ? k.ct_prof : one ? k.fleet_prof : k.epw2_prof;
  p.debug = p.split ? k.solver : (s.hfield_fixup && has(k.dbg_hfix)) ? k.dbg_hfix : general;
  // kept as reported so far: under two envs per wave the one-per-wave kernel's capacities, and a fix-up that is not launched
  p.lds_bytes = fleet.lds_bytes; p.contact_slots = fleet.contact_slots; p.pair_slots = fleet.pair_slots;
  p.fixup_contact_slots = fix.contact_slots;
  return p;
}

inline bool is_switch(const std::string& name) {
  for (const char* s : {"contact_twist", "fixup", "hfield_fixup", "split", "step_kernel", "envs_per_wave", "narrow_occupancy"})
    if (name == s) return true;
  return false;
}

// cosim_set_param of a switch (is_switch(which)): null if accepted (s updated), else the message it fails with (s untouched)
template <class FN>
const char* switch_set(const KernelSet<FN>& k, Switches& s, const std::string& which, int v, int n_envs) {
  if (which == "contact_twist") {   // 1: a dense-row fleet kernel -> its contact-twist variant; 0: nothing
    if (v == 0) return nullptr;
    if (!has(k.ct)) return "cosim_set_param: no contact-twist variant for this model / terrain";
    s.contact_twist = true; s.epw = 1;
  } else if (which == "fixup") {    // 0: no fix-up launches from here on; anything else: nothing
    if (v == 0) { s.fixup_off = true; s.hfield_fixup = false; }
  } else if (which == "hfield_fixup") {
    if (v != 0 && v != 1) return "cosim_set_param: hfield_fixup must be 0 or 1";
    if (!has(k.hfix) || s.fixup_off || s.epw != 1) return "cosim_set_param: no heightfield fix-up for this model / terrain / kernel variant";
    s.hfield_fixup = v != 0;
  } else if (which == "split") {
    if (v != 0 && !has(k.solver)) return "cosim_set_param: no split pipeline for this model / terrain";
    s.split = v != 0;
  } else if (which == "step_kernel") {
    if (v != 0 && v != 1) return "cosim_set_param: step_kernel must be 0 or 1";
    s.step_kernel = v != 0;
  } else if (which == "envs_per_wave") {
    if (v != 1 && !(v == 2 && has(k.epw2) && !s.contact_twist && n_envs % 2 == 0)) return "cosim_set_param: envs_per_wave not available for this model / env count";
    s.epw = v;
  } else s.narrow_occ = v;   // "narrow_occupancy"
  return nullptr;
}

}  // namespace cosim
