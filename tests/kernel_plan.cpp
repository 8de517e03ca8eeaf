// csrc/cosim_plan.h as a plain C++ program with int ids for launchers (no HIP, no GPU), driven by tests/test_kernel_plan_host.py.
//
// stdin, one record per line:
//   SET <name> <19 x (id lds_bytes contact_slots pair_slots geom_stage)>   a KernelSet, members in declaration order (id 0: none)
//   RUN <name> <n_envs> [<switch> <value>]...                              default switches, then the calls in order
// stdout per RUN: one plan row for the fresh engine and one per call, each
//   <refused 0|1> <epw> | reset narrow step fixup rollout rollout_fix prof debug (ids) | narrow_diag lds_bytes contact_slots pair_slots
//   fixup_contact_slots step_kernel split | <message if refused>
#include <cstdio>
#include <iostream>
#include <map>
#include <sstream>
#include <string>

#include "cosim_plan.h"

using namespace cosim;

static void row(const KernelSet<int>& k, const Switches& s, const char* refused) {
  const Plan<int> p = make_plan(k, s);
  std::printf("%d %d | %d %d %d %d %d %d %d %d | %d %d %d %d %d %d %d | %s\n", refused != nullptr, s.epw, p.reset.launch, p.narrow.launch,
              p.step.launch, p.fixup.launch, p.rollout.launch, p.rollout_fix.launch, p.prof.launch, p.debug.launch, (int)p.narrow_diag,
              p.lds_bytes, p.contact_slots, p.pair_slots, p.fixup_contact_slots, (int)p.step_kernel, (int)p.split, refused ? refused : "");
}

int main() {
  std::map<std::string, KernelSet<int>> sets;
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string what, name;
    if (!(in >> what >> name)) continue;
    if (what == "SET") {
      KernelSet<int> k;
      Kernel<int>* members[20] = {&k.fleet, &k.fleet_step, &k.fleet_prof, &k.epw2, &k.epw2_prof, &k.ct, &k.ct_prof, &k.fix, &k.roll, &k.roll_step,
                                  &k.roll_fix, &k.hfix, &k.stepfix, &k.dbg_hfix, &k.narrow[0], &k.narrow[1], &k.narrow[2], &k.narrow[3], &k.solver,
                                  nullptr};
      for (int i = 0; members[i]; i++) {
        Kernel<int>& m = *members[i];
        if (!(in >> m.launch >> m.lds_bytes >> m.contact_slots >> m.pair_slots >> m.geom_stage)) return 2;
      }
      sets[name] = k;
    } else if (what == "RUN") {
      if (!sets.count(name)) return 3;
      const KernelSet<int>& k = sets[name];
      int n_envs = 0, value = 0;
      std::string which;
      if (!(in >> n_envs)) return 4;
      Switches s;
      row(k, s, nullptr);
      while (in >> which >> value) {
        const Switches before = s;
        const char* refused = switch_set(k, s, which, value, n_envs);
        if (refused && (before.contact_twist != s.contact_twist || before.fixup_off != s.fixup_off || before.hfield_fixup != s.hfield_fixup ||
                        before.split != s.split || before.step_kernel != s.step_kernel || before.epw != s.epw || before.narrow_occ != s.narrow_occ))
          return 5;   // a refused call must leave the switches alone
        if (!is_switch(which)) return 6;
        row(k, s, refused);
      }
    } else return 1;
  }
  return 0;
}
