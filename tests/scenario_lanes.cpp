// Host driver of the scenario kernel's per-env body (cosim_amd/csrc/cosim_scenario.h), built by tests/test_scenario_host.py as plain
// C++: reads a table and a list of lanes from stdin, runs scenario_row / scenario_apply lane by lane the way scenario_step_kernel
// does, prints one line per lane.  Floats travel as their uint32 bits.
//   in:  S mode cd gid_off nkey npush | key_adr[S+1] | key_t[nkey] | key_cmd[nkey*cd] | push_adr[S+1] | push_t[2*npush] |
//        push_v[3*npush] | n_lanes | per lane: env ep t cmd_in[cd] quat[4]
//   out: per lane: row pushed cmd_out[cd] qvel[3]
#include <stdio.h>
#include <string.h>

#include <vector>

#include "cosim_scenario.h"

static float rd_f() {
  unsigned u = 0;
  if (scanf("%u", &u) != 1) u = 0;
  float f;
  memcpy(&f, &u, 4);
  return f;
}
static int rd_i() {
  int v = 0;
  if (scanf("%d", &v) != 1) v = 0;
  return v;
}
static unsigned bits(float f) {
  unsigned u;
  memcpy(&u, &f, 4);
  return u;
}

int main() {
  cosim::ScnTable T;
  memset(&T, 0, sizeof T);
  T.n_scn = rd_i(); T.mode = rd_i(); T.cd = rd_i(); T.gid_off = (unsigned)rd_i();
  const int nkey = rd_i(), npush = rd_i();
  if (T.n_scn < 1 || T.cd < 0 || T.cd > 6 || nkey < 0 || npush < 0) return 2;
  std::vector<int32_t> key_adr(T.n_scn + 1), key_t(nkey), push_adr(T.n_scn + 1), push_t(2 * npush);
  std::vector<float> key_cmd((size_t)nkey * T.cd), push_v(3 * (size_t)npush);
  for (auto& x : key_adr) x = rd_i();
  for (auto& x : key_t) x = rd_i();
  for (auto& x : key_cmd) x = rd_f();
  for (auto& x : push_adr) x = rd_i();
  for (auto& x : push_t) x = rd_i();
  for (auto& x : push_v) x = rd_f();
  T.key_adr = key_adr.data(); T.key_t = key_t.data(); T.key_cmd = key_cmd.data();
  T.push_adr = push_adr.data(); T.push_t = push_t.data(); T.push_v = push_v.data();
  const int n = rd_i();
  for (int i = 0; i < n; i++) {
    const int env = rd_i(), ep = rd_i(), t = rd_i();
    float cmd_in[6] = {0}, cmd_out[6] = {0}, quat[4], qvel[3] = {0.f, 0.f, 0.f};
    for (int c = 0; c < T.cd; c++) cmd_in[c] = rd_f();
    for (int c = 0; c < 4; c++) quat[c] = rd_f();
    const int row = cosim::scenario_row(T, env, ep);
    const int pushed = cosim::scenario_apply(T, row, t, cmd_in, cmd_out, quat, qvel, true);
    printf("%d %d", row, pushed);
    for (int c = 0; c < T.cd; c++) printf(" %u", bits(cmd_out[c]));
    for (int c = 0; c < 3; c++) printf(" %u", bits(qvel[c]));
    printf("\n");
  }
  return 0;
}
