// Host driver of the parameter-window kernel's per-env body (cosim_amd/csrc/cosim_scnparams.h), built by tests/test_scnparams_host.py
// as plain C++ (once more with -fsanitize=address,undefined): reads the items and a list of envs from stdin, runs scenario_row /
// scnparams_apply lane by lane with the lane count it is given, the way scnparams_step_kernel's wave does with 64, prints one line per
// env.  Floats travel as their uint32 bits.  Every buffer has exactly the size the rule may touch.
//   in:  S mode gid_off n | adr[S+1] | t[2n] | word[n] | op[n] | value[n] | p_stride lanes n_envs | per env: env ep t base[p_stride]
//   out: per env: row eff[p_stride]
#include <stdio.h>
#include <string.h>

#include <vector>

#include "cosim_scnparams.h"

static int rd_i() {
  int v = 0;
  if (scanf("%d", &v) != 1) v = 0;
  return v;
}
static float rd_f() {
  unsigned u = 0;
  if (scanf("%u", &u) != 1) u = 0;
  float f;
  memcpy(&f, &u, 4);
  return f;
}
static unsigned bits(float f) {
  unsigned u;
  memcpy(&u, &f, 4);
  return u;
}

int main() {
  cosim::ScnTable T;
  cosim::ScnParTable P;
  memset(&T, 0, sizeof T);
  memset(&P, 0, sizeof P);
  T.n_scn = rd_i(); T.mode = rd_i(); T.gid_off = (unsigned)rd_i();
  const int n = rd_i();
  if (T.n_scn < 1 || n < 0) return 2;
  std::vector<int32_t> adr(T.n_scn + 1), t(2 * (size_t)n), word(n), op(n);
  std::vector<float> value(n);
  for (auto& x : adr) x = rd_i();
  for (auto& x : t) x = rd_i();
  for (auto& x : word) x = rd_i();
  for (auto& x : op) x = rd_i();
  for (auto& x : value) x = rd_f();
  P.adr = adr.data(); P.t = t.data(); P.word = word.data(); P.op = op.data(); P.value = value.data(); P.n_scn = T.n_scn; P.n_items = n;
  const int p_stride = rd_i(), lanes = rd_i(), n_envs = rd_i();
  if (p_stride < 1 || lanes < 1 || n_envs < 0) return 2;
  for (int i = 0; i < n_envs; i++) {
    const int env = rd_i(), ep = rd_i(), tt = rd_i();
    std::vector<float> base(p_stride), eff(p_stride);
    for (auto& x : base) x = rd_f();
    const float unwritten = -12345.f;
    for (auto& x : eff) x = unwritten;
    const int row = cosim::scenario_row(T, env, ep);
    for (int lane = 0; lane < lanes; lane++) cosim::scnparams_apply(P, row, tt, base.data(), eff.data(), p_stride, lane, lanes);
    printf("%d", row);
    for (int w = 0; w < p_stride; w++) printf(" %u", bits(eff[w]));
    printf("\n");
  }
  return 0;
}
