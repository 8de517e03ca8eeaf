// Host driver of the observation-fault kernel's per-env body (cosim_amd/csrc/cosim_obsfault.h), built by tests/test_obsfault_host.py
// as plain C++ (once more with -fsanitize=address,undefined): reads the items and a list of envs from stdin, runs scenario_row /
// obsfault_apply lane by lane with the lane count it is given -- four passes per call as obsfault_step_kernel's wave makes them with
// 64 lanes, further calls for the passes a smaller lane count leaves -- and prints one line per env.  Words travel as uint32 / int32.
// Every buffer has exactly the size the rule may touch.
//   in:  S mode env_id0 n | adr[S+1] | item[4n] | sd stack_size frame_dim lanes seed_lo seed_hi n_envs |
//        per env: env ep t step_count stack[stack_size * sd] out[state_dim]
//   out: per env: row stack[stack_size * sd] out[state_dim]
#include <stdio.h>
#include <string.h>

#include <vector>

#include "cosim_obsfault.h"

static long long rd_i() {
  long long v = 0;
  if (scanf("%lld", &v) != 1) v = 0;
  return v;
}
static float rd_f() {
  const unsigned u = (unsigned)rd_i();
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
  cosim::ObsFaultTable F;
  memset(&T, 0, sizeof T);
  memset(&F, 0, sizeof F);
  T.n_scn = (int)rd_i(); T.mode = (int)rd_i();
  const long long env_id0 = rd_i();
  const int n = (int)rd_i();
  if (T.n_scn < 1 || n < 0) return 2;
  T.gid_off = (unsigned)(((env_id0 % T.n_scn) + T.n_scn) % T.n_scn);
  std::vector<int32_t> adr(T.n_scn + 1), item(4 * (size_t)(n + cosim::OBF_CHUNK - 1), 0);   // the padding the rule may fetch, and no more
  for (auto& x : adr) x = (int32_t)rd_i();
  for (size_t k = 0; k < 4 * (size_t)n; k++) item[k] = (int32_t)(unsigned)rd_i();
  F.adr = adr.data(); F.item = item.data(); F.n_scn = T.n_scn; F.n_items = n;
  const int sd = (int)rd_i(), S = (int)rd_i(), frame_dim = (int)rd_i(), lanes = (int)rd_i();
  const unsigned seed_lo = (unsigned)rd_i(), seed_hi = (unsigned)rd_i();
  const int n_envs = (int)rd_i();
  if (sd < 0 || S < 1 || frame_dim < sd || lanes < 1 || n_envs < 0) return 2;
  const int state_dim = S * sd + frame_dim - sd;
  constexpr int NP = 4;
  for (int i = 0; i < n_envs; i++) {
    const int env = (int)rd_i(), ep = (int)rd_i(), t = (int)rd_i();
    const unsigned c0 = (unsigned)rd_i();
    std::vector<float> stack((size_t)S * sd), out(state_dim);
    for (auto& x : stack) x = rd_f();
    for (auto& x : out) x = rd_f();
    const int row = cosim::scenario_row(T, env, ep);
    const unsigned long long gid = (unsigned long long)(env_id0 + env);
    cosim::ObsFaultEnv E;
    E.stack = stack.data(); E.out = out.data(); E.sd = sd; E.S = S; E.frame_dim = frame_dim;
    E.k0 = seed_lo; E.k1 = seed_hi; E.c0 = c0; E.g0 = (unsigned)gid; E.g1 = (unsigned)(gid >> 32);
    for (int pass0 = 0; pass0 * lanes < frame_dim; pass0 += NP)
      for (int lane = 0; lane < lanes; lane++) cosim::obsfault_apply<NP>(F, row, t, E, lane, lanes, pass0);
    printf("%d", row);
    for (float x : stack) printf(" %u", bits(x));
    for (float x : out) printf(" %u", bits(x));
    printf("\n");
  }
  return 0;
}
