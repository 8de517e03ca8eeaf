// Host driver of the action-fault kernels' per-env body (cosim_amd/csrc/cosim_actfault.h), built by tests/test_actfault_host.py as plain
// C++ (once more with -fsanitize=address,undefined): reads the items and a list of envs from stdin, runs scenario_row / actfault_apply
// lane by lane (lane = actuator, as actfault_step_kernel's wave makes them) and actfault_restore for every element of a made-up
// last_action field, and prints one line per env.  Words travel as uint32 / int32.  Every buffer has exactly the size the rule may touch.
//   in:  S mode env_id0 n | adr[S+1] | item[4n] | nu seed_lo seed_hi sd stack_size frame_dim e0 scale n_envs |
//        per env: env ep t step_count raw[nu] lastact[nu]
//   out: per env: row eff[nu] cache[frame_dim] stack[sd] out[stack_size * sd + frame_dim - sd]
// The observation of the restore part: last_action is the nu frame elements from e0 on, scaled by `scale`; the three buffers start
// as zeros, so the words the restore leaves alone print as 0.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "cosim_actfault.h"

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
  cosim::ActFaultTable F;
  memset(&T, 0, sizeof T);
  memset(&F, 0, sizeof F);
  T.n_scn = (int)rd_i(); T.mode = (int)rd_i();
  const long long env_id0 = rd_i();
  const int n = (int)rd_i();
  if (T.n_scn < 1 || n < 0) return 2;
  T.gid_off = (unsigned)(((env_id0 % T.n_scn) + T.n_scn) % T.n_scn);
  std::vector<int32_t> adr(T.n_scn + 1), item(4 * (size_t)(n + cosim::ACF_CHUNK - 1), 0);   // the padding the rule may fetch, and no more
  for (auto& x : adr) x = (int32_t)rd_i();
  for (size_t k = 0; k < 4 * (size_t)n; k++) item[k] = (int32_t)(unsigned)rd_i();
  F.adr = adr.data(); F.item = item.data(); F.n_scn = T.n_scn; F.n_items = n;
  const int nu = (int)rd_i();
  const unsigned seed_lo = (unsigned)rd_i(), seed_hi = (unsigned)rd_i();
  const int sd = (int)rd_i(), S = (int)rd_i(), frame_dim = (int)rd_i(), e0 = (int)rd_i();
  const float scale = rd_f();
  const int n_envs = (int)rd_i();
  if (nu < 1 || nu > 64 || sd < 0 || S < 1 || frame_dim < sd || e0 < 0 || e0 + nu > frame_dim || n_envs < 0) return 2;
  for (int i = 0; i < n_envs; i++) {
    const int env = (int)rd_i(), ep = (int)rd_i(), t = (int)rd_i();
    const unsigned c0 = (unsigned)rd_i();
    std::vector<float> raw(nu), lastact(nu), eff(nu);
    for (auto& x : raw) x = rd_f();
    for (auto& x : lastact) x = rd_f();
    const int row = cosim::scenario_row(T, env, ep);
    const unsigned long long gid = (unsigned long long)(env_id0 + env);
    cosim::ActFaultEnv E;
    E.lastact = lastact.data();
    E.k0 = seed_lo; E.k1 = seed_hi; E.c0 = c0; E.g0 = (unsigned)gid; E.g1 = (unsigned)(gid >> 32);
    for (int lane = 0; lane < nu; lane++) eff[lane] = cosim::actfault_apply(F, row, t, E, lane, raw[lane]);
    std::vector<float> cache(frame_dim, 0.f), stack(sd, 0.f), out((size_t)S * sd + frame_dim - sd, 0.f);
    for (int j = 0; j < nu; j++) cosim::actfault_restore(raw[j], scale, e0 + j, sd, S, cache.data(), stack.data(), out.data());
    printf("%d", row);
    for (float x : eff) printf(" %u", bits(x));
    for (float x : cache) printf(" %u", bits(x));
    for (float x : stack) printf(" %u", bits(x));
    for (float x : out) printf(" %u", bits(x));
    printf("\n");
  }
  return 0;
}
