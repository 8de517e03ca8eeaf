// Host driver of the latency kernels' per-env body (cosim_amd/csrc/cosim_latency.h), built by tests/test_latency_host.py as plain C++
// (once more with -fsanitize=address,undefined): reads the items and a run of steps of a list of envs from stdin, keeps the lines and
// headers the engine keeps, and per step and env runs what latency_act_kernel and latency_obs_kernel run, lane by lane (lane =
// actuator; lane = frame element in passes of 64), then prints one line.  Words travel as uint32 / int32.  Every buffer has exactly
// the size the rule may touch.
//   in:  S mode env_id0 D na no | act_adr[S+1] | obs_adr[S+1] | act_item[4 na] | obs_item[4 no] |
//        nu frame_dim sd stack_size seed_lo seed_hi n_envs steps |
//        per step, per env: cut | ep t step_count raw[nu] | ep t step_count frame[frame_dim]    (pre-step words, then post-step ones)
//   out: per step, per env: row_pre eff[nu] row_post delivered[frame_dim]
// cut != 0: the env's two headers are invalidated ahead of the step, as latency_cut_kernel does.  The observation part plays the
// step kernel: the clean frame goes to stack row 0 / the non-stacked tail of a state_out row, the rule rewrites them, and what they
// hold afterwards is printed (a stacked element's two copies must agree).
#include <stdio.h>
#include <string.h>

#include <vector>

#include "cosim_latency.h"

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

constexpr int PASSES = 4;   // of 64 lanes: the kernel's MAXFRAME / 64

int main() {
  cosim::ScnTable T;
  cosim::LatTable L;
  memset(&T, 0, sizeof T);
  memset(&L, 0, sizeof L);
  T.n_scn = (int)rd_i(); T.mode = (int)rd_i();
  const long long env_id0 = rd_i();
  const int D = (int)rd_i(), na = (int)rd_i(), no = (int)rd_i();
  if (T.n_scn < 1 || D < 1 || D > 64 || na < 0 || no < 0) return 2;
  T.gid_off = (unsigned)(((env_id0 % T.n_scn) + T.n_scn) % T.n_scn);
  std::vector<int32_t> act_adr(T.n_scn + 1), obs_adr(T.n_scn + 1), act_item(4 * (size_t)na), obs_item(4 * (size_t)no);
  for (auto& x : act_adr) x = (int32_t)rd_i();
  for (auto& x : obs_adr) x = (int32_t)rd_i();
  for (auto& x : act_item) x = (int32_t)(unsigned)rd_i();
  for (auto& x : obs_item) x = (int32_t)(unsigned)rd_i();
  L.act_adr = act_adr.data(); L.obs_adr = obs_adr.data(); L.act_item = act_item.data(); L.obs_item = obs_item.data();
  L.n_scn = T.n_scn; L.n_act = na; L.n_obs = no; L.depth = D;
  const int nu = (int)rd_i(), fd = (int)rd_i(), sd = (int)rd_i(), S = (int)rd_i();
  const unsigned seed_lo = (unsigned)rd_i(), seed_hi = (unsigned)rd_i();
  const int n_envs = (int)rd_i(), steps = (int)rd_i();
  if (nu < 1 || nu > 64 || fd < 1 || fd > 64 * PASSES || sd < 0 || sd > fd || S < 1 || n_envs < 0 || steps < 0) return 2;
  std::vector<std::vector<float>> act_line(n_envs, std::vector<float>((size_t)D * nu, 0.f)), obs_line(n_envs, std::vector<float>((size_t)D * fd, 0.f));
  std::vector<int> from_act(n_envs, -1), from_obs(n_envs, -1);
  for (int k = 0; k < steps; k++) {
    for (int env = 0; env < n_envs; env++) {
      if (rd_i() != 0) { from_act[env] = -1; from_obs[env] = -1; }
      const unsigned long long gid = (unsigned long long)(env_id0 + env);
      cosim::FaultKey K = {seed_lo, seed_hi, 0u, (unsigned)gid, (unsigned)(gid >> 32)};
      // ---- latency_act_kernel
      int ep = (int)rd_i(), t = (int)rd_i();
      K.c0 = (unsigned)rd_i();
      std::vector<float> raw(nu), eff(nu);
      for (auto& x : raw) x = rd_f();
      const int row_pre = cosim::scenario_row(T, env, ep);
      {
        const int from = from_act[env];
        int f = from;
        for (int lane = 0; lane < nu; lane++) {
          int kk[1];
          float y = raw[lane];
          if (cosim::latency_walk<1>(L.act_adr, L.act_item, row_pre, t, D, K, lane, 64, kk)) {
            f = cosim::latency_from(from, t);
            y = cosim::latency_act_word(act_line[env].data(), D, nu, lane, t, f, kk[0], raw[lane]);
          }
          eff[lane] = y;
        }
        from_act[env] = f;
      }
      // ---- the step, then latency_obs_kernel
      ep = (int)rd_i(); t = (int)rd_i();
      K.c0 = (unsigned)rd_i();
      std::vector<float> stack(sd, 0.f), out((size_t)S * sd + fd - sd, 0.f);
      for (int e = 0; e < fd; e++) {
        const float x = rd_f();
        if (e < sd) { stack[e] = x; out[e] = x; }
        else out[(size_t)S * sd + (e - sd)] = x;
      }
      const int row_post = cosim::scenario_row(T, env, ep);
      {
        const int from = from_obs[env];
        int f = from;
        for (int lane = 0; lane < 64; lane++) {
          int kk[PASSES];
          if (!cosim::latency_walk<PASSES>(L.obs_adr, L.obs_item, row_post, t, D, K, lane, 64, kk)) break;
          f = cosim::latency_from(from, t);
          for (int p = 0; p < PASSES; p++) {
            const int e = lane + 64 * p;
            if (e >= fd) break;
            float* word = e < sd ? &stack[e] : &out[(size_t)S * sd + (e - sd)];
            const float v = cosim::latency_obs_word(obs_line[env].data(), D, fd, e, t, f, kk[p], *word);
            if (kk[p] == 0) continue;
            *word = v;
            if (e < sd) out[e] = v;
          }
        }
        from_obs[env] = f;
      }
      printf("%d", row_pre);
      for (float x : eff) printf(" %u", bits(x));
      printf(" %d", row_post);
      for (int e = 0; e < fd; e++) {
        if (e < sd && bits(stack[e]) != bits(out[e])) return 3;
        printf(" %u", bits(e < sd ? stack[e] : out[(size_t)S * sd + (e - sd)]));
      }
      printf("\n");
    }
  }
  return 0;
}
