// Host driver of the check kernels' per-item bodies (cosim_amd/csrc/cosim_checks.h), built by tests/test_checks_host.py as plain C++
// (once more with -fsanitize=address,undefined): reads the items and a script of begins and control steps from stdin, runs
// checks_begin_lane / checks_step_lane / checks_open_lane lane by lane with the lane count it is given, the way the kernels' waves do
// with 64, and prints the rings, the counts and the open rows.  Floats travel as their uint32 bits.  Every buffer has exactly the
// size the rule may touch.  A step is issued as two env ranges, in either order.
//   in:  S mode gid_off n | adr[S+1] | t[2n] | signal[n] | index[n] | mode[n] | cmp[n] | bound[n]
//        | I slots lanes N info_dim nu cd nq nv reversed | events ...
//        event 1: begin  flag | mask[N] | meta0[N]
//        event 2: step   per env: te tr row meta0_after info[info_dim] cmd[cd] qpos[nq] qvel[nv]
//        event 3: open   ep[N] (meta word 11), then the output is printed and the program ends
//   out: rings N * slots * W ints | counts N | open N * W
#include <stdio.h>
#include <string.h>

#include <vector>

#include "cosim_checks.h"

using namespace cosim;

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

int main() {
  ChkArgs a;
  memset(&a, 0, sizeof a);
  ChkTable& T = a.tab;
  T.n_scn = rd_i();
  a.scn_mode = rd_i(); a.scn_off = (unsigned)rd_i();
  const int n = rd_i();
  if (T.n_scn < 1 || n < 1) return 2;
  std::vector<int32_t> adr(T.n_scn + 1), t(2 * (size_t)n), sig(n), idx(n), mode(n), cmp(n);
  std::vector<float> bound(n);
  for (auto& x : adr) x = rd_i();
  for (auto& x : t) x = rd_i();
  for (auto& x : sig) x = rd_i();
  for (auto& x : idx) x = rd_i();
  for (auto& x : mode) x = rd_i();
  for (auto& x : cmp) x = rd_i();
  for (auto& x : bound) x = rd_f();
  T.adr = adr.data(); T.t = t.data(); T.signal = sig.data(); T.index = idx.data(); T.mode = mode.data(); T.cmp = cmp.data(); T.bound = bound.data();
  T.n_items = n; T.I = rd_i();
  a.slots = rd_i();
  const int lanes = rd_i(), N = rd_i();
  a.info_dim = rd_i(); a.nu = rd_i(); a.cmd_stride = rd_i();
  const int nq = rd_i(), nv = rd_i(), reversed = rd_i();
  if (T.I < 2 || a.slots < 1 || lanes < 1 || N < 1) return 2;
  const int I = T.I, W = checks_words(I);
  a.n_envs = N; a.s_qpos = 0; a.s_qvel = nq; a.s_meta = nq + nv; a.s_stride = nq + nv + 16;
  std::vector<float> ext((size_t)N * I), state((size_t)N * a.s_stride, 0.f), info((size_t)N * a.info_dim), cmdv((size_t)N * a.cmd_stride);
  std::vector<int> aux((size_t)N * I), cn((size_t)N * I), cnt((size_t)N * CHK_NCNT, 0), ring((size_t)N * a.slots * W, 0), open((size_t)N * W, 0), rows(N);
  std::vector<double> sum((size_t)N * I);
  std::vector<uint8_t> term(N), trunc(N), mask(N);
  a.ext = ext.data(); a.aux = aux.data(); a.n = cn.data(); a.sum = sum.data(); a.cnt = cnt.data(); a.state = state.data();
  a.info = info.data(); a.cmd = a.cmd_stride > 0 ? cmdv.data() : nullptr; a.term = term.data(); a.trunc = trunc.data(); a.scn_row = rows.data();
  auto meta = [&](int env) { return reinterpret_cast<int*>(state.data() + (size_t)env * a.s_stride + a.s_meta); };
  for (;;) {
    const int ev = rd_i();
    if (ev == 1) {   // checks_begin_kernel
      a.flag = rd_i(); a.mask = mask.data(); a.rec = ring.data();
      for (auto& x : mask) x = (uint8_t)rd_i();
      for (int env = 0; env < N; env++) meta(env)[0] = rd_i();
      for (int env = 0; env < N; env++) {
        if (!checks_begin_applies(a, env)) continue;
        ChkCnt c = checks_load(cnt.data() + (size_t)env * CHK_NCNT);
        const ChkCnt c0 = c;
        for (int lane = 0; lane < lanes; lane++) { c = c0; checks_begin_lane(a, env, lane, lanes, c, meta(env)[0]); }
        checks_store(cnt.data() + (size_t)env * CHK_NCNT, c);
      }
    } else if (ev == 2) {   // checks_step_kernel, as two ranges
      a.rec = ring.data();
      for (int env = 0; env < N; env++) {
        term[env] = (uint8_t)rd_i(); trunc[env] = (uint8_t)rd_i(); rows[env] = rd_i(); meta(env)[0] = rd_i();
        for (int w = 0; w < a.info_dim; w++) info[(size_t)env * a.info_dim + w] = rd_f();
        for (int w = 0; w < a.cmd_stride; w++) cmdv[(size_t)env * a.cmd_stride + w] = rd_f();
        for (int w = 0; w < nq + nv; w++) state[(size_t)env * a.s_stride + w] = rd_f();
      }
      const int half = N / 2, first[2] = {reversed ? half : 0, reversed ? 0 : half}, count[2] = {reversed ? N - half : half, reversed ? half : N - half};
      for (int r = 0; r < 2; r++)
        for (int i = 0; i < count[r]; i++) {
          const int env = first[r] + i;
          int* cp = cnt.data() + (size_t)env * CHK_NCNT;
          ChkCnt c = checks_load(cp);
          const int te = term[env] != 0, tr = trunc[env] != 0;
          int* rec = (te | tr) ? ring.data() + ((size_t)env * a.slots + (size_t)(c.episode % a.slots)) * W : nullptr;
          unsigned long long f = 0ull, m = 0ull;
          for (int lane = 0; lane < lanes; lane++) checks_step_lane(a, env, lane, lanes, c, rows[env], rec, &f, &m);
          const ChkCnt c0 = c;
          const int flags = checks_advance(c, te, tr, meta(env)[0]);
          if (rec != nullptr)
            for (int w = 0; w < CHK_HDR; w++) rec[w] = checks_header_word(w, c0.episode, c0.length + 1, flags, rows[env] + 1, f, m);
          checks_store(cp, c);
        }
    } else if (ev == 3) {   // checks_open_kernel
      ScnTable S;
      memset(&S, 0, sizeof S);
      S.n_scn = T.n_scn; S.mode = a.scn_mode; S.gid_off = a.scn_off;
      for (int env = 0; env < N; env++) {
        const int row = scenario_row(S, env, rd_i());
        const ChkCnt c = checks_load(cnt.data() + (size_t)env * CHK_NCNT);
        int* out = open.data() + (size_t)env * W;
        unsigned long long f = 0ull, m = 0ull;
        for (int lane = 0; lane < lanes; lane++) checks_open_lane(a, env, lane, lanes, row, out, &f, &m);
        for (int w = 0; w < CHK_HDR; w++) out[w] = checks_header_word(w, c.episode, c.length, CHK_OPEN | c.oflags, row + 1, f, m);
      }
      break;
    } else return 2;
  }
  for (int x : ring) printf("%d ", x);
  printf("\n");
  for (int env = 0; env < N; env++) printf("%d ", cnt[(size_t)env * CHK_NCNT]);
  printf("\n");
  for (int x : open) printf("%d ", x);
  printf("\n");
  return 0;
}
