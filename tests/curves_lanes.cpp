// Host driver of the curve kernels' per-lane bodies (cosim_amd/csrc/cosim_curves.h), built by tests/test_curves_host.py as plain C++
// (once more with -fsanitize=address,undefined): reads the items and a script of begins, clears and control steps from stdin, runs
// curves_sample_lane / curves_fold_lane / curves_begin_lane lane by lane with the lane count it is given, the way the kernels' waves do
// with 64, and prints the cells.  The "atomics" are plain operations.  Floats travel as their uint32 bits.  Every buffer has exactly
// the size the rule may touch.  A step is issued as two env ranges, in either order.
//   in:  S n | adr[S+1] | t[3n] | signal[n] | index[n] | bins[n] | nt[n] | soff[n] | coff[n] | cw[n] | lo[n] | hi[n] | inv_w[n]
//        | SW words lanes N info_dim nu cd nq nv reversed | events ...
//        event 1: begin  mask[N] | meta0[N]
//        event 2: step   per env: te tr row meta0_after info[info_dim] cmd[cd] qpos[nq] qvel[nv]
//        event 3: end    the cells are printed and the program ends
//        event 4: clear  meta0[N]   (the cells back to empty, every env begins)
//   out: words uint32
#include <stdio.h>
#include <string.h>

#include <vector>

#include "cosim_curves.h"

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

struct PlainOps {
  void add(unsigned* p, unsigned v) { *p += v; }
  void add64(unsigned long long* p, unsigned long long v) { *p += v; }
  void min(unsigned* p, unsigned v) { if (v < *p) *p = v; }
  void max(unsigned* p, unsigned v) { if (v > *p) *p = v; }
};

int main() {
  CurArgs a;
  memset(&a, 0, sizeof a);
  CurTable& T = a.tab;
  T.n_scn = rd_i();
  const int n = rd_i();
  if (T.n_scn < 1 || n < 1) return 2;
  std::vector<int32_t> adr(T.n_scn + 1), t(3 * (size_t)n), sig(n), idx(n), bins(n), nt(n), soff(n), coff(n), cw(n);
  std::vector<float> lo(n), hi(n), inv_w(n);
  for (auto& x : adr) x = rd_i();
  for (auto& x : t) x = rd_i();
  for (auto& x : sig) x = rd_i();
  for (auto& x : idx) x = rd_i();
  for (auto& x : bins) x = rd_i();
  for (auto& x : nt) x = rd_i();
  for (auto& x : soff) x = rd_i();
  for (auto& x : coff) x = rd_i();
  for (auto& x : cw) x = rd_i();
  for (auto& x : lo) x = rd_f();
  for (auto& x : hi) x = rd_f();
  for (auto& x : inv_w) x = rd_f();
  T.adr = adr.data(); T.t = t.data(); T.signal = sig.data(); T.index = idx.data(); T.bins = bins.data(); T.nt = nt.data(); T.soff = soff.data();
  T.coff = coff.data(); T.cw = cw.data(); T.lo = lo.data(); T.hi = hi.data(); T.inv_w = inv_w.data();
  T.n_items = n; T.SW = rd_i();
  const int words = rd_i(), lanes = rd_i(), N = rd_i();
  a.info_dim = rd_i(); a.nu = rd_i(); a.cmd_stride = rd_i();
  const int nq = rd_i(), nv = rd_i(), reversed = rd_i();
  if (T.SW < 1 || words < 2 || lanes < 1 || N < 1) return 2;
  a.n_envs = N; a.s_qpos = 0; a.s_qvel = nq; a.s_meta = nq + nv; a.s_stride = nq + nv + 16;
  std::vector<float> state((size_t)N * a.s_stride, 0.f), info((size_t)N * a.info_dim), cmdv((size_t)N * a.cmd_stride);
  std::vector<int> stage((size_t)N * T.SW, CUR_NONE), clk(N, 0), rows(N);
  std::vector<unsigned long long> cells64(((size_t)words + 1) / 2, 0ull);   // 8-byte aligned, as the device allocation is
  unsigned* cells = reinterpret_cast<unsigned*>(cells64.data());
  std::vector<uint8_t> term(N), trunc(N), mask(N);
  a.stage = stage.data(); a.clk = clk.data(); a.cells = cells; a.state = state.data();
  a.info = info.data(); a.cmd = a.cmd_stride > 0 ? cmdv.data() : nullptr; a.term = term.data(); a.trunc = trunc.data(); a.scn_row = rows.data();
  auto meta = [&](int env) { return reinterpret_cast<int*>(state.data() + (size_t)env * a.s_stride + a.s_meta); };
  auto clear = [&]() {   // curves_clear_kernel
    for (int i = 0; i < n; i++)
      for (int cls = 0; cls < 2; cls++)
        for (int w = 0; w < cw[i]; w++) cells[(size_t)coff[i] + (size_t)cls * cw[i] + w] = curves_clear_word(w, nt[i]);
  };
  auto begin = [&]() {   // curves_begin_kernel
    for (int env = 0; env < N; env++) {
      if (!curves_begin_applies(a, env)) continue;
      for (int lane = 0; lane < lanes; lane++) curves_begin_lane(a, env, lane, lanes);
      clk[env] = meta(env)[0];
    }
  };
  clear();
  PlainOps ops;
  for (;;) {
    const int ev = rd_i();
    if (ev == 1) {
      a.mask = mask.data();
      for (auto& x : mask) x = (uint8_t)rd_i();
      for (int env = 0; env < N; env++) meta(env)[0] = rd_i();
      begin();
    } else if (ev == 4) {
      a.mask = nullptr;
      for (int env = 0; env < N; env++) meta(env)[0] = rd_i();
      clear();
      begin();
    } else if (ev == 2) {   // curves_step_kernel, as two ranges
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
          const int tnow = clk[env], te = term[env] != 0, tr = trunc[env] != 0;
          for (int lane = 0; lane < lanes; lane++) curves_sample_lane(a, env, lane, lanes, tnow, rows[env], (te | tr) != 0);
          if (te | tr)
            for (int lane = 0; lane < lanes; lane++) curves_fold_lane(a, env, lane, lanes, rows[env], te, ops);
          clk[env] = meta(env)[0];
        }
    } else if (ev == 3) {
      break;
    } else return 2;
  }
  for (int w = 0; w < words; w++) printf("%u ", cells[w]);
  printf("\n");
  return 0;
}
