// Host driver of the GROUPED curve rule (cosim_amd/csrc/cosim_curves.h: the group fields of CurArgs, curves_fold_group_lane), built by
// tests/test_curve_groups_host.py as plain C++ (once more with -fsanitize=address,undefined): tests/curves_lanes.cpp with a group word per
// env and step.  Reads the items and a script of control steps from stdin, runs curves_sample_lane / curves_fold_group_lane lane by lane
// the way curves_step_grouped_kernel's waves do with 64, and writes the G planes.  The "atomics" are plain operations.  Floats travel as
// their uint32 bits.  Every buffer has exactly the size the rule may touch: G planes of `words`, one `ungrouped` word.  A step is issued
// as two env ranges, in either order.
//   in:  S n | adr[S+1] | t[3n] | signal[n] | index[n] | bins[n] | nt[n] | soff[n] | coff[n] | cw[n] | lo[n] | hi[n] | inv_w[n]
//        | SW words lanes N info_dim nu cd nq nv reversed G | clock[N] (every env begins an episode at this clock) | events ...
//        event 2: step   per env: te tr row meta0_after group info[info_dim] cmd[cd] qpos[nq] qvel[nv]
//        event 3: end    the result is written and the program ends
//   out: raw little-endian uint32: G * words cell words | ungrouped | per env the stage words that still hold a sample
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
  const int nq = rd_i(), nv = rd_i(), reversed = rd_i(), G = rd_i();
  if (T.SW < 1 || words < 2 || (words & 1) || lanes < 1 || N < 1 || G < 1 || G > CUR_MAX_GROUPS) return 2;
  a.n_envs = N; a.s_qpos = 0; a.s_qvel = nq; a.s_meta = nq + nv; a.s_stride = nq + nv + 16;
  std::vector<float> state((size_t)N * a.s_stride, 0.f), info((size_t)N * a.info_dim), cmdv((size_t)N * a.cmd_stride);
  std::vector<int> stage((size_t)N * T.SW, CUR_NONE), clk(N, 0), rows(N);
  std::vector<int32_t> group(N, 0);
  std::vector<unsigned long long> cells64((size_t)G * words / 2, 0ull);   // 8-byte aligned, as the device allocation is; W is even
  unsigned* cells = reinterpret_cast<unsigned*>(cells64.data());
  unsigned ungrouped = 0;
  std::vector<uint8_t> term(N), trunc(N);
  a.stage = stage.data(); a.clk = clk.data(); a.cells = cells; a.state = state.data();
  a.info = info.data(); a.cmd = a.cmd_stride > 0 ? cmdv.data() : nullptr; a.term = term.data(); a.trunc = trunc.data(); a.scn_row = rows.data();
  a.group = group.data(); a.n_groups = G; a.plane_words = (size_t)words; a.ungrouped = &ungrouped;
  auto meta = [&](int env) { return reinterpret_cast<int*>(state.data() + (size_t)env * a.s_stride + a.s_meta); };
  for (int g = 0; g < G; g++)   // curves_clear_grouped_kernel
    for (int i = 0; i < n; i++)
      for (int cls = 0; cls < 2; cls++)
        for (int w = 0; w < cw[i]; w++) cells[(size_t)g * words + (size_t)coff[i] + (size_t)cls * cw[i] + w] = curves_clear_word(w, nt[i]);
  for (int env = 0; env < N; env++) clk[env] = meta(env)[0] = rd_i();   // curves_begin_kernel on an empty stage
  PlainOps ops;
  for (;;) {
    const int ev = rd_i();
    if (ev == 2) {   // curves_step_grouped_kernel, as two ranges
      for (int env = 0; env < N; env++) {
        term[env] = (uint8_t)rd_i(); trunc[env] = (uint8_t)rd_i(); rows[env] = rd_i(); meta(env)[0] = rd_i(); group[env] = rd_i();
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
          if (te | tr) {
            const int g = a.group[env];   // read once, the same value for every lane
            for (int lane = 0; lane < lanes; lane++) curves_fold_group_lane(a, env, lane, lanes, rows[env], te, g, ops);
          }
          clk[env] = meta(env)[0];
        }
    } else if (ev == 3) {
      break;
    } else return 2;
  }
  if (fwrite(cells, sizeof(unsigned), (size_t)G * words, stdout) != (size_t)G * words) return 3;
  if (fwrite(&ungrouped, sizeof ungrouped, 1, stdout) != 1) return 3;
  for (int env = 0; env < N; env++) {
    unsigned held = 0;
    for (int w = 0; w < T.SW; w++) held += stage[(size_t)env * T.SW + w] != CUR_NONE;
    if (fwrite(&held, sizeof held, 1, stdout) != 1) return 3;
  }
  return 0;
}
