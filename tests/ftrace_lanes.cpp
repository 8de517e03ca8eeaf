// Host driver of the failure-trace kernels' per-env bodies (cosim_amd/csrc/cosim_ftrace.h), built by tests/test_ftrace_host.py as
// plain C++ (a second time with -fsanitize=address,undefined): reads the sizes and a list of operations from stdin, runs
// ftrace_begin_lane / ftrace_step_lane lane by lane the way ftrace_begin_kernel / ftrace_step_kernel do -- every lane of an env
// starts from the counters as they were before any lane ran, the counters are stored once -- over two env ranges in either order,
// then ftrace_open_word, and prints buffers, counters and open headers.  Floats travel as their uint32 bits.
//   in:  N nq nv nu cd info_dim frames keep on_mask spawn_rows fall has_scn lanes reverse split
//        then operations:
//          3 | per env: qpos[nq] qvel[nv] meta4 meta14 meta15 meta11           the state records as they are from now on
//          2 flag | mask[N]                                                    ftrace_begin_kernel
//          1 | actions[N*nu] cmd[N*cd] info[N*info_dim] term[N] trunc[N] scn_row[N]   ftrace_step_kernel over [0, split) and [split, N)
//          0 | open_scn_rows, scn_mode, scn_off                                 ftrace_open_kernel and the dump
//   out: buffers, then counters [N][3], then open headers [N][16], one word per line
#include <stdio.h>
#include <string.h>

#include <vector>

#include "cosim_ftrace.h"
#include "cosim_scenario.h"

static int rd_i() {
  long long v = 0;
  if (scanf("%lld", &v) != 1) v = 0;
  return (int)(unsigned)v;   // floats arrive as uint32 bits
}

static bool same(const cosim::FtCnt& a, const cosim::FtCnt& b) { return memcmp(&a, &b, sizeof a) == 0; }

int main() {
  using namespace cosim;
  const int N = rd_i(), nq = rd_i(), nv = rd_i(), nu = rd_i(), cd = rd_i(), ni = rd_i(), frames = rd_i(), keep = rd_i(), on_mask = rd_i(),
            spawn_rows = rd_i(), fall = rd_i(), has_scn = rd_i(), lanes = rd_i(), reverse = rd_i(), split = rd_i();
  if (N < 1 || N > 4096 || nq < 0 || nv < 0 || nu < 0 || cd < 0 || ni < 0 || frames < 1 || frames > FT_MAX_FRAMES || keep < 1 || keep > FT_MAX_KEEP ||
      lanes < 1 || lanes > 64 || split < 0 || split > N || nq + nv + nu + cd + ni > 4096)
    return 2;
  FtArgs a;
  memset(&a, 0, sizeof a);
  a.n_envs = N; a.nq = nq; a.nv = nv; a.nu = nu; a.cd = cd; a.info_dim = ni; a.F = ftrace_frame_words(nq, nv, nu, cd, ni);
  a.s_qpos = 3; a.s_qvel = 3 + nq + 2; a.s_meta = a.s_qvel + nv + 1; a.s_stride = a.s_meta + 16 + 5;   // (gaps: the offsets are arguments)
  a.frames = frames; a.keep = keep; a.on_mask = on_mask; a.spawn_rows = spawn_rows; a.fall = fall;
  const size_t bw = ftrace_buf_words(frames, a.F);
  std::vector<int> buf((size_t)N * (keep + 1) * bw, 0), cnt((size_t)N * FT_NCNT, 0), scn_row(N, 0);
  std::vector<float> state((size_t)N * a.s_stride, 0.f), actions((size_t)N * nu), cmd((size_t)N * cd), info((size_t)N * ni);
  std::vector<uint8_t> term(N), trunc(N), mask(N);
  a.buf = buf.data(); a.cnt = cnt.data(); a.state = state.data();
  auto put = [&](float* dst) { const int u = rd_i(); memcpy(dst, &u, 4); };
  for (;;) {
    const int op = rd_i();
    if (op == 3) {
      for (int e = 0; e < N; e++) {
        float* rec = state.data() + (size_t)e * a.s_stride;
        for (int w = 0; w < nq; w++) put(rec + a.s_qpos + w);
        for (int w = 0; w < nv; w++) put(rec + a.s_qvel + w);
        int* meta = reinterpret_cast<int*>(rec + a.s_meta);
        meta[4] = rd_i(); meta[14] = rd_i(); meta[15] = rd_i(); meta[11] = rd_i();
      }
    } else if (op == 2) {
      a.flag = rd_i();
      for (auto& m : mask) m = (uint8_t)rd_i();
      a.mask = mask.data();
      for (int e = 0; e < N; e++) {
        if (!ftrace_begin_applies(a, e)) continue;
        const FtCnt c0 = ftrace_load(cnt.data() + (size_t)e * FT_NCNT);
        FtCnt first = c0;
        for (int l = 0; l < lanes; l++) {
          FtCnt c = c0;
          ftrace_begin_lane(a, e, l, lanes, c);
          if (l == 0) first = c;
          else if (!same(first, c)) return 3;
        }
        ftrace_store(cnt.data() + (size_t)e * FT_NCNT, first);
      }
      a.mask = nullptr;
    } else if (op == 1) {
      for (auto& x : actions) put(&x);
      for (auto& x : cmd) put(&x);
      for (auto& x : info) put(&x);
      for (auto& x : term) x = (uint8_t)rd_i();
      for (auto& x : trunc) x = (uint8_t)rd_i();
      for (auto& x : scn_row) x = rd_i();
      a.actions = actions.data(); a.cmd = cd > 0 ? cmd.data() : nullptr; a.info = info.data(); a.term = term.data(); a.trunc = trunc.data();
      a.scn_row = has_scn ? scn_row.data() : nullptr;
      const int ranges[2][2] = {{0, split}, {split, N - split}};
      for (int r = 0; r < 2; r++) {
        a.first = ranges[reverse ? 1 - r : r][0]; a.count = ranges[reverse ? 1 - r : r][1];
        for (int i = 0; i < a.count; i++) {
          const int e = a.first + i;
          const FtCnt c0 = ftrace_load(cnt.data() + (size_t)e * FT_NCNT);
          FtCnt first = c0;
          for (int l = lanes - 1; l >= 0; l--) {   // (no lane depends on another: any order)
            FtCnt c = c0;
            ftrace_step_lane(a, e, l, lanes, c);
            if (l == lanes - 1) first = c;
            else if (!same(first, c)) return 3;
          }
          ftrace_store(cnt.data() + (size_t)e * FT_NCNT, first);
        }
      }
    } else {
      break;
    }
  }
  std::vector<int> open_rows((size_t)N * FT_HDR, 0), open_scn(N, 0);
  for (auto& x : open_scn) x = rd_i();
  ScnTable T;
  memset(&T, 0, sizeof T);
  T.n_scn = has_scn; T.mode = rd_i(); T.gid_off = (unsigned)rd_i();
  for (int e = 0; e < N; e++) {
    const FtCnt c = ftrace_load(cnt.data() + (size_t)e * FT_NCNT);
    const int* meta = reinterpret_cast<const int*>(state.data() + (size_t)e * a.s_stride + a.s_meta);
    const int scn = has_scn ? scenario_row(T, e, meta[11]) + 1 : 0;   // as ftrace_open_kernel computes it
    if (has_scn && scn != open_scn[e] + 1) return 4;
    for (int w = 0; w < FT_HDR; w++) open_rows[(size_t)e * FT_HDR + w] = ftrace_open_word(a, e, w, c, scn);
  }
  for (int x : buf) printf("%d\n", x);
  for (int e = 0; e < N; e++) printf("%d\n%d\n%d\n", cnt[(size_t)e * FT_NCNT], cnt[(size_t)e * FT_NCNT + 1], cnt[(size_t)e * FT_NCNT + 2]);
  for (int x : open_rows) printf("%d\n", x);
  return 0;
}
