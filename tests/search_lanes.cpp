// Host driver of the limit search's rule (cosim_amd/csrc/cosim_search.h) and of its table rules (validate_search / pack_search,
// cosim_amd/csrc/cosim_tables.h), built by tests/test_search_host.py as plain C++ (once more with -fsanitize=address,undefined): runs
// the functions the kernels of cosim_search.hip call, lane by lane the way they call them.  Every word travels as a decimal int32,
// floats as their bits.  The first word picks the job:
//   0 rule:     table | fall flag N | row[N] meta4[N] | events until -1: 1 te[N] tr[N] meta4[N] meta15[N]  |  2 flag mask[N] meta4[N]
//               out: "rec <16 words>" per env, "ring <slots * 4 words>" per env, "remaining <n>"
//   1 apply:    S mode cd gid_off nkey npush | key_adr | key_t | key_cmd | push_adr | push_t | push_v | n | per lane: env ep t targets
//               level cmd_in[cd] quat[4]        out: per lane: row pushed cmd_out[cd] qvel[3]
//   2 validate: scn_S mode auto_reset | key_adr[scn_S + 1] | push_adr[scn_S + 1] | table
//               out: "ERR <message>" | "OK <n_items>", then "arr <word offset> <words>" per array read back through its patched pointer
//   table: S slots has[S] lo hi x0 d0 d_min rule trials targets fail_mask rev_skip ([S] each): the words of cosim_set_param "search"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <vector>

#include "cosim_tables.h"

using namespace cosim;

static int rd() {
  int v = 0;
  if (scanf("%d", &v) != 1) exit(2);
  return v;
}
static float rd_f() { return search_float(rd()); }

struct Words {
  int S = 0, slots = 0;
  std::unique_ptr<int32_t[]> w;   // exactly 11 S words
  SrchRaw raw() const {
    const int32_t* p = w.get();
    const size_t n = (size_t)S;
    const auto f = [&](int k) { return reinterpret_cast<const float*>(p + k * n); };
    return {S, slots, p, f(1), f(2), f(3), f(4), f(5), p + 6 * n, p + 7 * n, p + 8 * n, p + 9 * n, p + 10 * n};
  }
};
static Words rd_table() {
  Words t;
  t.S = rd(); t.slots = rd();
  if (t.S < 1 || t.S > 4096) exit(2);
  t.w.reset(new int32_t[11 * (size_t)t.S]);
  for (int k = 0; k < 11 * t.S; k++) t.w[k] = rd();
  return t;
}
// the table as the kernels see it: pointers into an image of its own
struct Placed {
  WordPacker pk;
  SrchTable tab = {};
  std::unique_ptr<int32_t[]> dev;
  explicit Placed(const Words& t) {
    SrchShape v;
    for (int s = 0; s < t.S; s++) v.n += t.w[s] != 0;
    pack_search(pk, tab, t.raw(), v);
    dev.reset(new int32_t[pk.words()]);
    memcpy(dev.get(), pk.data(), pk.bytes());
    pk.patch(dev.get());
  }
};

static int job_rule() {
  const Words t = rd_table();
  if (t.slots < 1 || t.slots > SRCH_MAX_SLOTS) return 2;
  const Placed P(t);
  const int fall = rd(), flag0 = rd(), N = rd();
  if (N < 1 || N > 4096) return 2;
  std::vector<int> row(N), meta4(N), te(N), tr(N), meta15(N), mask(N);
  for (auto& x : row) x = rd();
  for (auto& x : meta4) x = rd();
  std::vector<int> rec((size_t)N * SRCH_NCNT), ring((size_t)N * t.slots * SRCH_TRIAL_WORDS, 0);
  int remaining = 0;
  for (int i = 0; i < N; i++) {   // search_init_kernel
    const SrchItem it = search_item(P.tab, row[i]);
    search_init(&rec[(size_t)i * SRCH_NCNT], it, meta4[i], flag0);
    remaining += it.has;
  }
  for (int ev = rd(); ev != -1; ev = rd()) {
    if (ev == 1) {   // search_step_kernel
      for (auto& x : te) x = rd();
      for (auto& x : tr) x = rd();
      for (auto& x : meta4) x = rd();
      for (auto& x : meta15) x = rd();
      for (int i = 0; i < N; i++) {
        int meta[16] = {0};
        meta[4] = meta4[i]; meta[15] = meta15[i];
        remaining -= search_step_lane(&rec[(size_t)i * SRCH_NCNT], &ring[(size_t)i * t.slots * SRCH_TRIAL_WORDS], t.slots, search_item(P.tab, row[i]),
                                      te[i] != 0, tr[i] != 0, meta, fall);
      }
    } else if (ev == 2) {   // search_begin_kernel
      const int flag = rd();
      for (auto& x : mask) x = rd();
      for (auto& x : meta4) x = rd();
      for (int i = 0; i < N; i++)
        if (mask[i]) search_begin_lane(&rec[(size_t)i * SRCH_NCNT], flag, meta4[i]);
    } else return 2;
  }
  for (int i = 0; i < N; i++) {
    printf("rec");
    for (int w = 0; w < SRCH_NCNT; w++) printf(" %d", rec[(size_t)i * SRCH_NCNT + w]);
    printf("\n");
  }
  for (int i = 0; i < N; i++) {
    printf("ring");
    for (int w = 0; w < t.slots * SRCH_TRIAL_WORDS; w++) printf(" %d", ring[(size_t)i * t.slots * SRCH_TRIAL_WORDS + w]);
    printf("\n");
  }
  printf("remaining %d\n", remaining);
  return 0;
}

static int job_apply() {
  ScnTable T;
  memset(&T, 0, sizeof T);
  T.n_scn = rd(); T.mode = rd(); T.cd = rd(); T.gid_off = (unsigned)rd();
  const int nkey = rd(), npush = rd();
  if (T.n_scn < 1 || T.cd < 0 || T.cd > 6 || nkey < 0 || npush < 0) return 2;
  std::vector<int32_t> key_adr(T.n_scn + 1), key_t(nkey), push_adr(T.n_scn + 1), push_t(2 * npush);
  std::vector<float> key_cmd((size_t)nkey * T.cd), push_v(3 * (size_t)npush);
  for (auto& x : key_adr) x = rd();
  for (auto& x : key_t) x = rd();
  for (auto& x : key_cmd) x = rd_f();
  for (auto& x : push_adr) x = rd();
  for (auto& x : push_t) x = rd();
  for (auto& x : push_v) x = rd_f();
  T.key_adr = key_adr.data(); T.key_t = key_t.data(); T.key_cmd = key_cmd.data();
  T.push_adr = push_adr.data(); T.push_t = push_t.data(); T.push_v = push_v.data();
  const int n = rd();
  for (int i = 0; i < n; i++) {
    const int env = rd(), ep = rd(), t = rd(), targets = rd();
    const float level = rd_f();
    float cmd_in[6] = {0}, cmd_out[6] = {0}, quat[4], qvel[3] = {0.f, 0.f, 0.f};
    for (int c = 0; c < T.cd; c++) cmd_in[c] = rd_f();
    for (int c = 0; c < 4; c++) quat[c] = rd_f();
    const int row = scenario_row(T, env, ep);
    const int pushed = scenario_apply_scaled(T, row, t, cmd_in, cmd_out, quat, qvel, true, targets, level);
    printf("%d %d", row, pushed);
    for (int c = 0; c < T.cd; c++) printf(" %d", search_bits(cmd_out[c]));
    for (int c = 0; c < 3; c++) printf(" %d", search_bits(qvel[c]));
    printf("\n");
  }
  return 0;
}

static int job_validate() {
  const int scn_S = rd(), mode = rd(), auto_reset = rd();
  if (scn_S < 0 || scn_S > 4096) return 2;
  std::vector<int32_t> key_adr(scn_S + 1), push_adr(scn_S + 1);
  for (auto& x : key_adr) x = rd();
  for (auto& x : push_adr) x = rd();
  const Words t = rd_table();
  const SrchDims d = {scn_S, mode, auto_reset, key_adr.data(), push_adr.data()};
  const SrchShape v = validate_search(d, t.raw());
  if (!v.err.empty()) { printf("ERR %s\n", v.err.c_str()); return 0; }
  printf("OK %d\n", v.n);
  const Placed P(t);
  const int32_t* arrs[11] = {P.tab.has, (const int32_t*)P.tab.lo, (const int32_t*)P.tab.hi, (const int32_t*)P.tab.x0, (const int32_t*)P.tab.d0,
                             (const int32_t*)P.tab.d_min, P.tab.rule, P.tab.trials, P.tab.targets, P.tab.fail_mask, P.tab.rev_skip};
  for (const int32_t* a : arrs) {
    printf("arr %lld", (long long)(a - P.dev.get()));
    for (int s = 0; s < t.S; s++) printf(" %d", a[s]);
    printf("\n");
  }
  return 0;
}

int main() {
  switch (rd()) {
    case 0: return job_rule();
    case 1: return job_apply();
    case 2: return job_validate();
    default: return 2;
  }
}
