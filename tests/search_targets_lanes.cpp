// Host driver of what a limit search adds to its first form (cosim_amd/csrc/cosim_search.h, cosim_fault.h, cosim_actfault.h,
// cosim_obsfault.h, cosim_scnparams.h, cosim_tables.h): harder up / down, a check verdict as a failure criterion, the level multiplied
// into marked parameter windows, observation faults and action faults, the long table form and the rules of marked items.  Built by tests/test_search_targets_host.py as plain C++ (once more with
// -fsanitize=address,undefined); runs the functions the kernels call, lane by lane the way they call them.  Every word travels as a
// decimal int32, floats as their bits.  The first word picks the job:
//   0 rule:     table | fall flag N | row[N] meta4[N] | events until -1:
//                 1 te[N] tr[N] meta4[N] meta15[N] fail_lo[N] fail_hi[N] inc_lo[N] inc_hi[N]  |  2 flag mask[N] meta4[N]
//               out: "rec <16 words>" per env, "ring <slots * 4 words>" per env, "remaining <n>"
//   1 apply:    S mode env_id0 n | adr[S + 1] | item[4 n] | nu seed_lo seed_hi n_envs | per env: env ep t step_count level raw[nu] lastact[nu]
//               out: per env: row eff[nu] plain[nu]   (plain: actfault_apply, the walk without a search, of the same words)
//   2 validate: scn_S mode auto_reset | key_adr[scn_S + 1] | push_adr[scn_S + 1] | has_checks [chk_adr[scn_S + 1]] | has_params [adr] |
//               has_obs_faults [adr] | has_action_faults [adr] | table
//               out: "ERR <message>" | "OK <n_items>", then "arr <word offset> <words>" per array read back through its patched pointer
//   3 marks:    nu S n | adr[S + 1] | t[2 n] | elem[n] | op[n] | ord[n] | value[n] | armed | has[S] targets[S] lo[S] hi[S]
//               out: "ERR <message>" | "OK <n> <marked>", then "item <4 words>" per packed record
//               kind 16 action faults (nu = dim) | 8 observation faults (dim = frame_dim, every element stacked, stack_size 2):
//               the first word after the job is the kind, e.g. 3 16 nu S n ...
//   4 params:   S mode env_id0 n | adr[S + 1] | t[2 n] | word[n] | op[n] | value[n] | p_stride n_envs | per env: env ep t level base[p_stride]
//               out: per env: row eff[p_stride] plain[p_stride]   (plain: the form without a search, marks stripped by the caller's table)
//   5 parmarks: nu S n | adr[S + 1] | t[2 n] | field[n] | index[n] | op[n] | value[n] | armed | has[S] targets[S] lo[S] hi[S]
//               out: "ERR <message>" | "OK <n> <marked>"
//   6 obs:      S mode env_id0 n | adr[S + 1] | item[4 n] | sd stack_size frame_dim seed_lo seed_hi n_envs |
//               per env: env ep t step_count level stack[stack_size * sd] out[state_dim]      out: per env: row stack[...] out[...]
//   table: S slots cols | cols * S words: the words of cosim_set_param "search", cols = 11 (short form) or 14
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
  int S = 0, slots = 0, cols = 0;
  std::unique_ptr<int32_t[]> w;   // exactly cols * S words
  SrchRaw raw() const {
    const int32_t* p = w.get();
    const size_t n = (size_t)S;
    const auto f = [&](int k) { return reinterpret_cast<const float*>(p + k * n); };
    SrchRaw r = {S, slots, p, f(1), f(2), f(3), f(4), f(5), p + 6 * n, p + 7 * n, p + 8 * n, p + 9 * n, p + 10 * n};
    if (cols == 14) { r.harder = p + 11 * n; r.chk_lo = p + 12 * n; r.chk_hi = p + 13 * n; }
    return r;
  }
};
static Words rd_table() {
  Words t;
  t.S = rd(); t.slots = rd(); t.cols = rd();
  if (t.S < 1 || t.S > 4096 || (t.cols != 11 && t.cols != 14)) exit(2);
  t.w.reset(new int32_t[(size_t)t.cols * t.S]);
  for (int k = 0; k < t.cols * t.S; k++) t.w[k] = rd();
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
  std::vector<int> row(N), meta4(N), te(N), tr(N), meta15(N), mask(N), v4(N), v5(N), v6(N), v7(N);
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
    if (ev == 1) {   // search_step_checks_kernel
      for (auto* a : {&te, &tr, &meta4, &meta15, &v4, &v5, &v6, &v7})
        for (auto& x : *a) x = rd();
      for (int i = 0; i < N; i++) {
        int meta[16] = {0};
        meta[4] = meta4[i]; meta[15] = meta15[i];
        const int verdict[8] = {0, 0, 0, 0, v4[i], v5[i], v6[i], v7[i]};   // the header of a verdict record (cosim_checks.h)
        const SrchItem it = search_item(P.tab, row[i]);
        const bool ended = te[i] != 0 || tr[i] != 0;
        remaining -= search_step_lane(&rec[(size_t)i * SRCH_NCNT], &ring[(size_t)i * t.slots * SRCH_TRIAL_WORDS], t.slots, it, te[i] != 0, tr[i] != 0, meta, fall,
                                      ended && it.has && (it.chk_lo | it.chk_hi) != 0 ? verdict : nullptr);
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
  FaultTable F;
  memset(&T, 0, sizeof T);
  memset(&F, 0, sizeof F);
  T.n_scn = rd(); T.mode = rd();
  const long long env_id0 = rd();
  const int n = rd();
  if (T.n_scn < 1 || n < 0) return 2;
  T.gid_off = (unsigned)(((env_id0 % T.n_scn) + T.n_scn) % T.n_scn);
  std::vector<int32_t> adr(T.n_scn + 1), item(4 * (size_t)(n + FLT_CHUNK - 1), 0);   // the padding the rule may fetch, and no more
  for (auto& x : adr) x = rd();
  for (size_t k = 0; k < 4 * (size_t)n; k++) item[k] = rd();
  F.adr = adr.data(); F.item = item.data(); F.n_scn = T.n_scn; F.n_items = n;
  const int nu = rd();
  const unsigned seed_lo = (unsigned)rd(), seed_hi = (unsigned)rd();
  const int n_envs = rd();
  if (nu < 1 || nu > 64 || n_envs < 0) return 2;
  for (int i = 0; i < n_envs; i++) {
    const int env = rd(), ep = rd(), t = rd();
    const unsigned c0 = (unsigned)rd();
    const float level = rd_f();
    std::vector<float> raw(nu), lastact(nu);
    for (auto& x : raw) x = rd_f();
    for (auto& x : lastact) x = rd_f();
    const int row = scenario_row(T, env, ep);
    const unsigned long long gid = (unsigned long long)(env_id0 + env);
    ActFaultEnv E;
    E.lastact = lastact.data();
    E.k0 = seed_lo; E.k1 = seed_hi; E.c0 = c0; E.g0 = (unsigned)gid; E.g1 = (unsigned)(gid >> 32);
    printf("%d", row);
    for (int lane = 0; lane < nu; lane++) printf(" %d", search_bits(actfault_apply_scaled(F, row, t, E, lane, raw[lane], level)));
    for (int lane = 0; lane < nu; lane++) printf(" %d", search_bits(actfault_apply(F, row, t, E, lane, raw[lane])));
    printf("\n");
  }
  return 0;
}

static int job_validate() {
  const int scn_S = rd(), mode = rd(), auto_reset = rd();
  if (scn_S < 0 || scn_S > 4096) return 2;
  std::vector<int32_t> key_adr(scn_S + 1), push_adr(scn_S + 1), chk_adr;
  for (auto& x : key_adr) x = rd();
  for (auto& x : push_adr) x = rd();
  std::vector<int32_t> kind_adr[3];
  if (rd()) {
    chk_adr.resize(scn_S + 1);
    for (auto& x : chk_adr) x = rd();
  }
  for (auto& a : kind_adr)
    if (rd()) {
      a.resize(scn_S + 1);
      for (auto& x : a) x = rd();
    }
  const Words t = rd_table();
  SrchDims d = {scn_S, mode, auto_reset, key_adr.data(), push_adr.data(), chk_adr.empty() ? nullptr : chk_adr.data()};
  d.par_adr = kind_adr[0].empty() ? nullptr : kind_adr[0].data();
  d.obs_adr = kind_adr[1].empty() ? nullptr : kind_adr[1].data();
  d.act_adr = kind_adr[2].empty() ? nullptr : kind_adr[2].data();
  const SrchShape v = validate_search(d, t.raw());
  if (!v.err.empty()) { printf("ERR %s\n", v.err.c_str()); return 0; }
  printf("OK %d\n", v.n);
  const Placed P(t);
  std::vector<const int32_t*> arrs = {P.tab.has, (const int32_t*)P.tab.lo, (const int32_t*)P.tab.hi, (const int32_t*)P.tab.x0, (const int32_t*)P.tab.d0,
                                      (const int32_t*)P.tab.d_min, P.tab.rule, P.tab.trials, P.tab.targets, P.tab.fail_mask, P.tab.rev_skip};
  if (t.cols == 14) { arrs.push_back(P.tab.harder); arrs.push_back(P.tab.chk_lo); arrs.push_back(P.tab.chk_hi); }
  else if (P.tab.harder || P.tab.chk_lo || P.tab.chk_hi) return 3;   // the short form leaves the three pointers null
  for (const int32_t* a : arrs) {
    printf("arr %lld", (long long)(a - P.dev.get()));
    for (int s = 0; s < t.S; s++) printf(" %d", a[s]);
    printf("\n");
  }
  return 0;
}

static int job_marks() {
  const int kind = rd();
  const int nu = rd(), S = rd(), n = rd();
  if (S < 1 || S > 4096 || n < 0 || n > 65536) return 2;
  std::vector<int32_t> adr(S + 1), t(2 * (size_t)n), elem(n), op(n), ord(n), has(S), targets(S);
  std::vector<float> value(n), lo(S), hi(S);
  for (auto& x : adr) x = rd();
  for (auto& x : t) x = rd();
  for (auto& x : elem) x = rd();
  for (auto& x : op) x = rd();
  for (auto& x : ord) x = rd();
  for (auto& x : value) x = rd_f();
  const int armed = rd();
  for (auto& x : has) x = rd();
  for (auto& x : targets) x = rd();
  for (auto& x : lo) x = rd_f();
  for (auto& x : hi) x = rd_f();
  const FltRaw raw = {S, adr.data(), t.data(), elem.data(), op.data(), ord.data(), value.data()};
  const FltMarks marks = {kind, has.data(), targets.data(), lo.data(), hi.data()};
  std::vector<unsigned char> el_field(nu > 0 ? nu : 1, 0);
  const ObsDims od = {nu, nu, 2, el_field.data(), 255};
  const FltShape v = kind == SRCH_ACT_FAULTS ? validate_action_faults(nu, raw, armed ? &marks : nullptr) : validate_faults(od, raw, armed ? &marks : nullptr);
  if (!v.err.empty()) { printf("ERR %s\n", v.err.c_str()); return 0; }
  printf("OK %d %d\n", v.n, v.marked);
  for (int i = 0; i < v.n; i++) printf("item %d %d %d %d\n", v.item[4 * i], v.item[4 * i + 1], v.item[4 * i + 2], v.item[4 * i + 3]);
  return 0;
}

static int job_params() {
  ScnTable T;
  ScnParTable P;
  memset(&T, 0, sizeof T);
  memset(&P, 0, sizeof P);
  T.n_scn = rd(); T.mode = rd();
  const long long env_id0 = rd();
  const int n = rd();
  if (T.n_scn < 1 || n < 0) return 2;
  T.gid_off = (unsigned)(((env_id0 % T.n_scn) + T.n_scn) % T.n_scn);
  std::vector<int32_t> adr(T.n_scn + 1), t(2 * (size_t)n), word(n), op(n), plain_op(n);
  std::vector<float> value(n);
  for (auto& x : adr) x = rd();
  for (auto& x : t) x = rd();
  for (auto& x : word) x = rd();
  for (auto& x : op) x = rd();
  for (auto& x : value) x = rd_f();
  for (int i = 0; i < n; i++) plain_op[i] = op[i] & ~SCNPAR_MARK;
  P.adr = adr.data(); P.t = t.data(); P.word = word.data(); P.op = op.data(); P.value = value.data(); P.n_scn = T.n_scn; P.n_items = n;
  ScnParTable Q = P;
  Q.op = plain_op.data();
  const int p_stride = rd(), n_envs = rd();
  if (p_stride < 1 || p_stride > 4096 || n_envs < 0) return 2;
  for (int i = 0; i < n_envs; i++) {
    const int env = rd(), ep = rd(), tt = rd();
    const float level = rd_f();
    std::vector<float> base(p_stride), eff(p_stride), plain(p_stride);
    for (auto& x : base) x = rd_f();
    const int row = scenario_row(T, env, ep);
    for (int lane = 0; lane < 64; lane++) {   // the kernel's wave: lane = word, passes of 64
      scnparams_apply(P, row, tt, base.data(), eff.data(), p_stride, lane, 64, true, level);
      scnparams_apply(Q, row, tt, base.data(), plain.data(), p_stride, lane, 64);
    }
    printf("%d", row);
    for (float x : eff) printf(" %d", search_bits(x));
    for (float x : plain) printf(" %d", search_bits(x));
    printf("\n");
  }
  return 0;
}

static int job_parmarks() {
  const int nu = rd(), S = rd(), n = rd();
  if (S < 1 || S > 4096 || n < 0 || n > 65536) return 2;
  std::vector<int32_t> adr(S + 1), t(2 * (size_t)n), field(n), index(n), op(n), has(S), targets(S);
  std::vector<float> value(n), lo(S), hi(S);
  for (auto& x : adr) x = rd();
  for (auto& x : t) x = rd();
  for (auto& x : field) x = rd();
  for (auto& x : index) x = rd();
  for (auto& x : op) x = rd();
  for (auto& x : value) x = rd_f();
  const int armed = rd();
  for (auto& x : has) x = rd();
  for (auto& x : targets) x = rd();
  for (auto& x : lo) x = rd_f();
  for (auto& x : hi) x = rd_f();
  const TableDims d = {7 + nu, 6 + nu, nu, 8, 16, 4, 0, nu, 2 * nu, 2 * nu + 8};
  const ParRaw raw = {S, adr.data(), t.data(), field.data(), index.data(), op.data(), value.data()};
  const FltMarks marks = {SRCH_PARAMS, has.data(), targets.data(), lo.data(), hi.data()};
  const ParShape v = validate_params(d, raw, armed ? &marks : nullptr);
  if (!v.err.empty()) { printf("ERR %s\n", v.err.c_str()); return 0; }
  printf("OK %d %d\n", v.n, v.marked);
  return 0;
}

static int job_obs() {
  ScnTable T;
  FaultTable F;
  memset(&T, 0, sizeof T);
  memset(&F, 0, sizeof F);
  T.n_scn = rd(); T.mode = rd();
  const long long env_id0 = rd();
  const int n = rd();
  if (T.n_scn < 1 || n < 0) return 2;
  T.gid_off = (unsigned)(((env_id0 % T.n_scn) + T.n_scn) % T.n_scn);
  std::vector<int32_t> adr(T.n_scn + 1), item(4 * (size_t)(n + FLT_CHUNK - 1), 0);
  for (auto& x : adr) x = rd();
  for (size_t k = 0; k < 4 * (size_t)n; k++) item[k] = rd();
  F.adr = adr.data(); F.item = item.data(); F.n_scn = T.n_scn; F.n_items = n;
  const int sd = rd(), S = rd(), frame_dim = rd();
  const unsigned seed_lo = (unsigned)rd(), seed_hi = (unsigned)rd();
  const int n_envs = rd();
  if (sd < 0 || S < 1 || frame_dim < sd || frame_dim > 256 || n_envs < 0) return 2;
  const int state_dim = S * sd + frame_dim - sd;
  for (int i = 0; i < n_envs; i++) {
    const int env = rd(), ep = rd(), t = rd();
    const unsigned c0 = (unsigned)rd();
    const float level = rd_f();
    std::vector<float> stack((size_t)S * sd), out(state_dim);
    for (auto& x : stack) x = rd_f();
    for (auto& x : out) x = rd_f();
    const int row = scenario_row(T, env, ep);
    const unsigned long long gid = (unsigned long long)(env_id0 + env);
    ObsFaultEnv E;
    E.stack = stack.data(); E.out = out.data(); E.sd = sd; E.S = S; E.frame_dim = frame_dim;
    E.k0 = seed_lo; E.k1 = seed_hi; E.c0 = c0; E.g0 = (unsigned)gid; E.g1 = (unsigned)(gid >> 32);
    for (int lane = 0; lane < 64; lane++) obsfault_apply<4, true>(F, row, t, E, lane, 64, 0, level);   // the kernel's wave
    printf("%d", row);
    for (float x : stack) printf(" %d", search_bits(x));
    for (float x : out) printf(" %d", search_bits(x));
    printf("\n");
  }
  return 0;
}

int main() {
  switch (rd()) {
    case 0: return job_rule();
    case 1: return job_apply();
    case 2: return job_validate();
    case 3: return job_marks();
    case 4: return job_params();
    case 5: return job_parmarks();
    case 6: return job_obs();
    default: return 2;
  }
}
