// Host driver of the extended half of the policy table's host code (cosim_amd/csrc/cosim_poltab.h: PolExtRaw, check_extras,
// pack_policy_extras), built by tests/test_poltab_ext_host.py as plain C++ (once more with -fsanitize=address,undefined).  It reads one
// raw table with extras from stdin the way cosim_policy_table_create_ex is handed it, runs the validator and prints the refusal, or
// packs the image and prints it with both records of every policy.  Weights as tests/poltab_host.cpp makes them (64 k + 8 l + 1, bias
// + 2); the vectors of policy k are made here too, every word of one the same: input item i 10000 + 100 k + i, output item i 20000 +
// 100 k + i, scale of slot s 30000 + 100 k + s, bias 40000 + 100 k + s.  Every array has exactly the size its width asks for.
//   in:  K | nl dims act has_bias | n policy_of_row | n_ranges ranges | has_ext, and if 1 per policy:
//        n_in n_out | in_op x4 | out_op x4 | in_has_vec x4 | out_has_vec x4 | in_lo in_hi out_lo out_hi x4 each (floats) |
//        ln_where x7 | ln_eps x7 (floats) | ln_has_scale x7 | ln_has_bias x7
//        an int is a decimal; an array is its count (-1: a null pointer) and its ints; a float is what strtof reads ("inf", "nan")
//   out: "ERR <message>"  |  "OK", "maxd <n>", one "desc ..." per policy as poltab_host.cpp, "image <n> <words as ints>", "next <n>"
//        (0: no policy has extras) and one "ext <64 words as int32 bit patterns>" per policy
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <string>
#include <vector>

#include "cosim_poltab.h"

using namespace cosim;

static int rd() {
  int v = 0;
  if (scanf("%d", &v) != 1) exit(2);
  return v;
}
static float rdf() {
  char buf[64];
  if (scanf("%63s", buf) != 1) exit(2);
  return strtof(buf, nullptr);
}

struct Arr {
  std::unique_ptr<int32_t[]> p;
  int n = -1;
  const int32_t* get() const { return n < 0 ? nullptr : p.get(); }
};
static Arr rd_arr() {
  Arr a;
  a.n = rd();
  if (a.n < 0) return a;
  a.p.reset(new int32_t[a.n]);
  for (int k = 0; k < a.n; k++) a.p[k] = rd();
  return a;
}

int main() {
  const int K = rd();
  const Arr nl = rd_arr(), dims = rd_arr(), act = rd_arr(), has_bias = rd_arr();
  const int n = rd();
  const Arr por = rd_arr();
  const int n_ranges = rd();
  const Arr ranges = rd_arr();
  std::vector<std::unique_ptr<float[]>> keep;
  const auto filled = [&](int count, float value) {
    keep.emplace_back(new float[count > 0 ? count : 1]);
    for (int q = 0; q < count; q++) keep.back()[q] = value;
    return (const float*)keep.back().get();
  };
  std::vector<const float*> w, b;
  const bool shaped = K >= 1 && K <= POL_MAXK && nl.n == K && dims.n == K * (POL_MAXL + 1) && has_bias.n == K * POL_MAXL;
  const auto width = [&](int k, int l) {   // a width fit to size an array with, or 0
    if (!shaped || l < 0 || l > POL_MAXL) return 0;
    const int d = dims.p[k * (POL_MAXL + 1) + l];
    return d >= 1 && d <= POL_MAXD ? d : 0;
  };
  if (shaped) {
    w.assign((size_t)K * POL_MAXL, nullptr); b.assign((size_t)K * POL_MAXL, nullptr);
    for (int k = 0; k < K; k++)
      for (int l = 0; l < POL_MAXL && l < nl.p[k]; l++) {
        const int I = width(k, l), O = width(k, l + 1);
        if (!I || !O) continue;   // the validator refuses the table before it reads this layer
        w[k * POL_MAXL + l] = filled(I * O, (float)(64 * k + 8 * l + 1));
        if (has_bias.p[k * POL_MAXL + l]) b[k * POL_MAXL + l] = filled(O, (float)(64 * k + 8 * l + 2));
      }
  }
  std::vector<PolExtRaw> ext;
  if (rd() == 1 && shaped) {
    ext.resize(K);
    for (int k = 0; k < K; k++) {
      PolExtRaw& e = ext[k];
      memset(&e, 0, sizeof e);
      e.n_in = rd(); e.n_out = rd();
      int in_has[POL_MAXS], out_has[POL_MAXS], g_has[POL_MAXL + 1], b_has[POL_MAXL + 1];
      for (int i = 0; i < POL_MAXS; i++) e.in_op[i] = rd();
      for (int i = 0; i < POL_MAXS; i++) e.out_op[i] = rd();
      for (int i = 0; i < POL_MAXS; i++) in_has[i] = rd();
      for (int i = 0; i < POL_MAXS; i++) out_has[i] = rd();
      for (int i = 0; i < POL_MAXS; i++) e.in_lo[i] = rdf();
      for (int i = 0; i < POL_MAXS; i++) e.in_hi[i] = rdf();
      for (int i = 0; i < POL_MAXS; i++) e.out_lo[i] = rdf();
      for (int i = 0; i < POL_MAXS; i++) e.out_hi[i] = rdf();
      for (int s = 0; s <= POL_MAXL; s++) e.ln_where[s] = rd();
      for (int s = 0; s <= POL_MAXL; s++) e.ln_eps[s] = rdf();
      for (int s = 0; s <= POL_MAXL; s++) g_has[s] = rd();
      for (int s = 0; s <= POL_MAXL; s++) b_has[s] = rd();
      const int last = nl.p[k] >= 1 && nl.p[k] <= POL_MAXL ? nl.p[k] : 0;
      for (int i = 0; i < POL_MAXS; i++) {
        if (in_has[i]) e.in_vec[i] = filled(width(k, 0), (float)(10000 + 100 * k + i));
        if (out_has[i]) e.out_vec[i] = filled(width(k, last), (float)(20000 + 100 * k + i));
      }
      for (int s = 0; s <= POL_MAXL; s++) {
        if (g_has[s]) e.ln_gamma[s] = filled(width(k, s), (float)(30000 + 100 * k + s));
        if (b_has[s]) e.ln_beta[s] = filled(width(k, s), (float)(40000 + 100 * k + s));
      }
    }
  }
  const float* const dummy = nullptr;
  const PolRaw raw = {K, nl.get(), dims.get(), act.get(), nullptr, shaped ? w.data() : &dummy, shaped ? b.data() : nullptr, n, por.get(), n_ranges, ranges.get(),
                      ext.empty() ? nullptr : ext.data()};
  const PolShape v = validate_policy_table(raw, "cosim_policy_table_create_ex");
  if (!v.err.empty()) {
    printf("ERR %s\n", v.err.c_str());
    return 0;
  }
  const PolImage im = pack_policy_image(raw);
  printf("OK\nmaxd %d\n", v.maxd);
  for (const PolDesc& d : im.desc) {
    printf("desc %d", d.nl);
    for (int x : d.dims) printf(" %d", x);
    for (int x : d.act) printf(" %d", x);
    for (int x : d.woff) printf(" %d", x);
    for (int x : d.boff) printf(" %d", x);
    printf("\n");
  }
  printf("image %zu", im.words.size());
  for (float x : im.words) printf(" %d", (int)x);
  printf("\nnext %zu\n", im.ext.size());
  for (const PolExt& x : im.ext) {
    int32_t words[64];
    memcpy(words, &x, sizeof words);
    printf("ext");
    for (int32_t q : words) printf(" %d", q);
    printf("\n");
  }
  return 0;
}
