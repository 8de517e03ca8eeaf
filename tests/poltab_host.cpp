// Host driver of the policy table's host code (cosim_amd/csrc/cosim_poltab.h), built by tests/test_policy_table_host.py as plain C++
// (once more with -fsanitize=address,undefined): reads one raw table from stdin the way cosim_policy_table_create is handed it, runs
// the validator and prints the refusal, or builds the tile list and packs the image and prints both.  Every array has exactly the size
// the caller gave it.  The weights are made here: every word of layer l of policy k is 64 k + 8 l + 1, of its bias 64 k + 8 l + 2, so
// the image tells which array a word belongs to; padding is 0.
//   in:  K | nl dims act has_bias | n policy_of_row | n_ranges ranges
//        an int is a decimal; an array is its count (-1: a null pointer) and its ints; has_bias: [K][6] of 0 / 1
//   out: "ERR <message>"  |  "OK", then "rows <n> <ints>", one "tile <policy> <start> <count>" per tile, one "span <first> <count>" per
//        range, one "desc <nl> <dims x7> <act x6> <woff x6> <boff x6>" per policy and "image <n> <words as ints>"
#include <stdio.h>
#include <stdlib.h>

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
  // weights of exactly the size their dims ask for, where the dims are fit to be used at all
  std::vector<std::unique_ptr<float[]>> keep;
  std::vector<const float*> w, b;
  const bool shaped = K >= 1 && K <= POL_MAXK && nl.n == K && dims.n == K * (POL_MAXL + 1) && has_bias.n == K * POL_MAXL;
  if (shaped) {
    w.assign((size_t)K * POL_MAXL, nullptr); b.assign((size_t)K * POL_MAXL, nullptr);
    for (int k = 0; k < K; k++)
      for (int l = 0; l < POL_MAXL && l < nl.p[k]; l++) {
        const int I = dims.p[k * (POL_MAXL + 1) + l], O = dims.p[k * (POL_MAXL + 1) + l + 1];
        if (I < 1 || I > POL_MAXD || O < 1 || O > POL_MAXD) continue;   // the validator refuses the table before it reads this layer
        keep.emplace_back(new float[(size_t)I * O]);
        for (int q = 0; q < I * O; q++) keep.back()[q] = (float)(64 * k + 8 * l + 1);
        w[k * POL_MAXL + l] = keep.back().get();
        if (has_bias.p[k * POL_MAXL + l]) {
          keep.emplace_back(new float[O]);
          for (int q = 0; q < O; q++) keep.back()[q] = (float)(64 * k + 8 * l + 2);
          b[k * POL_MAXL + l] = keep.back().get();
        }
      }
  }
  const float* const dummy = nullptr;
  const PolRaw raw = {K, nl.get(), dims.get(), act.get(), nullptr, shaped ? w.data() : &dummy, shaped ? b.data() : nullptr, n, por.get(), n_ranges, ranges.get()};
  const PolShape v = validate_policy_table(raw);
  if (!v.err.empty()) {
    printf("ERR %s\n", v.err.c_str());
    return 0;
  }
  const PolTiles t = build_policy_tiles(raw.policy_of_row, K, raw.ranges, n_ranges);
  const PolImage im = pack_policy_image(raw);
  printf("OK\nmaxd %d\nrows %zu", v.maxd, t.rows.size());
  for (int32_t r : t.rows) printf(" %d", r);
  printf("\n");
  for (const PolTile& x : t.tiles) printf("tile %d %d %d\n", x.policy, x.start, x.count);
  for (size_t i = 0; i < t.tile_span.size(); i += 2) printf("span %d %d\n", t.tile_span[i], t.tile_span[i + 1]);
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
  printf("\n");
  return 0;
}
