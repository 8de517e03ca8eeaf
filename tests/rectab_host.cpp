// Host driver of the recurrent policy table's host code (cosim_amd/csrc/cosim_rectab.h), built by tests/test_recurrent_table_host.py as
// plain C++ (once more with -fsanitize=address,undefined): reads one raw table from stdin the way cosim_recurrent_table_create is handed
// it, runs the validator and prints the refusal, or builds the tile list and packs the image and prints both.  Every array has exactly
// the size the caller gave it.  The weights are made here: every word of an array of policy k is 1000 k + code, code = 10 l + 1 (+ 2: its
// bias) for encoder layer l, 51 / 52 / 53 for W / R / B and 60 + 10 l + 1 (+ 2) for head layer l, so the image tells which array a word
// belongs to; padding is 0.
//   in:  K | ne edims eact ehas_bias | lstm_in hidden has_B | nh hdims hact hhas_bias | n policy_of_row | n_ranges ranges | lds_limit
//        an int is a decimal; an array is its count (-1: a null pointer) and its ints; the has_* arrays hold 0 / 1
//   out: "ERR <message>"  |  "OK", then "shape <ld_m> <ld_x> <hmax> <lds bytes>", "rows <n> <ints>", one "tile <policy> <start> <count>"
//        per tile, one "span <first> <count>" per range, one "desc <40 words, the two alpha triples as ints>" per policy and
//        "image <n> <words as ints>"
#include <stdio.h>
#include <stdlib.h>

#include <memory>
#include <string>
#include <vector>

#include "cosim_rectab.h"

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

static std::vector<std::unique_ptr<float[]>> keep;
static const float* filled(long long n, int value) {
  keep.emplace_back(new float[(size_t)n]);
  for (long long q = 0; q < n; q++) keep.back()[q] = (float)value;
  return keep.back().get();
}
static bool width_ok(int w) { return w >= 1 && w <= POL_MAXD; }

int main() {
  const int K = rd();
  const Arr ne = rd_arr(), edims = rd_arr(), eact = rd_arr(), ehb = rd_arr();
  const Arr lstm_in = rd_arr(), hidden = rd_arr(), has_B = rd_arr();
  const Arr nh = rd_arr(), hdims = rd_arr(), hact = rd_arr(), hhb = rd_arr();
  const int n = rd();
  const Arr por = rd_arr();
  const int n_ranges = rd();
  const Arr ranges = rd_arr();
  const int lds_limit = rd();
  // weights of exactly the size their dims ask for, where the dims are fit to be used at all (the validator refuses the table before
  // it reads an array whose dims are not)
  const bool shaped = K >= 1 && K <= POL_MAXK && ne.n == K && nh.n == K && edims.n == K * (REC_MAXE + 1) && hdims.n == K * (REC_MAXH + 1) &&
                      ehb.n == K * REC_MAXE && hhb.n == K * REC_MAXH && lstm_in.n == K && hidden.n == K && has_B.n == K;
  std::vector<const float*> ew, eb, hw, hb, W, R, B;
  if (shaped) {
    ew.assign((size_t)K * REC_MAXE, nullptr); eb = ew;
    hw.assign((size_t)K * REC_MAXH, nullptr); hb = hw;
    W.assign(K, nullptr); R = W; B = W;
    for (int k = 0; k < K; k++) {
      for (int l = 0; l < REC_MAXE && l < ne.p[k]; l++) {
        const int I = edims.p[k * (REC_MAXE + 1) + l], O = edims.p[k * (REC_MAXE + 1) + l + 1];
        if (!width_ok(I) || !width_ok(O)) continue;
        ew[k * REC_MAXE + l] = filled((long long)I * O, 1000 * k + 10 * l + 1);
        if (ehb.p[k * REC_MAXE + l]) eb[k * REC_MAXE + l] = filled(O, 1000 * k + 10 * l + 2);
      }
      for (int l = 0; l < REC_MAXH && l < nh.p[k]; l++) {
        const int I = hdims.p[k * (REC_MAXH + 1) + l], O = hdims.p[k * (REC_MAXH + 1) + l + 1];
        if (!width_ok(I) || !width_ok(O)) continue;
        hw[k * REC_MAXH + l] = filled((long long)I * O, 1000 * k + 60 + 10 * l + 1);
        if (hhb.p[k * REC_MAXH + l]) hb[k * REC_MAXH + l] = filled(O, 1000 * k + 60 + 10 * l + 2);
      }
      const int I = lstm_in.p[k], H = hidden.p[k];
      if (width_ok(I) && width_ok(H)) {
        W[k] = filled(4LL * H * I, 1000 * k + 51);
        R[k] = filled(4LL * H * H, 1000 * k + 52);
        if (has_B.p[k]) B[k] = filled(8LL * H, 1000 * k + 53);
      } else {
        W[k] = R[k] = filled(1, 0);   // refused for its widths before either is read
      }
    }
  }
  const float* const dummy = nullptr;
  const RecRaw raw = {K, ne.get(), edims.get(), eact.get(), nullptr, shaped ? ew.data() : &dummy, shaped ? eb.data() : nullptr,
                      lstm_in.get(), hidden.get(), shaped ? W.data() : &dummy, shaped ? R.data() : &dummy, shaped ? B.data() : nullptr,
                      nh.get(), hdims.get(), hact.get(), nullptr, shaped ? hw.data() : &dummy, shaped ? hb.data() : nullptr,
                      n, por.get(), n_ranges, ranges.get()};
  const RecShape v = validate_recurrent_table(raw, lds_limit);
  if (!v.err.empty()) {
    printf("ERR %s\n", v.err.c_str());
    return 0;
  }
  const PolTiles t = build_policy_tiles(raw.policy_of_row, K, raw.ranges, n_ranges);
  const RecImage im = pack_recurrent_image(raw);
  printf("OK\nshape %d %d %d %lld\nrows %zu", v.ld_m, v.ld_x, v.hmax, rec_lds_bytes(v.ld_m, v.ld_x), t.rows.size());
  for (int32_t r : t.rows) printf(" %d", r);
  printf("\n");
  for (const PolTile& x : t.tiles) printf("tile %d %d %d\n", x.policy, x.start, x.count);
  for (size_t i = 0; i < t.tile_span.size(); i += 2) printf("span %d %d\n", t.tile_span[i], t.tile_span[i + 1]);
  for (const RecDesc& d : im.desc) {
    printf("desc %d", d.ne);
    for (int x : d.edims) printf(" %d", x);
    for (int x : d.eact) printf(" %d", x);
    for (float x : d.ealpha) printf(" %d", (int)x);
    for (int x : d.ewoff) printf(" %d", x);
    for (int x : d.eboff) printf(" %d", x);
    printf(" %d %d %d %d %d %d", d.I, d.H, d.woff, d.roff, d.boff, d.nh);
    for (int x : d.hdims) printf(" %d", x);
    for (int x : d.hact) printf(" %d", x);
    for (float x : d.halpha) printf(" %d", (int)x);
    for (int x : d.hwoff) printf(" %d", x);
    for (int x : d.hboff) printf(" %d", x);
    printf(" %d\n", d.vec);
  }
  printf("image %zu", im.words.size());
  for (float x : im.words) printf(" %d", (int)x);
  printf("\n");
  return 0;
}
