// cosim_poltab.h — what the host does with a policy table before it reaches the device (cosim_policy_table_create, include/cosim.h):
// K actor MLPs over one fleet, every env assigned to one of them, evaluated by ONE launch of mlp_grouped_kernel (cosim_mlp.hip).  The
// kernel trusts the row list, the tile list and the offsets it is given, so all of them are made and checked here: the descriptor
// of a policy, the validator, the tile-list builder and the packer of the weight image.  Plain C++ with no HIP in it, in the manner of
// cosim_tables.h: cosim_engine.hip and the host programs (tests/poltab_host.cpp, tests/poltab_ext_host.cpp) both compile it.  An EXTENDED
// actor (cosim_policy_table_create_ex: stages on observation and action, LayerNorm) adds a second record per policy, PolExt, with its
// validator and packer; a table without one is packed exactly as before.
//
// WordPacker (cosim_tables.h) is not used for the image: it lays arrays end to end and patches POINTERS, while a weight matrix has to
// begin at a multiple of 4 words (the kernel's float4 path) and a descriptor holds word OFFSETS, -1 among them.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <string>
#include <vector>

namespace cosim {

constexpr int POL_MAXK = 64;      // policies of a table
constexpr int POL_MAXL = 6;       // = MLP_MAXL
constexpr int POL_MAXD = 512;     // = MLP_MAXD
constexpr int POL_TILE = 32;      // envs of a tile: the rows of one MFMA tile
constexpr int POL_MAXS = 4;       // items of an input or output stage of an extended actor

// One policy as the kernel reads it: 32 words.  woff / boff: word offsets of layer l's weights [dims[l+1], dims[l]] (row-major) and
// bias [dims[l+1]] into the table's one weight image; boff -1: the layer has no bias.
struct PolDesc {
  int32_t nl;
  int32_t dims[POL_MAXL + 1];
  int32_t act[POL_MAXL];      // 0 none, 1 relu, 2 tanh, 3 elu, 4 sigmoid, 5 leaky relu
  float alpha[POL_MAXL];
  int32_t woff[POL_MAXL];
  int32_t boff[POL_MAXL];
};
static_assert(sizeof(PolDesc) == 32 * 4, "PolDesc is 32 words");

// ---- extended actors (cosim_policy_table_create_ex, cosim_mlp_forward_ex): what a policy has besides its Gemm / activation chain.
// Stage item: op 1 add, 2 sub, 3 mul, 4 div -- y (op) v[column], v a vector of the stage's width (the input stage: dims[0], the output
// stage: dims[nl]); 5 clip -- clamp to [lo, hi].  LayerNorm slot s (width dims[s]): 0 the observation, l + 1 the output of layer l;
// where: 0 none, 1 ahead of the layer's activation, 2 behind it (slot 0 has no activation: any of 1, 2).
// The caller's description of ONE policy: the layout of cosim_mlp_extras_t (include/cosim_actor.h).  The vectors are host pointers for a
// table and device pointers for cosim_mlp_forward_ex; the validator only asks whether they are null.
struct PolExtRaw {
  int32_t n_in, n_out;
  int32_t in_op[POL_MAXS], out_op[POL_MAXS];
  const float* in_vec[POL_MAXS];     // ops 1..4; ignored by a clip
  const float* out_vec[POL_MAXS];
  float in_lo[POL_MAXS], in_hi[POL_MAXS], out_lo[POL_MAXS], out_hi[POL_MAXS];   // a clip's bounds; -inf / +inf: none
  int32_t ln_where[POL_MAXL + 1];
  float ln_eps[POL_MAXL + 1];
  const float* ln_gamma[POL_MAXL + 1];
  const float* ln_beta[POL_MAXL + 1];   // null: no bias
};

// whether a policy of nl layers has any extras: the slots behind its last layer are not read, as in check_extras and the packer
inline bool ext_used(const PolExtRaw& e, int nl) {
  bool any = e.n_in != 0 || e.n_out != 0;
  for (int s = 0; s < nl && s <= POL_MAXL; s++) any = any || e.ln_where[s] != 0;
  return any;
}

// One policy's extras as the kernel reads them, the second per-policy record of a table: 64 words.  off / ln_g / ln_b: word offsets
// of the vectors into the table's weight image (each begun at a multiple of 4 words, like the matrices); -1: none.
struct PolStage { int32_t op, off; float lo, hi; };
struct PolExt {
  int32_t n_in, n_out, pad[2];
  PolStage in[POL_MAXS], out[POL_MAXS];
  int32_t ln_where[POL_MAXL + 1], ln_g[POL_MAXL + 1], ln_b[POL_MAXL + 1];
  float ln_eps[POL_MAXL + 1];
};
static_assert(sizeof(PolExt) == 64 * 4, "PolExt is 64 words");

// The refusal of one policy's extras, or an empty string; `who` names the entry point and the policy, nl: the policy's layers.
inline std::string check_extras(const std::string& who, const PolExtRaw& e, int nl) {
  const auto S = [](long long x) { return std::to_string(x); };
  for (int side = 0; side < 2; side++) {
    const char* label = side ? "output" : "input";
    const int n = side ? e.n_out : e.n_in;
    if (n < 0 || n > POL_MAXS) return who + ": " + label + " stage: " + S(n) + " items, outside 0..4";
    for (int i = 0; i < n; i++) {
      const int op = side ? e.out_op[i] : e.in_op[i];
      const std::string item = who + ": " + label + " stage, item " + S(i);
      if (op < 1 || op > 5) return item + ": unknown op code " + S(op) + " (1 add, 2 sub, 3 mul, 4 div, 5 clip)";
      if (op != 5 && !(side ? e.out_vec[i] : e.in_vec[i])) return item + ": null vector";
    }
  }
  for (int s = 0; s <= nl; s++) {
    const std::string slot = who + ": LayerNorm slot " + S(s);
    if (e.ln_where[s] == 0) continue;
    if (e.ln_where[s] < 0 || e.ln_where[s] > 2) return slot + ": unknown placement " + S(e.ln_where[s]) + " (0 none, 1 before the activation, 2 behind it)";
    if (s == nl) return slot + ": LayerNorm on the last layer";
    if (!isfinite(e.ln_eps[s]) || !(e.ln_eps[s] > 0.f)) return slot + ": eps " + std::to_string(e.ln_eps[s]) + " is not a positive finite number";
    if (!e.ln_gamma[s]) return slot + ": null scale vector";
  }
  return "";
}

// rows[start .. start + count) are the env-local rows of one tile, all of policy `policy`
struct PolTile { int32_t policy, start, count, pad; };

// the caller's arrays (host memory)
struct PolRaw {
  int K;
  const int32_t* nl;          // [K]
  const int32_t* dims;        // [K][7]
  const int32_t* act;         // [K][6]
  const float* alpha;         // [K][6] or null (1 everywhere)
  const float* const* w;      // [K][6] host pointers
  const float* const* b;      // [K][6] host pointers, null entries (or a null array): no bias
  int n;                      // envs
  const int32_t* policy_of_row;   // [n]
  int n_ranges;
  const int32_t* ranges;      // [n_ranges][2]: (first, count), ascending, covering [0, n)
  const PolExtRaw* ext = nullptr;   // [K] or null: no policy has extras (cosim_policy_table_create)
};

struct PolShape {
  std::string err;
  int maxd = 0;               // the widest layer of any policy
};

// ---- the checks both kinds of table make (cosim_rectab.h calls them too).  Each answers the refusal, or an empty string; `who` names
// the entry point and the policy, `label` is "", "encoder " or "head ".
inline std::string check_widths(const std::string& who, const char* label, const int32_t* dims, int nl) {
  for (int l = 0; l <= nl; l++)
    if (dims[l] < 1 || dims[l] > POL_MAXD)
      return who + ": " + label + "width " + std::to_string(dims[l]) + " of layer " + std::to_string(l) + " outside 1..512";
  return "";
}

inline std::string check_layers(const std::string& who, const char* label, const int32_t* act, const float* const* w, int nl) {
  for (int l = 0; l < nl; l++) {
    const std::string layer = who + ", " + label + "layer " + std::to_string(l);
    if (act[l] < 0 || act[l] > 5) return layer + ": unknown activation " + std::to_string(act[l]) + " (0 none .. 5 leaky relu)";
    if (!w[l]) return layer + ": null weight";
  }
  return "";
}

// the fleet half: every row's policy is in [0, K), and the ranges tile [0, n) in order
inline std::string check_fleet(const std::string& fn, int K, int n, const int32_t* policy_of_row, int n_ranges, const int32_t* ranges) {
  const auto S = [](long long x) { return std::to_string(x); };
  for (int i = 0; i < n; i++)
    if (policy_of_row[i] < 0 || policy_of_row[i] >= K)
      return fn + ": row " + S(i) + " is assigned to policy " + S(policy_of_row[i]) + ", outside [0, " + S(K) + ")";
  if (n_ranges < 1 || n_ranges > n) return fn + ": " + S(n_ranges) + " ranges, outside 1..n";
  long long next = 0;
  for (int i = 0; i < n_ranges; i++) {
    const long long first = ranges[2 * i], count = ranges[2 * i + 1];
    const std::string who = fn + ": range " + S(i) + " (" + S(first) + ", " + S(count) + ")";
    if (count < 1) return who + " is empty";
    if (first < next) return who + " overlaps the one before it";
    if (first > next) return who + " leaves rows from " + S(next) + " uncovered";
    next = first + count;
    if (next > n) return who + " ends past n " + S(n);
  }
  if (next != n) return fn + ": the ranges leave rows from " + S(next) + " uncovered";
  return "";
}

#define POL_TRY(expr) do { v.err = (expr); if (!v.err.empty()) return v; } while (0)

inline PolShape validate_policy_table(const PolRaw& r, const char* entry = "cosim_policy_table_create") {
  const std::string fn = entry;
  PolShape v;
  if (r.K < 1 || r.K > POL_MAXK) POL_TRY(fn + ": " + std::to_string(r.K) + " policies, outside 1..64");
  if (r.n <= 0) POL_TRY(fn + ": n " + std::to_string(r.n) + " is not positive");
  if (!r.nl || !r.dims || !r.act || !r.w || !r.policy_of_row || !r.ranges) POL_TRY(fn + ": null argument");
  for (int k = 0; k < r.K; k++) {
    const std::string who = fn + ": policy " + std::to_string(k);
    const int nl = r.nl[k];
    if (nl < 1 || nl > POL_MAXL) POL_TRY(who + ": " + std::to_string(nl) + " layers, outside 1..6");
    const int32_t* d = r.dims + (size_t)k * (POL_MAXL + 1);
    POL_TRY(check_widths(who, "", d, nl));
    for (int l = 0; l <= nl; l++) v.maxd = d[l] > v.maxd ? d[l] : v.maxd;
    const int32_t* d0 = r.dims;
    if (d[0] != d0[0])
      POL_TRY(who + ": input width " + std::to_string(d[0]) + " differs from policy 0's " + std::to_string(d0[0]));
    if (d[nl] != d0[r.nl[0]])
      POL_TRY(who + ": output width " + std::to_string(d[nl]) + " differs from policy 0's " + std::to_string(d0[r.nl[0]]));
    POL_TRY(check_layers(who, "", r.act + (size_t)k * POL_MAXL, r.w + (size_t)k * POL_MAXL, nl));
    if (r.ext) POL_TRY(check_extras(who, r.ext[k], nl));
  }
  POL_TRY(check_fleet(fn, r.K, r.n, r.policy_of_row, r.n_ranges, r.ranges));
  return v;
}

#undef POL_TRY

// ---- the tile list.  Of a VALIDATED table: per range, per policy, that policy's rows of the range in ascending order, cut into tiles
// of at most 32.  Every row is in exactly one tile, a tile has one policy and 1..32 rows, no tile crosses a range, and a range's tiles
// are tile_span[2 i] .. + tile_span[2 i + 1] of the list.
struct PolTiles {
  std::vector<int32_t> rows;        // [n]
  std::vector<PolTile> tiles;
  std::vector<int32_t> tile_span;   // [n_ranges][2]: (tile_first, tile_count)
};

inline PolTiles build_policy_tiles(const int32_t* policy_of_row, int K, const int32_t* ranges, int n_ranges) {
  PolTiles t;
  for (int i = 0; i < n_ranges; i++) {
    const int first = ranges[2 * i], count = ranges[2 * i + 1];
    const int tile_first = (int)t.tiles.size();
    for (int k = 0; k < K; k++) {
      int open = 0;   // rows of the tile being filled
      for (int r = first; r < first + count; r++) {
        if (policy_of_row[r] != k) continue;
        if (open == 0 || open == POL_TILE) {
          t.tiles.push_back({k, (int32_t)t.rows.size(), 0, 0});
          open = 0;
        }
        t.rows.push_back(r);
        t.tiles.back().count = ++open;
      }
    }
    t.tile_span.push_back(tile_first);
    t.tile_span.push_back((int32_t)t.tiles.size() - tile_first);
  }
  return t;
}

// ---- a ROTATING table (cosim_policy_table_rotate): the policy of a row changes when its env ends an episode, so the lists above are
// rebuilt on the device before every evaluation (poltab_regroup_kernel, cosim_mlp.hip).  The rule and the size of the buffers are here,
// for the host, the kernel and the host program alike.
#if defined(__HIPCC__)
#define POL_HD __host__ __device__
#else
#define POL_HD
#endif

// The policy of a row whose static assignment is `base` (in [0, K)) after `episodes` ended episodes: every `every` (>= 1) episodes the
// next one, (base + episodes / every) mod K.  The sum is never formed unreduced, so a count near INT32_MAX does not overflow; a
// negative count reads as 0.
POL_HD inline int32_t policy_at(int32_t base, int32_t episodes, int32_t every, int32_t K) {
  const uint32_t steps = (uint32_t)(episodes < 0 ? 0 : episodes) / (uint32_t)every;
  return (int32_t)(((uint32_t)base + steps % (uint32_t)K) % (uint32_t)K);
}

// The counter after a control step: one more if the env's episode ended, held at INT32_MAX.
POL_HD inline int32_t episodes_after(int32_t episodes, bool ended) {
  return (ended && episodes < INT32_MAX) ? episodes + 1 : episodes;
}

// The tiles a range of `count` rows can need under ANY assignment to K policies: a policy with c rows has c / 32 full tiles and at most
// one partial one, the full tiles of all policies are at most count / 32, and a partial tile needs a policy with a row.  One row on each
// of min(K, count) policies meets it.
POL_HD inline int32_t policy_tile_capacity(int32_t count, int32_t K) {
  return count / POL_TILE + (K < count ? K : count);
}

// ---- the image: per policy, per layer the weights (begun at a multiple of 4 words, so the float4 reads of a layer whose input width
// is a multiple of 4 are 16-byte aligned) and then the bias if there is one.  Of a VALIDATED table.
// A weight image as it grows: a matrix begins at a multiple of 4 words (zero padding), a bias follows what is there.  Both answer the
// word offset of what they appended; a null bias appends nothing and answers -1.
struct ImageWords : std::vector<float> {
  int32_t matrix(const float* p, size_t n) {
    resize((size() + 3) & ~(size_t)3, 0.f);
    return bias(p, n);
  }
  int32_t bias(const float* p, size_t n) {
    if (!p) return -1;
    const int32_t off = (int32_t)size();
    insert(end(), p, p + n);
    return off;
  }
};

struct PolImage {
  ImageWords words;
  std::vector<PolDesc> desc;   // [K]
  std::vector<PolExt> ext;     // [K], or empty: no policy has extras, and image and descriptors are what they always were
};

// One policy's record; its vectors go behind the policy's layers, each begun at a multiple of 4 words.
inline PolExt pack_policy_extras(ImageWords& words, const PolExtRaw& e, const PolDesc& d) {
  PolExt x;
  memset(&x, 0, sizeof x);
  x.n_in = e.n_in; x.n_out = e.n_out;
  for (int i = 0; i < POL_MAXS; i++) {
    x.in[i].off = -1; x.out[i].off = -1;
    if (i < e.n_in) {
      x.in[i].op = e.in_op[i]; x.in[i].lo = e.in_lo[i]; x.in[i].hi = e.in_hi[i];
      if (e.in_op[i] != 5) x.in[i].off = words.matrix(e.in_vec[i], (size_t)d.dims[0]);
    }
    if (i < e.n_out) {
      x.out[i].op = e.out_op[i]; x.out[i].lo = e.out_lo[i]; x.out[i].hi = e.out_hi[i];
      if (e.out_op[i] != 5) x.out[i].off = words.matrix(e.out_vec[i], (size_t)d.dims[d.nl]);
    }
  }
  for (int s = 0; s <= POL_MAXL; s++) {
    x.ln_g[s] = -1; x.ln_b[s] = -1;
    if (s < d.nl && e.ln_where[s] != 0) {
      x.ln_where[s] = e.ln_where[s]; x.ln_eps[s] = e.ln_eps[s];
      x.ln_g[s] = words.matrix(e.ln_gamma[s], (size_t)d.dims[s]);
      x.ln_b[s] = words.matrix(e.ln_beta[s], (size_t)d.dims[s]);   // a null bias appends at most padding and answers -1
    }
  }
  return x;
}

inline PolImage pack_policy_image(const PolRaw& r) {
  PolImage im;
  im.desc.resize(r.K);
  bool extras = false;
  for (int k = 0; r.ext && k < r.K; k++) extras = extras || ext_used(r.ext[k], r.nl[k]);
  if (extras) im.ext.resize(r.K);
  for (int k = 0; k < r.K; k++) {
    PolDesc& d = im.desc[k];
    memset(&d, 0, sizeof d);
    d.nl = r.nl[k];
    for (int l = 0; l <= POL_MAXL; l++) d.dims[l] = l <= d.nl ? r.dims[(size_t)k * (POL_MAXL + 1) + l] : 0;
    for (int l = 0; l < POL_MAXL; l++) { d.woff[l] = -1; d.boff[l] = -1; d.alpha[l] = 1.f; }
    for (int l = 0; l < d.nl; l++) {
      const size_t q = (size_t)k * POL_MAXL + l;
      d.act[l] = r.act[q];
      if (r.alpha) d.alpha[l] = r.alpha[q];
      d.woff[l] = im.words.matrix(r.w[q], (size_t)d.dims[l] * d.dims[l + 1]);
      d.boff[l] = im.words.bias(r.b ? r.b[q] : nullptr, (size_t)d.dims[l + 1]);
    }
    if (extras) im.ext[k] = pack_policy_extras(im.words, r.ext[k], d);
  }
  return im;
}

}  // namespace cosim
