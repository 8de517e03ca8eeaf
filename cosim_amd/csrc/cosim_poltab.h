// cosim_poltab.h — what the host does with a policy table before it reaches the device (cosim_policy_table_create, include/cosim.h):
// K actor MLPs over one fleet, every env assigned to one of them, evaluated by ONE launch of mlp_grouped_kernel (cosim_mlp.hip).  The
// kernel trusts the row list, the tile list and the offsets it is given, so all of them are made and checked here: the descriptor
// of a policy, the validator, the tile-list builder and the packer of the weight image.  Plain C++ with no HIP in it, in the manner of
// cosim_tables.h: cosim_engine.hip and a host program (tests/poltab_host.cpp) both compile it.
//
// WordPacker (cosim_tables.h) is not used for the image: it lays arrays end to end and patches POINTERS, while a weight matrix has to
// begin at a multiple of 4 words (the kernel's float4 path) and a descriptor holds word OFFSETS, -1 among them.
#pragma once
#include <stdint.h>
#include <string.h>

#include <string>
#include <vector>

namespace cosim {

constexpr int POL_MAXK = 64;      // policies of a table
constexpr int POL_MAXL = 6;       // = MLP_MAXL
constexpr int POL_MAXD = 512;     // = MLP_MAXD
constexpr int POL_TILE = 32;      // envs of a tile: the rows of one MFMA tile

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

inline PolShape validate_policy_table(const PolRaw& r) {
  const std::string fn = "cosim_policy_table_create";
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
};

inline PolImage pack_policy_image(const PolRaw& r) {
  PolImage im;
  im.desc.resize(r.K);
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
  }
  return im;
}

}  // namespace cosim
