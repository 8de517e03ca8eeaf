// cosim_rectab.h — what the host does with a RECURRENT policy table before it reaches the device (cosim_recurrent_table_create,
// include/cosim.h): K recurrent actors -- 0..3 encoder layers, one LSTM cell, 1..3 head layers -- over one fleet, every env assigned to
// one of them, evaluated by ONE launch of lstm_actor_grouped_kernel (cosim_mlp.hip).  The kernel trusts the row list, the tile list and
// the offsets it is given, so all of them are made and checked here.  The tile list is the policy table's own (PolTile,
// build_policy_tiles of cosim_poltab.h, unchanged); this header adds the descriptor of a recurrent policy, the validator, the packer of
// the weight image and the LDS byte rule.  Plain C++ with no HIP in it: cosim_engine.hip and a host program (tests/rectab_host.cpp) both
// compile it.
#pragma once
#include <stdint.h>
#include <string.h>

#include <string>
#include <vector>

#include "cosim_poltab.h"

namespace cosim {

constexpr int REC_MAXE = 3;          // encoder layers, 0 .. 3
constexpr int REC_MAXH = 3;          // head layers, 1 .. 3
constexpr int REC_MAXK = 1200;       // I_enc + H of the cell: cosim_lstm_cell's own bound
constexpr int REC_STATIC_LDS = 256;  // the kernel's two static arrays of 32 ints

// One policy as the kernel reads it: 40 words.  Offsets are word offsets into the table's one weight image; a bias offset of -1: no bias.
struct RecDesc {
  int32_t ne;                        // encoder layers
  int32_t edims[REC_MAXE + 1];       // edims[0]: the observation width; edims[ne] = I
  int32_t eact[REC_MAXE];            // 0 none, 1 relu, 2 tanh, 3 elu, 4 sigmoid, 5 leaky relu
  float ealpha[REC_MAXE];
  int32_t ewoff[REC_MAXE], eboff[REC_MAXE];
  int32_t I, H;                      // the cell: input width (I_enc) and hidden size
  int32_t woff, roff, boff;          // W [4H, I], R [4H, H], B [8H] (Wb then Rb)
  int32_t nh;                        // head layers
  int32_t hdims[REC_MAXH + 1];       // hdims[0] = H; hdims[nh]: the action width
  int32_t hact[REC_MAXH];
  float halpha[REC_MAXH];
  int32_t hwoff[REC_MAXH], hboff[REC_MAXH];
  int32_t vec;                       // I and H are multiples of 4: the cell reads W / R rows as float4
};
static_assert(sizeof(RecDesc) == 40 * 4, "RecDesc is 40 words");

// the caller's arrays (host memory)
struct RecRaw {
  int K;
  const int32_t* ne;                 // [K]
  const int32_t* edims;              // [K][4]
  const int32_t* eact;               // [K][3]
  const float* ealpha;               // [K][3] or null (1 everywhere)
  const float* const* ew;            // [K][3] host pointers
  const float* const* eb;            // [K][3] host pointers, null entries (or a null array): no bias
  const int32_t* lstm_in;            // [K]: the input width of W
  const int32_t* hidden;             // [K]
  const float* const* W;             // [K] host pointers: [4H, I]
  const float* const* R;             // [K]: [4H, H]
  const float* const* B;             // [K]: [8H]; a null entry (or a null array): no bias
  const int32_t* nh;                 // [K]
  const int32_t* hdims;              // [K][4]
  const int32_t* hact;               // [K][3]
  const float* halpha;               // [K][3] or null
  const float* const* hw;            // [K][3]
  const float* const* hb;            // [K][3]
  int n;                             // envs
  const int32_t* policy_of_row;      // [n]
  int n_ranges;
  const int32_t* ranges;             // [n_ranges][2]: (first, count), ascending, covering [0, n)
};

// ---- the LDS byte rule.  A policy needs two ping-pong tiles of 32 x ld_m words, ld_m = (its widest encoder / head layer, H among them) | 1,
// and the [x_enc | h] tile of 32 x ld_x words, ld_x = (I_enc + H) | 1 (odd leading dimensions: conflict-free column reads).  A table is
// launched with the largest ld_m and the largest ld_x of its policies, plus the kernel's static arrays.
inline int rec_ld_m(const RecDesc& d) {
  int m = d.H;
  for (int l = 0; l <= d.ne; l++) m = d.edims[l] > m ? d.edims[l] : m;
  for (int l = 0; l <= d.nh; l++) m = d.hdims[l] > m ? d.hdims[l] : m;
  return m | 1;
}
inline int rec_ld_x(const RecDesc& d) { return (d.I + d.H) | 1; }
inline long long rec_lds_dynamic(int ld_m, int ld_x) { return 4LL * 32 * (2LL * ld_m + ld_x); }
inline long long rec_lds_bytes(int ld_m, int ld_x) { return rec_lds_dynamic(ld_m, ld_x) + REC_STATIC_LDS; }

struct RecShape {
  std::string err;
  int ld_m = 0, ld_x = 0;            // of the table: the largest of any policy
  int hmax = 0;                      // the widest hidden size: the row stride of the state tensors
};

#define REC_TRY(expr) do { v.err = (expr); if (!v.err.empty()) return v; } while (0)

// lds_limit: the bytes of LDS a workgroup may use on the device (0: not checked)
inline RecShape validate_recurrent_table(const RecRaw& r, long long lds_limit) {
  const std::string fn = "cosim_recurrent_table_create";
  auto S = [](long long x) { return std::to_string(x); };
  RecShape v;
  if (r.K < 1 || r.K > POL_MAXK) REC_TRY(fn + ": " + S(r.K) + " policies, outside 1..64");
  if (r.n <= 0) REC_TRY(fn + ": n " + S(r.n) + " is not positive");
  if (!r.ne || !r.edims || !r.eact || !r.ew || !r.lstm_in || !r.hidden || !r.W || !r.R || !r.nh || !r.hdims || !r.hact || !r.hw ||
      !r.policy_of_row || !r.ranges)
    REC_TRY(fn + ": null argument");
  for (int k = 0; k < r.K; k++) {
    const std::string who = fn + ": policy " + S(k);
    const int ne = r.ne[k], nh = r.nh[k], I = r.lstm_in[k], H = r.hidden[k];
    if (ne < 0 || ne > REC_MAXE) REC_TRY(who + ": " + S(ne) + " encoder layers, outside 0..3");
    if (nh < 1 || nh > REC_MAXH) REC_TRY(who + ": " + S(nh) + " head layers, outside 1..3");
    if ((long long)I + H > REC_MAXK) REC_TRY(who + ": LSTM input width + hidden size " + S(I) + " + " + S(H) + " exceeds 1200");
    const int32_t* ed = r.edims + (size_t)k * (REC_MAXE + 1);
    const int32_t* hd = r.hdims + (size_t)k * (REC_MAXH + 1);
    REC_TRY(check_widths(who, "encoder ", ed, ne));
    if (H < 1 || H > POL_MAXD) REC_TRY(who + ": hidden size " + S(H) + " outside 1..512");
    REC_TRY(check_widths(who, "head ", hd, nh));
    if (ed[0] != r.edims[0]) REC_TRY(who + ": input width " + S(ed[0]) + " differs from policy 0's " + S(r.edims[0]));
    if (hd[nh] != r.hdims[r.nh[0]]) REC_TRY(who + ": output width " + S(hd[nh]) + " differs from policy 0's " + S(r.hdims[r.nh[0]]));
    if (I != ed[ne]) REC_TRY(who + ": the LSTM's input width " + S(I) + " differs from the encoder's output width " + S(ed[ne]));
    if (hd[0] != H) REC_TRY(who + ": the head's input width " + S(hd[0]) + " differs from the hidden size " + S(H));
    REC_TRY(check_layers(who, "encoder ", r.eact + (size_t)k * REC_MAXE, r.ew + (size_t)k * REC_MAXE, ne));
    REC_TRY(check_layers(who, "head ", r.hact + (size_t)k * REC_MAXH, r.hw + (size_t)k * REC_MAXH, nh));
    if (!r.W[k] || !r.R[k]) REC_TRY(who + ": null LSTM weight");
    RecDesc d;
    memset(&d, 0, sizeof d);
    d.ne = ne; d.nh = nh; d.I = I; d.H = H;
    for (int l = 0; l <= ne; l++) d.edims[l] = ed[l];
    for (int l = 0; l <= nh; l++) d.hdims[l] = hd[l];
    const int ld_m = rec_ld_m(d), ld_x = rec_ld_x(d);
    if (lds_limit > 0 && rec_lds_bytes(ld_m, ld_x) > lds_limit)
      REC_TRY(who + " needs " + S(rec_lds_bytes(ld_m, ld_x)) + " bytes of LDS (two tiles of 32 x " + S(ld_m) + " words, one of 32 x " + S(ld_x) +
              ", " + S(REC_STATIC_LDS) + " static), the device allows " + S(lds_limit));
    if (ld_m > v.ld_m) v.ld_m = ld_m;
    if (ld_x > v.ld_x) v.ld_x = ld_x;
    if (H > v.hmax) v.hmax = H;
  }
  // two policies that each fit may not fit together: the widest ld_m and the widest ld_x can come from different policies
  if (lds_limit > 0 && rec_lds_bytes(v.ld_m, v.ld_x) > lds_limit)
    REC_TRY(fn + ": the table needs " + S(rec_lds_bytes(v.ld_m, v.ld_x)) + " bytes of LDS (two tiles of 32 x " + S(v.ld_m) + " words, one of 32 x " +
            S(v.ld_x) + ", " + S(REC_STATIC_LDS) + " static), the device allows " + S(lds_limit));
  REC_TRY(check_fleet(fn, r.K, r.n, r.policy_of_row, r.n_ranges, r.ranges));
  return v;
}

#undef REC_TRY

// ---- the image: per policy the encoder layers, W, R, B and the head layers; every matrix begins at a multiple of 4 words (the float4
// reads of a layer whose input width is a multiple of 4 are then 16-byte aligned), a bias follows its matrix.  Of a VALIDATED table.
struct RecImage {
  ImageWords words;
  std::vector<RecDesc> desc;   // [K]
};

inline RecImage pack_recurrent_image(const RecRaw& r) {
  RecImage im;
  im.desc.resize(r.K);
  auto& words = im.words;
  for (int k = 0; k < r.K; k++) {
    RecDesc& d = im.desc[k];
    memset(&d, 0, sizeof d);
    d.ne = r.ne[k]; d.nh = r.nh[k]; d.I = r.lstm_in[k]; d.H = r.hidden[k];
    for (int l = 0; l < REC_MAXE; l++) { d.ewoff[l] = d.eboff[l] = -1; d.ealpha[l] = 1.f; }
    for (int l = 0; l < REC_MAXH; l++) { d.hwoff[l] = d.hboff[l] = -1; d.halpha[l] = 1.f; }
    for (int l = 0; l <= d.ne; l++) d.edims[l] = r.edims[(size_t)k * (REC_MAXE + 1) + l];
    for (int l = 0; l <= d.nh; l++) d.hdims[l] = r.hdims[(size_t)k * (REC_MAXH + 1) + l];
    for (int l = 0; l < d.ne; l++) {
      const size_t q = (size_t)k * REC_MAXE + l;
      d.eact[l] = r.eact[q];
      if (r.ealpha) d.ealpha[l] = r.ealpha[q];
      d.ewoff[l] = words.matrix(r.ew[q], (size_t)d.edims[l] * d.edims[l + 1]);
      d.eboff[l] = words.bias(r.eb ? r.eb[q] : nullptr, (size_t)d.edims[l + 1]);
    }
    d.woff = words.matrix(r.W[k], (size_t)4 * d.H * d.I);
    d.roff = words.matrix(r.R[k], (size_t)4 * d.H * d.H);
    d.boff = words.bias(r.B ? r.B[k] : nullptr, (size_t)8 * d.H);
    for (int l = 0; l < d.nh; l++) {
      const size_t q = (size_t)k * REC_MAXH + l;
      d.hact[l] = r.hact[q];
      if (r.halpha) d.halpha[l] = r.halpha[q];
      d.hwoff[l] = words.matrix(r.hw[q], (size_t)d.hdims[l] * d.hdims[l + 1]);
      d.hboff[l] = words.bias(r.hb ? r.hb[q] : nullptr, (size_t)d.hdims[l + 1]);
    }
    d.vec = (d.I % 4 == 0 && d.H % 4 == 0) ? 1 : 0;
  }
  return im;
}

}  // namespace cosim
