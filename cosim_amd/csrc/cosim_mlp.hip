// cosim_mlp.hip — fused forward pass of a small actor MLP on the matrix pipe.
//
// The reference evaluates its ONNX policy once per control step for one state (core/policy.py:11-21); for N environments
// the same network is [N, in] -> hidden ... -> [N, action_dim].  Those layers are tiny (52 -> 256 -> 128 -> 4 for the
// usual actor), so a chain of library GEMM + bias + activation launches is launch-bound: here one workgroup takes 32
// environments through all layers, activations stay in LDS, weights stream from L2 and every product runs as
// v_mfma_f32_32x32x2_f32 (exact fp32 FMA chains, like the CPU evaluation).
//
// Layout of one 32x32 output tile (lane l, register v): A[i = l & 31][k = l >> 5], B[k = l >> 5][j = l & 31];
// C/D: col = l & 31, row = (v & 3) + 8 (v >> 2) + 4 (l >> 5)  (the layout the step kernel's Hessian build uses).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cosim_poltab.h"
#include "cosim_rectab.h"

namespace cosim {

constexpr int MLP_MAXL = 6;      // layers
constexpr int MLP_MAXD = 512;    // widest layer: two ping-pong tiles of 32 x (width + 1) floats must fit the 160 KB LDS

struct MlpArgs {
  const float* x;      // [n, dims[0]]
  float* out;          // [n, dims[nl]]
  const float* w[MLP_MAXL];   // [dims[l+1], dims[l]] row-major (ONNX Gemm with transB = 1)
  const float* b[MLP_MAXL];   // [dims[l+1]] or null
  int dims[MLP_MAXL + 1];
  int act[MLP_MAXL];   // 0 none, 1 relu, 2 tanh, 3 elu, 4 sigmoid, 5 leaky relu
  float act_alpha[MLP_MAXL];
  int nl, n, ld;       // ld: leading dimension of the LDS tiles (widest layer + 1: odd, conflict-free column reads)
  // > 0: clamp the output to [-clip, clip].  Non-finite rule (the interpreter's clamp and the reference's np.clip, core/policy.py:20):
  // +-inf becomes +-clip, NaN stays NaN -- the clamp is two compares and selects, not fminf / fmaxf, which return the other operand
  // and would turn a NaN action into -clip.  Relu keeps NaN for the same reason.
  float clip;
};

__device__ __forceinline__ float mlp_act(float x, int kind, float alpha) {
  switch (kind) {
    case 1: return x < 0.f ? 0.f : x;   // not fmaxf: NaN stays NaN
    case 2: return tanhf(x);
    case 3: return x > 0.f ? x : alpha * (expf(x) - 1.f);
    case 4: return 1.f / (1.f + expf(-x));
    case 5: return x > 0.f ? x : alpha * x;
    default: return x;
  }
}

// One layer of the chain as the layer loop reads it.
struct MlpLayer {
  const float *W, *Bv;   // [O, I] row-major; [O] or null
  int I, O, act;
  float alpha;
};

// ---- what an EXTENDED actor adds to the chain (cosim_mlp_forward_ex, cosim_policy_table_create_ex): elementwise stages on the
// observation and on the action, and LayerNorm behind a layer.  The plain kernels compile none of it (mlp_layers<false>).
// One stage item: y = y (op) v[column] for op 1 add, 2 sub, 3 mul, 4 div; 5: clamp to [lo, hi] (an absent bound is -+inf).
struct MlpStage { int op; const float* v; float lo, hi; };
// LayerNorm of slot s (0: the observation, l + 1: layer l's output, width dims[s]): where 0 none, 1 ahead of the layer's activation,
// 2 behind it
struct MlpLn { int where; const float *g, *b; float eps; };
// an extended actor as cosim_mlp_forward_ex launches it: every vector a device pointer
struct MlpExt {
  int n_in, n_out;
  MlpStage in[POL_MAXS], out[POL_MAXS];
  MlpLn ln[POL_MAXL + 1];
  __device__ MlpStage in_item(int i) const { return in[i]; }
  __device__ MlpStage out_item(int i) const { return out[i]; }
  __device__ MlpLn ln_of(int s) const { return ln[s]; }
};
// the same out of a table's record: word offsets into the table's image
struct PolExtView {
  const PolExt* E;
  const float* image;
  const int n_out;
  __device__ MlpStage item(const PolStage& s) const { return MlpStage{s.op, s.off >= 0 ? image + s.off : nullptr, s.lo, s.hi}; }
  __device__ MlpStage in_item(int i) const { return item(E->in[i]); }
  __device__ MlpStage out_item(int i) const { return item(E->out[i]); }
  __device__ MlpLn ln_of(int s) const {
    return MlpLn{E->ln_where[s], E->ln_g[s] >= 0 ? image + E->ln_g[s] : nullptr, E->ln_b[s] >= 0 ? image + E->ln_b[s] : nullptr, E->ln_eps[s]};
  }
};
struct NoExt {};

// One stage item on one word: exactly the ONE fp32 operation the ONNX node names, so a stage gives the interpreter's bits.  No
// contraction (a Mul followed by an Add must not become an FMA), division correctly rounded, the clamp two compares and selects as
// MlpArgs::clip (NaN stays NaN, +-inf becomes the bound).
__device__ __forceinline__ float mlp_stage_op(float y, int op, float c, float lo, float hi) {
#pragma clang fp contract(off)
  switch (op) {
    case 1: return y + c;
    case 2: return y - c;
    case 3: return y * c;
    case 4: return __fdiv_rn(y, c);
    case 5: return y < lo ? lo : (y > hi ? hi : y);
    default: return y;
  }
}

// The input stage on the word of column c as it is loaded into the tile: the items in listed order.
template <class Ext>
__device__ __forceinline__ float mlp_input_stage(float v, int c, int n_in, const Ext& X) {
#pragma unroll
  for (int i = 0; i < POL_MAXS; i++)
    if (i < n_in) {
      const MlpStage s = X.in_item(i);
      v = mlp_stage_op(v, s.op, s.v != nullptr ? s.v[c] : 0.f, s.lo, s.hi);
    }
  return v;
}

// LayerNorm over the first W columns of every row of one 32-row tile, in place, then the activation `act` (0: none); all 256 threads,
// the caller synchronises on both sides.  Eight lanes per row (row = t >> 3, s = t & 7); lane s takes the columns 32 j + 4 s + k
// (k = 0..3), j and k ascending, and the eight partial sums meet in a butterfly over lane ^ 1, ^ 2, ^ 4 -- every lane of the row ends
// with the same bits (a + b = b + a).  Two passes: the mean, then the mean of squared deviations.  A row's statistics are a function of
// that row's W words alone: not of the tile row, the other rows, the launch's size or its kernel.  LDS: a ds_read_b32 is served in
// groups of 32 lanes = 4 rows x 8 lanes over 32 banks; with the columns 4 s + k the bank is (r ld + 4 s + k) mod 32, and r ld mod 4
// differs for the four rows because ld is odd: no conflict at any width.
__device__ __forceinline__ void mlp_layernorm(float* tl, int ld, int W, const float* g, const float* b, float eps, int act, float alpha) {
  const int t = threadIdx.x, s4 = 4 * (t & 7);
  float* r = tl + (t >> 3) * ld;
  float sum = 0.f;
  for (int c0 = s4; c0 < W; c0 += 32)
#pragma unroll
    for (int k = 0; k < 4; k++)
      if (c0 + k < W) sum += r[c0 + k];
  sum += __shfl_xor(sum, 1); sum += __shfl_xor(sum, 2); sum += __shfl_xor(sum, 4);
  const float mean = sum / (float)W;
  float sq = 0.f;
  for (int c0 = s4; c0 < W; c0 += 32)
#pragma unroll
    for (int k = 0; k < 4; k++)
      if (c0 + k < W) { const float d = r[c0 + k] - mean; sq += d * d; }
  sq += __shfl_xor(sq, 1); sq += __shfl_xor(sq, 2); sq += __shfl_xor(sq, 4);
  const float rstd = 1.f / sqrtf(sq / (float)W + eps);
  for (int c0 = s4; c0 < W; c0 += 32)
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const int c = c0 + k;
      if (c < W) {
        const float y = (r[c] - mean) * rstd * g[c] + (b != nullptr ? b[c] : 0.f);
        r[c] = mlp_act(y, act, alpha);
      }
    }
}

// The layer loop of one 32-env tile whose input rows stand in tile 0 of `lds` ([2][32][ld]; the caller has synchronised).  Both
// kernels below run it.  layer_of(L): layer L; out_row(r): the row of `out` that tile row r is written to, < 0 for none.  An output
// element is a chain of MFMA steps over k whose operands are the env's own inputs and the weights: which tile row the env sits in,
// and what the other rows hold, does not enter it.
// EXT (X: MlpExt or PolExtView; the plain kernels pass NoExt and compile what they always did): a layer with LayerNorm ahead of its
// activation stores the pre-activation and mlp_layernorm applies norm and activation to the finished tile; with LayerNorm behind it
// the epilogue is unchanged and the pass only normalises; the last layer's epilogue runs the output stage between the activation and
// the clip.  The two ping-pong tiles are all the LDS there is.
template <bool EXT, class LayerOf, class RowOf, class Ext>
__device__ __forceinline__ void mlp_layers(float* lds, int ld, int nl, float clip, float* out, LayerOf layer_of, RowOf out_row, const Ext& X) {
  typedef float f32x16 __attribute__((ext_vector_type(16)));
  auto tile = [&](int which, int r, int c) -> float& { return lds[(which * 32 + r) * ld + c]; };
  const int t = threadIdx.x, l = t & 63, wave = t >> 6;
  int cur = 0;
  for (int L = 0; L < nl; L++) {
    const MlpLayer ly = layer_of(L);
    const int I = ly.I, O = ly.O;
    const float* W = ly.W;
    const float* Bv = ly.Bv;
    const bool last = L == nl - 1;
    const int row_a = l & 31, kk = l >> 5;
    MlpLn ln = {0, nullptr, nullptr, 0.f};
    int n_out = 0;
    if constexpr (EXT) {
      if (!last) ln = X.ln_of(L + 1);
      else n_out = X.n_out;
    }
    for (int ti = wave; ti * 32 < O; ti += 4) {
      const int o0 = ti * 32, col = o0 + (l & 31);
      const float bias = (Bv != nullptr && col < O) ? Bv[col] : 0.f;
      MlpStage so[POL_MAXS];
      float sc[POL_MAXS];
      if constexpr (EXT) {
#pragma unroll
        for (int i = 0; i < POL_MAXS; i++) {
          so[i] = MlpStage{0, nullptr, 0.f, 0.f};
          sc[i] = 0.f;
          if (i < n_out) {
            so[i] = X.out_item(i);
            if (so[i].v != nullptr && col < O) sc[i] = so[i].v[col];
          }
        }
      }
      f32x16 acc;
#pragma unroll
      for (int v = 0; v < 16; v++) acc[v] = bias;
      const float* wrow = W + (size_t)(col < O ? col : 0) * I;
      if ((I & 3) == 0) {   // four weights of the lane's row per load: k0 + kk and k0 + 2 + kk feed two MFMA steps
        for (int k0 = 0; k0 < I; k0 += 4) {
          const float4 w4 = col < O ? *reinterpret_cast<const float4*>(wrow + k0) : make_float4(0.f, 0.f, 0.f, 0.f);
          const float a0 = tile(cur, row_a, k0 + kk), a1 = tile(cur, row_a, k0 + 2 + kk);
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, kk ? w4.y : w4.x, acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, kk ? w4.w : w4.z, acc, 0, 0, 0);
        }
      } else {
        for (int k0 = 0; k0 < I; k0 += 2) {
          const int k = k0 + kk;
          const float a = k < I ? tile(cur, row_a, k) : 0.f;
          const float b = (k < I && col < O) ? wrow[k] : 0.f;
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
        }
      }
#pragma unroll
      for (int v = 0; v < 16; v++) {
        const int row = (v & 3) + 8 * (v >> 2) + 4 * (l >> 5);
        float y;
        if constexpr (EXT) y = ln.where == 1 ? acc[v] : mlp_act(acc[v], ly.act, ly.alpha);
        else y = mlp_act(acc[v], ly.act, ly.alpha);
        if (last) {
          if constexpr (EXT) {
#pragma unroll
            for (int i = 0; i < POL_MAXS; i++)
              if (i < n_out) y = mlp_stage_op(y, so[i].op, sc[i], so[i].lo, so[i].hi);
          }
          if (clip > 0.f) y = y < -clip ? -clip : (y > clip ? clip : y);
          const long long orow = out_row(row);
          if (col < O && orow >= 0) out[(size_t)orow * O + col] = y;
        } else if (col < O)
          tile(cur ^ 1, row, col) = y;
      }
    }
    __syncthreads();
    cur ^= 1;
    if constexpr (EXT) {
      if (ln.where != 0) {   // uniform: the tile the layer has just finished, all 32 rows of it
        mlp_layernorm(lds + cur * 32 * ld, ld, O, ln.g, ln.b, ln.eps, ln.where == 1 ? ly.act : 0, ly.alpha);
        __syncthreads();
      }
    }
  }
}

// The observation's own LayerNorm (slot 0) on the input tile, behind the input stage; the caller has synchronised and does again.
template <class Ext>
__device__ __forceinline__ void mlp_input_layernorm(float* lds, int ld, int I, const Ext& X) {
  const MlpLn ln = X.ln_of(0);
  if (ln.where != 0) {
    mlp_layernorm(lds, ld, I, ln.g, ln.b, ln.eps, 0, 1.f);
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void mlp_forward_kernel(MlpArgs A) {
  extern __shared__ float mlp_lds[];   // [2][32][ld]
  const int ld = A.ld;
  const int t = threadIdx.x;
  const int n0 = blockIdx.x * 32;
  // the input tile, coalesced
  {
    const int I = A.dims[0];
    for (int e = t; e < 32 * I; e += 256) {
      const int r = e / I, c = e - r * I;
      mlp_lds[r * ld + c] = (n0 + r < A.n) ? A.x[(size_t)(n0 + r) * I + c] : 0.f;
    }
  }
  __syncthreads();
  mlp_layers<false>(mlp_lds, ld, A.nl, A.clip, A.out,
                    [&](int L) { return MlpLayer{A.w[L], A.b[L], A.dims[L], A.dims[L + 1], A.act[L], A.act_alpha[L]}; },
                    [&](int row) -> long long { return n0 + row < A.n ? (long long)(n0 + row) : -1; }, NoExt{});
}

// The extended instantiation of the kernel above (cosim_mlp_forward_ex): the input stage on every word of a real row as it is loaded
// (the rows behind n stay zero), the observation's LayerNorm, then the extended layer loop.
__global__ __launch_bounds__(256) void mlp_forward_ext_kernel(MlpArgs A, MlpExt X) {
  extern __shared__ float mlp_lds[];   // [2][32][ld]
  const int ld = A.ld;
  const int t = threadIdx.x;
  const int n0 = blockIdx.x * 32;
  const int I = A.dims[0];
  for (int e = t; e < 32 * I; e += 256) {
    const int r = e / I, c = e - r * I;
    mlp_lds[r * ld + c] = (n0 + r < A.n) ? mlp_input_stage(A.x[(size_t)(n0 + r) * I + c], c, X.n_in, X) : 0.f;
  }
  __syncthreads();
  mlp_input_layernorm(mlp_lds, ld, I, X);
  mlp_layers<true>(mlp_lds, ld, A.nl, A.clip, A.out,
                   [&](int L) { return MlpLayer{A.w[L], A.b[L], A.dims[L], A.dims[L + 1], A.act[L], A.act_alpha[L]}; },
                   [&](int row) -> long long { return n0 + row < A.n ? (long long)(n0 + row) : -1; }, X);
}

// K policies over one fleet in one launch (cosim_policy_table_forward; the table is made and checked by cosim_poltab.h): a workgroup
// takes one TILE -- up to 32 envs of one policy, rows[start .. start + count) -- gathers their input rows into the LDS tile (zeros
// behind `count`), runs the layer loop above with its policy's weights out of the table's one image, and scatters the output rows.
// A launch covers tiles tile_first .. tile_first + gridDim.x, so one range of envs can be evaluated alone on a stream of its own.
struct PolTabArgs {
  const float* x;          // [n, in_dim]
  float* out;              // [n, out_dim]
  const float* image;      // every policy's weights and biases
  const PolDesc* desc;     // [K]
  const int32_t* rows;     // [n] env-local rows grouped by (range, policy)
  const PolTile* tiles;
  int tile_first, ld;      // ld: (widest layer of any policy) | 1
  float clip;              // as MlpArgs::clip
};

__global__ __launch_bounds__(256) void mlp_grouped_kernel(PolTabArgs A) {
  extern __shared__ float mlp_lds[];   // [2][32][ld]
  __shared__ int tile_row[32];         // the env each tile row holds, -1 behind the tile's count
  const int ld = A.ld;
  const int t = threadIdx.x;
  // the tile and its policy: indices out of blockIdx alone, so wave-uniform (scalar loads)
  const PolTile T = A.tiles[A.tile_first + blockIdx.x];
  if (T.count == 0) return;            // a padding tile of a rotating table (poltab_regroup_kernel); a static table holds none
  const PolDesc* D = A.desc + T.policy;
  if (t < 32) tile_row[t] = t < T.count ? A.rows[T.start + t] : -1;
  __syncthreads();
  // the input tile: a row is dims[0] contiguous floats, consecutive lanes take consecutive words of it
  {
    const int I = D->dims[0];
    for (int e = t; e < 32 * I; e += 256) {
      const int r = e / I, c = e - r * I, src = tile_row[r];
      mlp_lds[r * ld + c] = src >= 0 ? A.x[(size_t)src * I + c] : 0.f;
    }
  }
  __syncthreads();
  mlp_layers<false>(mlp_lds, ld, D->nl, A.clip, A.out,
                    [&](int L) {
                      const int bo = D->boff[L];
                      return MlpLayer{A.image + D->woff[L], bo >= 0 ? A.image + bo : nullptr, D->dims[L], D->dims[L + 1], D->act[L], D->alpha[L]};
                    },
                    [&](int row) -> long long { return tile_row[row]; }, NoExt{});
}

// The extended instantiation of the grouped kernel: a table in which at least one policy has extras runs it for all of its tiles
// (`ext`: one record per policy, all zero for a plain one, which then gets the bits of the plain kernel: the same MFMA chains).
__global__ __launch_bounds__(256) void mlp_grouped_ext_kernel(PolTabArgs A, const PolExt* ext) {
  extern __shared__ float mlp_lds[];   // [2][32][ld]
  __shared__ int tile_row[32];
  const int ld = A.ld;
  const int t = threadIdx.x;
  const PolTile T = A.tiles[A.tile_first + blockIdx.x];
  if (T.count == 0) return;
  const PolDesc* D = A.desc + T.policy;
  const PolExtView X = {ext + T.policy, A.image, ext[T.policy].n_out};
  if (t < 32) tile_row[t] = t < T.count ? A.rows[T.start + t] : -1;
  __syncthreads();
  const int I = D->dims[0], n_in = X.E->n_in;
  for (int e = t; e < 32 * I; e += 256) {
    const int r = e / I, c = e - r * I, src = tile_row[r];
    mlp_lds[r * ld + c] = src >= 0 ? mlp_input_stage(A.x[(size_t)src * I + c], c, n_in, X) : 0.f;
  }
  __syncthreads();
  mlp_input_layernorm(mlp_lds, ld, I, X);
  mlp_layers<true>(mlp_lds, ld, D->nl, A.clip, A.out,
                   [&](int L) {
                     const int bo = D->boff[L];
                     return MlpLayer{A.image + D->woff[L], bo >= 0 ? A.image + bo : nullptr, D->dims[L], D->dims[L + 1], D->act[L], D->alpha[L]};
                   },
                   [&](int row) -> long long { return tile_row[row]; }, X);
}

// The lists of a ROTATING table, rebuilt on the device ahead of every grouped launch (cosim_policy_table_forward_rotating; rule and
// capacity: cosim_poltab.h).  One workgroup per env range.  It (1) advances the episode counter of every row whose done byte is set and
// takes the row's policy from the rule, (2) rewrites the range's span of `rows` and `tiles` to exactly what build_policy_tiles gives for
// that assignment -- policies ascending, rows ascending within a policy, tiles of at most 32 -- pads the span to its capacity with
// tiles of count 0 (the grouped kernels return on those, so their grid is the capacity: a constant) and leaves the true tile count in
// n_tiles[range].  A stable counting sort: a histogram of the range over policies (LDS integer adds: a sum, whatever their order),
// its scan, then the rows 1024 at a time in ascending order, each placed at (its policy's first slot) + (rows of that policy in earlier
// chunks: a cursor in LDS) + (in earlier waves of the chunk: wcnt) + (in lower lanes of its wave: a ballot).  No step depends on which
// lane or wave arrives first, so the lists are a function of the counters alone.
struct PolRange { int32_t first, count, tile_first, tile_cap; };   // rows [first, first + count), tiles [tile_first, tile_first + tile_cap)

struct PolRegroupArgs {
  const int32_t* base;              // [n] the static assignment, checked by create
  int32_t* episode;                 // [n] ended episodes per row, the caller's
  int32_t* policy_now;              // [n] or null: the policy each row is evaluated with
  const uint8_t *done_a, *done_b;   // [n] or null
  const PolRange* ranges;
  int32_t* rows;                    // [n]
  PolTile* tiles;                   // [sum of tile_cap]
  int32_t* n_tiles;                 // [ranges]
  int range_first, K, every;
};

constexpr int RG_THREADS = 1024, RG_WAVES = RG_THREADS / 64;   // the kernel is bound by the latency of a turn, not by its lanes: wide turns, few of them

__global__ __launch_bounds__(RG_THREADS) void poltab_regroup_kernel(PolRegroupArgs A) {
  __shared__ int hist[POL_MAXK];       // rows of each policy in the range
  __shared__ int slot[POL_MAXK];       // where the next row of each policy goes, relative to the range's span of rows
  __shared__ int tile0[POL_MAXK + 1];  // the first tile of each policy, relative to the range's span of tiles; [K]: the tile count
  __shared__ int wcnt[RG_WAVES][64];          // rows of each policy in each wave of the chunk at hand
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, K = A.K;
  const int ri = A.range_first + blockIdx.x;
  const PolRange R = A.ranges[ri];
  if (t < POL_MAXK) hist[t] = 0;
  wcnt[wave][lane] = 0;
  __syncthreads();
  for (int i = t; i < R.count; i += RG_THREADS) {
    const int r = R.first + i;
    const bool ended = (A.done_a != nullptr && A.done_a[r] != 0) || (A.done_b != nullptr && A.done_b[r] != 0);
    const int e = episodes_after(A.episode[r], ended);
    A.episode[r] = e;
    const int k = policy_at(A.base[r], e, A.every, K);
    if (A.policy_now != nullptr) A.policy_now[r] = k;
    atomicAdd(&hist[k], 1);
  }
  __syncthreads();
  if (t == 0) {   // K <= 64 words: a serial scan costs less than the barriers of a parallel one
    int r = 0, tl = 0;
    for (int k = 0; k < K; k++) {
      slot[k] = r; tile0[k] = tl;
      r += hist[k]; tl += (hist[k] + POL_TILE - 1) / POL_TILE;
    }
    tile0[K] = tl;
    A.n_tiles[ri] = tl;
  }
  __syncthreads();
  // the tiles: a policy's j-th tile begins 32 j rows into the policy's rows; behind the last one the padding
  for (int j = t; j < R.tile_cap; j += RG_THREADS) {
    PolTile T = {0, 0, 0, 0};
    if (j < tile0[K]) {
      int k = 0;
      while (tile0[k + 1] <= j) k++;   // ends: tile0[K] > j
      const int q = j - tile0[k], left = hist[k] - POL_TILE * q;
      T.policy = k; T.start = R.first + slot[k] + POL_TILE * q; T.count = left < POL_TILE ? left : POL_TILE;
    }
    A.tiles[R.tile_first + j] = T;
  }
  // the rows.  `slot` is first written behind two barriers of the first turn, when every thread has left the loop above
  for (int i0 = 0; i0 < R.count; i0 += RG_THREADS) {
    const int i = i0 + t, r = R.first + i;
    const bool valid = i < R.count;
    // episode[r] is this thread's own write of the first loop (same i = t + RG_THREADS m)
    const int k = valid ? policy_at(A.base[r], A.episode[r], A.every, K) : -1;
    int rank = 0;
    unsigned long long todo = __ballot(valid);
    while (todo) {   // one turn per policy met in the wave; `todo` comes from ballots, so the loop is wave-uniform
      const int leader = __ffsll(todo) - 1;
      const int kk = __shfl(k, leader);
      const unsigned long long same = __ballot(valid && k == kk);
      if (valid && k == kk) rank = __popcll(same & ((1ull << lane) - 1ull));
      if (lane == leader) wcnt[wave][kk] = __popcll(same);
      todo &= ~same;
    }
    __syncthreads();
    if (valid) {
      int pos = slot[k] + rank;
      for (int w = 0; w < wave; w++) pos += wcnt[w][k];
      A.rows[R.first + pos] = r;
    }
    __syncthreads();
    if (t < K) {
      int sum = 0;
      for (int w = 0; w < RG_WAVES; w++) { sum += wcnt[w][t]; wcnt[w][t] = 0; }
      slot[t] += sum;
    }
    __syncthreads();
  }
}

// One LSTM cell step for N environments (the recurrent policy of core/policy.py:24-47: the ONNX LSTM node with sequence length 1,
// one direction, default activations; gate order i, o, f, c as ONNX lays W / R / B out).  A workgroup takes 32 environments: [x | h]
// staged in LDS once, each wave owns 32 hidden units at a time and accumulates their four gates (x W^T + h R^T + Wb + Rb) as four
// 32 x 32 tiles on the matrix pipe, then applies c' = sigma(f) c + sigma(i) tanh(g), h' = sigma(o) tanh(c') in registers.
struct LstmArgs {
  const float *x, *h, *c;      // [n, I], [n, H], [n, H]
  const float *W, *R, *B;      // [4H, I], [4H, H], [8H] (Wb then Rb) or null
  float *h_out, *c_out;        // [n, H]; may alias h / c (each element is read before the workgroup that owns its rows writes it)
  int n, I, H, ld;
  int vec;                     // I and H are multiples of 4 and W, R are 16-byte aligned: the float4 path of lstm_gate_tiles
};

typedef float lstm_f32x16 __attribute__((ext_vector_type(16)));

// The cell's inner part, shared by lstm_cell_kernel and lstm_actor_grouped_kernel.  The four gate tiles (i, o, f, c) of 32 envs x the 32
// hidden units col - (l & 31) ..: `xh` is the LDS tile [32][ld] holding [x | h] of the envs, the accumulators start at Wb + Rb and take
// one MFMA step per pair (k, k + 1), k ascending over [x | h] -- that order is the contract (the bits of h' and c').  How the weights are
// fetched is not: with `vec` a lane reads four words of its W / R row at once and feeds two steps from them.
__device__ __forceinline__ void lstm_gate_tiles(const float* xh, int ld, int I, int H, const float* W, const float* R, const float* B, bool vec,
                                                int col, lstm_f32x16 (&acc)[4]) {
  const int l = threadIdx.x & 63, row_a = l & 31, kk = l >> 5, K = I + H;
  const bool cok = col < H;
  const int wc = cok ? col : 0;
#pragma unroll
  for (int q = 0; q < 4; q++) {
    const float bias = (B != nullptr && cok) ? B[q * H + col] + B[4 * H + q * H + col] : 0.f;
#pragma unroll
    for (int v = 0; v < 16; v++) acc[q][v] = bias;
  }
  // One loop for both ways of fetching.  A turn takes LSTM_QUADS quads of k -- per quad the pairs (k, k + 1) and (k + 2, k + 3) -- and
  // fetches the operands of all of them before the first MFMA: a wave runs alone on its SIMD here (the LDS tile leaves room for one or
  // two workgroups), so one round trip to L2 per quad was what a step cost; now it is one per turn.  The loads are unconditional (a
  // column or quad past the end reads a valid address and is zeroed or skipped), so they are not fenced in by branches.  With `vec`
  // neither pair straddles x and h and K is a multiple of 4.
  constexpr int LSTM_QUADS = 4;
  const float* a_row = xh + row_a * ld;
  for (int k0 = 0; k0 < K; k0 += 4 * LSTM_QUADS) {
    float a0[LSTM_QUADS], a1[LSTM_QUADS], w0[LSTM_QUADS][4], w1[LSTM_QUADS][4];
#pragma unroll
    for (int u = 0; u < LSTM_QUADS; u++) {
      const int ka = k0 + 4 * u + kk, kb = ka + 2;
      a0[u] = ka < K ? a_row[ka] : 0.f;
      a1[u] = kb < K ? a_row[kb] : 0.f;
    }
    if (vec) {
      float4 w4[LSTM_QUADS][4];
#pragma unroll
      for (int u = 0; u < LSTM_QUADS; u++) {
        const int kq = k0 + 4 * u, kc = kq < K ? kq : K - 4;
        const bool in_x = kc < I;
        const float* M = in_x ? W : R;
        const int width = in_x ? I : H, kw = in_x ? kc : kc - I;
#pragma unroll
        for (int q = 0; q < 4; q++) w4[u][q] = *reinterpret_cast<const float4*>(M + (size_t)(q * H + wc) * width + kw);
      }
#pragma unroll
      for (int u = 0; u < LSTM_QUADS; u++)
#pragma unroll
        for (int q = 0; q < 4; q++) {
          // the four words as they were loaded: without this the compiler narrows each load to the words a lane selects below, and
          // pays for it with a branch on kk and a full wait per load
          asm volatile("" : "+v"(w4[u][q].x), "+v"(w4[u][q].y), "+v"(w4[u][q].z), "+v"(w4[u][q].w));
          w0[u][q] = cok ? (kk ? w4[u][q].y : w4[u][q].x) : 0.f;
          w1[u][q] = cok ? (kk ? w4[u][q].w : w4[u][q].z) : 0.f;
        }
    } else {
#pragma unroll
      for (int u = 0; u < LSTM_QUADS; u++) {
        const int ka = k0 + 4 * u + kk, kb = ka + 2;
#pragma unroll
        for (int q = 0; q < 4; q++) {
          w0[u][q] = w1[u][q] = 0.f;
          if (cok && ka < K) w0[u][q] = ka < I ? W[(size_t)(q * H + col) * I + ka] : R[(size_t)(q * H + col) * H + (ka - I)];
          if (cok && kb < K) w1[u][q] = kb < I ? W[(size_t)(q * H + col) * I + kb] : R[(size_t)(q * H + col) * H + (kb - I)];
        }
      }
    }
#pragma unroll
    for (int u = 0; u < LSTM_QUADS; u++) {
      const int kq = k0 + 4 * u;   // the branches are wave-uniform: no step past K, as in a loop over pairs
      if (kq < K) {
#pragma unroll
        for (int q = 0; q < 4; q++) acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[u], w0[u][q], acc[q], 0, 0, 0);
      }
      if (kq + 2 < K) {
#pragma unroll
        for (int q = 0; q < 4; q++) acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[u], w1[u][q], acc[q], 0, 0, 0);
      }
    }
  }
}

// The gate arithmetic of one (env, hidden unit): pre-activations of i, o, f, c and the old cell state in, c' and h' out.
__device__ __forceinline__ void lstm_gates(float gi, float go, float gf, float gc, float c, float& c_new, float& h_new) {
  const float ig = 1.f / (1.f + expf(-gi)), og = 1.f / (1.f + expf(-go)), fg = 1.f / (1.f + expf(-gf));
  const float cn = fg * c + ig * tanhf(gc);
  c_new = cn;
  h_new = og * tanhf(cn);
}

__global__ __launch_bounds__(256) void lstm_cell_kernel(LstmArgs A) {
  extern __shared__ float lstm_lds[];   // [32][ld]: x then h of 32 environments
  const int t = threadIdx.x, l = t & 63, wave = t >> 6, n0 = blockIdx.x * 32, I = A.I, H = A.H, K = I + H, ld = A.ld;
  for (int e = t; e < 32 * K; e += 256) {
    const int r = e / K, k = e - r * K;
    float v = 0.f;
    if (n0 + r < A.n) v = k < I ? A.x[(size_t)(n0 + r) * I + k] : A.h[(size_t)(n0 + r) * H + (k - I)];
    lstm_lds[r * ld + k] = v;
  }
  __syncthreads();
  // every c this workgroup needs is read before any of its h / c is written (in-place update across launches is safe; h_out may
  // alias h because h was staged in LDS above and other workgroups own other rows)
  for (int ti = wave; ti * 32 < H; ti += 4) {
    const int col = ti * 32 + (l & 31);
    lstm_f32x16 acc[4];
    lstm_gate_tiles(lstm_lds, ld, I, H, A.W, A.R, A.B, A.vec != 0, col, acc);
#pragma unroll
    for (int v = 0; v < 16; v++) {
      const int row = (v & 3) + 8 * (v >> 2) + 4 * (l >> 5);
      if (col < H && n0 + row < A.n) {
        const size_t o = (size_t)(n0 + row) * H + col;
        float cn, hn;
        lstm_gates(acc[0][v], acc[1][v], acc[2][v], acc[3][v], A.c[o], cn, hn);
        A.c_out[o] = cn;
        A.h_out[o] = hn;
      }
    }
  }
}

// K recurrent actors over one fleet in one launch (cosim_recurrent_table_forward; the table is made and checked by cosim_rectab.h).  A
// workgroup takes one tile of the same tile list as mlp_grouped_kernel -- up to 32 envs of one policy -- and runs the whole actor on it:
// the encoder layers (if any) with mlp_layers, the LSTM cell with the functions above on the envs' rows of the table's state tensors h / c
// ([n, hmax], a policy of hidden size H uses columns 0 .. H), updated in place, and the head layers with mlp_layers on h'.  An env whose
// done_a / done_b byte is set starts from h = c = 0: the episode reset folded into the forward, a select, so a NaN state ends with its
// episode.  LDS: [2][32][ld_m] (encoder / head ping-pong) then [32][ld_x] ([x_enc | h]).  A row is in exactly one tile, h is staged before
// anything is written and c[o] is read by the lane that writes it, so the update in place is safe.
struct RecTabArgs {
  const float* x;          // [n, in_dim]
  float *h, *c;            // [n, hmax]
  float* out;              // [n, out_dim]
  const uint8_t *done_a, *done_b;   // [n] or null
  const float* image;
  const RecDesc* desc;     // [K]
  const int32_t* rows;
  const PolTile* tiles;
  int tile_first, ld_m, ld_x, hmax;
  float clip;              // as MlpArgs::clip
};

__global__ __launch_bounds__(256) void lstm_actor_grouped_kernel(RecTabArgs A) {
  extern __shared__ float rec_lds[];   // [2][32][ld_m], [32][ld_x]
  __shared__ int tile_row[32];         // the env each tile row holds, -1 behind the tile's count
  __shared__ int tile_fresh[32];       // != 0: the env's episode ended, its state reads as zero
  const int ld = A.ld_m, ldx = A.ld_x, hmax = A.hmax;
  const int t = threadIdx.x, l = t & 63, wave = t >> 6;
  float* xh = rec_lds + 2 * 32 * ld;
  // the tile and its policy: indices out of blockIdx alone, so wave-uniform (scalar loads)
  const PolTile T = A.tiles[A.tile_first + blockIdx.x];
  if (T.count == 0) return;            // a padding tile of a rotating table, as in mlp_grouped_kernel
  const RecDesc* D = A.desc + T.policy;
  if (t < 32) {
    const int r = t < T.count ? A.rows[T.start + t] : -1;
    int fresh = 0;
    if (r >= 0) fresh = (A.done_a != nullptr && A.done_a[r] != 0) || (A.done_b != nullptr && A.done_b[r] != 0);
    tile_row[t] = r;
    tile_fresh[t] = fresh;
  }
  __syncthreads();
  const int ne = D->ne, I0 = D->edims[0], I = D->I, H = D->H;
  {
    // the observation rows: into the encoder's input tile, or straight into [x | h] when there is no encoder
    float* dst = ne > 0 ? rec_lds : xh;
    const int dld = ne > 0 ? ld : ldx;
    for (int e = t; e < 32 * I0; e += 256) {
      const int r = e / I0, c = e - r * I0, src = tile_row[r];
      dst[r * dld + c] = src >= 0 ? A.x[(size_t)src * I0 + c] : 0.f;
    }
    for (int e = t; e < 32 * H; e += 256) {
      const int r = e / H, k = e - r * H, src = tile_row[r];
      xh[r * ldx + I + k] = (src >= 0 && !tile_fresh[r]) ? A.h[(size_t)src * hmax + k] : 0.f;
    }
  }
  __syncthreads();
  if (ne > 0) {
    // the last encoder layer reads tile (ne - 1) & 1; its output rows go to the other tile, [32][I], and from there into [x_enc | h]
    float* enc = rec_lds + (ne & 1) * 32 * ld;
    mlp_layers<false>(rec_lds, ld, ne, 0.f, enc,
               [&](int L) {
                 const int bo = D->eboff[L];
                 return MlpLayer{A.image + D->ewoff[L], bo >= 0 ? A.image + bo : nullptr, D->edims[L], D->edims[L + 1], D->eact[L], D->ealpha[L]};
               },
               [&](int row) -> long long { return row; }, NoExt{});
    for (int e = t; e < 32 * I; e += 256) {
      const int r = e / I, k = e - r * I;
      xh[r * ldx + k] = enc[r * I + k];
    }
    __syncthreads();
  }
  const float* W = A.image + D->woff;
  const float* R = A.image + D->roff;
  const float* B = D->boff >= 0 ? A.image + D->boff : nullptr;
  for (int ti = wave; ti * 32 < H; ti += 4) {
    const int col = ti * 32 + (l & 31);
    lstm_f32x16 acc[4];
    lstm_gate_tiles(xh, ldx, I, H, W, R, B, D->vec != 0, col, acc);
#pragma unroll
    for (int v = 0; v < 16; v++) {
      const int row = (v & 3) + 8 * (v >> 2) + 4 * (l >> 5), src = tile_row[row];
      if (col < H) {
        float hn = 0.f;
        if (src >= 0) {
          const size_t o = (size_t)src * hmax + col;
          float cn;
          lstm_gates(acc[0][v], acc[1][v], acc[2][v], acc[3][v], tile_fresh[row] ? 0.f : A.c[o], cn, hn);
          A.c[o] = cn;
          A.h[o] = hn;
        }
        rec_lds[row * ld + col] = hn;   // h' is the head's input tile
      }
    }
  }
  __syncthreads();
  mlp_layers<false>(rec_lds, ld, D->nh, A.clip, A.out,
             [&](int L) {
               const int bo = D->hboff[L];
               return MlpLayer{A.image + D->hwoff[L], bo >= 0 ? A.image + bo : nullptr, D->hdims[L], D->hdims[L + 1], D->hact[L], D->halpha[L]};
             },
             [&](int row) -> long long { return tile_row[row]; }, NoExt{});
}

// Reporter side of the loop (core/reporter.py:210-218, 429-442, 506-508): count / sum / sum of squares per metric column over
// the fleet in one launch.  Columns: info[0..4) as they are, |torque| (info[4 .. 4 + nu)), |command_i - measured_i| for
// i < ncmd (measured = lin_vel_x, lin_vel_y, ang_vel_yaw = info[1 + i]).  acc is [3][K] doubles, K = 4 + nu + ncmd <= 32.
__global__ __launch_bounds__(256) void fleet_stats_kernel(const float* info, int n, int info_dim, int nu, const float* cmd, int cmd_stride,
                                                          int ncmd, double* acc) {
  __shared__ float part[2][8][32];
  const int K = 4 + nu + ncmd, t = threadIdx.x, c = t & 31, g = t >> 5;
  float s = 0.f, q = 0.f;
  if (c < K)
    for (int r = blockIdx.x * 8 + g; r < n; r += gridDim.x * 8) {
      const float* row = info + (size_t)r * info_dim;
      float v;
      if (c < 4) v = row[c];
      else if (c < 4 + nu) v = fabsf(row[c]);
      else { const int i = c - 4 - nu; v = fabsf(cmd[(size_t)r * cmd_stride + i] - row[1 + i]); }
      s += v; q += v * v;
    }
  part[0][g][c] = s; part[1][g][c] = q;
  __syncthreads();
  if (t < 32 && t < K) {
    double ss = 0.0, qq = 0.0;
    for (int k = 0; k < 8; k++) { ss += (double)part[0][k][t]; qq += (double)part[1][k][t]; }
    atomicAdd(&acc[K + t], ss);
    atomicAdd(&acc[2 * K + t], qq);
    if (blockIdx.x == 0) atomicAdd(&acc[t], (double)n);
  }
}

// Percentiles of the same metric columns (N2: core/reporter.py:429-442, 506-530 plots the full series; a fleet keeps a mergeable
// sketch instead): one histogram per column, `nbins` equal bins over [0, hi[c]) (values are magnitudes; column 1..3, the signed base
// velocities, are binned by magnitude too), the last bin also takes everything above the range.  hist is [K][nbins] doubles, summed
// over steps and -- by the caller -- over ranks.
__global__ __launch_bounds__(256) void fleet_hist_kernel(const float* info, int n, int info_dim, int nu, const float* cmd, int cmd_stride,
                                                         int ncmd, const float* hi, int nbins, double* hist) {
  const int K = 4 + nu + ncmd, t = threadIdx.x, c = t & 31, g = t >> 5;
  if (c >= K) return;
  const float scale = (float)nbins / hi[c];
  for (int r = blockIdx.x * 8 + g; r < n; r += gridDim.x * 8) {
    const float* row = info + (size_t)r * info_dim;
    float v;
    if (c < 4 + nu) v = fabsf(row[c]);
    else { const int i = c - 4 - nu; v = fabsf(cmd[(size_t)r * cmd_stride + i] - row[1 + i]); }
    int b = (int)(v * scale);
    b = b < 0 ? 0 : (b >= nbins ? nbins - 1 : b);
    atomicAdd(&hist[(size_t)c * nbins + b], 1.0);
  }
}

}  // namespace cosim
