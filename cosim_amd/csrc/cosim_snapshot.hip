// cosim_snapshot.hip — full-state snapshot rows (cosim_snapshot / cosim_restore / history ring, include/cosim.h).
//
// A snapshot row is one env's whole state record (Layout::s_stride floats: qpos, qvel, warm start, delay line, last action, the 16
// meta words with sim_step and the Philox step counter, the per-field frequency cache, the observation stack) followed by its
// parameter record (Layout::p_stride floats).  Both strides are multiples of 32 floats, so a row is whole 128-byte lines and every
// 16-byte access below is aligned.  Nothing else outlives a control step: the split pipeline's xstate / xcon / xcnt are written by
// the first launch of a control step before any later launch of it reads them, and an overflow flag set by a fleet kernel is cleared
// by the fix-up launch right behind it on the same stream -- between two control steps every flag is 0.
//
// Two kernels, one wave64 per row, lanes striding over the row in float4 loads and stores:
//   snapshot_pack_kernel    live records of envs [env_first, env_first + env_count) -> rows (cosim_snapshot, the history ring)
//   snapshot_gather_kernel  rows[src[d]] -> live records of env d, state and parameter part in the same pass (cosim_restore)
// The gather's source is the caller's buffer, never the live state, so a permutation cannot alias.  Cold paths: no speed target,
// what matters is one launch, no host round trip and that the launch can be captured.
namespace cosim {

struct SnapArgs {
  float* state;            // [N][s_stride] live state records
  float* params;           // [N][p_stride] live parameter records
  float* rows;             // [.][s_stride + p_stride] snapshot rows: pack writes row `env`, gather reads row src[env]
  const int* src;          // gather: int32[N] source row per env, or null = row d
  const uint8_t* mask;     // gather: uint8[N] or null; envs with mask 0 are left untouched
  int* err;                // gather: [0] envs refused (source row outside [0, n_rows)), [1] n_envs - (first refused env); null with src null
  int s_stride, p_stride;  // floats, multiples of 32
  int n_envs, n_rows;      // envs of the engine; rows of the snapshot buffer
  int env_first, env_count;
  int with_params;         // gather: 1 = the parameter record too
};

__global__ __launch_bounds__(64) void snapshot_pack_kernel(SnapArgs a) {
  const int lane = threadIdx.x;
  const int env = a.env_first + (int)blockIdx.x;
  if ((int)blockIdx.x >= a.env_count || env >= a.n_envs) return;
  const int s4 = a.s_stride >> 2, p4 = a.p_stride >> 2;
  const float4* st = reinterpret_cast<const float4*>(a.state + (size_t)env * a.s_stride);
  const float4* pa = reinterpret_cast<const float4*>(a.params + (size_t)env * a.p_stride);
  float4* row = reinterpret_cast<float4*>(a.rows + (size_t)env * (size_t)(a.s_stride + a.p_stride));
  for (int i = lane; i < s4 + p4; i += 64) row[i] = i < s4 ? st[i] : pa[i - s4];
}

__global__ __launch_bounds__(64) void snapshot_gather_kernel(SnapArgs a) {
  const int lane = threadIdx.x;
  const int env = (int)blockIdx.x;
  if (env >= a.n_envs) return;
  // mask and source index: one read per row, wave-uniform
  if (a.mask != nullptr && __builtin_amdgcn_readfirstlane((int)a.mask[env]) == 0) return;
  const int s = a.src != nullptr ? __builtin_amdgcn_readfirstlane(a.src[env]) : env;
  if (s < 0 || s >= a.n_rows) {   // refused: the env keeps its state, the call reports it
    if (lane == 0 && a.err != nullptr) { atomicAdd(&a.err[0], 1); atomicMax(&a.err[1], a.n_envs - env); }
    return;
  }
  const int s4 = a.s_stride >> 2, p4 = a.with_params ? a.p_stride >> 2 : 0;
  const float4* row = reinterpret_cast<const float4*>(a.rows + (size_t)s * (size_t)(a.s_stride + a.p_stride));
  float4* st = reinterpret_cast<float4*>(a.state + (size_t)env * a.s_stride);
  float4* pa = reinterpret_cast<float4*>(a.params + (size_t)env * a.p_stride);
  for (int i = lane; i < s4 + p4; i += 64) {
    const float4 v = row[i];
    if (i < s4) st[i] = v;
    else pa[i - s4] = v;
  }
}

}  // namespace cosim
