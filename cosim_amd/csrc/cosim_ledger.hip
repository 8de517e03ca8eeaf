// cosim_ledger.hip — episode ledger (cosim_ledger_set / cosim_ledger_get, include/cosim.h): per-episode outcomes of every env, kept
// on the device.
//
// The step kernels hand back one control step's done flags and info rows; the next step overwrites them.  ledger_step_kernel runs
// behind a range's last launch of a control step (or of a rollout) on that range's own stream and distils those outputs into a
// per-env accumulator; when a row carries a done flag it closes the episode into one 16-word record in the env's ring and begins
// the next one.  Lane = env, no atomics, no cross-lane traffic: the ledger is a pure function of the step outputs, whatever the
// ranges and the launch order.  The arithmetic is fixed operation by operation (see the kernel) so that the numpy twin
// (cosim_amd/ledger.py reference_ledger) repeats it bit for bit: no products, so nothing the compiler could contract into an FMA.
//
// Accumulators are SoA [field][N] (coalesced lane loads and stores):
//   sum   double[LEDGER_NSUM][N]  0 action_diff_RMSE, 1 lin_vel_x, 2..4 tracking error i, 5 mean abs torque
//   peak  float[2][N]             0 abs torque, 1 tracking error 0
//   acc   int[LEDGER_NINT][N]     0 length, 1 steps_seen, 2 episodes ended (= ordinal of the open one), 3 open flags (bit 8),
//                                 4 spawn row the open episode started from, 5 meta[4] (nan_resets) at its start
//   rec   int[N][slots][16]       the ring: episode o of an env lies in slot o mod slots
// While a scenario table is set (cosim_scenario.hip) word 13 of a record is the scenario row of its episode + 1: for an episode that
// closes, the row scenario_step_kernel wrote ahead of the step that ended it; for an open one, the table's rule at the live meta words.
#include "cosim_scenario.h"
namespace cosim {

constexpr int LEDGER_NSUM = 6, LEDGER_NINT = 6, LEDGER_WORDS = 16;
enum { LEDGER_TERMINATED = 1, LEDGER_TRUNCATED = 2, LEDGER_NONFINITE = 4, LEDGER_NO_RESET = 8, LEDGER_OPEN = 16,
       LEDGER_FELL_TILT = 32, LEDGER_FELL_HEIGHT = 64, LEDGER_FELL_CONTACT = 128 };   // (meta word 15 & 7) << 5

struct LedgerArgs {
  const float* info;       // [K][N][info_dim] the caller's info rows
  const uint8_t* term;     // [K][N]
  const uint8_t* trunc;    // [K][N]
  const float* cmd;        // [N][cmd_stride] raw user commands, or null with ncmd 0
  const float* state;      // [N][s_stride] live state records (meta words 4, 14 and 15 are read)
  double* sum;
  float* peak;
  int* acc;
  int* rec;                // step: the ring; open: [N][16] output rows
  const uint8_t* mask;     // begin: uint8[N] or null
  const int* src;          // begin: the restore's source index or null; envs it refused (outside [0, n_rows)) are left alone
  int n_rows;
  int n_envs, first, count, rows;   // rows: K
  int info_dim, nu, ncmd, cmd_stride, s_stride, s_meta, slots, spawn_rows;
  int flag;                // begin: open flags of the new episode
  int fall;                // a fall rule is set (cosim_fall_set): meta word 15 holds the cause of the env's latest episode end
  const int* scn_row;      // [N] rows the scenario kernel wrote ahead of this step, or null: no table (word 13 stays 0)
  int scn_rows, scn_mode;
  unsigned scn_off;
};

__device__ __forceinline__ float ledger_mean(double s, int n) { return n > 0 ? (float)(s / (double)n) : 0.f; }

// one record from an accumulator, as four 16-byte stores
__device__ __forceinline__ void ledger_store(int* dst, int episode, int length, int flags, int spawn, int seen, const double* s, float pk_tq,
                                             float pk_tr, int scn = 0) {
  int4* d = reinterpret_cast<int4*>(dst);
  d[0] = make_int4(episode, length, flags, spawn);
  d[1] = make_int4(seen, __float_as_int(ledger_mean(s[0], length)), __float_as_int(ledger_mean(s[2], length)),
                   __float_as_int(ledger_mean(s[3], length)));
  d[2] = make_int4(__float_as_int(ledger_mean(s[4], length)), __float_as_int(ledger_mean(s[5], length)), __float_as_int(pk_tq),
                   __float_as_int(ledger_mean(s[1], length)));
  d[3] = make_int4(__float_as_int(pk_tr), scn, 0, 0);
}

// SCN: a scenario table is set.  The two cases are kernels of their own, so that an engine without a table launches the very
// code it launched before there were tables.
template <bool SCN>
__device__ __forceinline__ void ledger_step_body(const LedgerArgs& a) {
  const int i = (int)blockIdx.x * 64 + (int)threadIdx.x;
  if (i >= a.count) return;   // the last wave's tail
  const int env = a.first + i;
  if (env >= a.n_envs) return;
  const size_t N = (size_t)a.n_envs;
  double s[LEDGER_NSUM];
#pragma unroll
  for (int f = 0; f < LEDGER_NSUM; f++) s[f] = a.sum[f * N + env];
  float pk_tq = a.peak[env], pk_tr = a.peak[N + env];
  int length = a.acc[env], seen = a.acc[N + env], episode = a.acc[2 * N + env], oflags = a.acc[3 * N + env], spawn = a.acc[4 * N + env],
      nan0 = a.acc[5 * N + env];
  // the meta words as the range's last launch left them: [4] has advanced if a non-finite state reset the env, [14] is already the
  // row of the episode an auto-reset began, [15] is the cause of the latest episode end (like the other two exact per launch, not per
  // row of a rollout; with no fall rule the word is not read: a rule that was set and cleared may have left one behind)
  const int* meta = reinterpret_cast<const int*>(a.state + (size_t)env * a.s_stride + a.s_meta);
  const int nan_now = meta[4], spawn_now = a.spawn_rows > 0 ? meta[14] : -1;
  const int fell = a.fall ? (meta[15] & 7) << 5 : 0;
  const int scn = SCN ? a.scn_row[env] + 1 : 0;
  float c[3] = {0.f, 0.f, 0.f};
  for (int k = 0; k < 3; k++)
    if (k < a.ncmd) c[k] = a.cmd[(size_t)env * a.cmd_stride + k];
  const float fnu = (float)a.nu;
  for (int k = 0; k < a.rows; k++) {
    const size_t r = (size_t)k * N + env;
    const float* row = a.info + r * a.info_dim;
    length++; seen++;
    s[0] += (double)row[0];
    s[1] += (double)row[1];
    float e0 = 0.f;
    for (int q = 0; q < 3; q++)
      if (q < a.ncmd) {
        const float d = fabsf(c[q] - row[1 + q]);   // fp32 subtraction first (cosim_fleet_stats' convention)
        s[2 + q] += (double)d;
        if (q == 0) e0 = d;
      }
    float tq = 0.f, tmax = 0.f;
    for (int j = 0; j < a.nu; j++) {
      const float t = fabsf(row[4 + j]);
      tq = tq + t;
      tmax = fmaxf(tmax, t);
    }
    s[5] += (double)(tq / fnu);
    pk_tq = fmaxf(pk_tq, tmax);   // fmaxf ignores NaN
    if (a.ncmd > 0) pk_tr = fmaxf(pk_tr, e0);
    const int te = a.term[r] != 0, tr = a.trunc[r] != 0;
    if (te | tr) {
      const int flags = (te ? LEDGER_TERMINATED : 0) | (tr ? LEDGER_TRUNCATED : 0) | (nan_now != nan0 ? LEDGER_NONFINITE : 0) | oflags | fell;
      ledger_store(a.rec + ((size_t)env * a.slots + (size_t)(episode % a.slots)) * LEDGER_WORDS, episode, length, flags, spawn, seen, s,
                   pk_tq, pk_tr, scn);
      episode++;
#pragma unroll
      for (int f = 0; f < LEDGER_NSUM; f++) s[f] = 0.0;
      pk_tq = 0.f; pk_tr = 0.f; length = 0; oflags = 0; spawn = spawn_now; nan0 = nan_now;
    }
  }
#pragma unroll
  for (int f = 0; f < LEDGER_NSUM; f++) a.sum[f * N + env] = s[f];
  a.peak[env] = pk_tq; a.peak[N + env] = pk_tr;
  a.acc[env] = length; a.acc[N + env] = seen; a.acc[2 * N + env] = episode; a.acc[3 * N + env] = oflags; a.acc[4 * N + env] = spawn;
  a.acc[5 * N + env] = nan0;
}
__global__ __launch_bounds__(64) void ledger_step_kernel(LedgerArgs a) { ledger_step_body<false>(a); }
__global__ __launch_bounds__(64) void ledger_step_scn_kernel(LedgerArgs a) { ledger_step_body<true>(a); }

// the masked envs begin an episode; what they had open is discarded (an episode the host cut short is not an outcome)
__global__ __launch_bounds__(64) void ledger_begin_kernel(LedgerArgs a) {
  const int env = (int)blockIdx.x * 64 + (int)threadIdx.x;
  if (env >= a.n_envs) return;
  if (a.mask != nullptr && a.mask[env] == 0) return;
  if (a.src != nullptr && (a.src[env] < 0 || a.src[env] >= a.n_rows)) return;
  const size_t N = (size_t)a.n_envs;
#pragma unroll
  for (int f = 0; f < LEDGER_NSUM; f++) a.sum[f * N + env] = 0.0;
  a.peak[env] = 0.f; a.peak[N + env] = 0.f;
  const int* meta = reinterpret_cast<const int*>(a.state + (size_t)env * a.s_stride + a.s_meta);
  a.acc[env] = 0;
  a.acc[3 * N + env] = a.flag;
  a.acc[4 * N + env] = a.spawn_rows > 0 ? meta[14] : -1;
  a.acc[5 * N + env] = meta[4];
}

// the open accumulators as records (flag 16) into rec [N][16]
template <bool SCN>
__device__ __forceinline__ void ledger_open_body(const LedgerArgs& a) {
  const int env = (int)blockIdx.x * 64 + (int)threadIdx.x;
  if (env >= a.n_envs) return;
  const size_t N = (size_t)a.n_envs;
  double s[LEDGER_NSUM];
#pragma unroll
  for (int f = 0; f < LEDGER_NSUM; f++) s[f] = a.sum[f * N + env];
  const int* meta = reinterpret_cast<const int*>(a.state + (size_t)env * a.s_stride + a.s_meta);
  const int flags = LEDGER_OPEN | a.acc[3 * N + env] | (meta[4] != a.acc[5 * N + env] ? LEDGER_NONFINITE : 0);
  int scn = 0;
  if (SCN) {
    ScnTable T = {};
    T.n_scn = a.scn_rows; T.mode = a.scn_mode; T.gid_off = a.scn_off;
    scn = scenario_row(T, env, meta[11]) + 1;
  }
  ledger_store(a.rec + (size_t)env * LEDGER_WORDS, a.acc[2 * N + env], a.acc[env], flags, a.acc[4 * N + env], a.acc[N + env], s, a.peak[env],
               a.peak[N + env], scn);
}
__global__ __launch_bounds__(64) void ledger_open_kernel(LedgerArgs a) { ledger_open_body<false>(a); }
__global__ __launch_bounds__(64) void ledger_open_scn_kernel(LedgerArgs a) { ledger_open_body<true>(a); }

}  // namespace cosim
