// cosim_scenario.h — the per-env rule of a scenario table (cosim_scenario_set, include/cosim.h), as one inline function that the
// device kernel (cosim_scenario.hip) and a plain host C++ program (tests/test_scenario_host.py) both compile.
//
// A table is S scenarios in CSR form: scenario s owns command keyframes [key_adr[s], key_adr[s + 1]) -- times key_t strictly
// increasing, rows key_cmd[k][command_dim] -- and push windows [push_adr[s], push_adr[s + 1]) -- push_t[p] = (t0, t1), world
// velocity push_v[p][3].  Per env and control step, with t = meta[0] (steps of the running episode) and ep = meta[11] (episodes
// ended):
//   row  = gid mod S (mode 0, "env")  |  (gid mod S + ep mod S) mod S (mode 1, "cycle", ep as uint32)
//   cmd  = the last keyframe of the row with key_t <= t, whole row; none: the caller's command
//   push = the last LISTED window of the row with t0 <= t < t1; qvel[0:3] is then set as cosim_event_push sets it
// Everything is a function of words of the state record: nothing is kept per env.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define SCN_HD __host__ __device__ __forceinline__
#else
#define SCN_HD inline
#endif
// the table never changes while a kernel runs: on the device it is read through the constant address space, as the model block is
#if defined(__HIP_DEVICE_COMPILE__)
#define SCN_TAB(T) const T __attribute__((address_space(4)))*
#define SCN_TAB_CAST(T, p) ((SCN_TAB(T))(unsigned long long)(p))
#else
#define SCN_TAB(T) const T*
#define SCN_TAB_CAST(T, p) (p)
#endif

namespace cosim {

enum { SCN_MODE_ENV = 0, SCN_MODE_CYCLE = 1 };
constexpr int SCN_MAX_ROWS = 65536, SCN_MAX_ITEMS = 64, SCN_MAX_TIME = 1 << 30;

struct ScnTable {
  const int32_t* key_adr;    // [S + 1]
  const int32_t* key_t;      // [nkey]
  const float* key_cmd;      // [nkey][cd]
  const int32_t* push_adr;   // [S + 1]
  const int32_t* push_t;     // [npush][2]
  const float* push_v;       // [npush][3]
  int n_scn, mode, cd;
  unsigned gid_off;          // env_id0 mod S (non-negative): gid mod S = (gid_off + env) mod S
};

// The row of env `env` in its episode number `ep`; always inside [0, S) whatever `ep` holds.
SCN_HD int scenario_row(const ScnTable& T, int env, int ep) {
  const unsigned S = (unsigned)T.n_scn;
  unsigned row = (T.gid_off + (unsigned)env) % S;
  if (T.mode == SCN_MODE_CYCLE) row = (row + (unsigned)ep % S) % S;
  return (int)(row < S ? row : S - 1u);
}

// qvel[0:2] = (R^T v)[0:2], qvel[2] = v[2] with R from the raw quaternion (w, x, y, z): push_kernel's arithmetic (cosim_engine.hip),
// restated operation by operation in the order and with the fused multiply-adds that kernel compiles to, contraction off, so that
// a scheduled push gives the bits of cosim_event_push.
SCN_HD void scenario_push(const float* quat, float v0, float v1, float v2, float* qvel) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float w = quat[0], x = quat[1], y = quat[2], z = quat[3];
  const float x2 = x + x, y2 = y + y, z2 = z + z;
  const float zw = w * z2, yw = w * y2;
  const float R01 = fmaf(x2, y, -zw), R10 = fmaf(x2, y, zw);
  const float R00 = fmaf(-z, z2, fmaf(-y, y2, 1.f));
  const float R20 = fmaf(x2, z, -yw);
  const float R11 = fmaf(-z, z2, fmaf(-x, x2, 1.f));
  const float R21 = fmaf(w, x2, y2 * z);
  qvel[0] = fmaf(R20, v2, fmaf(v0, R00, v1 * R10));
  qvel[1] = fmaf(R21, v2, fmaf(R01, v0, R11 * v1));
  qvel[2] = v2;
}

// One env, one control step: cmd_out[0 .. cd) and, if `push` and a window is due, qvel[0:3].  Returns 1 if a push was applied.
SCN_HD int scenario_apply(const ScnTable& T, int row, int t, const float* cmd_in, float* cmd_out, const float* quat, float* qvel, bool push) {
  SCN_TAB(int32_t) key_adr = SCN_TAB_CAST(int32_t, T.key_adr);
  SCN_TAB(int32_t) key_t = SCN_TAB_CAST(int32_t, T.key_t);
  SCN_TAB(float) key_cmd = SCN_TAB_CAST(float, T.key_cmd);
  const int k0 = key_adr[row], k1 = key_adr[row + 1];
  int sel = -1;
  for (int k = k0; k < k1; k++) {   // sorted: stop at the first keyframe still ahead
    if (key_t[k] > t) break;
    sel = k;
  }
  for (int c = 0; c < T.cd; c++) cmd_out[c] = sel >= 0 ? key_cmd[(size_t)sel * T.cd + c] : cmd_in[c];
  if (!push) return 0;
  SCN_TAB(int32_t) push_adr = SCN_TAB_CAST(int32_t, T.push_adr);
  SCN_TAB(int32_t) push_t = SCN_TAB_CAST(int32_t, T.push_t);
  SCN_TAB(float) push_v = SCN_TAB_CAST(float, T.push_v);
  const int p0 = push_adr[row], p1 = push_adr[row + 1];
  int hit = -1;
  for (int p = p0; p < p1; p++)
    if (push_t[2 * p] <= t && t < push_t[2 * p + 1]) hit = p;   // the last listed window wins
  if (hit < 0) return 0;
  scenario_push(quat, push_v[3 * hit], push_v[3 * hit + 1], push_v[3 * hit + 2], qvel);
  return 1;
}

}  // namespace cosim
