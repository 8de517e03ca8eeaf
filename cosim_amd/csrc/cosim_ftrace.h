// cosim_ftrace.h — the per-env rules of the failure traces (cosim_ftrace_set / cosim_ftrace_get, include/cosim.h) as inline
// functions that the device kernels (cosim_ftrace.hip) and a plain host C++ program (tests/ftrace_lanes.cpp) both compile.
//
// Every env keeps a window of its last `frames` control steps; when an episode ends with a selected cause the window is frozen as
// a trace and the env carries on in a fresh window.  A frame is one control step, F 32-bit words (F a multiple of 4), every word a
// plain copy -- nothing here does arithmetic on a float:
//   [0] 1-based episode step   [1] 1 terminated | 2 truncated   [2..3] 0
//   qpos[nq] qvel[nv]          the state record as the previous step (or the reset) left it: the state the step started from
//   action[nu]                 the caller's raw action row      command[cd]  the applied command      info[info_dim]  the info row
// Storage per env: keep + 1 buffers of FT_HDR + frames * F words (a header, then a ring of frames), and FT_NCNT counters:
//   cnt [N][FT_NCNT]  0 working buffer, 1 traces triggered, 2 traces lost, 3 ring cursor, 4 length, 5 episode ordinal, 6 open
//                     flags (bit 8), 7 meta[4] (nan_resets) at the episode's start, 8 its spawn row, 9 steps_seen
// A trigger writes the header of the working buffer and moves the working index on, modulo keep + 1: nothing is copied, the keep
// buffers behind the working one are the latest keep traces.  An episode always starts at ring position 0.
//
// The bodies are written per lane: lane `lane` of `nl` handles the words lane, lane + nl, ... of whatever is copied, and every
// lane computes the same counters from the same loaded values (the caller stores them once, after all lanes have run).
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define FT_HD __host__ __device__ __forceinline__
#else
#define FT_HD inline
#endif

namespace cosim {

constexpr int FT_HDR = 16, FT_NCNT = 16, FT_FRAME_HDR = 4;
constexpr int FT_MAX_FRAMES = 1024, FT_MAX_KEEP = 64;
// the ledger's flag values (cosim_ledger.hip)
enum { FT_TERMINATED = 1, FT_TRUNCATED = 2, FT_NONFINITE = 4, FT_NO_RESET = 8, FT_OPEN = 16, FT_FELL_TILT = 32, FT_FELL_HEIGHT = 64,
       FT_FELL_CONTACT = 128, FT_ON_ALL = 1 | 2 | 4 | 32 | 64 | 128 };

struct FtArgs {
  const float* actions;    // [N][nu] the caller's action rows of this step
  const float* cmd;        // [N][cd] the applied command (scenario_cmd), or null with cd 0
  const float* info;       // [N][info_dim]
  const uint8_t* term;     // [N]
  const uint8_t* trunc;    // [N]
  const float* state;      // [N][s_stride] live state records
  int* buf;                // [N][keep + 1][FT_HDR + frames * F]
  int* cnt;                // [N][FT_NCNT]
  int* open_out;           // open: [N][FT_HDR] output rows
  const uint8_t* mask;     // begin: uint8[N] or null
  const int* src;          // begin: the restore's source index or null; envs it refused (outside [0, n_rows)) are left alone
  const int* scn_row;      // [N] rows the scenario kernel wrote ahead of this step, or null: no table (header word 6 stays 0)
  int n_rows;
  int n_envs, first, count;
  int nq, nv, nu, cd, info_dim, F;
  int s_stride, s_qpos, s_qvel, s_meta;
  int frames, keep, on_mask, spawn_rows, fall;
  int flag;                // begin: open flags of the new episode
  int scn_rows, scn_mode;  // open: the table's rule at the live meta words
  unsigned scn_off;
};

struct FtCnt { int work, trig, lost, cursor, length, episode, oflags, nan0, spawn, seen; };

FT_HD int ftrace_frame_words(int nq, int nv, int nu, int cd, int info_dim) { return (FT_FRAME_HDR + nq + nv + nu + cd + info_dim + 3) & ~3; }
FT_HD size_t ftrace_buf_words(int frames, int F) { return (size_t)FT_HDR + (size_t)frames * (size_t)F; }

FT_HD FtCnt ftrace_load(const int* c) {
  FtCnt k;
  k.work = c[0]; k.trig = c[1]; k.lost = c[2]; k.cursor = c[3]; k.length = c[4]; k.episode = c[5]; k.oflags = c[6]; k.nan0 = c[7];
  k.spawn = c[8]; k.seen = c[9];
  return k;
}
FT_HD void ftrace_store(int* c, const FtCnt& k) {
  c[0] = k.work; c[1] = k.trig; c[2] = k.lost; c[3] = k.cursor; c[4] = k.length; c[5] = k.episode; c[6] = k.oflags; c[7] = k.nan0;
  c[8] = k.spawn; c[9] = k.seen;
}

FT_HD int* ftrace_buffer(const FtArgs& a, int env, int b) {
  return a.buf + ((size_t)env * (size_t)(a.keep + 1) + (size_t)b) * ftrace_buf_words(a.frames, a.F);
}

// word w of a header
FT_HD int ftrace_header_word(int w, int episode, int length, int flags, int valid, int oldest, int spawn, int scn, int seen) {
  switch (w) {
    case 0: return episode;
    case 1: return length;
    case 2: return flags;
    case 3: return valid;
    case 4: return oldest;
    case 5: return spawn;
    case 6: return scn;
    case 7: return seen;
    default: return 0;
  }
}

// the state part of a frame from the live state record: the coalesced rec[l] loads of the step kernels, a contiguous store
FT_HD void ftrace_state_part(const FtArgs& a, int env, int* frame, int lane, int nl) {
  const int* rec = reinterpret_cast<const int*>(a.state + (size_t)env * a.s_stride);
  for (int w = lane; w < a.nq; w += nl) frame[FT_FRAME_HDR + w] = rec[a.s_qpos + w];
  for (int w = lane; w < a.nv; w += nl) frame[FT_FRAME_HDR + a.nq + w] = rec[a.s_qvel + w];
}

// One env behind one control step (ftrace_step_kernel).  `c`: the env's counters as loaded before any lane ran; updated in place.
FT_HD void ftrace_step_lane(const FtArgs& a, int env, int lane, int nl, FtCnt& c) {
  const int* meta = reinterpret_cast<const int*>(a.state + (size_t)env * a.s_stride + a.s_meta);
  // the meta words as the range's last launch left them (the ledger's reading): [4] has advanced if a non-finite state reset the
  // env, [14] is already the row of the episode an auto-reset began, [15] the cause of the latest episode end while a rule is set
  const int nan_now = meta[4], spawn_now = a.spawn_rows > 0 ? meta[14] : -1;
  const int fell = a.fall ? (meta[15] & 7) << 5 : 0;
  const int te = a.term[env] != 0, tr = a.trunc[env] != 0;
  c.length++; c.seen++;
  // 1. the outcome part of the cursor's frame
  int* frame = ftrace_buffer(a, env, c.work) + FT_HDR + (size_t)c.cursor * a.F;
  for (int w = lane; w < FT_FRAME_HDR; w += nl) frame[w] = w == 0 ? c.length : (w == 1 ? (te ? FT_TERMINATED : 0) | (tr ? FT_TRUNCATED : 0) : 0);
  int* out = frame + FT_FRAME_HDR + a.nq + a.nv;
  const int* act = reinterpret_cast<const int*>(a.actions + (size_t)env * a.nu);
  for (int w = lane; w < a.nu; w += nl) out[w] = act[w];
  out += a.nu;
  if (a.cd > 0) {
    const int* cm = reinterpret_cast<const int*>(a.cmd + (size_t)env * a.cd);
    for (int w = lane; w < a.cd; w += nl) out[w] = cm[w];
    out += a.cd;
  }
  const int* inf = reinterpret_cast<const int*>(a.info + (size_t)env * a.info_dim);
  for (int w = lane; w < a.info_dim; w += nl) out[w] = inf[w];
  if (te | tr) {
    // 2. the episode ends: freeze the window (a selected cause) or empty it in place, then begin the next episode
    const int flags = (te ? FT_TERMINATED : 0) | (tr ? FT_TRUNCATED : 0) | (nan_now != c.nan0 ? FT_NONFINITE : 0) | c.oflags | fell;
    if ((flags & a.on_mask) != 0) {
      const int valid = c.length < a.frames ? c.length : a.frames;
      const int oldest = c.length <= a.frames ? 0 : (c.cursor + 1) % a.frames;
      const int scn = a.scn_row != nullptr ? a.scn_row[env] + 1 : 0;
      int* hdr = ftrace_buffer(a, env, c.work);
      for (int w = lane; w < FT_HDR; w += nl) hdr[w] = ftrace_header_word(w, c.episode, c.length, flags, valid, oldest, c.spawn, scn, c.seen);
      c.work = (c.work + 1) % (a.keep + 1);
      c.trig++;
      if (c.trig > a.keep) c.lost++;   // the buffer that becomes the working one held the oldest kept trace
    }
    c.episode++;
    c.cursor = 0; c.length = 0; c.oflags = 0; c.spawn = spawn_now; c.nan0 = nan_now;
  } else {
    // 3. the window moves on
    c.cursor = (c.cursor + 1) % a.frames;
  }
  // 4. the state the next step starts from (after a done step under auto-reset: the new episode's reset pose)
  ftrace_state_part(a, env, ftrace_buffer(a, env, c.work) + FT_HDR + (size_t)c.cursor * a.F, lane, nl);
}

// whether ftrace_begin_lane applies to env (mask and restore source, as ledger_begin_kernel reads them)
FT_HD bool ftrace_begin_applies(const FtArgs& a, int env) {
  if (a.mask != nullptr && a.mask[env] == 0) return false;
  if (a.src != nullptr && (a.src[env] < 0 || a.src[env] >= a.n_rows)) return false;
  return true;
}

// One env behind a reset / restore / set (ftrace_begin_kernel): the open window is discarded, an episode begins at ring position 0.
FT_HD void ftrace_begin_lane(const FtArgs& a, int env, int lane, int nl, FtCnt& c) {
  const int* meta = reinterpret_cast<const int*>(a.state + (size_t)env * a.s_stride + a.s_meta);
  c.cursor = 0; c.length = 0; c.oflags = a.flag;
  c.spawn = a.spawn_rows > 0 ? meta[14] : -1;
  c.nan0 = meta[4];
  ftrace_state_part(a, env, ftrace_buffer(a, env, c.work) + FT_HDR, lane, nl);
}

// The header of an env's open window (ftrace_open_kernel), word w.  The cursor's frame already carries the next step's starting
// state, so an open window has at most frames - 1 whole frames: valid = min(length, frames - 1).
FT_HD int ftrace_open_word(const FtArgs& a, int env, int w, const FtCnt& c, int scn) {
  const int* meta = reinterpret_cast<const int*>(a.state + (size_t)env * a.s_stride + a.s_meta);
  const int flags = FT_OPEN | c.oflags | (meta[4] != c.nan0 ? FT_NONFINITE : 0);
  const int valid = c.length < a.frames - 1 ? c.length : a.frames - 1;
  const int oldest = c.length <= a.frames - 1 ? 0 : (c.cursor + 1) % a.frames;
  return ftrace_header_word(w, c.episode, c.length, flags, valid, oldest, c.spawn, scn, c.seen);
}

}  // namespace cosim
