// cosim_engine.hip — host side of libcosim_hip.so: the C ABI declared in include/cosim.h.
//
// Converts the fp64 ModelBlob into fp32 device tables, owns the per-env HBM records (state + randomised parameters),
// and launches the one-wave-per-env kernel (cosim_kernels.hip) specialised for the model's (nv, nbody).
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <time.h>
#include <string.h>

#include <atomic>
#include <memory>
#include <string>
#include <vector>

#include "../../include/cosim_actor.h"
#include "cosim_kernels.hip"
#include "cosim_mlp.hip"
#include "cosim_spawn.hip"
#include "cosim_snapshot.hip"
#include "cosim_ledger.hip"
#include "cosim_ftrace.hip"
#include "cosim_scenario.hip"
#include "cosim_scnparams.hip"
#include "cosim_obsfault.hip"
#include "cosim_actfault.hip"
#include "cosim_checks.hip"
#include "cosim_curves.hip"
#include "cosim_search.hip"
#include "cosim_latency.hip"
#include "cosim_devbuf.h"
#include "cosim_plan.h"
#include "cosim_ranges.h"
#include "cosim_tables.h"

using namespace cosim;

struct cosim_engine;
using launch_fn = void (*)(cosim_engine*, const KArgs&, int n, hipStream_t);

static thread_local std::string g_err;
static int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}
#define RC_TRY(...) do { const int _rc = (__VA_ARGS__); if (_rc) return _rc; } while (0)   // a COSIM_* code of a call that has set the message
#define HIP_TRY(expr)                                                                         \
  do {                                                                                        \
    hipError_t _e = (expr);                                                                   \
    if (_e != hipSuccess) return fail(COSIM_EHIP, std::string(#expr) + ": " + hipGetErrorString(_e)); \
  } while (0)
// the same for a call whose message names the entry point (`who`), not the expression; HIP_TRY_CLEAR also takes the error out of
// hipGetLastError, where it would otherwise stick
#define HIP_TRY_AS(who, expr)                                                                 \
  do {                                                                                        \
    const hipError_t _e = (expr);                                                             \
    if (_e != hipSuccess) return fail(COSIM_EHIP, std::string(who) + ": " + hipGetErrorString(_e)); \
  } while (0)
#define HIP_TRY_CLEAR(who, expr)                                                              \
  do {                                                                                        \
    const hipError_t _e = (expr);                                                             \
    if (_e != hipSuccess) { (void)hipGetLastError(); return fail(COSIM_EHIP, std::string(who) + ": " + hipGetErrorString(_e)); } \
  } while (0)

// ---- the allocator policies of DevBuf (cosim_devbuf.h): every allocation of the library is made and released here
// device allocations that are live in this process (cosim_query "device_buffers"): what a test compares to hold that nothing leaked
static std::atomic<int> g_device_buffers{0};

struct HipDevice {
  using error_t = hipError_t;
  static constexpr error_t ok = hipSuccess;
  static error_t malloc(void** p, size_t bytes) {
    const error_t r = hipMalloc(p, bytes);
    if (r == ok && *p) g_device_buffers.fetch_add(1, std::memory_order_relaxed);
    return r;
  }
  static void free(void* p) {
    (void)hipFree(p);
    g_device_buffers.fetch_sub(1, std::memory_order_relaxed);
  }
  static error_t memset(void* p, int v, size_t bytes) { return hipMemset(p, v, bytes); }
  static error_t to_device(void* dst, const void* host, size_t bytes) { return hipMemcpy(dst, host, bytes, hipMemcpyHostToDevice); }
  static error_t to_host(void* host, const void* src, size_t bytes) { return hipMemcpy(host, src, bytes, hipMemcpyDeviceToHost); }
};
struct HipPinned {   // page-locked host memory (not counted)
  using error_t = hipError_t;
  static constexpr error_t ok = hipSuccess;
  static error_t malloc(void** p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault); }
  static void free(void* p) { (void)hipHostFree(p); }
};
template <class T> using Dev = DevBuf<T, HipDevice>;
template <class T> using Pinned = DevBuf<T, HipPinned>;

// ---- what each feature holds on the device, with the scalars that mean something only beside it: assigning an empty group drops the
// feature.  The caller has waited for the device (table_quiesce / hipDeviceSynchronize): no launch in flight touches what goes.
// spawn table (cosim_spawn_set): base poses the reset block takes instead of init_qpos[0:7]; placed by spawn_place_kernel
struct Spawn {
  Dev<float> table;           // [rows][8]
  std::vector<float> host;    // host copy of the placed table (cosim_spawn_get)
  int rows = 0, mode = 0;
};
// the error word of the gather kernel and its pinned host copy ([2] each): both or neither
struct SnapErr {
  Dev<int> dev;
  Pinned<int> host;
};
// history ring (cosim_history_set): every `every`-th cosim_step packs each range's rows into slot (capture number) mod slots
struct History {
  Dev<float> ring;            // [slots][n_envs][snapshot_floats]
  int slots = 0, every = 0;
  long calls = 0, captures = 0;   // cosim_step calls / captures since cosim_history_set
  std::vector<long> call_of;      // per slot: the call count its capture was taken after
};
// episode ledger (cosim_ledger_set, cosim_ledger.hip): ledger_step_kernel behind every range's last launch of a step / rollout
struct Ledger {
  Dev<double> sum;            // [LEDGER_NSUM][n_envs]
  Dev<float> peak;            // [2][n_envs]
  Dev<int> acc;               // [LEDGER_NINT][n_envs]
  Dev<int> rec;               // [n_envs][slots][16]
  int slots = 0;
};
// failure traces (cosim_ftrace_set, cosim_ftrace.hip): ftrace_step_kernel behind every range's last launch of a step, behind the ledger's
struct Ftrace {
  Dev<int> buf;               // [n_envs][keep + 1][FT_HDR + frames * F]
  Dev<int> cnt;               // [n_envs][FT_NCNT]
  int frames = 0, keep = 0, mask = 0;
};
// scenario table (cosim_scenario_set, cosim_scenario.hip): scenario_step_kernel ahead of every range's first launch of a step / reset
struct Scenario {
  Dev<char> image;            // one allocation: key_adr | push_adr | key_t | push_t | key_cmd | push_v
  ScnTable tab = {};          // device pointers into the image; n_scn 0: no table, no scenario launches
  int nkey = 0, npush = 0;
  float* cmd_out = nullptr;   // [n_envs][command_dim] caller-owned: what the step kernels read as the command while a table is set
  int32_t* row_out = nullptr; // [n_envs] caller-owned
};
// parameter windows of the scenario table (cosim_scenario_params_set, cosim_scnparams.hip): scnparams_step_kernel behind every scenario launch
struct ScnParams {
  Dev<char> image;            // one allocation: adr | t | word | op | value
  ScnParTable tab = {};       // device pointers into the image; n_items 0: no windows, no launches, the step kernels read d_params
  Dev<float> eff;             // [n_envs][p_stride] effective records: what base_args hands the step kernels while windows are set
  int marked = 0;             // items whose op carries SCNPAR_MARK (scnparams_search_step_kernel scales them)
};
// observation faults (cosim_set_param "obs_faults", cosim_obsfault.hip): obsfault_step_kernel behind every step's / reset's last launch;
// action faults (cosim_set_param "action_faults", cosim_actfault.hip): actfault_step_kernel ahead of every control step's first launch,
// actfault_obs_kernel behind its last
struct Faults {
  Dev<char> image;            // one allocation: adr | item
  FaultTable tab = {};        // device pointers into the image; n_items 0: no faults, no launches
  int marked = 0;             // items that carry FLT_MARK (the *_search_step_kernel of the kind scales them)
};
// the two action rows, shared by the action faults and the latency's action items: there while either kind has items (action_rows_release)
struct ActionRows {
  Dev<float> eff;             // [n_envs][nu] effective actions: what the step kernels are handed while faults are set
  Dev<float> raw;             // [n_envs][nu] the caller's actions of the last step (last_action is rebuilt from them)
  // both or neither; zeroed, so that a read ahead of the first step finds no stale bytes
  hipError_t alloc(size_t count) {
    hipError_t r = eff.alloc_zeroed(count);
    if (r == hipSuccess) r = raw.alloc_zeroed(count);
    if (r != hipSuccess) eff.reset();
    return r;
  }
};
// latency lines of the scenario table (cosim_set_param "latency", cosim_latency.hip): latency_act_kernel ahead of actfault_step_kernel,
// latency_obs_kernel ahead of obsfault_step_kernel
struct Latency {
  Dev<char> image;            // one allocation: act_adr | obs_adr | act_item | obs_item
  LatTable tab = {};          // device pointers into the image; n_act + n_obs 0: no latency, no launches
  Dev<float> act_line;        // [n_envs][depth][nu], with action items
  Dev<float> obs_line;        // [n_envs][depth][frame_dim], with observation items
  Dev<int> from;              // [2][n_envs]: the clock each env's action / observation line is valid from (< 0: invalid)
  Dev<float> eff;             // [n_envs][nu] the delivered actions while action faults are set too: what actfault_step_kernel reads
  Dev<float> spare;           // [n_envs][nu] where actfault_step_kernel's copy of them goes then
};
// checks of the scenario table (cosim_scenario_checks_set, cosim_checks.hip): checks_step_kernel behind every range's last launch of a
// step, behind the ledger's
struct Checks {
  Dev<char> image;            // one allocation: adr | t | signal | index | mode | cmp | bound
  ChkTable tab = {};          // device pointers into the image; n_scn 0: no checks, no launches
  Dev<float> ext;             // [n_envs][I]
  Dev<int> aux, n;            // [n_envs][I]
  Dev<double> sum;            // [n_envs][I]
  Dev<int> cnt;               // [n_envs][CHK_NCNT]
  Dev<int> rec;               // [n_envs][slots][8 + 2 I]
  int slots = 0;
};
// response curves of the scenario table (cosim_scenario_curves_set, cosim_curves.hip): curves_step_kernel behind every range's last
// launch of a step, behind the checks'.  Groups (cosim_scenario_curves_groups): with G > 0 the cells are G planes of `words`, and the
// step launches curves_step_grouped_kernel, which reads the caller's group word of an env when its episode ends; they go with the cells they split
struct Curves {
  Dev<char> image;            // one allocation: adr | t | signal | index | bins | nt | soff | coff | cw | lo | hi | inv_w
  CurTable tab = {};          // device pointers into the image; n_scn 0: no curves, no launches
  Dev<int> stage;             // [n_envs][SW]
  Dev<int> clk;               // [n_envs]
  Dev<unsigned> cells;        // max(G, 1) planes of `words` 32-bit words
  size_t words = 0;
  int groups = 0;                     // G; 0: no groups, one plane, curves_step_kernel
  const int32_t* group = nullptr;     // [n_envs], the caller's
  Dev<unsigned> ungrouped;            // one word: ended episodes whose group word was outside [0, G)
};
// limit search of the scenario table (cosim_set_param "search", cosim_search.hip): scenario_search_step_kernel in the place of
// scenario_step_kernel, search_step_kernel behind every range's last launch of a step, behind the curves'
struct Search {
  Dev<char> image;            // one allocation: has | lo | hi | x0 | d0 | d_min | rule | trials | targets | fail_mask | rev_skip
  SrchTable tab = {};         // device pointers into the image; n_items 0: no search, no launches, scenario_step_kernel
  Dev<int> rec;               // [n_envs][SRCH_NCNT]
  Dev<int> ring;              // [n_envs][slots][4]
  Dev<int> rem;               // one word: envs with an item that are not done
  int slots = 0;
  // what the other setters hold their tables against while a search is armed: the host's copy of has | lo | hi | targets, the union
  // of the items' targets and whether an item fails on a check (search_step_checks_kernel in the place of search_step_kernel)
  std::vector<int32_t> has, targets;
  std::vector<float> lo, hi;
  int kinds = 0;
  bool on_check = false;
};

struct cosim_engine {
  int n_envs = 0, device = 0;
  cosim_model_t model;
  cosim_obs_config_t obs_cfg;
  DevModel hm;  // host copies
  DevObs ho;
  Layout lay;
  Dev<DevModel> d_model;
  Dev<DevObs> d_obs;
  Dev<float> d_state, d_params, d_hull_vert, d_hfield, d_hfield_mip, d_dbg;
  Dev<int> d_hull_adr, d_hull_nbr;
  Dev<float4> d_hull_cell;          // support maps of the hulls (cosim_hullmap.h)
  Dev<float4> d_hull_cand;
  int hullmap_of_geom[64];          // what DevModel::g_hullmap holds while "support_map" is on
  Dev<unsigned> d_pairs;         // robot-robot candidate pairs (geom1 | geom2 << 16)
  Dev<float4> d_gext;            // per geom: MPR centre (body frame), raw sliding friction
  std::vector<float> h_params;
  bool params_dirty = true;
  uint64_t seed = 0;
  int64_t env_id0 = 0;
  float tol32 = 1e-6f;
  float ls_scale = 1.f;
  int max_newton = -1;   // explicit Newton iteration cap ("max_newton"); < 0: none, the model's iterations hold
  int max_ls = 24;       // line-search cap below the model's ls_iterations (50 in every reference model): measured enough, see DESIGN.md
  int nsub_override = 0;
  int pair_coop = 1;
  int timing_stride = 1;   // kernel timing: an event pair around every n-th launch (the events themselves cost ~4 % of a short run at 1)
  unsigned launch_seq = 0;
  int block_cull = 1;
  int coop_walk = 0;
  int pair_boxbox = 1;
  int prio[4] = {3, 0, 2, 4};   // wave priority by solver lag (see the kernel): usual iterations per substep, lag thresholds
  // timing
  bool timing = false;
  std::vector<hipEvent_t> ev;  // event pairs (start, stop) of timed launches not yet read back
  int ev_used = 0;
  double t_accum_ms = 0.0;
  int t_launches = 0;
  // which kernel runs when (cosim_plan.h): what this model / terrain has (cosim_create fills it, constant afterwards), what
  // cosim_set_param asked for, and make_plan() of the two: recomputed after every accepted switch, read by every launch site and cosim_query
  KernelSet<launch_fn> kernels;
  Switches sw;
  Plan<launch_fn> plan;
  int narrow_waves = 6;   // split pipeline: waves per env of the narrowphase kernel
  Dev<float> d_xcon, d_xstate;   // split pipeline: contact record and state between the two kernels of a substep
  Dev<int> d_xcnt;
  Dev<int> d_ovf;   // [n_envs] flags, set by the fleet kernel, cleared by the fix-up kernel
  // range launches: the fleet is cut into n_ranges contiguous env ranges, carried by n_streams <= n_ranges engine-owned streams
  // (cosim_ranges.h: as many as the process has hardware queues for).  cosim_step issues one launch sequence per stream over the
  // union of its group of consecutive ranges, so that a group's next control step fills the tail of the others' launches (a launch
  // ends with its slowest env)
  int n_ranges = 1;
  int n_streams = 1;            // P: streams (= groups = launch sequences per step) in use
  int range_streams_req = 0;    // "range_streams": 0 auto (range_stream_count of the process's GPU_MAX_HW_QUEUES), >= 1 asked for
  bool deferred_join = false;   // true: cosim_step does not make the caller's stream wait for the range streams (cosim_join does)
  bool join_pending = false;
  std::vector<hipStream_t> rstream;   // [n_streams]
  std::vector<hipEvent_t> rdone;      // one per stream: recorded at join time
  hipEvent_t ev_in = nullptr;      // recorded on the caller's stream, waited on by the range streams: the step's inputs are ready
  std::vector<int> rfirst, rcount;   // [n_ranges] envs of each range
  std::vector<int> rgroup;           // [n_ranges] the stream (group) that carries the range
  std::vector<int> gfirst, gcount;   // [n_streams] envs of each group: the union of its ranges
  // flow control of the range launches: the host stays at most `inflight` control steps ahead of each stream (a ring of events per
  // stream; cosim_step blocks on the oldest).  Deep queues are slow on this runtime: with the host hundreds of steps ahead the four
  // range chains step at 12.0 M env-steps/s, held to 2 ... 16 steps ahead at 13.6 ... 13.7 M (1: 13.35, 64: 13.3; MI355X, ROCm 7.2).
  // Short runs gain most from a shallow queue (20 timed steps: 2 -> 12.9 M, 4 -> 12.4, 8 -> 12.2, 16 -> 11.4, unbounded 10.9).
  int inflight = 2;   // 0: unbounded
  std::vector<hipEvent_t> ring;   // [n_streams][inflight]
  long ring_pos = 0;
  Spawn spawn;
  // snapshots (cosim_snapshot.hip).  A restore with parameters leaves h_params behind the device: the mirror is read back before the
  // next per-env cosim_set_param edits it (that call rewrites the whole table from the mirror)
  bool params_mirror_stale = false;
  SnapErr snap_err;               // there from the first restore with a source index on
  History hist;
  Ledger led;
  Ftrace ft;
  bool stepped = false;           // stepped (or restored / overwritten) since the last whole-fleet reset: such an episode gets flag 8
  // the scenario table and what is set for its rows (scenario_free says what goes with it)
  Scenario scn;
  ScnParams par;
  Faults obsflt, actflt;
  ActionRows act;
  bool act_in_obs = false;        // the observation has last_action elements
  Latency lat;
  Checks chk;
  Curves cur;
  Search srch;
  // fall rules (cosim_fall_set): kernel arguments of every step launch; fall_mask 0 = none (meta word 15 is not written)
  float fall_min_up = -1.f, fall_min_height = 0.f;
  int fall_grace = 0, fall_mask = 0;
  int model_term_mode = 0;              // the model's own _is_done list, restored when a body-list override is cleared
  unsigned model_term_bodymask = 0u;
};

// One launcher for every kernel: n envs (narrowphase: envs x waves per env) at ENVS_PER_BLOCK envs per one-wave block -- 1, 2 (two envs
// per wave) or 64 (the fix-up kernels: a wave scans the flags of 64 envs)
// kernel launches issued through the two launchers below by every engine of the process (cosim_query "launches"): what a test
// compares between two runs to hold that a table which is not set launches nothing
static std::atomic<unsigned> g_launches{0u};

template <auto KERNEL, int ENVS_PER_BLOCK = 1>
static void launch_k(cosim_engine*, const KArgs& a, int n, hipStream_t s) {
  g_launches.fetch_add(1u, std::memory_order_relaxed);
  hipLaunchKernelGGL(KERNEL, dim3((n + ENVS_PER_BLOCK - 1) / ENVS_PER_BLOCK), dim3(64), 0, s, a);
}
// ... and one for the small kernels beside them (ledger, traces, scenario family, snapshots): `count` envs (rows, cell blocks) at
// PER_BLOCK of them per block of THREADS threads
template <int PER_BLOCK, int THREADS, class K, class A>
static int launch_small(K kernel, const A& a, int count, hipStream_t s) {
  g_launches.fetch_add(1u, std::memory_order_relaxed);
  hipLaunchKernelGGL(kernel, dim3((count + PER_BLOCK - 1) / PER_BLOCK), dim3(THREADS), 0, s, a);
  HIP_TRY(hipGetLastError());
  return COSIM_OK;
}
// a KernelSet entry: KERNEL behind its launcher, with the capacities of the LDS layout L it is instantiated with
template <class L, auto KERNEL, int ENVS_PER_BLOCK = 1>
static Kernel<launch_fn> entry(bool hf) { return {launch_k<KERNEL, ENVS_PER_BLOCK>, (int)sizeof(L), L::MC, L::MCP, hf ? 64 : L::NGS}; }

// The kernels of one robot on one ground type at one capacity.  MCT: ground-contact slots of a contact-twist kernel, 0: dense contact rows
template <int NV, int NB, int RPL, bool HF, int GTM, bool SC, int MCT>
struct Fam {
  // the LDS layout of kernel mode KM: 0 the fused kernels, 1 the narrowphase kernel, 2 the solver kernel and its substep fix-up
  template <int KM> using LK = typename KTraits<NV, NB, RPL, HF, SC, 1, MCT, KM>::L;
  template <auto KERNEL, int ENVS_PER_BLOCK = 1, int KM = 0> static Kernel<launch_fn> of() { return entry<LK<KM>, KERNEL, ENVS_PER_BLOCK>(HF); }
  // KMODE -1: the general instantiation; MODE_STEP: the step-only one (no reset branch, no debug dump).  PROF: the diagnostic build
  template <int KMODE = -1, bool PROF = false> static Kernel<launch_fn> fleet() { return of<env_kernel<NV, NB, RPL, HF, GTM, SC, PROF, 1, MCT, KMODE>>(); }
  static Kernel<launch_fn> prof() { return fleet<-1, true>(); }
  static Kernel<launch_fn> fix() { return of<env_fixup_kernel<NV, NB, RPL, HF, GTM, SC, MCT>, 64>(); }
  template <int KMODE = -1> static Kernel<launch_fn> roll() { return of<env_rollout_kernel<NV, NB, RPL, HF, GTM, SC, MCT, KMODE>>(); }
  static Kernel<launch_fn> roll_fix() { return of<env_rollout_fix_kernel<NV, NB, RPL, HF, GTM, SC, MCT>, 64>(); }
  static Kernel<launch_fn> solver() { return of<env_step_kernel<NV, NB, RPL, HF, GTM, SC, MCT>, 1, 2>(); }
  template <int OCC, bool PROF = false> static Kernel<launch_fn> narrow() { return of<env_narrow_kernel<NV, NB, RPL, HF, GTM, SC, MCT, OCC, PROF>, 1, 1>(); }
  // The heightfield fix-ups behind a fleet kernel with MCT_FLEET slots: MCT = 50 (mjMAXCONPAIR, XC) x the robot's ground geoms, at the
  // register budget of the kernel they follow (waves per SIMD its LDS admits): hfix behind the fused kernel, stepfix behind the solver
  template <int MCT_FLEET, int KM> static constexpr int OCC = waves_per_simd(163840 / (int)sizeof(typename KTraits<NV, NB, RPL, true, SC, 1, MCT_FLEET, KM>::L));
  template <int MCT_FLEET> static Kernel<launch_fn> hfix() {
    static_assert(HF && sizeof(LK<0>) <= 163840, "heightfield fix-up: the env's LDS exceeds the 160 KiB of a CU");
    static_assert(MCT % XC == 0 && MCT <= XG * XC, "heightfield fix-up: whole geoms' worth of slots, within the split record");
    return of<env_hf_fixup_kernel<NV, NB, RPL, GTM, SC, MCT, OCC<MCT_FLEET, 0>>, 64>();
  }
  template <int MCT_FLEET> static Kernel<launch_fn> stepfix() {
    static_assert(HF && sizeof(LK<2>) <= 163840, "heightfield fix-up: the env's LDS exceeds the 160 KiB of a CU");
    return of<env_step_fixup_kernel<NV, NB, RPL, GTM, SC, MCT, OCC<MCT_FLEET, 2>>, 64, 2>();
  }
};

// What each robot has on the plane / a heightfield / a COARSE heightfield (cells of 10 cm or more: the reference's rocky_* and slope_*
// fields have 55 cm cells, a geom lies over a handful of prisms, and the slots that stairs with 1 cm cells need would only cost
// resident waves).  RPL = constraint rows per lane; the kernels are specialised on the geom types present.
constexpr int G_LIGHT = GT_SPHERE | GT_CYLINDER | GT_MESH, G_MESH = GT_MESH, G_HUM = GT_BOX | GT_CYLINDER | GT_MESH;

static KernelSet<launch_fn> light_v1_kernels(bool hf, bool coarse) {
  KernelSet<launch_fn> k;
  if (hf) {   // 13 ground geoms
    k.fleet = coarse ? Fam<18, 14, 1, true, G_LIGHT, false, 48>::fleet() : Fam<18, 14, 1, true, G_LIGHT, false, 128>::fleet();
    using X = Fam<18, 14, 1, true, G_LIGHT, false, 650>;
    k.hfix = X::hfix<128>(); k.dbg_hfix = X::fleet();
    return k;
  }
  using D = Fam<18, 14, 1, false, G_LIGHT, false, 0>;    // dense rows: 14 contacts
  k.fleet = D::fleet(); k.fleet_step = D::fleet<MODE_STEP>(); k.fleet_prof = D::prof();
  k.roll = D::roll(); k.roll_step = D::roll<MODE_STEP>();
  // (kept: pair_slots answers the dense layout's 1 although this robot has no pairs)
  using L2 = typename KTraits<18, 14, 2, false, false, 2, 0>::L;
  k.epw2 = entry<L2, env_kernel<18, 14, 2, false, G_LIGHT, false, false, 2>, 2>(false);
  k.epw2_prof = entry<L2, env_kernel<18, 14, 2, false, G_LIGHT, false, true, 2>, 2>(false);
  // the same robot with its ground contacts in twist space (32 slots instead of 14; cosim_set_param "contact_twist")
  using T = Fam<18, 14, 1, false, G_LIGHT, false, 32>;
  k.ct = T::fleet(); k.ct_prof = T::prof();
  k.ct.pair_slots = k.fleet.pair_slots;   // (kept: "contact_twist" 1 left the answer at the dense kernel's 1; this kernel has none)
  // ... and with 40 slots (four per ground geom at most: 7 hulls, 2 cylinders, 4 spheres -> 40 is the most the plane narrowphase
  // can emit) as the kernel that redoes the rare control step with more than 14 contacts: nothing is ever left out
  using X = Fam<18, 14, 1, false, G_LIGHT, false, 40>;
  k.fix = X::fix(); k.roll_fix = X::roll_fix();
  return k;
}

static KernelSet<launch_fn> p_v3_kernels(bool hf, bool) {
  KernelSet<launch_fn> k;
  if (hf) {   // 8 ground geoms
    // one row per lane: with the ground contacts in twist space the dense rows are the robot-robot contacts (8 slots = 32 rows), 8
    // frictionloss rows and at most 8 limit rows (8 hinges)
    // (no coarse-cell variant: at one row per lane the 64-slot kernel already fits the 12 waves per CU its registers allow)
    k.fleet = Fam<14, 10, 1, true, G_MESH, true, 64>::fleet();
    k.hfix = Fam<14, 10, 1, true, G_MESH, true, 400>::hfix<64>();
    return k;
  }
  // Plane: dense rows, like flamingo_light_v1.  With the friction-loss and limit rows in their dofs' lanes all 64 slots are contact
  // rows: 16 contacts, ground and robot-robot together (most seen in the bench: 16), and the dense solver iteration is cheaper
  // than the contact-twist one at these counts (kernel 0.325 ms against 0.400 per 1024 envs).  A control step with more is redone
  // by the contact-twist kernel (32 ground slots = four per geom, the narrowphase's maximum, + 8 pair slots) right behind it;
  // cosim_set_param "contact_twist" 1 makes that kernel the fleet kernel, as in round 2.
  using D = Fam<14, 10, 1, false, G_MESH, true, 0>;
  using T = Fam<14, 10, 1, false, G_MESH, true, 32>;
  k.fleet = D::fleet(); k.fleet_prof = D::prof(); k.roll = D::roll();
  k.fleet.pair_slots = 0;   // (kept: the dense kernel's pairs share the one contact list, the answer has been 0)
  k.ct = T::fleet(); k.ct_prof = T::prof(); k.fix = T::fix(); k.roll_fix = T::roll_fix();
  return k;
}

static KernelSet<launch_fn> w4_kernels(bool hf, bool coarse) {
  KernelSet<launch_fn> k;
  // plane: at most 4 contacts per geom (17 geoms); 80 slots keep the env at 19 KB of LDS = the 8 waves per CU its 256 registers allow
  if (!hf) k.fleet = Fam<22, 18, 2, false, G_MESH, true, 80>::fleet();
  else if (coarse) { k.fleet = Fam<22, 18, 2, true, G_MESH, true, 48>::fleet(); k.fleet_prof = Fam<22, 18, 2, true, G_MESH, true, 48>::prof(); }
  else k.fleet = Fam<22, 18, 2, true, G_MESH, true, 128>::fleet();
  if (hf) k.hfix = Fam<22, 18, 2, true, G_MESH, true, 850>::hfix<128>();   // 17 ground geoms
  return k;
}

static KernelSet<launch_fn> humanoid_kernels(bool hf, bool) {
  KernelSet<launch_fn> k;
  // plane: at most 4 contacts per geom (22 geoms); 96 slots = 6 waves per CU instead of 5
  if (!hf) { k.fleet = Fam<29, 26, 2, false, G_HUM, true, 96>::fleet(); return k; }
  using H = Fam<29, 26, 2, true, G_HUM, true, 256>;
  using X = Fam<29, 26, 2, true, G_HUM, true, 1100>;   // 22 ground geoms
  k.fleet = H::fleet(); k.fleet_prof = H::prof();
  // the prism walk in a kernel of its own, several waves per env (default; cosim_set_param "split" 0 goes back to the fused kernel)
  k.narrow[0] = H::narrow<2, true>(); k.narrow[1] = H::narrow<2>(); k.narrow[2] = H::narrow<3>(); k.narrow[3] = H::narrow<4>();
  k.solver = H::solver();
  k.hfix = X::hfix<256>(); k.stepfix = X::stepfix<256>();
  return k;
}

static int round_up(int x, int m) { return (x + m - 1) / m * m; }

static int build_dev_model(cosim_engine* e) {
  const cosim_model_t& m = e->model;
  DevModel& d = e->hm;
  memset(&d, 0, sizeof d);
  d.nq = m.nq; d.nv = m.nv; d.nu = m.nu; d.nbody = m.nbody; d.njnt = m.njnt; d.ngeom = m.ngeom; d.neq = m.neq; d.npair = m.npair;
  d.frame_skip = m.frame_skip; d.iterations = m.iterations; d.ls_iterations = m.ls_iterations;
  d.ground_type = m.ground_type; d.hfield_nrow = m.hfield_nrow; d.hfield_ncol = m.hfield_ncol; d.nhullvert = m.nhullvert;
  d.imu_body = m.imu_bodyid; d.term_mode = m.term_mode; d.nterm_body = m.nterm_body;
  d.timestep = (float)m.timestep; d.tolerance = (float)m.tolerance; d.ls_tolerance = (float)m.ls_tolerance; d.impratio = (float)m.impratio;
  for (int k = 0; k < 3; k++) { d.gravity[k] = (float)m.gravity[k]; d.ground_pos[k] = (float)m.ground_pos[k]; d.imu_pos[k] = (float)m.imu_pos[k]; }
  for (int k = 0; k < 4; k++) { d.hfield_size[k] = (float)m.hfield_size[k]; d.imu_quat[k] = (float)m.imu_quat[k]; }
  d.gyro_cutoff = (float)m.gyro_cutoff; d.vel_cutoff = (float)m.velocimeter_cutoff; d.heightmap_miss = (float)m.heightmap_miss;
  if (m.solver != CS_SOLVER_NEWTON) return fail(COSIM_EINVAL, "only solver=\"Newton\" (the reference models' setting) is implemented");
  if (m.ground_type != CS_GEOM_PLANE && (m.hfield_nrow < 2 || m.hfield_ncol < 2)) return fail(COSIM_EINVAL, "heightfield ground without elevation data");
  if (m.nbody > 32 || m.nv > 32 || m.ngeom > 32 || m.nq > 64) return fail(COSIM_EINVAL, "model exceeds the per-lane record capacity");
  if (m.neq > MAXEQ) return fail(COSIM_EINVAL, "too many equalities");
  if (m.ngeom > 24 || m.nu > m.nv - 6 || m.nq != m.nv + 1) return fail(COSIM_EINVAL, "model exceeds the per-env LDS tables (geoms <= 24, nu <= nv - 6, one free joint)");
  int maxdepth = 0;
  for (int j = 0; j < m.njnt; j++)
    if (m.jnt_type[j] == CS_JNT_HINGE && (m.jnt_pos[j][0] != 0.0 || m.jnt_pos[j][1] != 0.0 || m.jnt_pos[j][2] != 0.0)) d.any_jpos = 1;
  // dof ancestor masks
  unsigned anc[MAXD];
  for (int i = 0; i < m.nv; i++) anc[i] = (1u << i) | (m.dof_parentid[i] >= 0 ? anc[m.dof_parentid[i]] : 0u);
  for (int b = 0; b < m.nbody; b++) {
    LaneRec& r = d.rec[b];
    r.b_parent = m.body_parentid[b];
    int lev = 0;
    for (int p = b; p > 0; p = m.body_parentid[p]) lev++;
    r.b_level = lev;
    if (lev > maxdepth) maxdepth = lev;
    if (m.body_jntnum[b] > 1) return fail(COSIM_EINVAL, "more than one joint per body is not supported");
    r.b_jtype = m.body_jntnum[b] == 1 ? m.jnt_type[m.body_jntadr[b]] : -1;
    r.b_qadr = m.body_jntnum[b] == 1 ? m.jnt_qposadr[m.body_jntadr[b]] : 0;
    r.b_dadr = m.body_jntnum[b] == 1 ? m.jnt_dofadr[m.body_jntadr[b]] : 0;
    int a = b;
    while (a > 0 && m.body_dofnum[a] == 0) a = m.body_parentid[a];
    r.b_lastdof = a > 0 ? m.body_dofadr[a] + m.body_dofnum[a] - 1 : -1;
    r.b_dofmask = r.b_lastdof >= 0 ? anc[r.b_lastdof] : 0u;
    unsigned mask = 0;
    for (int c = 0; c < m.nbody; c++) {
      int q = c;
      while (q > 0 && q != b) q = m.body_parentid[q];
      if (q == b && (b > 0 || c == 0)) mask |= 1u << c;
    }
    r.b_subtree = mask;
    for (int k = 0; k < 3; k++) { r.b_pos[k] = (float)m.body_pos[b][k]; r.b_ipos[k] = (float)m.body_ipos[b][k]; r.b_inertia[k] = (float)m.body_inertia[b][k]; }
    for (int k = 0; k < 4; k++) { r.b_quat[k] = (float)m.body_quat[b][k]; r.b_iquat[k] = (float)m.body_iquat[b][k]; }
    if (m.body_jntnum[b] == 1) {
      int j = m.body_jntadr[b];
      for (int k = 0; k < 3; k++) { r.j_pos[k] = (float)m.jnt_pos[j][k]; r.j_axis[k] = (float)m.jnt_axis[j][k]; }
      r.j_q0 = m.jnt_type[j] == CS_JNT_HINGE ? (float)m.qpos0[m.jnt_qposadr[j]] : 0.f;
      r.j_limited = m.jnt_limited[j];
      r.j_margin = (float)m.jnt_margin[j];
      for (int k = 0; k < 2; k++) { r.j_range[k] = (float)m.jnt_range[j][k]; r.j_solref[k] = (float)m.jnt_solref[j][k]; }
      for (int k = 0; k < 5; k++) r.j_solimp[k] = (float)m.jnt_solimp[j][k];
    }
  }
  d.maxdepth = maxdepth;
  d.imu_dofmask = d.rec[m.imu_bodyid].b_dofmask;
  int nfric = 0;
  for (int i = 0; i < m.nv; i++) {
    LaneRec& r = d.rec[i];
    r.d_body = m.dof_bodyid[i]; r.d_parent = m.dof_parentid[i]; r.d_ancmask = anc[i];
    r.d_armature = (float)m.dof_armature[i]; r.d_damping = (float)m.dof_damping[i];
    for (int k = 0; k < 2; k++) r.d_solref[k] = (float)m.dof_solref[i][k];
    for (int k = 0; k < 5; k++) r.d_solimp[k] = (float)m.dof_solimp[i][k];
    int j = m.dof_jntid[i];
    r.d_frclimited = m.jnt_type[j] == CS_JNT_HINGE ? m.jnt_actfrclimited[j] : 0;
    r.d_frcrange[0] = (float)m.jnt_actfrcrange[j][0]; r.d_frcrange[1] = (float)m.jnt_actfrcrange[j][1];
    r.d_act = -1;
    if (m.dof_frictionloss[i] > 0) d.rec[nfric++].d_fric = i;
  }
  d.nfric = nfric;
  for (int g = 0; g < m.ngeom; g++) {
    LaneRec& r = d.rec[g];
    r.g_type = m.geom_type[g]; r.g_body = m.geom_bodyid[g]; r.g_ground = m.geom_ground[g];
    r.g_hulladr = m.geom_hulladr[g]; r.g_hullnum = m.geom_hullnum[g];
    int condim = m.geom_condim[g] > m.ground_condim ? m.geom_condim[g] : m.ground_condim;
    if (m.geom_ground[g] && condim != 3) return fail(COSIM_EINVAL, "only condim 3 contacts are implemented");
    for (int k = 0; k < 3; k++) { r.g_pos[k] = (float)m.geom_pos[g][k]; r.g_size[k] = (float)m.geom_size[g][k]; r.g_rcenter[k] = (float)m.geom_rcenter[g][k]; }
    for (int k = 0; k < 4; k++) r.g_quat[k] = (float)m.geom_quat[g][k];
    r.g_rbound = (float)m.geom_rbound[g];
    for (int k = 0; k < 3; k++) r.g_half[k] = (float)m.geom_aabb[g][3 + k];
    for (int k = 0; k < 3; k++) if (fabs(m.geom_aabb[g][k] - m.geom_rcenter[g][k]) > 1e-12) return fail(COSIM_EINVAL, "geom_aabb centre must equal geom_rcenter");
    // mj_contactParam with equal priorities: solmix-weighted solref/solimp, margins by max
    double s1 = m.ground_solmix, s2 = m.geom_solmix[g], mix;
    if (s1 >= 1e-15 && s2 >= 1e-15) mix = s1 / (s1 + s2);
    else if (s1 < 1e-15 && s2 < 1e-15) mix = 0.5;
    else mix = s1 < 1e-15 ? 0.0 : 1.0;
    for (int k = 0; k < 2; k++)
      r.g_solref[k] = (m.ground_solref[0] > 0 && m.geom_solref[g][0] > 0)
                          ? (float)(mix * m.ground_solref[k] + (1 - mix) * m.geom_solref[g][k])
                          : (float)fmin(m.ground_solref[k], m.geom_solref[g][k]);
    for (int k = 0; k < 5; k++) r.g_solimp[k] = (float)(mix * m.ground_solimp[k] + (1 - mix) * m.geom_solimp[g][k]);
    double margin = fmax(m.ground_margin, m.geom_margin[g]), gap = fmax(m.ground_gap, m.geom_gap[g]);
    r.g_margin = (float)margin;
    r.g_incmargin = (float)(margin - gap);
  }
  for (int q = 0; q < m.neq; q++) {
    LaneRec& r = d.rec[q];
    r.e_body1 = m.eq_body1[q]; r.e_body2 = m.eq_body2[q];
    for (int k = 0; k < 3; k++) { r.e_anchor1[k] = (float)m.eq_anchor1[q][k]; r.e_anchor2[k] = (float)m.eq_anchor2[q][k]; }
    for (int k = 0; k < 2; k++) r.e_solref[k] = (float)m.eq_solref[q][k];
    for (int k = 0; k < 5; k++) r.e_solimp[k] = (float)m.eq_solimp[q][k];
  }
  // solref -> (K, B) of mj_makeImpedance once on the host (they depend on solref, solimp[1] and the timestep only): the
  // *_solref slots of the device records carry K and B from here on
  {
    auto kb = [&](float* solref, const float* solimp) {
      const double dmax = fmin(0.9999, fmax(0.0001, (double)solimp[1]));
      double K, B;
      if (solref[0] > 0.f) {
        const double tc = fmax((double)solref[0], 2.0 * m.timestep), dr = solref[1];   // refsafe
        K = 1.0 / fmax(1e-15, dmax * dmax * tc * tc * dr * dr);
        B = 2.0 / fmax(1e-15, dmax * tc);
      } else { K = -(double)solref[0] / fmax(1e-15, dmax * dmax); B = -(double)solref[1] / fmax(1e-15, dmax); }
      solref[0] = (float)K; solref[1] = (float)B;
    };
    for (int b = 0; b < m.nbody; b++) if (m.body_jntnum[b] == 1) kb(d.rec[b].j_solref, d.rec[b].j_solimp);
    for (int i = 0; i < m.nv; i++) kb(d.rec[i].d_solref, d.rec[i].d_solimp);
    for (int g = 0; g < m.ngeom; g++) kb(d.rec[g].g_solref, d.rec[g].g_solimp);
    for (int q = 0; q < m.neq; q++) kb(d.rec[q].e_solref, d.rec[q].e_solimp);
  }
  for (int u = 0; u < m.nu; u++) {
    LaneRec& r = d.rec[u];
    r.a_dof = m.act_dofid[u]; r.a_ctrllimited = m.act_ctrllimited[u]; r.a_gear = (float)m.act_gear[u];
    r.a_ctrlrange[0] = (float)m.act_ctrlrange[u][0]; r.a_ctrlrange[1] = (float)m.act_ctrlrange[u][1];
    if (d.rec[m.act_dofid[u]].d_act >= 0) return fail(COSIM_EINVAL, "two motors on one dof are not supported");
    d.rec[m.act_dofid[u]].d_act = u;
    r.a_velmode = m.ctl_velmode[u]; r.a_qadr = m.ctl_qadr[u]; r.a_dadr = m.ctl_dadr[u];
    r.a_scale = (float)m.ctl_scale[u]; r.a_cgear = (float)m.ctl_gear[u]; r.a_gamma = (float)m.ctl_gamma[u];
    r.a_maxtq = (float)m.ctl_maxtq[u];
  }
  d.nobs_pos = m.nobs_pos; d.nobs_vel = m.nobs_vel; d.ninfo_state = m.ninfo_state; d.init_noise_nq = m.init_noise_nq;
  for (int i = 0; i < CS_MAXOBSJ; i++) { d.rec[i].o_qadr = m.obs_qadr[i]; d.rec[i].o_dadr = m.obs_dadr[i]; d.rec[i].o_qgear = (float)m.obs_qgear[i]; d.rec[i].o_dgear = (float)m.obs_dgear[i]; }
  for (int i = 0; i < CS_MAXINFOSTATE; i++) { d.rec[i].i_kind = m.info_kind[i]; d.rec[i].i_adr = m.info_adr[i]; d.rec[i].i_gear = (float)m.info_gear[i]; }
  for (int i = 0; i < CS_MAXQ; i++) { d.rec[i].n_qadr = m.init_noise_qadr[i]; d.rec[i].init_qpos = (float)m.init_qpos[i]; }
  for (int i = 0; i < CS_MAXBODY; i++) d.rec[i].t_body = m.term_body[i];
  for (int i = 0; i < m.nterm_body; i++) d.term_bodymask |= 1u << m.term_body[i];
  d.ntri = m.nv * (m.nv + 1) / 2;
  for (int r = 0, e2 = 0; r < m.nv; r++)
    for (int c = 0; c <= r; c++, e2++) { d.tri_row[e2] = (unsigned char)r; d.tri_col[e2] = (unsigned char)c; }
  return COSIM_OK;
}

static int build_dev_obs(cosim_engine* e) {
  const cosim_obs_config_t& c = e->obs_cfg;
  DevObs& o = e->ho;
  memset(&o, 0, sizeof o);
  if (c.stack_size < 1 || c.command_dim < 0 || c.command_dim > CS_MAXCMD) return fail(COSIM_EINVAL, "bad stack_size / command_dim");
  if (c.n_stacked < 0 || c.n_stacked > CS_MAXFIELD || c.n_non_stacked < 0 || c.n_non_stacked > CS_MAXFIELD) return fail(COSIM_EINVAL, "bad field lists");
  o.stack_size = c.stack_size; o.command_dim = c.command_dim; o.position_command = c.position_command;
  o.max_sim_step = c.max_sim_step; o.auto_reset = c.auto_reset; o.noise_enabled = c.noise_enabled;
  o.action_delay_prob = c.action_delay_prob; o.init_noise = c.init_noise;
  for (int i = 0; i < CS_MAXCMD; i++) o.command_scales[i] = c.command_scales[i];
  o.hm_res_x = c.hm_res_x; o.hm_res_y = c.hm_res_y; o.hm_size_x = c.hm_size_x; o.hm_size_y = c.hm_size_y;
  for (int f = 0; f < 8; f++) {
    o.noise_mean[f] = c.noise_mean[f]; o.noise_std[f] = c.noise_std[f]; o.noise_lower[f] = c.noise_lower[f]; o.noise_upper[f] = c.noise_upper[f];
    const double sd = c.noise_std[f] > 0 ? c.noise_std[f] : 1.0;
    o.noise_ca[f] = (float)(0.5 * erfc(-((double)c.noise_lower[f] - c.noise_mean[f]) / sd / sqrt(2.0)));
    o.noise_cb[f] = (float)(0.5 * erfc(-((double)c.noise_upper[f] - c.noise_mean[f]) / sd / sqrt(2.0)));
  }
  int el = 0;
  for (int pass = 0; pass < 2; pass++) {
    const int* list = pass ? c.non_stacked_field : c.stacked_field;
    int n = pass ? c.n_non_stacked : c.n_stacked;
    for (int i = 0; i < n; i++) {
      int f = list[i];
      if (f < 0 || f > 7) return fail(COSIM_EINVAL, "unknown observation field id");
      if (f == CS_OBS_HEIGHT_MAP && (e->model.ground_type != CS_GEOM_HFIELD || c.hm_res_x * c.hm_res_y != c.field_dim[f] || c.field_dim[f] < 1))
        return fail(COSIM_EINVAL, "height_map observation needs a heightfield terrain (mj_rayHfield on a plane is an error in the reference too) and res_x * res_y elements");
      int dim = c.field_dim[f];
      if (c.field_interval[f] < 1 && f != CS_OBS_COMMAND) return fail(COSIM_EINVAL, "observation interval must be >= 1");
      for (int k = 0; k < dim; k++) {
        if (el >= MAXFRAME) return fail(COSIM_EINVAL, "observation frame too large");
        o.el_field[el] = (unsigned char)f; o.el_index[el] = (unsigned short)k;
        o.el_interval[el] = (unsigned char)(f == CS_OBS_COMMAND ? 1 : (c.field_interval[f] > 255 ? 255 : c.field_interval[f]));
        o.el_scale[el] = c.field_scale[f];
        el++;
      }
    }
    if (pass == 0) o.stacked_dim = el;
  }
  o.frame_dim = el;
  o.non_stacked_dim = el - o.stacked_dim;
  o.state_dim = o.stack_size * o.stacked_dim + o.non_stacked_dim;
  o.info_dim = 4 + 2 * e->model.nu + e->model.ninfo_state;
  return COSIM_OK;
}

static void build_layout(cosim_engine* e) {
  const cosim_model_t& m = e->model;
  Layout& L = e->lay;
  int o = 0;
  L.s_qpos = o; o += m.nq;
  L.s_qvel = o; o += m.nv;
  L.s_warm = o; o += m.nv;
  L.s_delay = o; o += m.nu;
  L.s_lastact = o; o += m.nu;
  L.s_meta = o; o += Layout::NMETA;
  L.s_cache = o; o += e->ho.frame_dim;
  L.s_stack = o; o += e->ho.stack_size * e->ho.stacked_dim;
  L.s_stride = round_up(o, 32);
  int p = 0;
  L.p_mass = p; p += m.nbody;
  L.p_binvw = p; p += m.nbody;
  L.p_dinvw = p; p += m.nv;
  L.p_floss = p; p += m.nv;
  L.p_gmu = p; p += m.ngeom;
  L.p_kp = p; p += m.nu;
  L.p_kd = p; p += m.nu;
  L.p_mean = p; p += 1;
  L.p_stride = round_up(p, 32);
}

static void default_params(cosim_engine* e) {
  const cosim_model_t& m = e->model;
  const Layout& L = e->lay;
  e->h_params.assign((size_t)e->n_envs * L.p_stride, 0.f);
  for (int n = 0; n < e->n_envs; n++) {
    float* p = e->h_params.data() + (size_t)n * L.p_stride;
    for (int b = 0; b < m.nbody; b++) { p[L.p_mass + b] = (float)m.body_mass[b]; p[L.p_binvw + b] = (float)m.body_invweight0[b][0]; }
    for (int i = 0; i < m.nv; i++) { p[L.p_dinvw + i] = (float)m.dof_invweight0[i]; p[L.p_floss + i] = (float)m.dof_frictionloss[i]; }
    for (int g = 0; g < m.ngeom; g++) p[L.p_gmu + g] = (float)fmax(1e-5, fmax(m.ground_friction[0], m.geom_friction[g][0]));
    for (int u = 0; u < m.nu; u++) { p[L.p_kp + u] = (float)m.ctl_kp[u]; p[L.p_kd + u] = (float)m.ctl_kd[u]; }
    p[L.p_mean] = (float)m.meaninertia;
  }
  e->params_dirty = true;
}

static int refresh_param_mirror(cosim_engine* e);

static int upload_params(cosim_engine* e) {
  if (!e->params_dirty) return COSIM_OK;
  HIP_TRY(hipMemcpy(e->d_params.get(), e->h_params.data(), e->h_params.size() * sizeof(float), hipMemcpyHostToDevice));
  e->params_dirty = false;
  return COSIM_OK;
}

// GPU_MAX_HW_QUEUES as this process was started with, read once (the runtime reads it at its first call too)
static int process_hw_queues() {
  static const int q = hw_queues_from_env(getenv("GPU_MAX_HW_QUEUES"));
  return q;
}

// n contiguous ranges of n_envs / n envs (the first n_envs % n one longer; even sizes for the two-envs-per-wave kernel) in
// P = range_streams_in_use(...) groups of consecutive ranges, each group with a non-blocking stream of its own and a "done" event
static int set_ranges(cosim_engine* e, int n) {
  if (n < 1 || n > 16 || n > e->n_envs) return fail(COSIM_EINVAL, "cosim_set_param: ranges must be 1..16 and at most n_envs");
  HIP_TRY(hipSetDevice(e->device));
  for (hipStream_t x : e->rstream) { HIP_TRY(hipStreamSynchronize(x)); HIP_TRY(hipStreamDestroy(x)); }
  for (hipEvent_t x : e->rdone) HIP_TRY(hipEventDestroy(x));
  e->rstream.clear(); e->rdone.clear(); e->rfirst.clear(); e->rcount.clear(); e->rgroup.clear(); e->gfirst.clear(); e->gcount.clear();
  e->join_pending = false;
  e->n_ranges = n;
  const int P = e->n_streams = range_streams_in_use(e->range_streams_req, n, process_hw_queues());
  for (hipEvent_t x : e->ring) HIP_TRY(hipEventDestroy(x));
  e->ring.clear();
  e->ring_pos = 0;
  for (int i = 0; i < P * e->inflight; i++) { hipEvent_t ev; HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming)); e->ring.push_back(ev); }
  if (n == 1) return COSIM_OK;
  if (!e->ev_in) HIP_TRY(hipEventCreateWithFlags(&e->ev_in, hipEventDisableTiming));
  const int unit = e->sw.epw == 2 ? 2 : 1;
  for (int i = 0; i < n; i++) {
    int first, cnt;
    range_bounds(e->n_envs, n, unit, i, &first, &cnt);
    e->rfirst.push_back(first); e->rcount.push_back(cnt); e->rgroup.push_back(group_of(i, n, P));
  }
  for (int g = 0; g < P; g++) {
    const int r0 = group_first(g, n, P), r1 = group_first(g + 1, n, P);
    hipStream_t st; hipEvent_t ev;
    HIP_TRY(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    e->rstream.push_back(st);
    HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    e->rdone.push_back(ev);
    e->gfirst.push_back(e->rfirst[r0]); e->gcount.push_back(e->rfirst[r1 - 1] + e->rcount[r1 - 1] - e->rfirst[r0]);
  }
  return COSIM_OK;
}

// `stream` waits for everything the range streams have been given so far: the "done" events are recorded here, at join time (an
// event marks everything enqueued before it), not after every range launch -- a deferred-join caller pays no marker packets per step
static int join_ranges(cosim_engine* e, hipStream_t stream) {
  if (!e->join_pending) return COSIM_OK;
  for (int i = 0; i < (int)e->rstream.size(); i++) {
    HIP_TRY(hipEventRecord(e->rdone[i], e->rstream[i]));
    HIP_TRY(hipStreamWaitEvent(stream, e->rdone[i], 0));
  }
  e->join_pending = false;
  return COSIM_OK;
}

// ---- snapshots and the history ring (cosim_snapshot.hip)
static const char* const HIST_CAPTURE_MSG =
    "cosim_step: a history is set (cosim_history_set) and the stream is being captured into a graph: a replayed graph would repeat "
    "whatever step parity was captured; switch the history off or step eagerly";

static SnapArgs snap_args(cosim_engine* e) {
  SnapArgs a;
  memset(&a, 0, sizeof a);
  a.state = e->d_state.get(); a.params = e->d_params.get(); a.s_stride = e->lay.s_stride; a.p_stride = e->lay.p_stride;
  a.n_envs = e->n_envs; a.n_rows = e->n_envs; a.env_first = 0; a.env_count = e->n_envs;
  return a;
}

// h_params <- d_params after a restore with parameters (cold: blocks until the device is idle)
static int refresh_param_mirror(cosim_engine* e) {
  if (!e->params_mirror_stale) return COSIM_OK;
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(e->h_params.data(), e->d_params.get(), e->h_params.size() * sizeof(float), hipMemcpyDeviceToHost));
  e->params_mirror_stale = false;
  return COSIM_OK;
}

// this cosim_step call is the `every`-th since the last capture
static bool history_due(const cosim_engine* e) { return e->hist.slots > 0 && (e->hist.calls + 1) % e->hist.every == 0; }

static int history_pack(cosim_engine* e, int first, int count, hipStream_t s) {
  SnapArgs a = snap_args(e);
  a.rows = e->hist.ring.get() + (size_t)(e->hist.captures % e->hist.slots) * e->n_envs * (size_t)(a.s_stride + a.p_stride);
  a.env_first = first; a.env_count = count;
  return launch_small<1, 64>(snapshot_pack_kernel, a, count, s);
}

static void history_count(cosim_engine* e) {   // after a cosim_step call was issued in full
  if (e->hist.slots <= 0) return;
  const bool due = history_due(e);
  e->hist.calls++;
  if (due) { e->hist.call_of[e->hist.captures % e->hist.slots] = e->hist.calls; e->hist.captures++; }
}

// ---- episode ledger (cosim_ledger.hip)
static const char* const LEDGER_INFO_MSG =
    ": a ledger is set (cosim_ledger_set) and info_out_dev is NULL: the ledger is built from the step's info rows; pass an info "
    "buffer or switch the ledger off";

static LedgerArgs ledger_args(cosim_engine* e) {
  LedgerArgs a;
  memset(&a, 0, sizeof a);
  a.state = e->d_state.get(); a.sum = e->led.sum.get(); a.peak = e->led.peak.get(); a.acc = e->led.acc.get(); a.rec = e->led.rec.get();
  a.n_envs = e->n_envs; a.first = 0; a.count = e->n_envs; a.rows = 1;
  a.info_dim = e->ho.info_dim; a.nu = e->model.nu; a.ncmd = e->ho.command_dim < 3 ? e->ho.command_dim : 3; a.cmd_stride = e->ho.command_dim;
  a.s_stride = e->lay.s_stride; a.s_meta = e->lay.s_meta; a.slots = e->led.slots; a.spawn_rows = e->spawn.rows;
  a.fall = e->fall_mask != 0;
  if (e->scn.tab.n_scn > 0) { a.scn_row = e->scn.row_out; a.scn_rows = e->scn.tab.n_scn; a.scn_mode = e->scn.tab.mode; a.scn_off = e->scn.tab.gid_off; }
  return a;
}

// rows [0, K) of the step outputs of envs [first, first + count), behind the launches that wrote them on the same stream
static int ledger_step(cosim_engine* e, int first, int count, int K, const float* info, const uint8_t* term, const uint8_t* trunc,
                       const float* cmd, hipStream_t s) {
  LedgerArgs a = ledger_args(e);
  a.info = info; a.term = term; a.trunc = trunc; a.cmd = a.ncmd > 0 ? cmd : nullptr;
  a.first = first; a.count = count; a.rows = K;
  return launch_small<64, 64>(a.scn_row != nullptr ? ledger_step_scn_kernel : ledger_step_kernel, a, count, s);
}

// the masked envs (null: all; with a restore's source index: those it did not refuse) begin an episode, what they had open is dropped
static int ledger_begin(cosim_engine* e, const uint8_t* mask, const int* src, int n_rows, int flag, hipStream_t s) {
  if (e->led.slots <= 0) return COSIM_OK;
  LedgerArgs a = ledger_args(e);
  a.mask = mask; a.src = src; a.n_rows = n_rows; a.flag = flag;
  return launch_small<64, 64>(ledger_begin_kernel, a, e->n_envs, s);
}

// ---- scenario table (cosim_scenario.hip)
// the command buffer the step kernels, the ledger and the reporter read: the scenario kernel's output while a table is set
static const float* scenario_cmd(const cosim_engine* e, const float* commands_dev) {
  return e->scn.tab.n_scn > 0 && e->ho.command_dim > 0 ? e->scn.cmd_out : commands_dev;
}

// ahead of the step (reset: of the reset, for the envs under its mask) of envs [first, first + count) on the same stream
static int scenario_launch(cosim_engine* e, int first, int count, const float* commands_dev, const uint8_t* mask, int reset, hipStream_t s) {
  ScnArgs a;
  memset(&a, 0, sizeof a);
  a.tab = e->scn.tab; a.state = e->d_state.get(); a.cmd_in = commands_dev; a.cmd_out = e->scn.cmd_out; a.row_out = e->scn.row_out; a.mask = mask;
  a.n_envs = e->n_envs; a.first = first; a.count = count;
  a.s_stride = e->lay.s_stride; a.s_meta = e->lay.s_meta; a.s_qpos = e->lay.s_qpos; a.s_qvel = e->lay.s_qvel; a.reset = reset;
  if (e->srch.tab.n_items > 0) {   // a search is armed: the same schedule with every env's level multiplied in
    ScnSearchArgs sa;
    memset(&sa, 0, sizeof sa);
    sa.scn = a; sa.srch = e->srch.tab; sa.rec = e->srch.rec.get();
    return launch_small<64, 64>(scenario_search_step_kernel, sa, count, s);
  }
  return launch_small<64, 64>(scenario_step_kernel, a, count, s);
}

// directly behind scenario_launch, same envs, same stream: the effective parameter records of this step (reset: of the masked envs at t = 0)
static int scnparams_launch(cosim_engine* e, int first, int count, const uint8_t* mask, int reset, hipStream_t s) {
  ScnParArgs a;
  memset(&a, 0, sizeof a);
  a.tab = e->scn.tab; a.par = e->par.tab; a.state = e->d_state.get(); a.base = e->d_params.get(); a.eff = e->par.eff.get(); a.mask = mask;
  a.n_envs = e->n_envs; a.first = first; a.count = count;
  a.s_stride = e->lay.s_stride; a.s_meta = e->lay.s_meta; a.p_stride = e->lay.p_stride; a.reset = reset;
  if (e->srch.tab.n_items > 0 && (e->srch.kinds & SRCH_PARAMS)) {   // a search whose targets name the windows is armed: marked items are scaled by the env's level
    const ScnParSearchArgs sa = {a, e->srch.rec.get(), SRCH_NCNT};
    return launch_small<SCNPAR_WAVES, 64 * SCNPAR_WAVES>(scnparams_search_step_kernel, sa, count, s);
  }
  return launch_small<SCNPAR_WAVES, 64 * SCNPAR_WAVES>(scnparams_step_kernel, a, count, s);
}

// a search whose targets name the observation faults is armed: obsfault_search_step_kernel in the place of obsfault_step_kernel, and at
// the step site behind the search's kernel
static bool obsfault_searched(const cosim_engine* e) { return e->srch.tab.n_items > 0 && (e->srch.kinds & SRCH_OBS_FAULTS) != 0; }

// behind the last launch of a step (reset: of the reset, for the envs under its mask) that writes the state record or state_out of
// envs [first, first + count), same stream: what the policy sees of those envs
static int obsfault_launch(cosim_engine* e, int first, int count, float* state_out, const uint8_t* mask, hipStream_t s) {
  ObsFaultArgs a;
  memset(&a, 0, sizeof a);
  a.tab = e->scn.tab; a.flt = e->obsflt.tab; a.state = e->d_state.get(); a.state_out = state_out; a.mask = mask;
  a.n_envs = e->n_envs; a.first = first; a.count = count;
  a.s_stride = e->lay.s_stride; a.s_meta = e->lay.s_meta; a.s_stack = e->lay.s_stack;
  a.sd = e->ho.stacked_dim; a.S = e->ho.stack_size; a.frame_dim = e->ho.frame_dim; a.state_dim = e->ho.state_dim;
  a.seed_lo = (unsigned)e->seed; a.seed_hi = (unsigned)(e->seed >> 32); a.env_id0 = e->env_id0;
  if (obsfault_searched(e)) {   // marked items are scaled by the level of the episode the observation belongs to
    const ObsFaultSearchArgs sa = {a, e->srch.rec.get(), SRCH_NCNT};
    return launch_small<FLT_WAVES, 64 * FLT_WAVES>(obsfault_search_step_kernel, sa, count, s);
  }
  return launch_small<FLT_WAVES, 64 * FLT_WAVES>(obsfault_step_kernel, a, count, s);
}

// the two action rows go when neither the action faults nor the latency's action items need them: called behind every change of either
static void action_rows_release(cosim_engine* e) {
  if (e->actflt.tab.n_items == 0 && e->lat.tab.n_act == 0) e->act = {};
}

// ahead of the first launch of a control step of envs [first, first + count), same stream, behind the scenario and parameter-window
// kernels: the effective and the raw action rows of those envs
// (`raw`: where the kernel's copy of `actions` goes: d_actions_raw, or a spare while the latency kernel has written that buffer)
static int actfault_launch(cosim_engine* e, int first, int count, const float* actions, float* raw, hipStream_t s) {
  ActFaultArgs a;
  memset(&a, 0, sizeof a);
  a.tab = e->scn.tab; a.flt = e->actflt.tab; a.state = e->d_state.get(); a.actions = actions; a.eff = e->act.eff.get(); a.raw = raw;
  a.n_envs = e->n_envs; a.first = first; a.count = count;
  a.s_stride = e->lay.s_stride; a.s_meta = e->lay.s_meta; a.s_lastact = e->lay.s_lastact; a.nu = e->model.nu;
  a.seed_lo = (unsigned)e->seed; a.seed_hi = (unsigned)(e->seed >> 32); a.env_id0 = e->env_id0;
  // a search whose targets name the action faults is armed: the same walk with every env's level multiplied into its marked items
  if (e->srch.tab.n_items > 0 && (e->srch.kinds & SRCH_ACT_FAULTS)) {
    const ActFaultSearchArgs sa = {a, e->srch.rec.get(), SRCH_NCNT};
    return launch_small<FLT_WAVES, 64 * FLT_WAVES>(actfault_search_step_kernel, sa, count, s);
  }
  return launch_small<FLT_WAVES, 64 * FLT_WAVES>(actfault_step_kernel, a, count, s);
}

// behind the last launch of the step that writes the state record or state_out of those envs, same stream: last_action as the policy
// put it out
static int actfault_obs_launch(cosim_engine* e, int first, int count, float* state_out, hipStream_t s) {
  ActObsArgs a;
  memset(&a, 0, sizeof a);
  a.ob = e->d_obs.get(); a.state = e->d_state.get(); a.state_out = state_out; a.raw = e->act.raw.get();
  a.n_envs = e->n_envs; a.first = first; a.count = count;
  a.s_stride = e->lay.s_stride; a.s_meta = e->lay.s_meta; a.s_cache = e->lay.s_cache; a.s_stack = e->lay.s_stack; a.nu = e->model.nu;
  return launch_small<FLT_WAVES, 64 * FLT_WAVES>(actfault_obs_kernel, a, count, s);
}

// ---- latency lines of the scenario table (cosim_latency.hip)
// ahead of actfault_launch and of the first launch of a control step of envs [first, first + count), same stream: the delivered and
// the raw action rows of those envs.  With action faults set too the delivered rows go to d_lat_eff, which the fault kernel then reads.
static int latency_act_launch(cosim_engine* e, int first, int count, const float* actions, hipStream_t s) {
  LatActArgs a;
  memset(&a, 0, sizeof a);
  a.tab = e->scn.tab; a.lat = e->lat.tab; a.state = e->d_state.get(); a.actions = actions;
  a.eff = e->actflt.tab.n_items > 0 ? e->lat.eff.get() : e->act.eff.get(); a.raw = e->act.raw.get();
  a.line = e->lat.act_line.get(); a.from = e->lat.from.get();
  a.n_envs = e->n_envs; a.first = first; a.count = count;
  a.s_stride = e->lay.s_stride; a.s_meta = e->lay.s_meta; a.nu = e->model.nu;
  a.seed_lo = (unsigned)e->seed; a.seed_hi = (unsigned)(e->seed >> 32); a.env_id0 = e->env_id0;
  return launch_small<FLT_WAVES, 64 * FLT_WAVES>(latency_act_kernel, a, count, s);
}

// behind the last launch of a step (reset: of the reset, for the envs under its mask) that writes the state record or state_out of
// those envs and behind actfault_obs_kernel, ahead of obsfault_launch, same stream
static int latency_obs_launch(cosim_engine* e, int first, int count, float* state_out, const uint8_t* mask, hipStream_t s) {
  LatObsArgs a;
  memset(&a, 0, sizeof a);
  a.tab = e->scn.tab; a.lat = e->lat.tab; a.state = e->d_state.get(); a.state_out = state_out; a.mask = mask;
  a.line = e->lat.obs_line.get(); a.from = e->lat.from.get() + e->n_envs;
  a.n_envs = e->n_envs; a.first = first; a.count = count;
  a.s_stride = e->lay.s_stride; a.s_meta = e->lay.s_meta; a.s_stack = e->lay.s_stack;
  a.sd = e->ho.stacked_dim; a.S = e->ho.stack_size; a.frame_dim = e->ho.frame_dim; a.state_dim = e->ho.state_dim;
  a.seed_lo = (unsigned)e->seed; a.seed_hi = (unsigned)(e->seed >> 32); a.env_id0 = e->env_id0;
  return launch_small<FLT_WAVES, 64 * FLT_WAVES>(latency_obs_kernel, a, count, s);
}

// behind a set / restore on the same stream: the lines of the masked envs (null: all; with a restore's source index: those it did
// not refuse) are invalid; each restarts at the clock its kernel finds next.  (A reset needs none: both kernels restart a line at clock 0.)
static int latency_cut(cosim_engine* e, const uint8_t* mask, const int* src, int n_rows, hipStream_t s) {
  if (e->lat.tab.n_act + e->lat.tab.n_obs == 0) return COSIM_OK;
  const LatCutArgs a = {e->lat.from.get(), e->lat.from.get() + e->n_envs, mask, src, n_rows, e->n_envs};
  return launch_small<64, 64>(latency_cut_kernel, a, e->n_envs, s);
}

// ---- checks of the scenario table (cosim_checks.hip)
static const char* const CHECKS_INFO_MSG =
    ": scenario checks are set (cosim_scenario_checks_set) and info_out_dev is NULL: the checks sample the step's info row; pass an "
    "info buffer or clear the checks";

static ChkArgs checks_args(cosim_engine* e) {
  ChkArgs a;
  memset(&a, 0, sizeof a);
  a.tab = e->chk.tab; a.state = e->d_state.get(); a.scn_row = e->scn.row_out;
  a.ext = e->chk.ext.get(); a.aux = e->chk.aux.get(); a.n = e->chk.n.get(); a.sum = e->chk.sum.get(); a.cnt = e->chk.cnt.get(); a.rec = e->chk.rec.get();
  a.n_envs = e->n_envs; a.first = 0; a.count = e->n_envs;
  a.info_dim = e->ho.info_dim; a.nu = e->model.nu; a.cmd_stride = e->ho.command_dim;
  a.s_stride = e->lay.s_stride; a.s_qpos = e->lay.s_qpos; a.s_qvel = e->lay.s_qvel; a.s_meta = e->lay.s_meta; a.slots = e->chk.slots;
  a.scn_mode = e->scn.tab.mode; a.scn_off = e->scn.tab.gid_off;
  return a;
}

// this step's samples of envs [first, first + count), behind the launches that wrote the step's outputs on the same stream
static int checks_step(cosim_engine* e, int first, int count, const float* cmd, const float* info, const uint8_t* term, const uint8_t* trunc,
                       hipStream_t s) {
  ChkArgs a = checks_args(e);
  a.cmd = a.cmd_stride > 0 ? cmd : nullptr; a.info = info; a.term = term; a.trunc = trunc;
  a.first = first; a.count = count;
  return launch_small<CHK_WAVES, 64 * CHK_WAVES>(checks_step_kernel, a, count, s);
}

// the masked envs (null: all; with a restore's source index: those it did not refuse) begin an episode with clean accumulators
static int checks_begin(cosim_engine* e, const uint8_t* mask, const int* src, int n_rows, int flag, hipStream_t s) {
  if (e->chk.tab.n_scn <= 0) return COSIM_OK;
  ChkArgs a = checks_args(e);
  a.mask = mask; a.src = src; a.n_rows = n_rows; a.flag = flag;
  return launch_small<CHK_WAVES, 64 * CHK_WAVES>(checks_begin_kernel, a, e->n_envs, s);
}

// ---- response curves of the scenario table (cosim_curves.hip)
static const char* const CURVES_INFO_MSG =
    ": response curves are set (cosim_scenario_curves_set) and info_out_dev is NULL: the curves sample the step's info row; pass an "
    "info buffer or clear the curves";

static CurArgs curves_args(cosim_engine* e) {
  CurArgs a;
  memset(&a, 0, sizeof a);
  a.tab = e->cur.tab; a.state = e->d_state.get(); a.scn_row = e->scn.row_out;
  a.stage = e->cur.stage.get(); a.clk = e->cur.clk.get(); a.cells = e->cur.cells.get();
  a.n_envs = e->n_envs; a.first = 0; a.count = e->n_envs;
  a.info_dim = e->ho.info_dim; a.nu = e->model.nu; a.cmd_stride = e->ho.command_dim;
  a.s_stride = e->lay.s_stride; a.s_qpos = e->lay.s_qpos; a.s_qvel = e->lay.s_qvel; a.s_meta = e->lay.s_meta;
  if (e->cur.groups > 0) { a.group = e->cur.group; a.n_groups = e->cur.groups; a.plane_words = e->cur.words; a.ungrouped = e->cur.ungrouped.get(); }
  return a;
}

// this step's samples and folds of envs [first, first + count), behind the launches that wrote the step's outputs on the same stream
static int curves_step(cosim_engine* e, int first, int count, const float* cmd, const float* info, const uint8_t* term, const uint8_t* trunc,
                       hipStream_t s) {
  CurArgs a = curves_args(e);
  a.cmd = a.cmd_stride > 0 ? cmd : nullptr; a.info = info; a.term = term; a.trunc = trunc;
  a.first = first; a.count = count;
  return launch_small<CUR_WAVES, 64 * CUR_WAVES>(e->cur.groups > 0 ? curves_step_grouped_kernel : curves_step_kernel, a, count, s);
}

// the masked envs (null: all; with a restore's source index: those it did not refuse) begin an episode with an empty stage
static int curves_begin(cosim_engine* e, const uint8_t* mask, const int* src, int n_rows, hipStream_t s) {
  if (e->cur.tab.n_scn <= 0) return COSIM_OK;
  CurArgs a = curves_args(e);
  a.mask = mask; a.src = src; a.n_rows = n_rows;
  return launch_small<CUR_WAVES, 64 * CUR_WAVES>(curves_begin_kernel, a, e->n_envs, s);
}

// every cell back to empty; with groups every plane, and the `ungrouped` word to zero
static int curves_zero(cosim_engine* e, hipStream_t s) {
  if (e->cur.groups > 0) return launch_small<1, 256>(curves_clear_grouped_kernel, curves_args(e), 2 * e->cur.tab.n_items * e->cur.groups, s);
  return launch_small<1, 256>(curves_clear_kernel, curves_args(e), 2 * e->cur.tab.n_items, s);
}

// ---- limit search of the scenario table (cosim_search.hip)
static SrchArgs search_args(cosim_engine* e) {
  SrchArgs a;
  memset(&a, 0, sizeof a);
  a.tab = e->srch.tab; a.state = e->d_state.get(); a.scn_row = e->scn.row_out;
  a.rec = e->srch.rec.get(); a.ring = e->srch.ring.get(); a.remaining = e->srch.rem.get();
  a.n_envs = e->n_envs; a.first = 0; a.count = e->n_envs;
  a.s_stride = e->lay.s_stride; a.s_meta = e->lay.s_meta; a.slots = e->srch.slots;
  a.fall = e->fall_mask != 0; a.scn_off = e->scn.tab.gid_off;
  return a;
}

// this step's outcome of envs [first, first + count), behind the launches that wrote the step's outputs on the same stream
static int search_step(cosim_engine* e, int first, int count, const uint8_t* term, const uint8_t* trunc, hipStream_t s) {
  SrchArgs a = search_args(e);
  a.term = term; a.trunc = trunc; a.first = first; a.count = count;
  if (e->srch.on_check && e->chk.tab.n_scn > 0) {   // an item fails on a check: the same rule with the verdict record checks_step_kernel closed behind this step
    const SrchChkArgs ca = {a, {e->chk.cnt.get(), e->chk.rec.get(), CHK_NCNT, e->chk.slots, checks_words(e->chk.tab.I)}};
    return launch_small<64, 64>(search_step_checks_kernel, ca, count, s);
  }
  return launch_small<64, 64>(search_step_kernel, a, count, s);
}

// the masked envs (null: all; with a restore's source index: those it did not refuse) begin an episode; their levels stay
static int search_begin(cosim_engine* e, const uint8_t* mask, const int* src, int n_rows, int flag, hipStream_t s) {
  if (e->srch.tab.n_items <= 0) return COSIM_OK;
  SrchArgs a = search_args(e);
  a.mask = mask; a.src = src; a.n_rows = n_rows; a.flag = flag;
  return launch_small<64, 64>(search_begin_kernel, a, e->n_envs, s);
}

// what is set for the rows of a table (the caller has waited for the device): another S drops it
static void scenario_rows_drop(cosim_engine* e) {
  e->par = {}; e->obsflt = {}; e->actflt = {}; e->lat = {}; e->chk = {}; e->cur = {};
  action_rows_release(e);
}
// the table and everything that goes with it
static void scenario_free(cosim_engine* e) {
  e->srch = {};
  scenario_rows_drop(e);
  e->scn = {};
}

// ---- failure traces (cosim_ftrace.hip)
static const char* const FTRACE_INFO_MSG =
    ": failure traces are set (cosim_ftrace_set) and info_out_dev is NULL: a frame holds the step's info row; pass an info buffer or "
    "switch the traces off";

static int ftrace_words(const cosim_engine* e) {
  return ftrace_frame_words(e->model.nq, e->model.nv, e->model.nu, e->ho.command_dim, e->ho.info_dim);
}

static FtArgs ftrace_args(cosim_engine* e) {
  FtArgs a;
  memset(&a, 0, sizeof a);
  a.state = e->d_state.get(); a.buf = e->ft.buf.get(); a.cnt = e->ft.cnt.get();
  a.n_envs = e->n_envs; a.first = 0; a.count = e->n_envs;
  a.nq = e->model.nq; a.nv = e->model.nv; a.nu = e->model.nu; a.cd = e->ho.command_dim; a.info_dim = e->ho.info_dim; a.F = ftrace_words(e);
  a.s_stride = e->lay.s_stride; a.s_qpos = e->lay.s_qpos; a.s_qvel = e->lay.s_qvel; a.s_meta = e->lay.s_meta;
  a.frames = e->ft.frames; a.keep = e->ft.keep; a.on_mask = e->ft.mask; a.spawn_rows = e->spawn.rows; a.fall = e->fall_mask != 0;
  if (e->scn.tab.n_scn > 0) { a.scn_row = e->scn.row_out; a.scn_rows = e->scn.tab.n_scn; a.scn_mode = e->scn.tab.mode; a.scn_off = e->scn.tab.gid_off; }
  return a;
}

// this step's frame of envs [first, first + count), behind the launches that wrote the step's outputs on the same stream
static int ftrace_step(cosim_engine* e, int first, int count, const float* actions, const float* cmd, const float* info, const uint8_t* term,
                       const uint8_t* trunc, hipStream_t s) {
  FtArgs a = ftrace_args(e);
  a.actions = actions; a.cmd = a.cd > 0 ? cmd : nullptr; a.info = info; a.term = term; a.trunc = trunc;
  a.first = first; a.count = count;
  return launch_small<1, 64>(ftrace_step_kernel, a, count, s);
}

// the masked envs (null: all; with a restore's source index: those it did not refuse) begin an episode in an empty window
static int ftrace_begin(cosim_engine* e, const uint8_t* mask, const int* src, int n_rows, int flag, hipStream_t s) {
  if (e->ft.frames <= 0) return COSIM_OK;
  FtArgs a = ftrace_args(e);
  a.mask = mask; a.src = src; a.n_rows = n_rows; a.flag = flag;
  return launch_small<1, 64>(ftrace_begin_kernel, a, e->n_envs, s);
}

// ---- the observers: ledger, failure traces, checks, curves, limit search -- in that order at every site.  Each kernel writes only its own buffers.
static_assert(LEDGER_NO_RESET == FT_NO_RESET && FT_NO_RESET == CHK_NO_RESET && CHK_NO_RESET == SRCH_NO_RESET, "one flag value for \"did not begin at a reset\"");

// behind a reset / set / restore on the same stream: the masked envs (null: all; with a restore's source index: those it did not
// refuse) begin an episode; flag 0 or LEDGER_NO_RESET.  Behind the reset because meta[14] is the new episode's spawn row
static int observers_begin(cosim_engine* e, const uint8_t* mask, const int* src, int n_rows, int flag, hipStream_t s) {
  if (flag == LEDGER_NO_RESET) RC_TRY(latency_cut(e, mask, src, n_rows, s));   // a host cut that is no reset: the latency lines of those envs restart
  RC_TRY(ledger_begin(e, mask, src, n_rows, flag, s));
  RC_TRY(ftrace_begin(e, mask, src, n_rows, flag, s));
  RC_TRY(checks_begin(e, mask, src, n_rows, flag, s));
  RC_TRY(curves_begin(e, mask, src, n_rows, s));
  return search_begin(e, mask, src, n_rows, flag, s);
}

// behind the last launch of a step (rollout: of `rows` steps, where only the ledger can be armed) of envs [first, first + count) on
// the same stream: plain device work, capturable.  They only read what the step wrote, and the caller's action rows, which outlive it
static int observers_step(cosim_engine* e, int first, int count, int rows, const float* actions, const float* cmd, const float* info,
                          const uint8_t* term, const uint8_t* trunc, hipStream_t s) {
  if (e->led.slots > 0) RC_TRY(ledger_step(e, first, count, rows, info, term, trunc, cmd, s));
  if (e->ft.frames > 0) RC_TRY(ftrace_step(e, first, count, actions, cmd, info, term, trunc, s));
  if (e->chk.tab.n_scn > 0) RC_TRY(checks_step(e, first, count, cmd, info, term, trunc, s));
  if (e->cur.tab.n_scn > 0) RC_TRY(curves_step(e, first, count, cmd, info, term, trunc, s));
  if (e->srch.tab.n_items > 0 && rows == 1) RC_TRY(search_step(e, first, count, term, trunc, s));   // reads no info row
  return COSIM_OK;
}

// why a step without info_out_dev is refused: the first armed observer's words, null if none is armed
static const char* observers_info_msg(const cosim_engine* e) {
  return e->led.slots > 0 ? LEDGER_INFO_MSG : e->ft.frames > 0 ? FTRACE_INFO_MSG : e->chk.tab.n_scn > 0 ? CHECKS_INFO_MSG : e->cur.tab.n_scn > 0 ? CURVES_INFO_MSG : nullptr;
}

// what cosim_policy_table_rotate adds to a table (cosim_poltab.h, poltab_regroup_kernel): `every` 0 means not armed
struct PolRotate {
  int every = 0;
  Dev<int32_t> base;       // [n] create's policy_of_row
  Dev<PolRange> ranges;    // [n_ranges]
  Dev<int32_t> ntiles;     // [n_ranges] the tiles each range holds now
};

// what both kinds of table are made of: the device copies of a checked table and the launch shape of every range
struct TableCore {
  int n = 0, device = 0, K = 0, n_tiles = 0;
  Dev<float> image;
  Dev<int32_t> rows;
  Dev<PolTile> tiles;
  std::vector<int32_t> tile_span;   // [n_ranges][2]: (tile_first, tile_count); armed: (tile_first, capacity)
  std::vector<int32_t> por, ranges; // create's policy_of_row [n] and ranges [n_ranges][2]
  PolRotate rot;
};

// what cosim_policy_table_create hands out: the core, the descriptors and the launch's leading dimension
struct cosim_policy_table : TableCore {
  Dev<PolDesc> desc;
  Dev<PolExt> ext;   // [K] or empty: no policy has extras, the plain grouped kernel runs
  int ld = 0;
};

// what cosim_recurrent_table_create hands out: as above, with the launch's two leading dimensions and the state tensors' row stride
struct cosim_recurrent_table : TableCore {
  Dev<RecDesc> desc;
  int ld_m = 0, ld_x = 0, hmax = 0;
};

// `Kernel` needs `lds` bytes of dynamic LDS on the current device: the attribute is raised when that is more than any call before asked
// for.  The high-water marks are per kernel and per device -- the attribute belongs to the function on the device it was set on.
template <auto Kernel>
static int kernel_needs_lds(size_t lds, const char* fn) {
  static size_t lds_allowed[64] = {0};
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  if (dev < 0 || dev >= 64) return fail(COSIM_EINVAL, std::string(fn) + ": device index out of range");
  if (lds > lds_allowed[dev]) {
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    lds_allowed[dev] = lds;
  }
  return COSIM_OK;
}

// Fills a fresh core on the current device from create's checked arrays: the image, the descriptors (into the table's own `desc`),
// the row list and the tile list.  On an error the caller deletes the table, whose members release what was allocated so far.
template <class Desc>
static int table_upload(TableCore& t, const std::vector<float>& image, const std::vector<Desc>& desc, Dev<Desc>& d_desc, const PolTiles& tl) {
  t.n = (int)tl.rows.size(); t.n_tiles = (int)tl.tiles.size(); t.tile_span = tl.tile_span;
  HIP_TRY(hipGetDevice(&t.device));
  HIP_TRY(t.image.upload(image.data(), image.size()));
  HIP_TRY(d_desc.upload(desc.data(), desc.size()));
  HIP_TRY(t.rows.upload(tl.rows.data(), tl.rows.size()));
  HIP_TRY(t.tiles.upload(tl.tiles.data(), tl.tiles.size()));
  return COSIM_OK;
}

// ---- rotation, the same for both kinds of table (fn: the entry point's name for the messages)
// Arms a table: keeps create's assignment on the device as the base, lays the static lists out again with every range's span of
// tiles as wide as policy_tile_capacity (padding: count 0) and swaps the tile buffer for that one.  The table is unchanged on failure.
static int table_rotate(TableCore* p, int every, const std::string& fn) {
  if (!p) return fail(COSIM_EINVAL, fn + ": null argument");
  if (every < 1) return fail(COSIM_EINVAL, fn + ": every " + std::to_string(every) + " is below 1");
  if (p->rot.every) return fail(COSIM_EINVAL, fn + ": the table already rotates (every " + std::to_string(p->rot.every) + ")");
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  if (dev != p->device)
    return fail(COSIM_EINVAL, fn + ": the table lives on device " + std::to_string(p->device) + ", the current device is " + std::to_string(dev));
  const int n_ranges = (int)p->ranges.size() / 2;
  const PolTiles tl = build_policy_tiles(p->por.data(), p->K, p->ranges.data(), n_ranges);
  std::vector<PolRange> rg(n_ranges);
  std::vector<int32_t> nt(n_ranges), span(2 * n_ranges);
  int cap_total = 0;
  for (int i = 0; i < n_ranges; i++) {
    rg[i] = {p->ranges[2 * i], p->ranges[2 * i + 1], cap_total, policy_tile_capacity(p->ranges[2 * i + 1], p->K)};
    nt[i] = tl.tile_span[2 * i + 1];
    span[2 * i] = cap_total; span[2 * i + 1] = rg[i].tile_cap;
    cap_total += rg[i].tile_cap;
  }
  std::vector<PolTile> tiles((size_t)cap_total, PolTile{0, 0, 0, 0});
  for (int i = 0; i < n_ranges; i++)
    for (int j = 0; j < nt[i]; j++) tiles[(size_t)rg[i].tile_first + j] = tl.tiles[(size_t)tl.tile_span[2 * i] + j];
  PolRotate r;   // build, then commit
  Dev<PolTile> d_tiles;
  HIP_TRY(r.base.upload(p->por.data(), p->por.size()));
  HIP_TRY(r.ranges.upload(rg.data(), rg.size()));
  HIP_TRY(r.ntiles.upload(nt.data(), nt.size()));
  HIP_TRY(d_tiles.upload(tiles.data(), tiles.size()));
  HIP_TRY(hipMemcpy(p->rows.get(), tl.rows.data(), tl.rows.size() * 4, hipMemcpyHostToDevice));
  p->tiles = std::move(d_tiles); p->n_tiles = cap_total; p->tile_span = span;
  r.every = every;
  p->rot = std::move(r);
  return COSIM_OK;
}

// What the plain and the rotating forward of both tables check (pointers: the entry point's own arrays are all there).  0 or the error.
static int table_forward_checks(TableCore* p, bool pointers, bool rotating, const int32_t* episode_dev, int range, const char* fn) {
  const auto who = [fn]() { return std::string(fn); };   // a message is only put together where a call is refused
  if (!p || !pointers || (rotating && !episode_dev)) return fail(COSIM_EINVAL, who() + ": null argument");
  if (rotating && !p->rot.every) return fail(COSIM_EINVAL, who() + ": the table does not rotate (cosim_*_table_rotate arms it)");
  if (!rotating && p->rot.every)
    return fail(COSIM_EINVAL, who() + ": the table rotates (every " + std::to_string(p->rot.every) + "): its lists change per step, use " + who() + "_rotating");
  const int n_ranges = (int)p->tile_span.size() / 2;
  if (range < -1 || range >= n_ranges)
    return fail(COSIM_EINVAL, who() + ": range " + std::to_string(range) + " outside -1.." + std::to_string(n_ranges - 1));
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  if (dev != p->device)
    return fail(COSIM_EINVAL, who() + ": the table lives on device " + std::to_string(p->device) + ", the current device is " + std::to_string(dev));
  return COSIM_OK;
}

static int table_regroup(TableCore* p, int32_t* episode_dev, int32_t* policy_now_dev, const uint8_t* done_a_dev, const uint8_t* done_b_dev, int range,
                         hipStream_t s) {
  PolRegroupArgs g;
  g.base = p->rot.base.get(); g.episode = episode_dev; g.policy_now = policy_now_dev; g.done_a = done_a_dev; g.done_b = done_b_dev;
  g.ranges = p->rot.ranges.get(); g.rows = p->rows.get(); g.tiles = p->tiles.get(); g.n_tiles = p->rot.ntiles.get();
  g.range_first = range < 0 ? 0 : range; g.K = p->K; g.every = p->rot.every;
  hipLaunchKernelGGL(poltab_regroup_kernel, dim3(range < 0 ? (int)p->tile_span.size() / 2 : 1), dim3(RG_THREADS), 0, s, g);
  HIP_TRY(hipGetLastError());
  return COSIM_OK;
}

// one range's lists as they stand, after everything queued on the device: rows_host [count of the range], tiles_host [its capacity][4]
static int table_lists(TableCore* p, int range, int* rows_host, int* tiles_host, int* n_tiles_out, const std::string& fn) {
  if (!p || !rows_host || !tiles_host || !n_tiles_out) return fail(COSIM_EINVAL, fn + ": null argument");
  const int n_ranges = (int)p->tile_span.size() / 2;
  if (range < 0 || range >= n_ranges) return fail(COSIM_EINVAL, fn + ": range " + std::to_string(range) + " outside 0.." + std::to_string(n_ranges - 1));
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  if (dev != p->device)
    return fail(COSIM_EINVAL, fn + ": the table lives on device " + std::to_string(p->device) + ", the current device is " + std::to_string(dev));
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(rows_host, p->rows.get() + p->ranges[2 * range], (size_t)p->ranges[2 * range + 1] * 4, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(tiles_host, p->tiles.get() + p->tile_span[2 * range], (size_t)p->tile_span[2 * range + 1] * sizeof(PolTile), hipMemcpyDeviceToHost));
  if (p->rot.every) HIP_TRY(hipMemcpy(n_tiles_out, p->rot.ntiles.get() + range, 4, hipMemcpyDeviceToHost));
  else *n_tiles_out = p->tile_span[2 * range + 1];
  return COSIM_OK;
}

// cosim_mlp_extras_t (include/cosim_actor.h) is handed to cosim_poltab.h as PolExtRaw: the same layout, field by field
#define EXTRAS_SAME(f) (offsetof(cosim_mlp_extras_t, f) == offsetof(PolExtRaw, f) && sizeof(cosim_mlp_extras_t::f) == sizeof(PolExtRaw::f))
static_assert(sizeof(cosim_mlp_extras_t) == sizeof(PolExtRaw) && EXTRAS_SAME(n_in) && EXTRAS_SAME(n_out) && EXTRAS_SAME(in_op) && EXTRAS_SAME(out_op) &&
              EXTRAS_SAME(in_vec) && EXTRAS_SAME(out_vec) && EXTRAS_SAME(in_lo) && EXTRAS_SAME(in_hi) && EXTRAS_SAME(out_lo) && EXTRAS_SAME(out_hi) &&
              EXTRAS_SAME(ln_where) && EXTRAS_SAME(ln_eps) && EXTRAS_SAME(ln_gamma) && EXTRAS_SAME(ln_beta),
              "cosim_mlp_extras_t is PolExtRaw (cosim_poltab.h)");
#undef EXTRAS_SAME

// cosim_mlp_forward and cosim_mlp_forward_ex (fn: the entry point's name for the messages; ext null: the plain one)
static int mlp_forward_any(const char* fn, const float* x_dev, int n, int n_layers, const int* dims, const float* const* w_dev,
                           const float* const* b_dev, const int* act, const float* act_alpha, const PolExtRaw* ext, float clip, float* out_dev,
                           void* stream) {
  const auto who = [fn]() { return std::string(fn); };
  if (!x_dev || !dims || !w_dev || !act || !out_dev || n <= 0) return fail(COSIM_EINVAL, who() + ": bad argument");
  if (n_layers < 1 || n_layers > MLP_MAXL) return fail(COSIM_EINVAL, who() + ": 1..6 layers");
  MlpArgs a;
  memset(&a, 0, sizeof a);
  int maxd = 0;
  for (int l = 0; l <= n_layers; l++) {
    if (dims[l] < 1 || dims[l] > MLP_MAXD) return fail(COSIM_EINVAL, who() + ": layer width outside 1..512");
    a.dims[l] = dims[l];
    if (dims[l] > maxd) maxd = dims[l];
  }
  for (int l = 0; l < n_layers; l++) {
    if (!w_dev[l]) return fail(COSIM_EINVAL, who() + ": null weight");
    a.w[l] = w_dev[l]; a.b[l] = b_dev ? b_dev[l] : nullptr; a.act[l] = act[l]; a.act_alpha[l] = act_alpha ? act_alpha[l] : 1.f;
  }
  a.x = x_dev; a.out = out_dev; a.nl = n_layers; a.n = n; a.clip = clip; a.ld = maxd | 1;
  const size_t lds = (size_t)2 * 32 * a.ld * sizeof(float);
  if (ext) {
    const std::string err = check_extras(who(), *ext, n_layers);
    if (!err.empty()) return fail(COSIM_EINVAL, err);
  }
  if (ext && ext_used(*ext, n_layers)) {
    MlpExt x;
    memset(&x, 0, sizeof x);
    x.n_in = ext->n_in; x.n_out = ext->n_out;
    for (int i = 0; i < ext->n_in; i++) x.in[i] = MlpStage{ext->in_op[i], ext->in_op[i] != 5 ? ext->in_vec[i] : nullptr, ext->in_lo[i], ext->in_hi[i]};
    for (int i = 0; i < ext->n_out; i++) x.out[i] = MlpStage{ext->out_op[i], ext->out_op[i] != 5 ? ext->out_vec[i] : nullptr, ext->out_lo[i], ext->out_hi[i]};
    for (int s = 0; s < n_layers; s++)
      if (ext->ln_where[s]) x.ln[s] = MlpLn{ext->ln_where[s], ext->ln_gamma[s], ext->ln_beta[s], ext->ln_eps[s]};
    RC_TRY(kernel_needs_lds<mlp_forward_ext_kernel>(lds, fn));
    hipLaunchKernelGGL(mlp_forward_ext_kernel, dim3((n + 31) / 32), dim3(256), lds, (hipStream_t)stream, a, x);
  } else {
    RC_TRY(kernel_needs_lds<mlp_forward_kernel>(lds, fn));
    hipLaunchKernelGGL(mlp_forward_kernel, dim3((n + 31) / 32), dim3(256), lds, (hipStream_t)stream, a);
  }
  HIP_TRY(hipGetLastError());
  return COSIM_OK;
}

extern "C" {

// Fused actor MLP (cosim_mlp.hip): out = clip(act_L(... act_1(x W_1^T + b_1) ...)).  All pointers are device pointers; dims has
// n_layers + 1 entries; act / act_alpha one entry per layer (0 none, 1 relu, 2 tanh, 3 elu, 4 sigmoid, 5 leaky relu).
int cosim_mlp_forward(const float* x_dev, int n, int n_layers, const int* dims, const float* const* w_dev, const float* const* b_dev,
                      const int* act, const float* act_alpha, float clip, float* out_dev, void* stream) {
  return mlp_forward_any("cosim_mlp_forward", x_dev, n, n_layers, dims, w_dev, b_dev, act, act_alpha, nullptr, clip, out_dev, stream);
}

// The same with an extended actor's stages and LayerNorms (cosim_mlp.hip: mlp_forward_ext_kernel); null or empty extras: the launch above.
int cosim_mlp_forward_ex(const float* x_dev, int n, int n_layers, const int* dims, const float* const* w_dev, const float* const* b_dev,
                         const int* act, const float* act_alpha, const cosim_mlp_extras_t* extras, float clip, float* out_dev, void* stream) {
  return mlp_forward_any("cosim_mlp_forward_ex", x_dev, n, n_layers, dims, w_dev, b_dev, act, act_alpha, reinterpret_cast<const PolExtRaw*>(extras),
                         clip, out_dev, stream);
}

// Policy table (cosim_poltab.h, mlp_grouped_kernel): K actors over one fleet, one launch per evaluation.  create checks and packs the
// host arrays, builds the tile list and uploads everything once; forward only launches.
static int policy_table_make(const char* fn, const PolRaw& raw, cosim_policy_table** out) {
  if (!out) return fail(COSIM_EINVAL, std::string(fn) + ": null argument");
  *out = nullptr;
  const PolShape shape = validate_policy_table(raw, fn);
  if (!shape.err.empty()) return fail(COSIM_EINVAL, shape.err);
  const PolImage im = pack_policy_image(raw);
  std::unique_ptr<cosim_policy_table> p(new cosim_policy_table);
  p->K = raw.K; p->ld = shape.maxd | 1;
  p->por.assign(raw.policy_of_row, raw.policy_of_row + raw.n); p->ranges.assign(raw.ranges, raw.ranges + 2 * raw.n_ranges);
  const size_t lds = (size_t)2 * 32 * p->ld * sizeof(float);
  int rc = im.ext.empty() ? kernel_needs_lds<mlp_grouped_kernel>(lds, fn) : kernel_needs_lds<mlp_grouped_ext_kernel>(lds, fn);
  if (!rc) rc = table_upload(*p, im.words, im.desc, p->desc, build_policy_tiles(raw.policy_of_row, raw.K, raw.ranges, raw.n_ranges));
  if (rc) return rc;
  if (!im.ext.empty()) HIP_TRY(p->ext.upload(im.ext.data(), im.ext.size()));
  *out = p.release();
  return COSIM_OK;
}

int cosim_policy_table_create(int n_policies, const int* n_layers, const int* dims, const int* act, const float* act_alpha,
                              const float* const* w_host, const float* const* b_host, int n, const int* policy_of_row, int n_ranges,
                              const int* ranges, cosim_policy_table** out) {
  const PolRaw raw = {n_policies, n_layers, dims, act, act_alpha, w_host, b_host, n, policy_of_row, n_ranges, ranges};
  return policy_table_make("cosim_policy_table_create", raw, out);
}

int cosim_policy_table_create_ex(int n_policies, const int* n_layers, const int* dims, const int* act, const float* act_alpha,
                                 const float* const* w_host, const float* const* b_host, const cosim_mlp_extras_t* extras, int n,
                                 const int* policy_of_row, int n_ranges, const int* ranges, cosim_policy_table** out) {
  const PolRaw raw = {n_policies, n_layers, dims, act, act_alpha, w_host, b_host, n, policy_of_row, n_ranges, ranges,
                      reinterpret_cast<const PolExtRaw*>(extras)};
  return policy_table_make("cosim_policy_table_create_ex", raw, out);
}

// range: an index into the ranges given to create, or -1 for all of them.  No allocation, no host read of device memory and no
// synchronisation: the launch can be captured in a graph.
static int policy_table_launch(cosim_policy_table* p, const float* x_dev, float* out_dev, int range, float clip, hipStream_t s) {
  PolTabArgs a;
  a.x = x_dev; a.out = out_dev; a.image = p->image.get(); a.desc = p->desc.get(); a.rows = p->rows.get(); a.tiles = p->tiles.get();
  a.tile_first = range < 0 ? 0 : p->tile_span[2 * range]; a.ld = p->ld; a.clip = clip;
  const int tile_count = range < 0 ? p->n_tiles : p->tile_span[2 * range + 1];
  const size_t lds = (size_t)2 * 32 * p->ld * sizeof(float);
  if (p->ext) hipLaunchKernelGGL(mlp_grouped_ext_kernel, dim3(tile_count), dim3(256), lds, s, a, (const PolExt*)p->ext.get());
  else hipLaunchKernelGGL(mlp_grouped_kernel, dim3(tile_count), dim3(256), lds, s, a);
  HIP_TRY(hipGetLastError());
  return COSIM_OK;
}

int cosim_policy_table_forward(cosim_policy_table* p, const float* x_dev, float* out_dev, int range, float clip, void* stream) {
  RC_TRY(table_forward_checks(p, x_dev && out_dev, false, nullptr, range, "cosim_policy_table_forward"));
  return policy_table_launch(p, x_dev, out_dev, range, clip, (hipStream_t)stream);
}

// Rotation (cosim_poltab.h): arm once, then every evaluation is the regroup launch and the grouped launch over the capacity, both
// with constant grids -- no allocation, no host read, no synchronisation, so the pair can be captured.
int cosim_policy_table_rotate(cosim_policy_table* p, int every) { return table_rotate(p, every, "cosim_policy_table_rotate"); }

int cosim_policy_table_forward_rotating(cosim_policy_table* p, const float* x_dev, float* out_dev, int32_t* episode_dev, int32_t* policy_now_dev,
                                        const uint8_t* done_a_dev, const uint8_t* done_b_dev, int range, float clip, void* stream) {
  RC_TRY(table_forward_checks(p, x_dev && out_dev, true, episode_dev, range, "cosim_policy_table_forward_rotating"));
  RC_TRY(table_regroup(p, episode_dev, policy_now_dev, done_a_dev, done_b_dev, range, (hipStream_t)stream));
  return policy_table_launch(p, x_dev, out_dev, range, clip, (hipStream_t)stream);
}

int cosim_policy_table_lists(cosim_policy_table* p, int range, int* rows_host, int* tiles_host, int* n_tiles_out) {
  return table_lists(p, range, rows_host, tiles_host, n_tiles_out, "cosim_policy_table_lists");
}

int cosim_policy_table_destroy(cosim_policy_table* p) {
  delete p;
  return COSIM_OK;
}

// Recurrent policy table (cosim_rectab.h, lstm_actor_grouped_kernel): K recurrent actors over one fleet, one launch per evaluation.
// create checks and packs the host arrays, builds the tile list and uploads everything once; forward only launches.
int cosim_recurrent_table_create(int n_policies, const int* n_enc, const int* enc_dims, const int* enc_act, const float* enc_alpha,
                                 const float* const* enc_w_host, const float* const* enc_b_host, const int* lstm_in, const int* hidden,
                                 const float* const* lstm_w_host, const float* const* lstm_r_host, const float* const* lstm_b_host,
                                 const int* n_head, const int* head_dims, const int* head_act, const float* head_alpha,
                                 const float* const* head_w_host, const float* const* head_b_host, int n, const int* policy_of_row,
                                 int n_ranges, const int* ranges, cosim_recurrent_table** out) {
  if (!out) return fail(COSIM_EINVAL, "cosim_recurrent_table_create: null argument");
  *out = nullptr;
  const RecRaw raw = {n_policies, n_enc, enc_dims, enc_act, enc_alpha, enc_w_host, enc_b_host, lstm_in, hidden, lstm_w_host, lstm_r_host, lstm_b_host,
                      n_head, head_dims, head_act, head_alpha, head_w_host, head_b_host, n, policy_of_row, n_ranges, ranges};
  int dev = 0, lds_limit = 0;
  HIP_TRY(hipGetDevice(&dev));
  if (dev < 0 || dev >= 64) return fail(COSIM_EINVAL, "cosim_recurrent_table_create: device index out of range");
  HIP_TRY(hipDeviceGetAttribute(&lds_limit, hipDeviceAttributeMaxSharedMemoryPerBlock, dev));
  const RecShape shape = validate_recurrent_table(raw, lds_limit);
  if (!shape.err.empty()) return fail(COSIM_EINVAL, shape.err);
  const RecImage im = pack_recurrent_image(raw);
  std::unique_ptr<cosim_recurrent_table> p(new cosim_recurrent_table);
  p->K = n_policies; p->ld_m = shape.ld_m; p->ld_x = shape.ld_x; p->hmax = shape.hmax;
  p->por.assign(policy_of_row, policy_of_row + n); p->ranges.assign(ranges, ranges + 2 * n_ranges);
  int rc = kernel_needs_lds<lstm_actor_grouped_kernel>((size_t)rec_lds_dynamic(p->ld_m, p->ld_x), "cosim_recurrent_table_create");
  if (!rc) rc = table_upload(*p, im.words, im.desc, p->desc, build_policy_tiles(policy_of_row, n_policies, ranges, n_ranges));
  if (rc) return rc;
  *out = p.release();
  return COSIM_OK;
}

// h_dev / c_dev: the table's state, [n, hmax] with hmax the widest hidden size, updated in place.  done_a_dev / done_b_dev: [n] bytes
// or null; a row with either set starts from a zero state.  No allocation, no host read of device memory and no synchronisation.
static int recurrent_table_launch(cosim_recurrent_table* p, const float* x_dev, float* h_dev, float* c_dev, float* out_dev, const uint8_t* done_a_dev,
                                  const uint8_t* done_b_dev, int range, float clip, hipStream_t s) {
  RecTabArgs a;
  a.x = x_dev; a.h = h_dev; a.c = c_dev; a.out = out_dev; a.done_a = done_a_dev; a.done_b = done_b_dev;
  a.image = p->image.get(); a.desc = p->desc.get(); a.rows = p->rows.get(); a.tiles = p->tiles.get();
  a.tile_first = range < 0 ? 0 : p->tile_span[2 * range]; a.ld_m = p->ld_m; a.ld_x = p->ld_x; a.hmax = p->hmax; a.clip = clip;
  const int tile_count = range < 0 ? p->n_tiles : p->tile_span[2 * range + 1];
  hipLaunchKernelGGL(lstm_actor_grouped_kernel, dim3(tile_count), dim3(256), (size_t)rec_lds_dynamic(p->ld_m, p->ld_x), s, a);
  HIP_TRY(hipGetLastError());
  return COSIM_OK;
}

int cosim_recurrent_table_forward(cosim_recurrent_table* p, const float* x_dev, float* h_dev, float* c_dev, float* out_dev,
                                  const uint8_t* done_a_dev, const uint8_t* done_b_dev, int range, float clip, void* stream) {
  RC_TRY(table_forward_checks(p, x_dev && h_dev && c_dev && out_dev, false, nullptr, range, "cosim_recurrent_table_forward"));
  return recurrent_table_launch(p, x_dev, h_dev, c_dev, out_dev, done_a_dev, done_b_dev, range, clip, (hipStream_t)stream);
}

// Rotation, as the MLP table's.  The done bytes do both jobs: the regroup launch counts the ended episode and moves the row to its
// next policy, the actor launch behind it starts that policy from h = c = 0.
int cosim_recurrent_table_rotate(cosim_recurrent_table* p, int every) { return table_rotate(p, every, "cosim_recurrent_table_rotate"); }

int cosim_recurrent_table_forward_rotating(cosim_recurrent_table* p, const float* x_dev, float* h_dev, float* c_dev, float* out_dev,
                                           int32_t* episode_dev, int32_t* policy_now_dev, const uint8_t* done_a_dev, const uint8_t* done_b_dev,
                                           int range, float clip, void* stream) {
  RC_TRY(table_forward_checks(p, x_dev && h_dev && c_dev && out_dev, true, episode_dev, range, "cosim_recurrent_table_forward_rotating"));
  RC_TRY(table_regroup(p, episode_dev, policy_now_dev, done_a_dev, done_b_dev, range, (hipStream_t)stream));
  return recurrent_table_launch(p, x_dev, h_dev, c_dev, out_dev, done_a_dev, done_b_dev, range, clip, (hipStream_t)stream);
}

int cosim_recurrent_table_lists(cosim_recurrent_table* p, int range, int* rows_host, int* tiles_host, int* n_tiles_out) {
  return table_lists(p, range, rows_host, tiles_host, n_tiles_out, "cosim_recurrent_table_lists");
}

int cosim_recurrent_table_destroy(cosim_recurrent_table* p) {
  delete p;
  return COSIM_OK;
}

int cosim_lstm_cell(const float* x_dev, const float* h_dev, const float* c_dev, int n, int in_dim, int hidden, const float* w_dev,
                    const float* r_dev, const float* b_dev, float* h_out_dev, float* c_out_dev, void* stream) {
  if (!x_dev || !h_dev || !c_dev || !w_dev || !r_dev || !h_out_dev || !c_out_dev || n <= 0) return fail(COSIM_EINVAL, "cosim_lstm_cell: bad argument");
  if (in_dim < 1 || hidden < 1 || in_dim + hidden > 1200) return fail(COSIM_EINVAL, "cosim_lstm_cell: in_dim + hidden outside 2..1200");
  LstmArgs a;
  a.x = x_dev; a.h = h_dev; a.c = c_dev; a.W = w_dev; a.R = r_dev; a.B = b_dev; a.h_out = h_out_dev; a.c_out = c_out_dev;
  a.n = n; a.I = in_dim; a.H = hidden; a.ld = (in_dim + hidden) | 1;
  a.vec = in_dim % 4 == 0 && hidden % 4 == 0 && ((uintptr_t)w_dev | (uintptr_t)r_dev) % 16 == 0;
  const size_t lds = (size_t)32 * a.ld * sizeof(float);
  RC_TRY(kernel_needs_lds<lstm_cell_kernel>(lds, "cosim_lstm_cell"));
  hipLaunchKernelGGL(lstm_cell_kernel, dim3((n + 31) / 32), dim3(256), lds, (hipStream_t)stream, a);
  HIP_TRY(hipGetLastError());
  return COSIM_OK;
}

int cosim_fleet_stats(const float* info_dev, int n, int info_dim, int nu, const float* cmd_dev, int cmd_stride, int ncmd, double* acc_dev,
                      void* stream) {
  if (!info_dev || !acc_dev || n <= 0 || nu < 0 || ncmd < 0 || ncmd > 3 || 4 + nu + ncmd > 32 || info_dim < 4 + nu || (ncmd > 0 && !cmd_dev))
    return fail(COSIM_EINVAL, "cosim_fleet_stats: bad argument");
  const int blocks = n >= 8 * 64 ? 64 : (n + 7) / 8;
  hipLaunchKernelGGL(fleet_stats_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, info_dev, n, info_dim, nu, cmd_dev, cmd_stride, ncmd,
                     acc_dev);
  HIP_TRY(hipGetLastError());
  return COSIM_OK;
}

int cosim_fleet_hist(const float* info_dev, int n, int info_dim, int nu, const float* cmd_dev, int cmd_stride, int ncmd, const float* hi_dev,
                     int nbins, double* hist_dev, void* stream) {
  if (!info_dev || !hi_dev || !hist_dev || n <= 0 || nu < 0 || ncmd < 0 || ncmd > 3 || 4 + nu + ncmd > 32 || info_dim < 4 + nu || nbins < 2 ||
      (ncmd > 0 && !cmd_dev))
    return fail(COSIM_EINVAL, "cosim_fleet_hist: bad argument");
  const int blocks = n >= 8 * 64 ? 64 : (n + 7) / 8;
  hipLaunchKernelGGL(fleet_hist_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, info_dev, n, info_dim, nu, cmd_dev, cmd_stride, ncmd,
                     hi_dev, nbins, hist_dev);
  HIP_TRY(hipGetLastError());
  return COSIM_OK;
}

const char* cosim_last_error(void) { return g_err.c_str(); }
int cosim_model_sizeof(void) { return (int)sizeof(cosim_model_t); }
int cosim_obs_config_sizeof(void) { return (int)sizeof(cosim_obs_config_t); }

// everything cosim_create allocates, into a fresh engine; on an error the caller destroys the engine, whose members release what was allocated so far
static int create_fill(cosim_engine* e, const cosim_model_t* model, const float* hull_vert, const int* hull_adr, const int* hull_nbr,
                       const float* hfield, int n_envs) {
  int rc = build_dev_model(e);
  if (rc == COSIM_OK) rc = build_dev_obs(e);
  if (rc != COSIM_OK) return rc;
  build_layout(e);
  const int nv = model->nv, nb = model->nbody;
  // kernel instantiations: (nv, nbody) of the four cosim robots; RPL = constraint rows per lane
  const bool hf = model->ground_type == CS_GEOM_HFIELD;
  // coarse field: both cell edges at least 10 cm (see select_t)
  const bool coarse = hf && model->hfield_ncol > 1 && model->hfield_nrow > 1 && 2.0 * model->hfield_size[0] / (model->hfield_ncol - 1) >= 0.1 &&
                      2.0 * model->hfield_size[1] / (model->hfield_nrow - 1) >= 0.1;
  int gtm = 0;   // geom types present: the kernel is specialised on them (bit 0 sphere, 1 cylinder, 2 box, 3 mesh)
  std::vector<char> in_pair(model->ngeom > 0 ? model->ngeom : 1, 0);
  for (int p = 0; p < model->npair; p++) { in_pair[model->pair_geom1[p]] = 1; in_pair[model->pair_geom2[p]] = 1; }
  for (int g = 0; g < model->ngeom; g++) {
    if (!model->geom_ground[g] && !in_pair[g]) continue;
    switch (model->geom_type[g]) {
      case CS_GEOM_SPHERE: gtm |= GT_SPHERE; break;
      case CS_GEOM_CYLINDER: gtm |= GT_CYLINDER; break;
      case CS_GEOM_BOX: gtm |= GT_BOX; break;
      case CS_GEOM_MESH: gtm |= GT_MESH; break;
      default: return fail(COSIM_EINVAL, "cosim_create: collision geom type not implemented in the HIP engine");
    }
  }
  KernelSet<launch_fn> ks;
  if (nv == 18 && nb <= 14 && (gtm & ~G_LIGHT) == 0) ks = light_v1_kernels(hf, coarse);
  else if (nv == 14 && nb <= 10 && (gtm & ~G_MESH) == 0) ks = p_v3_kernels(hf, coarse);
  else if (nv == 22 && nb <= 18 && (gtm & ~G_MESH) == 0) ks = w4_kernels(hf, coarse);
  else if (nv == 29 && nb <= 26 && (gtm & ~G_HUM) == 0) ks = humanoid_kernels(hf, coarse);
  else { return fail(COSIM_EINVAL, "cosim_create: no kernel instantiation for this (nv, nbody); add one in cosim_engine.hip"); }
  if (nv != 18 && model->neq > 0) { return fail(COSIM_EINVAL, "cosim_create: this robot's kernels keep no rows for connect equalities"); }
  if (model->ngeom > ks.fleet.geom_stage) { return fail(COSIM_EINVAL, "cosim_create: more collision geoms than the plane kernel stages contacts for"); }
  if (has(ks.hfix)) {   // the fix-up capacity must hold 50 contacts per ground geom; a model with more ground geoms has no heightfield fix-up
    int nground = 0;
    for (int g = 0; g < model->ngeom; g++) nground += model->geom_ground[g] != 0;
    if (nground * XC > ks.hfix.contact_slots) ks.hfix = ks.stepfix = ks.dbg_hfix = {};
  }
  e->kernels = ks;
  e->plan = make_plan(e->kernels, e->sw);
  {
    // support maps of the mesh geoms' hulls (geoms that share a hull slice share the map)
    std::vector<float> cells, cand;
    for (int g = 0; g < 64; g++) e->hullmap_of_geom[g] = -1;
    for (int g = 0; g < model->ngeom; g++) {
      if (model->geom_type[g] != CS_GEOM_MESH || model->geom_hullnum[g] < HM_MIN_VERTS || !hull_vert || !hull_adr || !hull_nbr) continue;
      for (int h = 0; h < g; h++)
        if (e->hullmap_of_geom[h] >= 0 && model->geom_hulladr[h] == model->geom_hulladr[g] && model->geom_hullnum[h] == model->geom_hullnum[g])
          e->hullmap_of_geom[g] = e->hullmap_of_geom[h];
      if (e->hullmap_of_geom[g] >= 0) continue;
      const int adr = model->geom_hulladr[g], num = model->geom_hullnum[g];
      if (adr < 0 || adr + num > model->nhullvert) { return fail(COSIM_EINVAL, "cosim_create: geom hull slice outside the hull vertex array"); }
      for (int v = adr; v < adr + num; v++)
        for (int k = hull_adr[v]; k < hull_adr[v + 1]; k++)
          if (k < 0 || k >= model->nhulledge || hull_nbr[k] < 0 || hull_nbr[k] >= num) { return fail(COSIM_EINVAL, "cosim_create: hull neighbour graph out of range"); }
      e->hullmap_of_geom[g] = (int)(cells.size() / (4 * HM_REC));
      build_support_map(hull_vert + 3 * (size_t)adr, num, hull_adr + adr, hull_nbr, cells, cand);
    }
    for (int g = 0; g < 64; g++) e->hm.g_hullmap[g] = e->hullmap_of_geom[g];
    if (cells.empty()) cells.assign(4 * HM_REC, 0.f);
    if (cand.empty()) cand.assign(4, 0.f);
    HIP_TRY(e->d_hull_cell.upload(reinterpret_cast<const float4*>(cells.data()), cells.size() / 4));
    HIP_TRY(e->d_hull_cand.upload(reinterpret_cast<const float4*>(cand.data()), cand.size() / 4));
  }
  e->model_term_mode = e->hm.term_mode; e->model_term_bodymask = e->hm.term_bodymask;
  HIP_TRY(e->d_model.upload(&e->hm, 1));
  HIP_TRY(e->d_obs.upload(&e->ho, 1));
  HIP_TRY(e->d_state.alloc_zeroed((size_t)n_envs * e->lay.s_stride));
  HIP_TRY(e->d_params.alloc((size_t)n_envs * e->lay.p_stride));
  HIP_TRY(e->d_dbg.alloc(8192));
  if (has(e->kernels.solver)) {   // the split pipeline's buffers
    HIP_TRY(e->d_xcon.alloc((size_t)n_envs * XG * XC * 8));
    HIP_TRY(e->d_xcnt.alloc_zeroed((size_t)n_envs * XG));
    HIP_TRY(e->d_xstate.alloc_zeroed((size_t)n_envs * XS));
  }
  HIP_TRY(e->d_ovf.alloc_zeroed((size_t)n_envs));
  int nhv = model->nhullvert > 0 ? model->nhullvert : 1, nhe = model->nhulledge > 0 ? model->nhulledge : 1;
  HIP_TRY(e->d_hull_vert.alloc((size_t)nhv * 4));   // 16 bytes per vertex on the device: one load each
  HIP_TRY(e->d_hull_adr.alloc((size_t)nhv + 1));
  HIP_TRY(e->d_hull_nbr.alloc((size_t)nhe));
  if (model->nhullvert > 0) {
    if (!hull_vert || !hull_adr || !hull_nbr) return fail(COSIM_EINVAL, "cosim_create: model has mesh geoms but no hull arrays were passed");
    std::vector<float> hv4((size_t)model->nhullvert * 4, 0.f);
    for (int i = 0; i < model->nhullvert; i++) for (int k = 0; k < 3; k++) hv4[4 * (size_t)i + k] = hull_vert[3 * (size_t)i + k];
    HIP_TRY(hipMemcpy(e->d_hull_vert.get(), hv4.data(), hv4.size() * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(e->d_hull_adr.get(), hull_adr, (size_t)(model->nhullvert + 1) * sizeof(int), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(e->d_hull_nbr.get(), hull_nbr, (size_t)model->nhulledge * sizeof(int), hipMemcpyHostToDevice));
  }
  {
    std::vector<unsigned> hp(model->npair > 0 ? model->npair : 1, 0u);
    for (int p = 0; p < model->npair; p++) hp[p] = (unsigned)model->pair_geom1[p] | ((unsigned)model->pair_geom2[p] << 16);
    std::vector<float4> hg(model->ngeom > 0 ? model->ngeom : 1);
    for (int g = 0; g < model->ngeom; g++)
      hg[g] = make_float4((float)model->geom_center[g][0], (float)model->geom_center[g][1], (float)model->geom_center[g][2], (float)model->geom_friction[g][0]);
    HIP_TRY(e->d_pairs.upload(hp.data(), hp.size()));
    HIP_TRY(e->d_gext.upload(hg.data(), hg.size()));
  }
  if (model->ground_type == CS_GEOM_HFIELD) {
    // any cell size: the narrowphase walks however many prisms lie under a geom (1 cm cells of the stairs_* terrains included);
    // contacts beyond the kernel variant's slots are counted (cosim_get "meta", word 8), never dropped silently
    if (!hfield) return fail(COSIM_EINVAL, "cosim_create: heightfield ground but no elevation data was passed");
    size_t nh = (size_t)model->hfield_nrow * model->hfield_ncol;
    HIP_TRY(e->d_hfield.upload(hfield, nh));
    // tile maxima for the coarse terrain test ahead of the prism walk (terrain_max_under)
    const int mrow = (model->hfield_nrow + HF_TILE - 1) / HF_TILE, mcol = (model->hfield_ncol + HF_TILE - 1) / HF_TILE;
    std::vector<float> mip((size_t)mrow * mcol, 0.f);
    for (int r = 0; r < model->hfield_nrow; r++)
      for (int c = 0; c < model->hfield_ncol; c++) {
        float& m = mip[(size_t)(r / HF_TILE) * mcol + c / HF_TILE];
        const float h = hfield[(size_t)r * model->hfield_ncol + c];
        m = ((r % HF_TILE) == 0 && (c % HF_TILE) == 0) ? h : (h > m ? h : m);
      }
    HIP_TRY(e->d_hfield_mip.upload(mip.data(), mip.size()));
  }
  default_params(e);
  return set_ranges(e, 1);   // (allocates the pacing events of the single-launch path)
}


int cosim_create(const cosim_model_t* model, const float* hull_vert, const int* hull_adr, const int* hull_nbr, const float* hfield,
                 const cosim_obs_config_t* obs, int n_envs, int device, uint64_t seed, int64_t env_id0, cosim_engine_t** out) {
  if (!model || !obs || !out || n_envs < 1) return fail(COSIM_EINVAL, "cosim_create: null argument or n_envs < 1");
  if (model->magic != CS_MODEL_MAGIC || model->magic_end != CS_MODEL_MAGIC) return fail(COSIM_EINVAL, "cosim_create: model blob magic mismatch (layout drift?)");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return fail(COSIM_ENOGPU, "cosim_create: no HIP device available");
  if (device < 0 || device >= ndev) return fail(COSIM_EINVAL, "cosim_create: bad device index");
  HIP_TRY(hipSetDevice(device));
  cosim_engine* e = new cosim_engine();
  e->n_envs = n_envs; e->device = device; e->model = *model; e->obs_cfg = *obs; e->seed = seed; e->env_id0 = env_id0;
  const int rc = create_fill(e, model, hull_vert, hull_adr, hull_nbr, hfield, n_envs);
  if (rc != COSIM_OK) {   // one cleanup path: the engine's streams and events, then the engine with its buffers (the message survives it)
    const std::string msg = g_err;
    cosim_destroy(e);
    g_err = msg;
    return rc;
  }
  *out = e;
  return COSIM_OK;
}

int cosim_destroy(cosim_engine_t* e) {
  if (!e) return COSIM_OK;
  hipSetDevice(e->device);
  for (hipEvent_t x : e->ev) hipEventDestroy(x);
  for (hipStream_t x : e->rstream) hipStreamDestroy(x);
  for (hipEvent_t x : e->rdone) hipEventDestroy(x);
  for (hipEvent_t x : e->ring) hipEventDestroy(x);   // the pacing events: [n_streams][inflight]
  if (e->ev_in) hipEventDestroy(e->ev_in);
  delete e;   // every buffer goes with the member that owns it
  return COSIM_OK;
}

// The iteration caps the solver runs with: the model's counts (iterations per precision level: 50 / 50 / 75 / 75 / 100), lowered
// only by an explicit "max_newton" / "max_ls".  cosim_query reports the same numbers.
static int newton_cap(const cosim_engine* e) {
  return e->max_newton < 0 ? e->model.iterations : (e->max_newton < e->model.iterations ? e->max_newton : e->model.iterations);
}
static int ls_cap(const cosim_engine* e) { return e->max_ls < 0 ? e->model.ls_iterations : (e->max_ls < e->model.ls_iterations ? e->max_ls : e->model.ls_iterations); }

// "scenario_curve_ungrouped": joins the ranges, waits and reads the device word (0 with no groups); held at INT_MAX
// envs with a search item that have trials left (cosim_query "search_remaining"): joins the ranges and reads the one word
static int search_remaining(cosim_engine* e) {
  if (e->srch.tab.n_items <= 0) return 0;
  HIP_TRY(hipSetDevice(e->device));
  RC_TRY(join_ranges(e, 0));
  HIP_TRY(hipDeviceSynchronize());
  int v = 0;
  HIP_TRY(hipMemcpy(&v, e->srch.rem.get(), sizeof v, hipMemcpyDeviceToHost));
  return v;
}

static int curves_ungrouped(cosim_engine* e) {
  if (e->cur.groups <= 0) return 0;
  HIP_TRY(hipSetDevice(e->device));
  RC_TRY(join_ranges(e, 0));
  HIP_TRY(hipDeviceSynchronize());
  unsigned v = 0;
  HIP_TRY(hipMemcpy(&v, e->cur.ungrouped.get(), sizeof v, hipMemcpyDeviceToHost));
  return v > 2147483647u ? 2147483647 : (int)v;
}

int cosim_query(const cosim_engine_t* e, const char* name) {
  if (!e || !name) return fail(COSIM_EINVAL, "cosim_query: null argument");
  std::string n(name);
  if (n == "state_dim") return e->ho.state_dim;
  if (n == "action_dim") return e->model.nu;
  if (n == "command_dim") return e->ho.command_dim;
  if (n == "info_dim") return e->ho.info_dim;
  if (n == "nq") return e->model.nq;
  if (n == "nv") return e->model.nv;
  if (n == "nbody") return e->model.nbody;
  if (n == "ngeom") return e->model.ngeom;
  if (n == "n_envs") return e->n_envs;
  if (n == "state_stride") return e->lay.s_stride;
  if (n == "param_stride") return e->lay.p_stride;
  if (n == "lds_bytes") return e->plan.lds_bytes;
  if (n == "contact_slots") return e->plan.contact_slots;
  if (n == "fixup_contact_slots") return e->plan.fixup_contact_slots;   // 0: no large-capacity kernel behind this one
  if (n == "ranges") return e->n_ranges;
  if (n == "range_streams") return e->n_streams;   // P: engine-owned streams (launch sequences per step) that carry the ranges
  if (n == "step_kernel") return e->plan.step_kernel;   // 1: steps run the step-only instantiation of the fleet kernel
  if (n == "rollout") return has(e->plan.rollout);      // 1: cosim_rollout is available for this model / terrain
  if (n == "split") return e->plan.split * e->narrow_waves;   // waves per env of the narrowphase kernel; 0: fused kernel
  if (n == "pair_slots") return e->plan.pair_slots;
  if (n == "stacked_dim") return e->ho.stacked_dim;
  if (n == "frame_dim") return e->ho.frame_dim;
  if (n == "max_newton") return newton_cap(e);   // Newton iterations per substep the solver may take
  if (n == "max_ls") return ls_cap(e);           // line-search evaluations per Newton iteration
  if (n == "frame_skip") return e->model.frame_skip;
  if (n == "spawn_rows") return e->spawn.rows;   // rows of the spawn table (0: none, resets go to init_qpos)
  if (n == "spawn_mode") return e->spawn.mode;   // 0: row = global env id mod rows; 1: drawn per episode
  if (n == "snapshot_floats") return e->lay.s_stride + e->lay.p_stride;   // float32 words of a snapshot row: state record + parameter record
  if (n == "history_slots") return e->hist.slots;
  if (n == "history_every") return e->hist.every;
  if (n == "ledger_slots") return e->led.slots;   // records per env the episode ledger keeps (0: no ledger, no ledger launches)
  if (n == "ftrace_frames") return e->ft.frames;  // frames per failure-trace window (0: no traces, no trace launches)
  if (n == "ftrace_keep") return e->ft.keep;      // traces kept per env
  if (n == "ftrace_frame_words") return ftrace_words(e);   // F: 32-bit words of a frame for this model (answered with traces off too)
  if (n == "ftrace_mask") return e->ft.mask;      // ledger flags that freeze a window
  if (n == "scenario_rows") return e->scn.tab.n_scn;  // scenarios of the table (0: none, no scenario launches)
  if (n == "scenario_param_items") return e->par.tab.n_items;   // expanded parameter-window items of the table (0: none, no launches)
  if (n == "obs_faults") return e->obsflt.tab.n_items;   // expanded observation-fault items of the table (0: none, no launches)
  if (n == "launches") return (int)(g_launches.load(std::memory_order_relaxed) & 0x7fffffffu);   // kernel launches the engines of this process have issued through launch_k / launch_small, modulo 2^31 (a capture counts what it records, a replay nothing)
  if (n == "device_buffers") return g_device_buffers.load(std::memory_order_relaxed);   // device allocations of this library that are live in this process, every engine and table together: equal before and after means nothing leaked
  if (n == "latency") return e->lat.tab.n_act + e->lat.tab.n_obs;   // expanded latency items of the table, both kinds (0: none, no launches, no pointer changes)
  if (n == "latency_action_items") return e->lat.tab.n_act;     // ... of the command channel
  if (n == "latency_obs_items") return e->lat.tab.n_obs;        // ... of observation elements
  if (n == "latency_depth") return e->lat.tab.depth;            // D: clocks a line holds (0: none)
  if (n == "action_faults") return e->actflt.tab.n_items;   // expanded action-fault items of the table (0: none, no launches, the caller's action pointer)
  if (n == "scenario_check_items") return e->chk.tab.n_scn > 0 ? e->chk.tab.I : 0;   // I: items per env a verdict record holds (0: no checks, no launches)
  if (n == "scenario_check_slots") return e->chk.slots;                      // verdict records per env
  if (n == "scenario_curve_items") return e->cur.tab.n_items;   // curve items of the table (0: no curves, no launches)
  if (n == "scenario_curve_words") return (int)e->cur.words;   // 32-bit words of all cells (at most 2^26)
  if (n == "scenario_curve_groups") return e->cur.groups;   // G of cosim_scenario_curves_groups (0: no groups)
  if (n == "scenario_curve_ungrouped") return curves_ungrouped(const_cast<cosim_engine_t*>(e));   // synchronising: joins, reads one device word
  if (n == "scenario_curve_stage_words") return e->cur.tab.n_scn > 0 ? e->cur.tab.SW : 0;   // stage words per env
  if (n == "scenario_check_words") return e->chk.tab.n_scn > 0 ? checks_words(e->chk.tab.I) : 0;   // 32-bit words of a verdict record: 8 + 2 I
  if (n == "search") return e->srch.tab.n_items;      // scenarios of the table with a search item armed (0: no search, no launches, scenario_step_kernel)
  if (n == "search_slots") return e->srch.slots;  // trial records per env
  if (n == "search_targets") return e->srch.tab.n_items > 0 ? e->srch.kinds : 0;   // union of the armed items' targets (16: actfault_search_step_kernel in the place of actfault_step_kernel)
  if (n == "search_checks") return e->srch.tab.n_items > 0 && e->srch.on_check;          // an armed item fails on a check (search_step_checks_kernel in the place of search_step_kernel)
  if (n == "action_faults_marked") return e->actflt.marked;                     // action-fault items the search scales
  if (n == "obs_faults_marked") return e->obsflt.marked;                        // observation-fault items the search scales
  if (n == "scenario_param_items_marked") return e->par.marked;              // parameter items the search scales
  if (n == "search_remaining") return search_remaining(const_cast<cosim_engine_t*>(e));   // synchronising: joins, reads one device word
  if (n == "scenario_mode") return e->scn.tab.mode;   // 0: row = global env id mod rows; 1: advanced by one per episode of the env
  if (n == "fall") return e->fall_mask;           // fall rules in force (cosim_fall_set): 1 tilt | 2 height | 4 body contact; 0: none
  return fail(COSIM_EINVAL, "cosim_query: unknown name " + n);
}

static int obsfault_set(cosim_engine* e, const int32_t* words, int count);   // (below, with the other tables of the scenario family)
static int actfault_set(cosim_engine* e, const int32_t* words, int count);
static int search_set(cosim_engine* e, const int32_t* words, int count);
static int latency_set(cosim_engine* e, const int32_t* words, int count);

int cosim_set_param(cosim_engine_t* e, const char* name, const float* host, int count) {
  if (!e || !name || !host) return fail(COSIM_EINVAL, "cosim_set_param: null argument");
  std::string n(name);
  const cosim_model_t& m = e->model;
  const Layout& L = e->lay;
  int off, width;
  if (n == "body_mass") { off = L.p_mass; width = m.nbody; }
  else if (n == "body_invweight0") { off = L.p_binvw; width = m.nbody; }
  else if (n == "dof_invweight0") { off = L.p_dinvw; width = m.nv; }
  else if (n == "dof_frictionloss") { off = L.p_floss; width = m.nv; }
  else if (n == "geom_friction") { off = L.p_gmu; width = m.ngeom; }
  else if (n == "kp") { off = L.p_kp; width = m.nu; }
  else if (n == "kd") { off = L.p_kd; width = m.nu; }
  else if (n == "meaninertia") { off = L.p_mean; width = 1; }
  else if (n == "obs_faults") return obsfault_set(e, reinterpret_cast<const int32_t*>(host), count);   // a table of 32-bit words, not floats (include/cosim.h)
  else if (n == "action_faults") return actfault_set(e, reinterpret_cast<const int32_t*>(host), count);   // likewise
  else if (n == "search") return search_set(e, reinterpret_cast<const int32_t*>(host), count);   // likewise
  else if (n == "latency") return latency_set(e, reinterpret_cast<const int32_t*>(host), count);   // likewise
  else if (n == "solver_tolerance") { e->tol32 = host[0]; return COSIM_OK; }
  else if (n == "ls_tolerance_scale") { e->ls_scale = host[0]; return COSIM_OK; }
  else if (n == "max_newton") { e->max_newton = (int)host[0]; return COSIM_OK; }
  else if (n == "max_ls") { e->max_ls = (int)host[0]; return COSIM_OK; }
  else if (n == "wave_priority") {   // [usual Newton iterations per substep, lag thresholds of priority 1, 2, 3]; a huge first threshold switches it off
    if (count != 4) return fail(COSIM_EINVAL, "cosim_set_param: wave_priority takes 4 values");
    for (int k = 0; k < 4; k++) e->prio[k] = (int)host[k];
    return COSIM_OK;
  }
  else if (n == "debug_substeps") { e->nsub_override = (int)host[0]; return COSIM_OK; }
  else if (n == "ranges") return set_ranges(e, (int)host[0]);
  else if (n == "range_streams") {   // streams that carry the ranges: >= 1 asks for that many (at most one per range), 0: by the hardware queues
    const int v = (int)host[0];
    if (v < 0 || v > 16) return fail(COSIM_EINVAL, "cosim_set_param: range_streams must be 0..16 (0: as many as the hardware queues carry)");
    e->range_streams_req = v;
    return set_ranges(e, e->n_ranges);
  }
  else if (n == "deferred_join") {   // 1: cosim_step leaves the join of the range streams to cosim_join (or to the next call that touches the state)
    e->deferred_join = (int)host[0] != 0;
    return COSIM_OK;
  }
  else if (n == "inflight") {   // control steps the host may run ahead of each range stream (0: unbounded)
    const int v = (int)host[0];
    if (v < 0 || v > 1024) return fail(COSIM_EINVAL, "cosim_set_param: inflight must be 0..1024");
    e->inflight = v;
    return set_ranges(e, e->n_ranges);
  }
  else if (n == "narrow_waves") {   // waves per env of the narrowphase kernel (wave w takes the geoms g % waves == w)
    const int v = (int)host[0];
    if (v < 1 || v > 24) return fail(COSIM_EINVAL, "cosim_set_param: narrow_waves must be 1..24");
    e->narrow_waves = v;
    return COSIM_OK;
  }
  else if (n == "support_map") {   // 0: mesh support queries scan the whole hull (A/B and tests); 1: through the support maps (default)
    HIP_TRY(hipDeviceSynchronize());
    for (int g = 0; g < 64; g++) e->hm.g_hullmap[g] = (int)host[0] != 0 ? e->hullmap_of_geom[g] : -1;
    HIP_TRY(hipMemcpy(e->d_model.get(), &e->hm, sizeof(DevModel), hipMemcpyHostToDevice));
    return COSIM_OK;
  }
  else if (is_switch(n)) {   // "split", "narrow_occupancy", "step_kernel", "fixup", "hfield_fixup", "contact_twist", "envs_per_wave": DESIGN 4.17
    if (const char* refused = switch_set(e->kernels, e->sw, n, (int)host[0], e->n_envs)) return fail(COSIM_EINVAL, refused);
    e->plan = make_plan(e->kernels, e->sw);
    // two envs per wave: even range sizes (kept: "contact_twist" 1 under two envs per wave goes back to one without splitting again)
    return n == "envs_per_wave" && e->n_ranges > 1 ? set_ranges(e, e->n_ranges) : COSIM_OK;
  }
  else if (n == "timing_stride") { e->timing_stride = (int)host[0] >= 1 ? (int)host[0] : 1; return COSIM_OK; }   // time every n-th launch
  else if (n == "coop_walk") { e->coop_walk = (int)host[0] != 0; return COSIM_OK; }   // 1: the round-2 cooperative walk of hulls with few prisms under them (A/B)
  else if (n == "block_cull") { e->block_cull = (int)host[0] != 0; return COSIM_OK; }   // narrowphase kernel's block tests (default 1); 0 for A/B runs and tests
  else if (n == "boxbox_mode") { e->pair_boxbox = (int)host[0] != 0; return COSIM_OK; }   // 1: box-box pairs through mjc_BoxBox (default), 0: through MPR
  else if (n == "pair_mode") { e->pair_coop = (int)host[0] != 0; return COSIM_OK; }   // 1: hull pairs one at a time, wave-cooperative scans
  else return fail(COSIM_EINVAL, "cosim_set_param: unknown parameter " + n);
  if (count != e->n_envs * width) return fail(COSIM_EINVAL, "cosim_set_param: " + n + " expects n_envs*" + std::to_string(width) + " values");
  int rc = refresh_param_mirror(e);
  if (rc) return rc;
  for (int i = 0; i < e->n_envs; i++)
    memcpy(e->h_params.data() + (size_t)i * L.p_stride + off, host + (size_t)i * width, width * sizeof(float));
  e->params_dirty = true;
  return COSIM_OK;
}

static int drain_events(cosim_engine* e) {
  for (int i = 0; i + 1 < e->ev_used; i += 2) {
    HIP_TRY(hipEventSynchronize(e->ev[i + 1]));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, e->ev[i], e->ev[i + 1]));
    e->t_accum_ms += ms;
    e->t_launches++;
  }
  e->ev_used = 0;
  return COSIM_OK;
}

static KArgs base_args(cosim_engine* e) {
  KArgs a;
  memset(&a, 0, sizeof a);
  a.dm = e->d_model.get(); a.ob = e->d_obs.get(); a.lay = e->lay; a.state = e->d_state.get();
  a.params = e->par.tab.n_items > 0 ? e->par.eff.get() : e->d_params.get();   // parameter windows: the effective records (cosim_scnparams.hip)
  a.hull_vert = e->d_hull_vert.get(); a.hull_adr = e->d_hull_adr.get(); a.hull_nbr = e->d_hull_nbr.get(); a.hfield = e->d_hfield.get();
  a.hull_cell = e->d_hull_cell.get(); a.hull_cand = e->d_hull_cand.get(); a.hfield_mip = e->d_hfield_mip.get();
  a.pairs = e->d_pairs.get(); a.gext = e->d_gext.get();
  a.n_envs = e->n_envs; a.seed_lo = (unsigned)e->seed; a.seed_hi = (unsigned)(e->seed >> 32); a.env_id0 = e->env_id0;
  a.tol32 = e->tol32; a.ls_scale = e->ls_scale; a.max_newton = newton_cap(e); a.max_ls = ls_cap(e); a.nsub_override = e->nsub_override; a.pair_coop = e->pair_coop; a.pair_boxbox = e->pair_boxbox; a.block_cull = e->block_cull; a.coop_walk = e->coop_walk;
  for (int k = 0; k < 4; k++) a.prio[k] = e->prio[k];
  a.ovf = nullptr; a.roll_steps = 1;
  a.spawn = e->spawn.table.get(); a.spawn_rows = e->spawn.rows; a.spawn_mode = e->spawn.mode;
  a.spawn_off = e->spawn.rows > 0 ? (unsigned)(((e->env_id0 % e->spawn.rows) + e->spawn.rows) % e->spawn.rows) : 0u;
  a.xcon = e->d_xcon.get(); a.xcnt = e->d_xcnt.get(); a.xstate = e->d_xstate.get(); a.nw = e->narrow_waves; a.sub_index = 0; a.sub_total = 0;
  a.fall_min_up = e->fall_min_up; a.fall_min_height = e->fall_min_height; a.fall_grace = e->fall_grace; a.fall_mask = e->fall_mask;
  return a;
}

int cosim_reset(cosim_engine_t* e, const uint8_t* mask_dev, const float* commands_dev, float* state_out_dev, void* stream) {
  if (!e || !state_out_dev) return fail(COSIM_EINVAL, "cosim_reset: null argument");
  HIP_TRY(hipSetDevice(e->device));
  RC_TRY(upload_params(e));
  RC_TRY(join_ranges(e, (hipStream_t)stream));
  if (e->scn.tab.n_scn > 0) {   // the reset's state vector carries the scenario's first command
    if (e->ho.command_dim > 0 && !commands_dev)
      return fail(COSIM_EINVAL, "cosim_reset: a scenario table is set (cosim_scenario_set) and commands_dev is NULL: the scenario kernel passes the caller's command through where a scenario has no keyframe yet");
    RC_TRY(scenario_launch(e, 0, e->n_envs, commands_dev, mask_dev, 1, (hipStream_t)stream));
    if (e->par.tab.n_items > 0) RC_TRY(scnparams_launch(e, 0, e->n_envs, mask_dev, 1, (hipStream_t)stream));
  }
  KArgs a = base_args(e);
  a.mode = MODE_RESET; a.mask = mask_dev; a.commands = scenario_cmd(e, commands_dev); a.state_out = state_out_dev;
  e->plan.reset.launch(e, a, e->n_envs, (hipStream_t)stream);
  HIP_TRY(hipGetLastError());
  if (e->lat.tab.n_obs > 0) RC_TRY(latency_obs_launch(e, 0, e->n_envs, state_out_dev, mask_dev, (hipStream_t)stream));   // clock 0: the line restarts with the first reading
  if (e->obsflt.tab.n_items > 0) RC_TRY(obsfault_launch(e, 0, e->n_envs, state_out_dev, mask_dev, (hipStream_t)stream));   // the reset's observation is a fill at clock 0
  if (mask_dev == nullptr) e->stepped = false;
  return observers_begin(e, mask_dev, nullptr, 0, 0, (hipStream_t)stream);
}

int cosim_step(cosim_engine_t* e, const float* actions_dev, const float* commands_dev, float* state_out_dev, uint8_t* terminated_dev,
               uint8_t* truncated_dev, float* info_out_dev, void* stream) {
  if (!e) return fail(COSIM_EINVAL, "cosim_step: null argument");
  if (e->n_ranges <= 1) {   // one launch on the caller's stream, paced like the range launches below
    HIP_TRY(hipSetDevice(e->device));
    hipStreamCaptureStatus cap1 = hipStreamCaptureStatusNone;
    HIP_TRY(hipStreamIsCapturing((hipStream_t)stream, &cap1));
    if (e->hist.slots > 0 && cap1 != hipStreamCaptureStatusNone) return fail(COSIM_EINVAL, HIST_CAPTURE_MSG);
    const bool paced = e->inflight > 0 && cap1 == hipStreamCaptureStatusNone && (int)e->ring.size() >= e->inflight;
    if (paced && e->ring_pos >= e->inflight) HIP_TRY(hipEventSynchronize(e->ring[e->ring_pos % e->inflight]));
    int rc = cosim_step_range(e, 0, e->n_envs, actions_dev, commands_dev, state_out_dev, terminated_dev, truncated_dev, info_out_dev, stream);
    if (rc) return rc;
    if (history_due(e)) { rc = history_pack(e, 0, e->n_envs, (hipStream_t)stream); if (rc) return rc; }
    history_count(e);
    if (paced) { HIP_TRY(hipEventRecord(e->ring[e->ring_pos % e->inflight], (hipStream_t)stream)); e->ring_pos++; }
    return COSIM_OK;
  }
  // fork: the range streams wait for whatever the caller's stream has been given so far (the step's inputs), then each steps its
  // group of ranges as one launch sequence over their union; join: the caller's stream waits for every range -- now, or (deferred_join) at the next cosim_join / state access, which
  // is what lets a range's next control step overlap the tail of the others' current one
  HIP_TRY(hipSetDevice(e->device));
  hipStream_t cs = (hipStream_t)stream;
  // The inputs are ready once everything given to the caller's stream so far has run.  If that stream is idle they are ready now, and
  // the range streams need no wait: a cross-queue wait is a barrier packet ahead of every range launch (measured: 12.6 -> 11.0 M with
  // an idle caller stream).  Not while capturing: a query is illegal there, and the fork edge is what ties the range streams in.
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  HIP_TRY(hipStreamIsCapturing(cs, &cap));
  if (e->hist.slots > 0 && cap != hipStreamCaptureStatusNone) return fail(COSIM_EINVAL, HIST_CAPTURE_MSG);
  bool wait_in = true;
  if (cap == hipStreamCaptureStatusNone) {
    const hipError_t q = hipStreamQuery(cs);
    if (q == hipSuccess) wait_in = false;
    else if (q != hipErrorNotReady) return fail(COSIM_EHIP, std::string("hipStreamQuery: ") + hipGetErrorString(q));
    (void)hipGetLastError();   // hipErrorNotReady is sticky in hipGetLastError
  }
  if (wait_in) HIP_TRY(hipEventRecord(e->ev_in, cs));
  for (int i = 0; i < e->n_streams; i++) {
    if (wait_in) HIP_TRY(hipStreamWaitEvent(e->rstream[i], e->ev_in, 0));
    // (not while capturing: a captured step is replayed, the host does not pace it)
    const bool paced = e->inflight > 0 && cap == hipStreamCaptureStatusNone;
    if (paced && e->ring_pos >= e->inflight)   // the step `inflight` steps back has left this stream
      HIP_TRY(hipEventSynchronize(e->ring[(size_t)i * e->inflight + e->ring_pos % e->inflight]));
    int rc = cosim_step_range(e, e->gfirst[i], e->gcount[i], actions_dev, commands_dev, state_out_dev, terminated_dev, truncated_dev, info_out_dev,
                              e->rstream[i]);
    if (rc) return rc;
    // history capture: the group's rows on the group's own stream, behind its last launch of the step; no join, no extra event
    if (history_due(e)) { rc = history_pack(e, e->gfirst[i], e->gcount[i], e->rstream[i]); if (rc) return rc; }
    if (paced) HIP_TRY(hipEventRecord(e->ring[(size_t)i * e->inflight + e->ring_pos % e->inflight], e->rstream[i]));
  }
  history_count(e);
  if (e->inflight > 0 && cap == hipStreamCaptureStatusNone) e->ring_pos++;
  e->join_pending = true;
  if (!e->deferred_join) return join_ranges(e, cs);
  return COSIM_OK;
}

// The reference's loop with an action table (core/tester.py:66-97 with policy.get_action replaced by a lookup): `steps` control steps
// in ONE launch per range; row k of the [steps][N][...] buffers is what cosim_step would have been given / would have returned at
// step k.  Returns with the caller's stream waiting for everything (eager join).
int cosim_rollout(cosim_engine_t* e, int steps, const float* actions_dev, const float* commands_dev, float* state_out_dev, uint8_t* terminated_dev,
                  uint8_t* truncated_dev, float* info_out_dev, void* stream) {
  if (!e || !actions_dev || !state_out_dev || !terminated_dev || !truncated_dev || steps < 1) return fail(COSIM_EINVAL, "cosim_rollout: bad argument");
  const Plan<launch_fn>& p = e->plan;
  if (!has(p.rollout)) return fail(COSIM_EINVAL, "cosim_rollout: no rollout kernel for this model / terrain / kernel variant");
  if (e->ho.command_dim > 0 && !commands_dev) return fail(COSIM_EINVAL, "cosim_rollout: commands_dev is required when command_dim > 0");
  if (e->led.slots > 0 && !info_out_dev) return fail(COSIM_EINVAL, std::string("cosim_rollout") + LEDGER_INFO_MSG);
  if (e->ft.frames > 0)
    return fail(COSIM_EINVAL, "cosim_rollout: failure traces are set (cosim_ftrace_set): one launch leaves one state record for all its steps, so the per-step state is not there to copy; step with cosim_step or switch the traces off");
  if (e->lat.tab.n_act + e->lat.tab.n_obs > 0)
    return fail(COSIM_EINVAL, "cosim_rollout: latency is set (cosim_set_param \"latency\"): one launch takes all its steps and the delay lines are written between steps; step with cosim_step or clear the latency");
  if (e->scn.tab.n_scn > 0)
    return fail(COSIM_EINVAL, "cosim_rollout: a scenario table is set (cosim_scenario_set): one launch reads one command row; step with cosim_step or clear the table");
  e->stepped = true;
  HIP_TRY(hipSetDevice(e->device));
  RC_TRY(upload_params(e));
  hipStream_t cs = (hipStream_t)stream;
  RC_TRY(join_ranges(e, cs));
  KArgs a = base_args(e);
  a.mode = MODE_STEP; a.actions = actions_dev; a.commands = commands_dev; a.state_out = state_out_dev;
  a.terminated = terminated_dev; a.truncated = truncated_dev; a.info = info_out_dev; a.roll_steps = steps;
  a.ovf = has(p.rollout_fix) ? e->d_ovf.get() : nullptr;
  const int nr = e->n_ranges > 1 ? e->n_streams : 1;   // launch sequences: one per group of ranges
  if (e->n_ranges > 1) HIP_TRY(hipEventRecord(e->ev_in, cs));
  for (int i = 0; i < nr; i++) {
    hipStream_t s = e->n_ranges > 1 ? e->rstream[i] : cs;
    if (e->n_ranges > 1) HIP_TRY(hipStreamWaitEvent(s, e->ev_in, 0));
    a.env_first = e->n_ranges > 1 ? e->gfirst[i] : 0;
    a.env_count = e->n_ranges > 1 ? e->gcount[i] : e->n_envs;
    int slot = -1;
    if (e->timing && e->ev_used + 2 <= (int)e->ev.size()) { slot = e->ev_used; e->ev_used += 2; HIP_TRY(hipEventRecord(e->ev[slot], s)); }
    p.rollout.launch(e, a, a.env_count, s);
    HIP_TRY(hipGetLastError());
    if (slot >= 0) HIP_TRY(hipEventRecord(e->ev[slot + 1], s));
    if (a.ovf) { p.rollout_fix.launch(e, a, a.env_count, s); HIP_TRY(hipGetLastError()); }
    RC_TRY(observers_step(e, a.env_first, a.env_count, steps, actions_dev, commands_dev, info_out_dev, terminated_dev, truncated_dev, s));
  }
  if (e->n_ranges > 1) { e->join_pending = true; return join_ranges(e, cs); }
  return COSIM_OK;
}

// Test hook, host only (no GPU call): the support map of ONE hull (cosim_hullmap.h) against the full scan it replaces, with the
// kernels' fp32 comparisons: for each of `ndir` directions (hull frame) the arg-max vertex through the map -> out_map_idx and by
// scanning all n vertices -> out_scan_idx.  out_stats: [0] candidates in the table, [1] largest cell, [2] cells.
int cosim_hull_support_check(const float* verts, int n, const int* adr, const int* nbr, const float* dirs, int ndir, int* out_map_idx,
                             int* out_scan_idx, int* out_stats) {
  if (!verts || !adr || !nbr || !dirs || !out_map_idx || !out_scan_idx || n < 1 || ndir < 0) return fail(COSIM_EINVAL, "cosim_hull_support_check: bad argument");
  std::vector<float> cells, cand;
  build_support_map(verts, n, adr, nbr, cells, cand);
  auto as_int = [](float f) { union { int i; float f; } u; u.f = f; return u.i; };
  int biggest = 0, total = 0;
  for (int c = 0; c < HM_CELLS; c++) { const int k = as_int(cells[4 * (size_t)HM_REC * c]); biggest = k > biggest ? k : biggest; total += k; }
  if (out_stats) { out_stats[0] = total; out_stats[1] = biggest; out_stats[2] = HM_CELLS; }
  for (int d = 0; d < ndir; d++) {
    const float* l = dirs + 3 * (size_t)d;
    float best = -3.0e38f;
    int bi = 0;
    for (int i = 0; i < n; i++) {
      const float t = l[0] * verts[3 * i] + l[1] * verts[3 * i + 1] + l[2] * verts[3 * i + 2];
      if (t > best) { best = t; bi = i; }
    }
    out_scan_idx[d] = bi;
    const float* rec = &cells[4 * (size_t)HM_REC * support_cell(l)];
    const int count = as_int(rec[0]), ovf = as_int(rec[1]);
    best = -3.0e38f;
    union { int i; float f; } ix;
    ix.f = rec[4 + 3];
    for (int i = 0; i < count; i++) {
      const float* x = i < HM_INLINE ? rec + 4 * (1 + i) : &cand[4 * (size_t)(ovf + i - HM_INLINE)];
      const float t = l[0] * x[0] + l[1] * x[1] + l[2] * x[2];
      if (t > best) { best = t; ix.f = x[3]; }
    }
    out_map_idx[d] = ix.i;
  }
  return COSIM_OK;
}

int cosim_join(cosim_engine_t* e, void* stream) {
  if (!e) return fail(COSIM_EINVAL, "cosim_join: null engine");
  HIP_TRY(hipSetDevice(e->device));
  return join_ranges(e, (hipStream_t)stream);
}

int cosim_range(const cosim_engine_t* e, int i, int* first, int* count, void** stream) {
  if (!e || i < 0 || i >= e->n_ranges) return fail(COSIM_EINVAL, "cosim_range: bad argument");
  if (first) *first = e->n_ranges > 1 ? e->rfirst[i] : 0;
  if (count) *count = e->n_ranges > 1 ? e->rcount[i] : e->n_envs;
  if (stream) *stream = e->n_ranges > 1 ? (void*)e->rstream[e->rgroup[i]] : nullptr;   // ranges of one group report the same stream
  return COSIM_OK;
}

// After something was enqueued on range stream i from outside (a per-range policy, a reporter reduction): re-arm the range's "done"
// event so that a later join also waits for that work.
int cosim_range_mark(cosim_engine_t* e, int i) {
  if (!e || i < 0 || i >= e->n_ranges || e->n_ranges <= 1) return fail(COSIM_EINVAL, "cosim_range_mark: bad argument");
  e->join_pending = true;   // (the "done" events are recorded at join time: everything on the range stream by then is covered)
  return COSIM_OK;
}

int cosim_step_range(cosim_engine_t* e, int first, int count, const float* actions_dev, const float* commands_dev, float* state_out_dev,
                     uint8_t* terminated_dev, uint8_t* truncated_dev, float* info_out_dev, void* stream) {
  if (!e || !actions_dev || !state_out_dev || !terminated_dev || !truncated_dev) return fail(COSIM_EINVAL, "cosim_step: null argument");
  if (e->ho.command_dim > 0 && !commands_dev) return fail(COSIM_EINVAL, "cosim_step: commands_dev is required when command_dim > 0");
  if (first < 0 || count < 1 || first + count > e->n_envs) return fail(COSIM_EINVAL, "cosim_step_range: range outside the fleet");
  if (e->sw.epw == 2 && ((first | count) & 1)) return fail(COSIM_EINVAL, "cosim_step_range: two-environments-per-wave kernel needs even ranges");
  if (!info_out_dev && observers_info_msg(e)) return fail(COSIM_EINVAL, std::string("cosim_step") + observers_info_msg(e));
  e->stepped = true;
  HIP_TRY(hipSetDevice(e->device));
  RC_TRY(upload_params(e));
  KArgs a = base_args(e);
  a.mode = MODE_STEP; a.actions = actions_dev; a.commands = scenario_cmd(e, commands_dev); a.state_out = state_out_dev;
  a.terminated = terminated_dev; a.truncated = truncated_dev; a.info = info_out_dev;
  a.env_first = first; a.env_count = count;
  const Plan<launch_fn>& p = e->plan;
  if (p.narrow_diag) a.dbg = e->d_dbg.get();   // diagnostic narrowphase build accumulates its counters there
  // the fix-up behind this launch: the split pipeline's after each solver launch ("hfield_fixup"), else the one after the fleet kernel
  a.ovf = has(p.fixup) ? e->d_ovf.get() : nullptr;
  hipStream_t s = (hipStream_t)stream;
  // kernel timing: one HIP event pair per launch on the launch stream, read back in cosim_kernel_time() (no sync here)
  int slot = -1;
  if (e->timing && (e->launch_seq++ % (unsigned)e->timing_stride) == 0) {
    if (e->ev_used + 2 > (int)e->ev.size()) {
      if (e->ev.size() >= 4096) { int rc2 = drain_events(e); if (rc2) return rc2; }
      else for (int i = 0; i < 2; i++) { hipEvent_t x; HIP_TRY(hipEventCreate(&x)); e->ev.push_back(x); }
    }
    slot = e->ev_used;
    e->ev_used += 2;
    HIP_TRY(hipEventRecord(e->ev[slot], s));
  }
  // scenario table: this step's command and push of every env of the range, ahead of the step's first launch (plain device work:
  // capturable); inside the timing pair, so cosim_kernel_time() includes it
  if (e->scn.tab.n_scn > 0) RC_TRY(scenario_launch(e, first, count, commands_dev, nullptr, 0, s));
  // parameter windows: this step's effective parameter records of the range, ahead of every launch that reads them (the substep
  // launches of the split pipeline and the fix-up kernels' redo included: all are handed the same pointer by base_args)
  if (e->par.tab.n_items > 0) RC_TRY(scnparams_launch(e, first, count, nullptr, 0, s));
  // action faults: this step's effective actions of the range, ahead of every launch that reads the action (the fused and step-only
  // kernels, the two-envs-per-wave kernel, the split pipeline's first substep and the fix-up kernels' redo: all read a.actions)
  // latency comes first: the delivered action is what the action faults take as the caller's word; with latency alone the step
  // kernels read the delivered rows themselves
  const bool act_faults = e->actflt.tab.n_items > 0, act_lat = e->lat.tab.n_act > 0;
  if (act_lat) {
    RC_TRY(latency_act_launch(e, first, count, actions_dev, s));
    a.actions = e->act.eff.get();
  }
  if (act_faults) {
    RC_TRY(actfault_launch(e, first, count, act_lat ? e->lat.eff.get() : actions_dev, act_lat ? e->lat.spare.get() : e->act.raw.get(), s));
    a.actions = e->act.eff.get();
  }
  if (p.split) {
    // one pair of launches per substep: the prism walk (narrow_waves waves per env), then the solver with the contacts it left; with
    // "hfield_fixup", the substeps the solver gave up (more ground contacts than its slots) are redone right behind it from the same
    // record.  The narrowphase kernel never flags: it is given no ovf.
    KArgs an = a;
    an.ovf = nullptr;
    const int fs = e->nsub_override > 0 ? e->nsub_override : e->model.frame_skip;
    for (int sub = 0; sub < fs; sub++) {
      a.sub_index = sub; a.sub_total = fs; an.sub_index = sub; an.sub_total = fs;
      p.narrow.launch(e, an, count * e->narrow_waves, s);
      p.step.launch(e, a, count, s);
      if (a.ovf) p.fixup.launch(e, a, count, s);
    }
  } else p.step.launch(e, a, count, s);
  HIP_TRY(hipGetLastError());
  const bool faults = e->obsflt.tab.n_items > 0;   // observation faults: the timing pair closes behind their launch
  if (slot >= 0 && !faults) HIP_TRY(hipEventRecord(e->ev[slot + 1], s));
  if (a.ovf && !p.split) {   // envs the fleet kernel flagged (more contacts than it has slots for) are redone by the large-capacity kernel
    p.fixup.launch(e, a, count, s);
    HIP_TRY(hipGetLastError());
  }
  // observation faults: behind the last launch that writes the range's state records or state_out (the redo included: a redone env's
  // observation is faulted once), ahead of the observers and the history pack, which then hold what the policy saw
  // action faults: last_action is what the policy put out, not what the bus delivered; the observation faults compose on top
  if ((act_faults || act_lat) && e->act_in_obs) RC_TRY(actfault_obs_launch(e, first, count, state_out_dev, s));
  // latency of observation elements: on the newest frame as the step (and the restore above) left it, ahead of the observation faults
  if (e->lat.tab.n_obs > 0) RC_TRY(latency_obs_launch(e, first, count, state_out_dev, nullptr, s));
  // While a search scales observation faults the launch goes BEHIND the observers: the observation a step that ended an episode
  // returns is clock 0 of the next one and takes the level search_step_kernel has just moved.  No observer reads what the fault kernel
  // writes (stack row 0 of the record, state_out): they read the info row, the flags, the command, qpos / qvel and the meta words, so
  // the two orders give the observers the same words.  The history pack stays behind both (the caller issues it after this returns).
  // The timing pair closes behind the fault launch in either order, so in the moved order a timed launch's span also holds the
  // observers' kernels (ledger, traces, checks, curves, search), which it does not hold otherwise: kernel_ms of such a run is not
  // comparable with one of the plain order.
  const bool faults_last = faults && obsfault_searched(e);
  if (faults && !faults_last) {
    RC_TRY(obsfault_launch(e, first, count, state_out_dev, nullptr, s));
    if (slot >= 0) HIP_TRY(hipEventRecord(e->ev[slot + 1], s));
  }
  RC_TRY(observers_step(e, first, count, 1, actions_dev, scenario_cmd(e, commands_dev), info_out_dev, terminated_dev, truncated_dev, s));
  if (faults_last) {
    RC_TRY(obsfault_launch(e, first, count, state_out_dev, nullptr, s));
    if (slot >= 0) HIP_TRY(hipEventRecord(e->ev[slot + 1], s));
  }
  return COSIM_OK;
}

// Spawn table: validate on the host (a message that names the row), upload, place every row on the heightfield with
// spawn_place_kernel, keep the [rows][8] table on the device and a copy on the host.  Blocks until the table is placed (cold path).
int cosim_spawn_set(cosim_engine_t* e, const float* xyyaw_host, int rows, const float* footprint_host, int n_foot, float clearance,
                    int per_episode, void* stream) {
  if (!e || rows < 0 || rows > (1 << 24)) return fail(COSIM_EINVAL, "cosim_spawn_set: null engine or rows outside 0..2^24");
  HIP_TRY(hipSetDevice(e->device));
  hipStream_t cs = (hipStream_t)stream;
  { int rc = join_ranges(e, cs); if (rc) return rc; }
  if (rows == 0) {   // clear: resets go back to init_qpos (launches already enqueued keep the table they were given)
    HIP_TRY(hipStreamSynchronize(cs));
    e->spawn = {};
    return COSIM_OK;
  }
  const cosim_model_t& m = e->model;
  const bool hf = m.ground_type == CS_GEOM_HFIELD;
  if (!xyyaw_host || n_foot < 0 || n_foot > 64 || (n_foot > 0 && !footprint_host)) return fail(COSIM_EINVAL, "cosim_spawn_set: bad argument");
  if (!(clearance >= 0.f) || !std::isfinite(clearance)) return fail(COSIM_EINVAL, "cosim_spawn_set: clearance must be finite and >= 0");
  if (hf && (long long)m.hfield_nrow * m.hfield_ncol > 0x7fffffffLL) return fail(COSIM_EINVAL, "cosim_spawn_set: heightfield too large");
  for (int g = 0; g < 4 * n_foot; g++)
    if (!std::isfinite(footprint_host[g])) return fail(COSIM_EINVAL, "cosim_spawn_set: non-finite footprint entry");
  for (int g = 0; g < n_foot; g++)
    if (footprint_host[4 * g + 2] < 0.f || footprint_host[4 * g + 3] < 0.f) return fail(COSIM_EINVAL, "cosim_spawn_set: footprint radius / free height must be >= 0");
  for (int r = 0; r < rows; r++) {
    const float x = xyyaw_host[3 * (size_t)r], y = xyyaw_host[3 * (size_t)r + 1], yaw = xyyaw_host[3 * (size_t)r + 2];
    if (!std::isfinite(x) || !std::isfinite(y) || !std::isfinite(yaw))
      return fail(COSIM_EINVAL, "cosim_spawn_set: row " + std::to_string(r) + " is not finite");
    if (!hf) continue;
    const double c = cos((double)yaw), s = sin((double)yaw);
    for (int g = 0; g < n_foot; g++) {   // every footprint window must lie on the field: |l| + r <= s
      const double ox = footprint_host[4 * g], oy = footprint_host[4 * g + 1], rb = footprint_host[4 * g + 2];
      const double lx = (double)x + (c * ox - s * oy) - (double)(float)m.ground_pos[0], ly = (double)y + (s * ox + c * oy) - (double)(float)m.ground_pos[1];
      if (fabs(lx) + rb > (double)(float)m.hfield_size[0] || fabs(ly) + rb > (double)(float)m.hfield_size[1])
        return fail(COSIM_EINVAL, "cosim_spawn_set: row " + std::to_string(r) + " puts footprint geom " + std::to_string(g) + " off the heightfield");
    }
  }
  if (rows != e->spawn.rows) {   // a new size: a new table (the same size is rewritten in place, the pointer stays for captured graphs)
    HIP_TRY(hipStreamSynchronize(cs));
    e->spawn.table.reset(); e->spawn.rows = 0; e->spawn.host.clear();   // drop first
    HIP_TRY(e->spawn.table.alloc((size_t)rows * 8));
  }
  const char* const fn = "cosim_spawn_set";
  Dev<float> d_in, d_foot;   // the two input buffers live for this call
  std::vector<float> placed((size_t)rows * 8);
  HIP_TRY_AS(fn, d_in.upload(xyyaw_host, (size_t)rows * 3));
  HIP_TRY_AS(fn, d_foot.alloc((size_t)(n_foot > 0 ? n_foot : 1) * 4));
  if (n_foot > 0) HIP_TRY_AS(fn, hipMemcpy(d_foot.get(), footprint_host, (size_t)n_foot * 4 * sizeof(float), hipMemcpyHostToDevice));
  SpawnArgs a;
  memset(&a, 0, sizeof a);
  a.xyyaw = d_in.get(); a.foot = reinterpret_cast<const float4*>(d_foot.get()); a.out = e->spawn.table.get(); a.hfield = hf ? e->d_hfield.get() : nullptr;
  a.rows = rows; a.n_foot = n_foot; a.nrow = m.hfield_nrow; a.ncol = m.hfield_ncol;
  a.sx = (float)m.hfield_size[0]; a.sy = (float)m.hfield_size[1]; a.sz = (float)m.hfield_size[2];
  a.gx = (float)m.ground_pos[0]; a.gy = (float)m.ground_pos[1];
  a.init_z = (float)m.init_qpos[2]; a.clearance = clearance;
  for (int k = 0; k < 4; k++) a.iq[k] = (float)m.init_qpos[3 + k];
  hipLaunchKernelGGL(spawn_place_kernel, dim3(rows), dim3(64), 0, cs, a);   // behind the steps already on the stream: they keep the old rows
  HIP_TRY_AS(fn, hipGetLastError());
  HIP_TRY_AS(fn, hipStreamSynchronize(cs));   // (the input buffers go behind it)
  HIP_TRY_AS(fn, e->spawn.table.download(placed.data(), placed.size()));
  e->spawn.host.swap(placed);
  e->spawn.rows = rows; e->spawn.mode = per_episode != 0;
  return COSIM_OK;
}

// ---- fall rules (the rule itself is in env_body, cosim_kernels.hip)
int cosim_fall_set(cosim_engine_t* e, float min_up, float min_height, int grace_steps, const int32_t* body_ids, int n_bodies) {
  if (!e) return fail(COSIM_EINVAL, "cosim_fall_set: null engine");
  if (!std::isfinite(min_up)) return fail(COSIM_EINVAL, "cosim_fall_set: min_up is not finite");
  if (!std::isfinite(min_height)) return fail(COSIM_EINVAL, "cosim_fall_set: min_height is not finite");
  if (grace_steps < 0) return fail(COSIM_EINVAL, "cosim_fall_set: grace_steps " + std::to_string(grace_steps) + " is negative");
  if (n_bodies > 0 && !body_ids) return fail(COSIM_EINVAL, "cosim_fall_set: n_bodies > 0 and body_ids is NULL");
  if (n_bodies > CS_MAXBODY) return fail(COSIM_EINVAL, "cosim_fall_set: more than " + std::to_string(CS_MAXBODY) + " bodies");
  unsigned bodymask = 0u;
  for (int i = 0; i < n_bodies; i++) {
    if (body_ids[i] <= 0 || body_ids[i] >= e->model.nbody)
      return fail(COSIM_EINVAL, "cosim_fall_set: body id " + std::to_string(body_ids[i]) + " is not a body of the robot (1.." +
                                    std::to_string(e->model.nbody - 1) + ")");
    bodymask |= 1u << body_ids[i];
  }
  const int term_mode = n_bodies < 0 ? e->model_term_mode : (bodymask != 0u ? 1 : 0);
  if (n_bodies < 0) bodymask = e->model_term_bodymask;
  if (term_mode != e->hm.term_mode || bodymask != e->hm.term_bodymask) {   // the device model changes: no launch may be reading it
    HIP_TRY(hipSetDevice(e->device));
    int rc = join_ranges(e, nullptr);
    if (rc) return rc;
    HIP_TRY(hipDeviceSynchronize());
    e->hm.term_mode = term_mode; e->hm.term_bodymask = bodymask;
    HIP_TRY(hipMemcpy(e->d_model.get(), &e->hm, sizeof(DevModel), hipMemcpyHostToDevice));
  }
  const int posture = (min_up > -1.f ? 1 : 0) | (min_height > 0.f ? 2 : 0);
  const bool on = posture != 0 || n_bodies >= 0;   // everything off: the model's own list, no cause bookkeeping
  e->fall_min_up = min_up; e->fall_min_height = min_height; e->fall_grace = grace_steps;
  e->fall_mask = on ? (posture | (term_mode == 1 ? 4 : 0)) : 0;
  return COSIM_OK;
}

int cosim_spawn_get(cosim_engine_t* e, float* poses_host, int capacity) {
  if (!e || (capacity > 0 && !poses_host)) return fail(COSIM_EINVAL, "cosim_spawn_get: null argument");
  const int n = e->spawn.rows < capacity ? e->spawn.rows : capacity;
  for (int r = 0; r < n; r++) memcpy(poses_host + 7 * (size_t)r, e->spawn.host.data() + 8 * (size_t)r, 7 * sizeof(float));
  return e->spawn.rows;
}

static int locate(cosim_engine* e, const std::string& n, int* off, int* width) {
  if (n == "qpos") { *off = e->lay.s_qpos; *width = e->model.nq; }
  else if (n == "qvel") { *off = e->lay.s_qvel; *width = e->model.nv; }
  else if (n == "qacc_warmstart") { *off = e->lay.s_warm; *width = e->model.nv; }
  else if (n == "meta") { *off = e->lay.s_meta; *width = Layout::NMETA; }
  else return fail(COSIM_EINVAL, "unknown state field " + n);
  return COSIM_OK;
}

int cosim_get(cosim_engine_t* e, const char* name, float* out_dev, void* stream) {
  if (!e || !name || !out_dev) return fail(COSIM_EINVAL, "cosim_get: null argument");
  HIP_TRY(hipSetDevice(e->device));
  const bool act_eff = std::string(name) == "action_effective";
  if (act_eff || std::string(name) == "action_raw") {   // [N][nu], contiguous: the last step's rows of the action faults' buffers
    if (e->actflt.tab.n_items == 0 && e->lat.tab.n_act == 0)
      return fail(COSIM_EINVAL, std::string("cosim_get: ") + name + ": no action faults are set (cosim_set_param \"action_faults\") and no latency of the command channel (cosim_set_param \"latency\")");
    RC_TRY(join_ranges(e, (hipStream_t)stream));
    HIP_TRY(hipMemcpyAsync(out_dev, act_eff ? e->act.eff.get() : e->act.raw.get(), (size_t)e->n_envs * e->model.nu * sizeof(float),
                           hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return COSIM_OK;
  }
  const bool srch_state = std::string(name) == "search_state";
  if (srch_state || std::string(name) == "search_trials") {   // int32 [N][16] / [N][slots][4], contiguous: the search's records / trial rings
    if (e->srch.tab.n_items == 0) return fail(COSIM_EINVAL, std::string("cosim_get: ") + name + ": no search is armed (cosim_set_param \"search\")");
    RC_TRY(join_ranges(e, (hipStream_t)stream));
    const size_t words = (size_t)e->n_envs * (srch_state ? (size_t)SRCH_NCNT : (size_t)e->srch.slots * SRCH_TRIAL_WORDS);
    HIP_TRY(hipMemcpyAsync(out_dev, srch_state ? e->srch.rec.get() : e->srch.ring.get(), words * sizeof(int), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return COSIM_OK;
  }
  int off, width;
  int rc = locate(e, name, &off, &width);
  if (rc) return rc;
  rc = join_ranges(e, (hipStream_t)stream);
  if (rc) return rc;
  HIP_TRY(hipMemcpy2DAsync(out_dev, width * sizeof(float), e->d_state.get() + off, e->lay.s_stride * sizeof(float), width * sizeof(float),
                           e->n_envs, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return COSIM_OK;
}

int cosim_set(cosim_engine_t* e, const char* name, const float* in_dev, void* stream) {
  if (!e || !name || !in_dev) return fail(COSIM_EINVAL, "cosim_set: null argument");
  HIP_TRY(hipSetDevice(e->device));
  int off, width;
  RC_TRY(locate(e, name, &off, &width));
  RC_TRY(join_ranges(e, (hipStream_t)stream));
  HIP_TRY(hipMemcpy2DAsync(e->d_state.get() + off, e->lay.s_stride * sizeof(float), in_dev, width * sizeof(float), width * sizeof(float),
                           e->n_envs, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  e->stepped = true;
  return observers_begin(e, nullptr, nullptr, 0, LEDGER_NO_RESET, (hipStream_t)stream);
}

int cosim_snapshot(cosim_engine_t* e, float* out_dev, void* stream) {
  if (!e || !out_dev) return fail(COSIM_EINVAL, "cosim_snapshot: null argument");
  if ((uintptr_t)out_dev & 15) return fail(COSIM_EINVAL, "cosim_snapshot: out_dev must be 16-byte aligned");
  HIP_TRY(hipSetDevice(e->device));
  RC_TRY(upload_params(e));   // the row holds the parameters the next step would run with
  RC_TRY(join_ranges(e, (hipStream_t)stream));
  SnapArgs a = snap_args(e);
  a.rows = out_dev;
  return launch_small<1, 64>(snapshot_pack_kernel, a, e->n_envs, (hipStream_t)stream);
}

int cosim_restore(cosim_engine_t* e, const float* snap_dev, int snap_rows, const int32_t* src_index_dev, const uint8_t* mask_dev,
                  int with_params, void* stream) {
  if (!e || !snap_dev || snap_rows < 1) return fail(COSIM_EINVAL, "cosim_restore: null argument or snap_rows < 1");
  if ((uintptr_t)snap_dev & 15) return fail(COSIM_EINVAL, "cosim_restore: snap_dev must be 16-byte aligned");
  if (!src_index_dev && snap_rows != e->n_envs)
    return fail(COSIM_EINVAL, "cosim_restore: without a source index snap_rows must equal n_envs (" + std::to_string(e->n_envs) + "), got " +
                                  std::to_string(snap_rows));
  HIP_TRY(hipSetDevice(e->device));
  hipStream_t cs = (hipStream_t)stream;
  RC_TRY(upload_params(e));   // a pending upload first: the envs this restore leaves alone get their new parameters, the others the row's
  RC_TRY(join_ranges(e, cs));
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  HIP_TRY(hipStreamIsCapturing(cs, &cap));
  if (src_index_dev) {
    if (!e->snap_err.dev) {
      if (cap != hipStreamCaptureStatusNone) return fail(COSIM_EINVAL, "cosim_restore: the first restore with a source index allocates; call it once outside the capture");
      SnapErr pair;   // both or neither: a failure of the second leaves no device word behind for the next call to trust
      HIP_TRY(pair.dev.alloc(2));
      HIP_TRY(pair.host.alloc(2));
      e->snap_err = std::move(pair);
    }
    HIP_TRY(hipMemsetAsync(e->snap_err.dev.get(), 0, 2 * sizeof(int), cs));
  }
  SnapArgs a = snap_args(e);
  a.rows = const_cast<float*>(snap_dev); a.n_rows = snap_rows; a.src = src_index_dev; a.mask = mask_dev;
  a.err = src_index_dev ? e->snap_err.dev.get() : nullptr; a.with_params = with_params != 0;
  RC_TRY(launch_small<1, 64>(snapshot_gather_kernel, a, e->n_envs, cs));
  if (with_params) e->params_mirror_stale = true;
  e->stepped = true;
  RC_TRY(observers_begin(e, mask_dev, src_index_dev, snap_rows, LEDGER_NO_RESET, cs));
  if (src_index_dev && cap == hipStreamCaptureStatusNone) {   // the kernel skipped what it refused; report it
    HIP_TRY(hipMemcpyAsync(e->snap_err.host.get(), e->snap_err.dev.get(), 2 * sizeof(int), hipMemcpyDeviceToHost, cs));
    HIP_TRY(hipStreamSynchronize(cs));
    if (e->snap_err.host.get()[0] > 0)
      return fail(COSIM_EINVAL, "cosim_restore: source index of env " + std::to_string(e->n_envs - e->snap_err.host.get()[1]) + " is outside [0, " +
                                    std::to_string(snap_rows) + "); " + std::to_string(e->snap_err.host.get()[0]) + " env(s) were left untouched");
  }
  return COSIM_OK;
}

int cosim_history_set(cosim_engine_t* e, int slots, int every) {
  if (!e || slots < 0 || slots > 65536 || (slots > 0 && every < 1)) return fail(COSIM_EINVAL, "cosim_history_set: slots must be 0..65536 and every >= 1");
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipDeviceSynchronize());   // launches in flight may still write the old ring
  e->hist = {};   // drop first: the ring can be gigabytes
  if (slots == 0) return COSIM_OK;
  HIP_TRY(e->hist.ring.alloc((size_t)slots * e->n_envs * (size_t)(e->lay.s_stride + e->lay.p_stride)));
  e->hist.slots = slots; e->hist.every = every; e->hist.call_of.assign(slots, 0);
  return COSIM_OK;
}

int cosim_history_get(cosim_engine_t* e, int age, float* out_dev, int* steps_ago, void* stream) {
  if (!e || !out_dev) return fail(COSIM_EINVAL, "cosim_history_get: null argument");
  if (e->hist.slots <= 0) return fail(COSIM_EINVAL, "cosim_history_get: no history is set (cosim_history_set)");
  if (age < 0 || age >= e->hist.slots) return fail(COSIM_EINVAL, "cosim_history_get: age " + std::to_string(age) + " outside the ring of " + std::to_string(e->hist.slots) + " slots");
  if ((long)age >= e->hist.captures)
    return fail(COSIM_EINVAL, "cosim_history_get: capture of age " + std::to_string(age) + " does not exist yet (" + std::to_string(e->hist.captures) + " taken)");
  HIP_TRY(hipSetDevice(e->device));
  int rc = join_ranges(e, (hipStream_t)stream);
  if (rc) return rc;
  const int slot = (int)((e->hist.captures - 1 - age) % e->hist.slots);
  const size_t row_floats = (size_t)e->n_envs * (size_t)(e->lay.s_stride + e->lay.p_stride);
  HIP_TRY(hipMemcpyAsync(out_dev, e->hist.ring.get() + slot * row_floats, row_floats * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
  if (steps_ago) *steps_ago = (int)(e->hist.calls - e->hist.call_of[slot]);
  return COSIM_OK;
}

int cosim_ledger_set(cosim_engine_t* e, int slots) {
  if (!e || slots < 0 || slots > 4096) return fail(COSIM_EINVAL, "cosim_ledger_set: slots must be 0..4096");
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipDeviceSynchronize());   // every range's launches in flight may still write the old buffers
  e->led = {};   // drop first
  if (slots == 0) return COSIM_OK;
  const size_t N = (size_t)e->n_envs;
  Ledger led;
  HIP_TRY_AS("cosim_ledger_set", led.sum.alloc(LEDGER_NSUM * N));
  HIP_TRY_AS("cosim_ledger_set", led.peak.alloc(2 * N));
  HIP_TRY_AS("cosim_ledger_set", led.acc.alloc_zeroed(LEDGER_NINT * N));
  HIP_TRY_AS("cosim_ledger_set", led.rec.alloc_zeroed(N * slots * LEDGER_WORDS));
  e->led = std::move(led);
  e->led.slots = slots;
  // every env starts an open episode at length 0 (the range streams do not order with the null stream: wait here, cold path)
  RC_TRY(ledger_begin(e, nullptr, nullptr, 0, e->stepped ? LEDGER_NO_RESET : 0, 0));
  HIP_TRY(hipDeviceSynchronize());
  return COSIM_OK;
}

int cosim_ledger_get(cosim_engine_t* e, int32_t* records_dev, int32_t* counts_dev, int32_t* open_dev, void* stream) {
  if (!e || !records_dev || !counts_dev) return fail(COSIM_EINVAL, "cosim_ledger_get: null argument");
  if (e->led.slots <= 0) return fail(COSIM_EINVAL, "cosim_ledger_get: no ledger is set (cosim_ledger_set)");
  if (open_dev && ((uintptr_t)open_dev & 15)) return fail(COSIM_EINVAL, "cosim_ledger_get: open_dev must be 16-byte aligned");
  HIP_TRY(hipSetDevice(e->device));
  hipStream_t cs = (hipStream_t)stream;
  RC_TRY(join_ranges(e, cs));
  const size_t N = (size_t)e->n_envs;
  HIP_TRY(hipMemcpyAsync(records_dev, e->led.rec.get(), N * e->led.slots * LEDGER_WORDS * sizeof(int), hipMemcpyDeviceToDevice, cs));
  HIP_TRY(hipMemcpyAsync(counts_dev, e->led.acc.get() + 2 * N, N * sizeof(int), hipMemcpyDeviceToDevice, cs));
  if (open_dev) {
    LedgerArgs a = ledger_args(e);
    a.rec = open_dev;
    return launch_small<64, 64>(a.scn_row != nullptr ? ledger_open_scn_kernel : ledger_open_kernel, a, e->n_envs, cs);
  }
  return COSIM_OK;
}

int cosim_ftrace_set(cosim_engine_t* e, int frames, int keep, int on_mask) {
  if (!e) return fail(COSIM_EINVAL, "cosim_ftrace_set: null engine");
  if (frames < 0 || frames > FT_MAX_FRAMES) return fail(COSIM_EINVAL, "cosim_ftrace_set: frames " + std::to_string(frames) + " outside 0..1024 (0 switches the traces off)");
  if (frames > 0 && (keep < 1 || keep > FT_MAX_KEEP)) return fail(COSIM_EINVAL, "cosim_ftrace_set: keep " + std::to_string(keep) + " outside 1..64");
  if (frames > 0 && (on_mask == 0 || (on_mask & ~FT_ON_ALL) != 0))
    return fail(COSIM_EINVAL, "cosim_ftrace_set: on_mask " + std::to_string(on_mask) + " must be a non-empty subset of 1|2|4|32|64|128");
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipDeviceSynchronize());   // every range's launches in flight may still write the old buffers
  e->ft = {};   // drop first: the windows can be gigabytes
  if (frames == 0) return COSIM_OK;
  const size_t N = (size_t)e->n_envs;
  const size_t words = N * (size_t)(keep + 1) * ftrace_buf_words(frames, ftrace_words(e));
  const auto who = [&]() { return "cosim_ftrace_set: " + std::to_string(words * sizeof(int)) + " bytes of trace buffers"; };
  Ftrace ft;
  HIP_TRY_CLEAR(who(), ft.buf.alloc_zeroed(words));
  HIP_TRY_CLEAR(who(), ft.cnt.alloc_zeroed(N * FT_NCNT));
  e->ft = std::move(ft);
  e->ft.frames = frames; e->ft.keep = keep; e->ft.mask = on_mask;
  // every env starts an open episode in an empty window (the range streams do not order with the null stream: wait here, cold path)
  RC_TRY(ftrace_begin(e, nullptr, nullptr, 0, e->stepped ? FT_NO_RESET : 0, 0));
  HIP_TRY(hipDeviceSynchronize());
  return COSIM_OK;
}

int cosim_ftrace_get(cosim_engine_t* e, int32_t* buffers_dev, int32_t* counts_dev, int32_t* open_dev, void* stream) {
  if (!e || !buffers_dev || !counts_dev) return fail(COSIM_EINVAL, "cosim_ftrace_get: null argument");
  if (e->ft.frames <= 0) return fail(COSIM_EINVAL, "cosim_ftrace_get: no failure traces are set (cosim_ftrace_set)");
  HIP_TRY(hipSetDevice(e->device));
  hipStream_t cs = (hipStream_t)stream;
  RC_TRY(join_ranges(e, cs));
  const size_t N = (size_t)e->n_envs;
  const size_t bytes = N * (size_t)(e->ft.keep + 1) * ftrace_buf_words(e->ft.frames, ftrace_words(e)) * sizeof(int);
  HIP_TRY(hipMemcpyAsync(buffers_dev, e->ft.buf.get(), bytes, hipMemcpyDeviceToDevice, cs));
  // counters 0..2 of every env: working buffer, traces triggered, traces lost
  HIP_TRY(hipMemcpy2DAsync(counts_dev, 3 * sizeof(int), e->ft.cnt.get(), FT_NCNT * sizeof(int), 3 * sizeof(int), N, hipMemcpyDeviceToDevice, cs));
  if (open_dev) {
    FtArgs a = ftrace_args(e);
    a.open_out = open_dev;
    return launch_small<64, 64>(ftrace_open_kernel, a, e->n_envs, cs);
  }
  return COSIM_OK;
}

// ---- the setters of the scenario family: clear, refusals, validator (cosim_tables.h), join and wait, pack, in place or fresh, upload
static TableDims table_dims(const cosim_engine* e) {
  return {e->model.nq, e->model.nv, e->model.nu, e->model.ngeom, e->ho.info_dim, e->ho.command_dim, e->lay.p_kp, e->lay.p_kd, e->lay.p_gmu, e->lay.p_floss};
}

// every range's launches in flight may still read a table and write the buffers that go with it: join the ranges, wait for the device
static int table_quiesce(cosim_engine* e, hipStream_t s) {
  RC_TRY(join_ranges(e, s));
  HIP_TRY(hipDeviceSynchronize());
  return COSIM_OK;
}

// n_scn = 0 clears
static int table_clear(cosim_engine* e, hipStream_t s, void (*drop)(cosim_engine*)) {
  RC_TRY(table_quiesce(e, s));
  drop(e);
  return COSIM_OK;
}

// windows, checks and curves (`what`) are rows of the scenario table that is set
static int table_rows_match(const cosim_engine* e, const std::string& fn, const char* what, int n_scn) {
  if (e->scn.tab.n_scn == 0) return fail(COSIM_EINVAL, fn + ": no scenario table is set (cosim_scenario_set): " + what + " are rows of a table; set the table first");
  if (n_scn != e->scn.tab.n_scn) return fail(COSIM_EINVAL, fn + ": " + std::to_string(n_scn) + " scenarios, the table that is set has " + std::to_string(e->scn.tab.n_scn));
  return COSIM_OK;
}

// the image that is set, read back for the in-place test (cold path)
static int table_download(const char* d, const WordPacker& pk, std::vector<int32_t>& old) {
  old.resize(pk.words());
  HIP_TRY(hipMemcpy(old.data(), d, pk.bytes(), hipMemcpyDeviceToHost));
  return COSIM_OK;
}

// Scenario table.  A table of the sizes of the one that is set is rewritten in place: the device pointers stay, captured graphs pick
// it up.
int cosim_scenario_set(cosim_engine_t* e, int n_scn, const int32_t* key_adr, const int32_t* key_t, const float* key_cmd, const int32_t* push_adr,
                       const int32_t* push_t, const float* push_v, int mode, float* cmd_out_dev, int32_t* row_out_dev, void* stream) {
  if (!e) return fail(COSIM_EINVAL, "cosim_scenario_set: null engine");
  HIP_TRY(hipSetDevice(e->device));
  if (n_scn == 0) return table_clear(e, (hipStream_t)stream, scenario_free);
  const int cd = e->ho.command_dim;
  if (n_scn < 1 || n_scn > SCN_MAX_ROWS) return fail(COSIM_EINVAL, "cosim_scenario_set: " + std::to_string(n_scn) + " scenarios: must be 1..65536 (0 clears the table)");
  if (mode != SCN_MODE_ENV && mode != SCN_MODE_CYCLE) return fail(COSIM_EINVAL, "cosim_scenario_set: mode must be 0 (env) or 1 (cycle)");
  if (mode == SCN_MODE_CYCLE && !e->ho.auto_reset)
    return fail(COSIM_EINVAL, "cosim_scenario_set: mode cycle needs auto_reset: without it the episode count advances on every flagged step");
  if (!row_out_dev || (cd > 0 && !cmd_out_dev)) return fail(COSIM_EINVAL, "cosim_scenario_set: null argument");
  const ScnRaw raw = {n_scn, key_adr, key_t, key_cmd, push_adr, push_t, push_v};
  const ScnShape v = validate_scenario(table_dims(e), raw);
  if (!v.err.empty()) return fail(COSIM_EINVAL, v.err);
  if (n_scn == e->scn.tab.n_scn && mode == SCN_MODE_CYCLE && e->actflt.marked + e->obsflt.marked + e->par.marked > 0)
    return fail(COSIM_EINVAL, "cosim_scenario_set: mode cycle drops the limit search and " + std::to_string(e->actflt.marked + e->obsflt.marked + e->par.marked) +
                                  " parameter or fault items are marked for it: clear or unmark them first");
  RC_TRY(table_quiesce(e, (hipStream_t)stream));
  ScnTable tab = {};
  WordPacker pk;
  pack_scenario(pk, tab, cd, raw, v);
  // other sizes: a new allocation, which replaces the old one only once it is filled (a failure leaves the table that was set)
  const bool in_place = n_scn == e->scn.tab.n_scn && v.nkey == e->scn.nkey && v.npush == e->scn.npush;
  Dev<char> fresh;
  if (!in_place) HIP_TRY(fresh.alloc(pk.bytes()));
  const hipError_t r = hipMemcpy(in_place ? e->scn.image.get() : fresh.get(), pk.data(), pk.bytes(), hipMemcpyHostToDevice);
  if (r != hipSuccess) {   // a new allocation is dropped and the old table stays; an in-place rewrite may be half written: no table then
    if (in_place) scenario_free(e);
    return fail(COSIM_EHIP, std::string("cosim_scenario_set: ") + hipGetErrorString(r));
  }
  if (!in_place) e->scn.image = std::move(fresh);
  if (n_scn != e->scn.tab.n_scn || mode == SCN_MODE_CYCLE) e->srch = {};   // so is the search; its one record per env needs mode env
  if (n_scn != e->scn.tab.n_scn) scenario_rows_drop(e);   // parameter windows, faults, latency, checks and curves are rows of the table they were set for: another S drops them
  pk.patch(e->scn.image.get());
  tab.mode = mode;
  tab.gid_off = (unsigned)(((e->env_id0 % n_scn) + n_scn) % n_scn);
  e->scn.tab = tab;
  e->scn.nkey = v.nkey; e->scn.npush = v.npush;
  e->scn.cmd_out = cmd_out_dev; e->scn.row_out = row_out_dev;
  return COSIM_OK;
}

// Parameter windows of the scenario table that is set; every env's effective record is written once.  Items of the count of the ones
// that are set are rewritten in place: the device pointers stay, captured graphs pick the new values up.
int cosim_scenario_params_set(cosim_engine_t* e, int n_scn, const int32_t* adr, const int32_t* t, const int32_t* field, const int32_t* index,
                              const int32_t* op, const float* value) {
  if (!e) return fail(COSIM_EINVAL, "cosim_scenario_params_set: null engine");
  HIP_TRY(hipSetDevice(e->device));
  if (n_scn == 0) return table_clear(e, 0, [](cosim_engine* x) { x->par = {}; });
  RC_TRY(table_rows_match(e, "cosim_scenario_params_set", "parameter windows", n_scn));
  const ParRaw raw = {n_scn, adr, t, field, index, op, value};
  const FltMarks marks = {SRCH_PARAMS, e->srch.has.data(), e->srch.targets.data(), e->srch.lo.data(), e->srch.hi.data()};
  const bool armed = e->srch.tab.n_items > 0 && (e->srch.kinds & SRCH_PARAMS) && n_scn == e->srch.tab.n_scn;
  const ParShape v = validate_params(table_dims(e), raw, armed ? &marks : nullptr);
  if (!v.err.empty()) return fail(COSIM_EINVAL, v.err);
  RC_TRY(upload_params(e));   // the effective records written below are built from the current base
  RC_TRY(table_quiesce(e, 0));
  ScnParTable tab = {};
  WordPacker pk;
  pack_params(pk, tab, raw, v);
  const bool in_place = e->par.tab.n_items == v.n && e->par.tab.n_scn == n_scn;
  Dev<char> fresh;
  Dev<float> eff;
  if (!in_place) HIP_TRY(fresh.alloc(pk.bytes()));
  if (!e->par.eff) HIP_TRY_AS("cosim_scenario_params_set", eff.alloc((size_t)e->n_envs * e->lay.p_stride));
  const hipError_t r = hipMemcpy(in_place ? e->par.image.get() : fresh.get(), pk.data(), pk.bytes(), hipMemcpyHostToDevice);
  if (r != hipSuccess) {   // new allocations are dropped and the old items stay; an in-place rewrite may be half written: no windows then
    if (in_place) e->par = {};
    return fail(COSIM_EHIP, std::string("cosim_scenario_params_set: ") + hipGetErrorString(r));
  }
  if (!in_place) e->par.image = std::move(fresh);
  if (eff) e->par.eff = std::move(eff);
  pk.patch(e->par.image.get());
  e->par.tab = tab;
  e->par.marked = v.marked;
  // every env's effective record once, at its current clock: no row is ever unwritten
  RC_TRY(scnparams_launch(e, 0, e->n_envs, nullptr, 0, 0));
  HIP_TRY(hipDeviceSynchronize());
  return COSIM_OK;
}

// Faults of the scenario table that is set, either kind (cosim_set_param "obs_faults" / "action_faults"): `words` is S | adr[S + 1] |
// t[n][2] | elem[n] | op[n] | ord[n] | value[n] (float bits), n = adr[S]; S = 0 clears.  Items of the counts of the ones that are
// set are rewritten in place: the device pointers stay, captured graphs pick the new values up.  Nothing is launched: the faults
// act from the next step (observations: or reset) on.  The kind gives its group, how it is dropped, its validator (cosim_tables.h)
// and whether it needs the two action rows beside the table: they are allocated ahead of the copy.
static int fault_table_set(cosim_engine* e, const std::string& fn, const char* what, Faults& set, void (*drop)(cosim_engine*), bool action_rows,
                           FltShape (*validate)(const cosim_engine*, const FltRaw&), const int32_t* words, int count) {
  if (count < 1) return fail(COSIM_EINVAL, fn + ": an empty table (one word, 0, clears the faults)");
  const int n_scn = words[0];
  HIP_TRY(hipSetDevice(e->device));
  if (n_scn == 0) return table_clear(e, 0, drop);
  RC_TRY(table_rows_match(e, fn, what, n_scn));
  if (count < n_scn + 2) return fail(COSIM_EINVAL, fn + ": " + std::to_string(count) + " words do not hold the row addresses of " + std::to_string(n_scn) + " scenarios");
  const int32_t* adr = words + 1;
  const long long n = adr[n_scn];   // (the validator holds every row inside [0, adr[S]] before it reads an item by these addresses)
  if (n < 0 || (long long)count != n_scn + 2 + 6 * n)
    return fail(COSIM_EINVAL, fn + ": " + std::to_string(count) + " words, a table of " + std::to_string(n_scn) + " scenarios and " + std::to_string(n) + " items takes " +
                                  std::to_string(n_scn + 2 + 6 * (n < 0 ? 0 : n)));
  const int32_t *t = adr + n_scn + 1, *elem = t + 2 * n, *op = elem + n, *ord = op + n;
  const FltRaw raw = {n_scn, adr, t, elem, op, ord, reinterpret_cast<const float*>(ord + n)};
  const FltShape v = validate(e, raw);
  if (!v.err.empty()) return fail(COSIM_EINVAL, v.err);
  RC_TRY(table_quiesce(e, 0));
  FaultTable tab = {};
  WordPacker pk;
  pack_faults(pk, tab, raw, v);
  const bool in_place = set.tab.n_items == v.n && set.tab.n_scn == n_scn;
  Dev<char> fresh;
  ActionRows rows;
  if (!in_place) HIP_TRY(fresh.alloc(pk.bytes()));
  if (action_rows && !e->act.eff) HIP_TRY_AS(fn, rows.alloc((size_t)e->n_envs * e->model.nu));
  const hipError_t r = hipMemcpy(in_place ? set.image.get() : fresh.get(), pk.data(), pk.bytes(), hipMemcpyHostToDevice);
  if (r != hipSuccess) {   // new allocations are dropped and the old items stay; an in-place rewrite may be half written: no faults then
    if (in_place) drop(e);
    return fail(COSIM_EHIP, fn + ": " + hipGetErrorString(r));
  }
  if (!in_place) set.image = std::move(fresh);
  if (rows.eff) e->act = std::move(rows);
  pk.patch(set.image.get());
  set.tab = tab;
  return COSIM_OK;
}

// the items of a fault table that passed its validator (S + 2 + 6 n words) whose element carries FLT_MARK
static int fault_words_marked(const int32_t* words) {
  const int n_scn = words[0], n = words[1 + n_scn];
  const int32_t* elem = words + 1 + (n_scn + 1) + 2 * (size_t)n;
  int m = 0;
  for (int i = 0; i < n; i++) m += ((unsigned)elem[i] & FLT_MARK) != 0;
  return m;
}
static FltShape obsfault_validate(const cosim_engine* e, const FltRaw& raw) {
  const FltMarks marks = {SRCH_OBS_FAULTS, e->srch.has.data(), e->srch.targets.data(), e->srch.lo.data(), e->srch.hi.data()};
  const bool armed = obsfault_searched(e) && raw.n_scn == e->srch.tab.n_scn;
  return validate_faults({e->ho.frame_dim, e->ho.stacked_dim, e->ho.stack_size, e->ho.el_field, CS_OBS_COMMAND}, raw, armed ? &marks : nullptr);
}
static int obsfault_set(cosim_engine* e, const int32_t* words, int count) {
  RC_TRY(fault_table_set(e, OBF_SETTER, "observation faults", e->obsflt, [](cosim_engine* x) { x->obsflt = {}; }, false, obsfault_validate, words, count));
  e->obsflt.marked = e->obsflt.tab.n_items > 0 ? fault_words_marked(words) : 0;
  return COSIM_OK;
}

// marked items are held against the search that is armed, if its targets name the action faults
static FltShape actfault_validate(const cosim_engine* e, const FltRaw& raw) {
  const FltMarks marks = {SRCH_ACT_FAULTS, e->srch.has.data(), e->srch.targets.data(), e->srch.lo.data(), e->srch.hi.data()};
  const bool armed = e->srch.tab.n_items > 0 && (e->srch.kinds & SRCH_ACT_FAULTS) && raw.n_scn == e->srch.tab.n_scn;
  return validate_action_faults(e->model.nu, raw, armed ? &marks : nullptr);
}
static int actfault_set(cosim_engine* e, const int32_t* words, int count) {
  RC_TRY(fault_table_set(e, ACF_SETTER, "action faults", e->actflt, [](cosim_engine* x) { x->actflt = {}; action_rows_release(x); }, true, actfault_validate, words, count));
  e->actflt.marked = e->actflt.tab.n_items > 0 ? fault_words_marked(words) : 0;
  e->act_in_obs = false;
  for (int el = 0; el < e->ho.frame_dim; el++) e->act_in_obs = e->act_in_obs || e->ho.el_field[el] == CS_OBS_LAST_ACTION;
  return COSIM_OK;
}

// Latency lines of the scenario table that is set (cosim_set_param "latency"): `words` is S | act_adr[S + 1] | obs_adr[S + 1] |
// act[na][6] | obs[no][6], an item being (t0, t1, el, ord, steps, jitter), na = act_adr[S], no = obs_adr[S]; the one word 0 clears.
// A table with the row addresses of the one that is set whose largest delay still fits the depth D is rewritten in place: the device
// pointers, D and the lines stay, captured graphs pick the new items up.  Anything else is a fresh allocation: D = the largest
// steps + jitter, plus 1, and every line invalid (it restarts at the clock its kernel finds next).  Nothing is launched.
static int latency_set(cosim_engine* e, const int32_t* words, int count) {
  const std::string fn = LAT_SETTER;
  if (count < 1) return fail(COSIM_EINVAL, fn + ": an empty table (one word, 0, clears the latency)");
  const int n_scn = words[0];
  HIP_TRY(hipSetDevice(e->device));
  if (n_scn == 0) return table_clear(e, 0, [](cosim_engine* x) { x->lat = {}; action_rows_release(x); });
  RC_TRY(table_rows_match(e, fn, "latency items", n_scn));
  const size_t S1 = (size_t)n_scn + 1;
  if ((size_t)count < 1 + 2 * S1) return fail(COSIM_EINVAL, fn + ": " + std::to_string(count) + " words do not hold the row addresses of " + std::to_string(n_scn) + " scenarios");
  const int32_t *act_adr = words + 1, *obs_adr = act_adr + S1;
  const long long na = act_adr[n_scn], no = obs_adr[n_scn];   // (the validator holds every row inside [0, adr[S]] before it reads an item by these addresses)
  if (na < 0 || no < 0 || (long long)count != 1 + 2 * (long long)S1 + 6 * (na + no))
    return fail(COSIM_EINVAL, fn + ": " + std::to_string(count) + " words, a table of " + std::to_string(n_scn) + " scenarios and " + std::to_string(na) + " + " + std::to_string(no) +
                                  " items takes " + std::to_string(1 + 2 * (long long)S1 + 6 * ((na < 0 ? 0 : na) + (no < 0 ? 0 : no))));
  const LatRaw raw = {n_scn, act_adr, obs_adr, obs_adr + S1, obs_adr + S1 + 6 * na};
  const LatShape v = validate_latency(e->model.nu, {e->ho.frame_dim, e->ho.stacked_dim, e->ho.stack_size, e->ho.el_field, CS_OBS_COMMAND}, raw);
  if (!v.err.empty()) return fail(COSIM_EINVAL, v.err);
  const int N = e->n_envs, nu = e->model.nu, fd = e->ho.frame_dim;
  LatTable tab = {};
  WordPacker pk;
  pack_latency(pk, tab, raw, v);
  RC_TRY(table_quiesce(e, 0));
  bool in_place = e->lat.tab.n_scn == n_scn && e->lat.tab.n_act == v.n_act && e->lat.tab.n_obs == v.n_obs && v.max_delay + 1 <= e->lat.tab.depth;
  if (in_place) {   // ... and every scenario keeps its counts: an env keeps the kinds it has a line for
    std::vector<int32_t> old;
    RC_TRY(table_download(e->lat.image.get(), pk, old));
    in_place = latency_same_rows(pk, tab, old.data());
  }
  if (in_place) {
    const hipError_t r = hipMemcpy(e->lat.image.get(), pk.data(), pk.bytes(), hipMemcpyHostToDevice);
    if (r != hipSuccess) { e->lat = {}; action_rows_release(e); return fail(COSIM_EHIP, fn + ": " + hipGetErrorString(r)); }   // may be half written: no latency then
    tab.depth = e->lat.tab.depth;
    pk.patch(e->lat.image.get());
    e->lat.tab = tab;
    return COSIM_OK;
  }
  const int D = v.max_delay + 1;
  const size_t cap = (size_t)256 << 20;
  const size_t act_bytes = (size_t)N * D * nu * sizeof(float), obs_bytes = (size_t)N * D * fd * sizeof(float);
  if (v.n_act > 0 && act_bytes > cap)
    return fail(COSIM_EINVAL, fn + ": the action lines take " + std::to_string(N) + " envs x depth " + std::to_string(D) + " x " + std::to_string(nu) + " actuators x 4 = " +
                                  std::to_string(act_bytes) + " bytes, more than 256 MiB: fewer envs or a shorter delay");
  if (v.n_obs > 0 && obs_bytes > cap)
    return fail(COSIM_EINVAL, fn + ": the observation lines take " + std::to_string(N) + " envs x depth " + std::to_string(D) + " x " + std::to_string(fd) + " frame elements x 4 = " +
                                  std::to_string(obs_bytes) + " bytes, more than 256 MiB: fewer envs or a shorter delay");
  // a fresh group replaces the one that is set only once it is complete: a failure leaves the latency that was set
  Latency fresh;
  ActionRows act;
  const size_t rows = (size_t)N * nu;
  HIP_TRY_AS(fn, fresh.image.alloc(pk.bytes()));
  HIP_TRY_AS(fn, fresh.from.alloc(2 * (size_t)N));
  HIP_TRY_AS(fn, hipMemset(fresh.from.get(), 0xff, 2 * (size_t)N * sizeof(int)));   // -1: every line invalid
  if (v.n_act > 0) {
    HIP_TRY_AS(fn, fresh.act_line.alloc_zeroed(rows * D));
    HIP_TRY_AS(fn, fresh.eff.alloc_zeroed(rows));
    HIP_TRY_AS(fn, fresh.spare.alloc_zeroed(rows));
    if (!e->act.eff) HIP_TRY_AS(fn, act.alloc(rows));
  }
  if (v.n_obs > 0) HIP_TRY_AS(fn, fresh.obs_line.alloc_zeroed((size_t)N * D * fd));
  HIP_TRY_AS(fn, hipMemcpy(fresh.image.get(), pk.data(), pk.bytes(), hipMemcpyHostToDevice));
  pk.patch(fresh.image.get());
  tab.depth = D;
  fresh.tab = tab;
  e->lat = std::move(fresh);
  if (act.eff) e->act = std::move(act);
  action_rows_release(e);   // no action items now and no action faults: the two rows go
  e->act_in_obs = false;
  for (int el = 0; el < e->ho.frame_dim; el++) e->act_in_obs = e->act_in_obs || e->ho.el_field[el] == CS_OBS_LAST_ACTION;
  return COSIM_OK;
}

// Limit search of the scenario table that is set (cosim_set_param "search"): `words` is S | slots | has[S] | lo | hi | x0 | d0 | d_min |
// rule | trials | targets | fail_mask | rev_skip ([S] each, floats as their bits), 2 + 11 S words, or with harder | chk_lo | chk_hi
// behind them 2 + 14 S; the one word 0 clears.  While marked items are set (action faults) the search they are held against is
// neither replaced nor cleared: clear or unmark them first.  A table with the S, the
// slots and the has[] of the one that is armed is rewritten in place and the records stay (captured graphs pick the new bounds up);
// anything else allocates anew and search_init_kernel begins every env's search at its item's start level.
static int search_set(cosim_engine* e, const int32_t* words, int count) {
  const std::string fn = "cosim_set_param \"search\"";
  if (count < 1) return fail(COSIM_EINVAL, fn + ": an empty table (one word, 0, clears the search)");
  const int n_scn = words[0];
  HIP_TRY(hipSetDevice(e->device));
  if (e->actflt.marked > 0)
    return fail(COSIM_EINVAL, fn + ": " + std::to_string(e->actflt.marked) + " action-fault items are marked for the search that is armed: clear or unmark them "
                                   "(cosim_set_param \"action_faults\") before the search is replaced or cleared");
  if (e->obsflt.marked > 0)
    return fail(COSIM_EINVAL, fn + ": " + std::to_string(e->obsflt.marked) + " observation-fault items are marked for the search that is armed: clear or unmark them "
                                   "(cosim_set_param \"obs_faults\") before the search is replaced or cleared");
  if (e->par.marked > 0)
    return fail(COSIM_EINVAL, fn + ": " + std::to_string(e->par.marked) + " parameter items are marked for the search that is armed: clear or unmark them "
                                   "(cosim_scenario_params_set) before the search is replaced or cleared");
  if (n_scn == 0) return table_clear(e, 0, [](cosim_engine* x) { x->srch = {}; });
  const bool long_form = n_scn > 0 && (long long)count == 2 + 14ll * n_scn;
  if (n_scn < 0 || ((long long)count != 2 + 11ll * n_scn && !long_form))
    return fail(COSIM_EINVAL, fn + ": " + std::to_string(count) + " words, a table of " + std::to_string(n_scn) + " scenarios takes " + std::to_string(2 + 11ll * (n_scn < 0 ? 0 : n_scn)) +
                                  " or, with harder and the check masks, " + std::to_string(2 + 14ll * (n_scn < 0 ? 0 : n_scn)));
  const int32_t* w = words + 2;
  const size_t S = (size_t)n_scn;
  const auto f = [&](int k) { return reinterpret_cast<const float*>(w + k * S); };
  SrchRaw raw = {n_scn, words[1], w, f(1), f(2), f(3), f(4), f(5), w + 6 * S, w + 7 * S, w + 8 * S, w + 9 * S, w + 10 * S};
  if (long_form) { raw.harder = w + 11 * S; raw.chk_lo = w + 12 * S; raw.chk_hi = w + 13 * S; }
  RC_TRY(table_quiesce(e, 0));
  std::vector<int32_t> adr;   // key_adr | push_adr of the table that is set: the head of its image
  if (n_scn == e->scn.tab.n_scn) {
    adr.resize(2 * (S + 1));
    HIP_TRY(hipMemcpy(adr.data(), e->scn.image.get(), adr.size() * 4, hipMemcpyDeviceToHost));
  }
  std::vector<int32_t> chk_adr;   // the row addresses of the checks that are armed: the head of their image
  if (n_scn == e->chk.tab.n_scn) {
    chk_adr.resize(S + 1);
    HIP_TRY(hipMemcpy(chk_adr.data(), e->chk.image.get(), chk_adr.size() * 4, hipMemcpyDeviceToHost));
  }
  SrchDims dims = {e->scn.tab.n_scn, e->scn.tab.mode, e->ho.auto_reset, adr.data(), adr.data() + S + 1, chk_adr.empty() ? nullptr : chk_adr.data()};
  std::vector<int32_t> kind_adr[3];   // the row addresses of the item tables that are set: the head of each image
  const struct { const char* d; int n_scn, n_items; const int32_t** slot; } kinds[3] = {
      {e->par.image.get(), e->par.tab.n_scn, e->par.tab.n_items, &dims.par_adr}, {e->obsflt.image.get(), e->obsflt.tab.n_scn, e->obsflt.tab.n_items, &dims.obs_adr}, {e->actflt.image.get(), e->actflt.tab.n_scn, e->actflt.tab.n_items, &dims.act_adr}};
  for (int k = 0; k < 3; k++) {
    if (kinds[k].n_items <= 0 || kinds[k].n_scn != n_scn) continue;
    kind_adr[k].resize(S + 1);
    HIP_TRY(hipMemcpy(kind_adr[k].data(), kinds[k].d, (S + 1) * 4, hipMemcpyDeviceToHost));
    *kinds[k].slot = kind_adr[k].data();
  }
  const SrchShape v = validate_search(dims, raw);
  if (!v.err.empty()) return fail(COSIM_EINVAL, v.err);
  SrchTable tab = {};
  WordPacker pk;
  pack_search(pk, tab, raw, v);
  bool in_place = e->srch.tab.n_scn == n_scn && e->srch.tab.n_items == v.n && e->srch.slots == raw.slots && (e->srch.tab.harder != nullptr) == long_form;
  if (in_place) {
    std::vector<int32_t> old;
    RC_TRY(table_download(e->srch.image.get(), pk, old));
    in_place = search_same_rows(pk, tab, old.data());
  }
  const size_t N = (size_t)e->n_envs;
  if (!in_place) {   // drop first, then everything anew
    e->srch = {};
    Search fresh;
    HIP_TRY_CLEAR(fn, fresh.image.alloc(pk.bytes()));
    HIP_TRY_CLEAR(fn, fresh.rec.alloc(N * SRCH_NCNT));
    HIP_TRY_CLEAR(fn, fresh.ring.alloc(N * raw.slots * SRCH_TRIAL_WORDS));
    HIP_TRY_CLEAR(fn, fresh.rem.alloc(1));
    e->srch = std::move(fresh);
  }
  const hipError_t r = hipMemcpy(e->srch.image.get(), pk.data(), pk.bytes(), hipMemcpyHostToDevice);
  if (r != hipSuccess) { e->srch = {}; (void)hipGetLastError(); return fail(COSIM_EHIP, fn + ": " + hipGetErrorString(r)); }
  pk.patch(e->srch.image.get());
  e->srch.tab = tab;
  e->srch.slots = raw.slots;
  e->srch.has.assign(raw.has, raw.has + S); e->srch.targets.assign(raw.targets, raw.targets + S);
  e->srch.lo.assign(raw.lo, raw.lo + S); e->srch.hi.assign(raw.hi, raw.hi + S);
  e->srch.kinds = 0; e->srch.on_check = false;
  for (size_t k = 0; k < S; k++) {
    if (!raw.has[k]) continue;
    e->srch.kinds |= raw.targets[k];
    e->srch.on_check = e->srch.on_check || (long_form && (raw.chk_lo[k] | raw.chk_hi[k]) != 0);
  }
  if (in_place) return COSIM_OK;
  // every env's record, ring and the remaining word once (the range streams do not order with the null stream: wait here, cold path)
  SrchArgs a = search_args(e);
  a.flag = e->stepped ? SRCH_NO_RESET : 0;
  for (int env = 0; env < e->n_envs; env++) a.n_armed += raw.has[(e->scn.tab.gid_off + (unsigned)env) % (unsigned)n_scn];
  RC_TRY(launch_small<64, 64>(search_init_kernel, a, e->n_envs, 0));
  HIP_TRY(hipDeviceSynchronize());
  return COSIM_OK;
}

// The effective parameter records [N][param_stride] as the last step / reset / cosim_scenario_params_set left them (with no windows
// set: the base records), to host memory; joins first.  Returns param_stride.
int cosim_scenario_params_get(cosim_engine_t* e, float* host, int capacity) {
  if (!e || !host) return fail(COSIM_EINVAL, "cosim_scenario_params_get: null argument");
  const size_t words = (size_t)e->n_envs * e->lay.p_stride;
  if (capacity < 0 || (size_t)capacity < words)
    return fail(COSIM_EINVAL, "cosim_scenario_params_get: capacity " + std::to_string(capacity) + " floats, the records take " + std::to_string(words));
  HIP_TRY(hipSetDevice(e->device));
  int rc = upload_params(e);
  if (rc) return rc;
  rc = join_ranges(e, 0);
  if (rc) return rc;
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(host, e->par.tab.n_items > 0 ? e->par.eff.get() : e->d_params.get(), words * sizeof(float), hipMemcpyDeviceToHost));
  return e->lay.p_stride;
}

// Checks of the scenario table that is set; every env's episode begins with clean accumulators.  Items of the counts of the ones that
// are set (same S, same row addresses, same slots) are rewritten in place: the device pointers, the counters and the records stay,
// and captured graphs pick the new values up.
int cosim_scenario_checks_set(cosim_engine_t* e, int n_scn, const int32_t* adr, const int32_t* t, const int32_t* signal, const int32_t* index,
                              const int32_t* mode, const int32_t* cmp, const float* bound, int slots) {
  if (!e) return fail(COSIM_EINVAL, "cosim_scenario_checks_set: null engine");
  HIP_TRY(hipSetDevice(e->device));
  const char* const srch_msg = ": the limit search that is armed fails on a check: clear the search (cosim_set_param \"search\") before the checks are cleared or laid out anew";
  if (n_scn == 0 && e->srch.on_check) return fail(COSIM_EINVAL, std::string("cosim_scenario_checks_set") + srch_msg);
  if (n_scn == 0) return table_clear(e, 0, [](cosim_engine* x) { x->chk = {}; });
  RC_TRY(table_rows_match(e, "cosim_scenario_checks_set", "checks", n_scn));
  const ChkRaw raw = {n_scn, adr, t, signal, index, mode, cmp, bound, slots};
  const ChkShape v = validate_checks(table_dims(e), raw);
  if (!v.err.empty()) return fail(COSIM_EINVAL, v.err);
  RC_TRY(table_quiesce(e, 0));
  ChkTable tab = {};
  WordPacker pk;
  pack_checks(pk, tab, raw, v);
  bool in_place = e->chk.tab.n_scn == n_scn && e->chk.tab.n_items == v.n && e->chk.tab.I == v.I && e->chk.slots == slots;
  if (in_place) {
    std::vector<int32_t> old;
    RC_TRY(table_download(e->chk.image.get(), pk, old));
    in_place = checks_same_rows(pk, tab, old.data());
  }
  if (!in_place && e->srch.on_check) return fail(COSIM_EINVAL, std::string("cosim_scenario_checks_set") + srch_msg);
  const size_t N = (size_t)e->n_envs, I = (size_t)v.I, W = (size_t)checks_words(v.I);
  if (!in_place) {   // drop first, then everything anew: the table, clean accumulators, counters and records at zero
    const char* const fn = "cosim_scenario_checks_set";
    e->chk = {};
    Checks fresh;
    HIP_TRY_CLEAR(fn, fresh.image.alloc(pk.bytes()));
    HIP_TRY_CLEAR(fn, fresh.ext.alloc(N * I));
    HIP_TRY_CLEAR(fn, fresh.aux.alloc(N * I));
    HIP_TRY_CLEAR(fn, fresh.n.alloc(N * I));
    HIP_TRY_CLEAR(fn, fresh.sum.alloc(N * I));
    HIP_TRY_CLEAR(fn, fresh.cnt.alloc_zeroed(N * CHK_NCNT));
    HIP_TRY_CLEAR(fn, fresh.rec.alloc_zeroed(N * slots * W));
    e->chk = std::move(fresh);
  }
  const hipError_t r = hipMemcpy(e->chk.image.get(), pk.data(), pk.bytes(), hipMemcpyHostToDevice);
  if (r != hipSuccess) { e->chk = {}; (void)hipGetLastError(); return fail(COSIM_EHIP, std::string("cosim_scenario_checks_set: ") + hipGetErrorString(r)); }
  pk.patch(e->chk.image.get());
  e->chk.tab = tab;
  e->chk.slots = slots;
  // every env starts an open episode with clean accumulators at its current clock -- in place too: no verdict mixes two sets of values
  // (the range streams do not order with the null stream: wait here, cold path)
  RC_TRY(checks_begin(e, nullptr, nullptr, 0, e->stepped ? CHK_NO_RESET : 0, 0));
  // a search that fails on a check judges an episode by its verdict: the episode that lost its samples here is no trial
  if (e->srch.on_check) RC_TRY(search_begin(e, nullptr, nullptr, 0, e->stepped ? SRCH_NO_RESET : 0, 0));
  HIP_TRY(hipDeviceSynchronize());
  return COSIM_OK;
}

// The verdict rings int32[N][slots][words], the ended-episode counts int32[N] and (or NULL) the open episodes as flag-16 records
// int32[N][words]; joins the ranges, asynchronous on the caller's stream otherwise.
int cosim_scenario_checks_get(cosim_engine_t* e, int32_t* records_dev, int32_t* counts_dev, int32_t* open_dev, void* stream) {
  if (!e || !records_dev || !counts_dev) return fail(COSIM_EINVAL, "cosim_scenario_checks_get: null argument");
  if (e->chk.tab.n_scn <= 0) return fail(COSIM_EINVAL, "cosim_scenario_checks_get: no checks are set (cosim_scenario_checks_set)");
  HIP_TRY(hipSetDevice(e->device));
  hipStream_t cs = (hipStream_t)stream;
  RC_TRY(join_ranges(e, cs));
  const size_t N = (size_t)e->n_envs, W = (size_t)checks_words(e->chk.tab.I);
  HIP_TRY(hipMemcpyAsync(records_dev, e->chk.rec.get(), N * e->chk.slots * W * sizeof(int), hipMemcpyDeviceToDevice, cs));
  HIP_TRY(hipMemcpy2DAsync(counts_dev, sizeof(int), e->chk.cnt.get(), CHK_NCNT * sizeof(int), sizeof(int), N, hipMemcpyDeviceToDevice, cs));
  if (open_dev) {
    ChkArgs a = checks_args(e);
    a.rec = open_dev;
    return launch_small<CHK_WAVES, 64 * CHK_WAVES>(checks_open_kernel, a, e->n_envs, cs);
  }
  return COSIM_OK;
}

// Response curves of the scenario table that is set; the cells are emptied and every env's episode begins with an empty stage.  Items
// of the counts and sizes of the ones that are set (same S, same row addresses, same T and B item by item) are rewritten in place:
// the device pointers stay, and captured graphs pick the new values up.
int cosim_scenario_curves_set(cosim_engine_t* e, int n_scn, const int32_t* adr, const int32_t* t, const int32_t* signal, const int32_t* index,
                              const float* lo, const float* hi, const int32_t* bins) {
  if (!e) return fail(COSIM_EINVAL, "cosim_scenario_curves_set: null engine");
  HIP_TRY(hipSetDevice(e->device));
  if (n_scn == 0) return table_clear(e, 0, [](cosim_engine* x) { x->cur = {}; });
  RC_TRY(table_rows_match(e, "cosim_scenario_curves_set", "curves", n_scn));
  const CurRaw raw = {n_scn, adr, t, signal, index, lo, hi, bins};
  const CurShape v = validate_curves(table_dims(e), e->n_envs, raw);
  if (!v.err.empty()) return fail(COSIM_EINVAL, v.err);
  RC_TRY(table_quiesce(e, 0));
  CurTable tab = {};
  WordPacker pk;
  pack_curves(pk, tab, raw, v);
  bool in_place = e->cur.tab.n_scn == n_scn && e->cur.tab.n_items == v.n && e->cur.tab.SW == (int)v.SW && e->cur.words == v.cells;
  if (in_place) {
    std::vector<int32_t> old;
    RC_TRY(table_download(e->cur.image.get(), pk, old));
    in_place = curves_same_sizes(pk, tab, old.data());
  }
  const size_t N = (size_t)e->n_envs;
  if (!in_place) {   // drop first (the groups too), then everything anew: the table, the stage, the clocks and the cells
    const char* const fn = "cosim_scenario_curves_set";
    e->cur = {};
    Curves fresh;
    HIP_TRY_CLEAR(fn, fresh.image.alloc(pk.bytes()));
    HIP_TRY_CLEAR(fn, fresh.stage.alloc(N * v.SW > 0 ? N * v.SW : 1));
    HIP_TRY_CLEAR(fn, fresh.clk.alloc(N));
    HIP_TRY_CLEAR(fn, fresh.cells.alloc(v.cells));
    e->cur = std::move(fresh);
  }
  const hipError_t r = hipMemcpy(e->cur.image.get(), pk.data(), pk.bytes(), hipMemcpyHostToDevice);
  if (r != hipSuccess) { e->cur = {}; (void)hipGetLastError(); return fail(COSIM_EHIP, std::string("cosim_scenario_curves_set: ") + hipGetErrorString(r)); }
  pk.patch(e->cur.image.get());
  e->cur.tab = tab;
  e->cur.words = v.cells;
  return cosim_scenario_curves_clear(e);
}

// Every cell back to empty and every env's episode begun anew with an empty stage at its current clock (the range streams do not
// order with the null stream: join and wait, cold path).
int cosim_scenario_curves_clear(cosim_engine_t* e) {
  if (!e) return fail(COSIM_EINVAL, "cosim_scenario_curves_clear: null engine");
  if (e->cur.tab.n_scn <= 0) return fail(COSIM_EINVAL, "cosim_scenario_curves_clear: no curves are set (cosim_scenario_curves_set)");
  HIP_TRY(hipSetDevice(e->device));
  RC_TRY(join_ranges(e, 0));
  HIP_TRY(hipDeviceSynchronize());
  RC_TRY(curves_zero(e, 0));
  RC_TRY(curves_begin(e, nullptr, nullptr, 0, 0));
  HIP_TRY(hipDeviceSynchronize());
  return COSIM_OK;
}

// Groups of the curves that are set: the cells become n_groups planes, and an ended episode is folded into the plane its env's word of
// group_dev ([n_envs] int32, the caller's, kept alive by the caller) names when the fold reads it.  n_groups = 0: back to one plane.
// Every call empties the cells.  Refusals first, then join and wait, allocate, clear, begin.
int cosim_scenario_curves_groups(cosim_engine_t* e, int n_groups, const int32_t* group_dev) {
  if (!e) return fail(COSIM_EINVAL, "cosim_scenario_curves_groups: null engine");
  if (e->cur.tab.n_scn <= 0) return fail(COSIM_EINVAL, "cosim_scenario_curves_groups: no curves are set (cosim_scenario_curves_set): groups split the cells of curves");
  if (n_groups < 0 || n_groups > CUR_MAX_GROUPS)
    return fail(COSIM_EINVAL, "cosim_scenario_curves_groups: n_groups " + std::to_string(n_groups) + " outside 0..64 (0: no groups)");
  if (n_groups > 0 && !group_dev) return fail(COSIM_EINVAL, "cosim_scenario_curves_groups: n_groups " + std::to_string(n_groups) + " with a null group_dev");
  if ((size_t)n_groups * e->cur.words * sizeof(unsigned) > CUR_MAX_BYTES)
    return fail(COSIM_EINVAL, "cosim_scenario_curves_groups: " + std::to_string(n_groups) + " planes of " + std::to_string(e->cur.words) +
                                  " words: the cells would exceed 256 MiB (a design limit)");
  HIP_TRY(hipSetDevice(e->device));
  RC_TRY(table_quiesce(e, 0));
  // the new planes replace the old ones only once both allocations stand (a failure leaves the cells and the groups that were set)
  Dev<unsigned> cells, lost;
  HIP_TRY_CLEAR("cosim_scenario_curves_groups", cells.alloc((size_t)(n_groups > 0 ? n_groups : 1) * e->cur.words));
  if (n_groups > 0 && !e->cur.ungrouped) HIP_TRY_CLEAR("cosim_scenario_curves_groups", lost.alloc(1));
  e->cur.cells = std::move(cells);
  if (lost) e->cur.ungrouped = std::move(lost);
  e->cur.groups = n_groups; e->cur.group = n_groups > 0 ? group_dev : nullptr;
  return cosim_scenario_curves_clear(e);
}

// The cells, uint32[max(G, 1) * scenario_curve_words] (plane after plane), of the episodes that have ended; joins the ranges,
// asynchronous on the caller's stream otherwise.
int cosim_scenario_curves_get(cosim_engine_t* e, uint32_t* cells_dev, void* stream) {
  if (!e || !cells_dev) return fail(COSIM_EINVAL, "cosim_scenario_curves_get: null argument");
  if (e->cur.tab.n_scn <= 0) return fail(COSIM_EINVAL, "cosim_scenario_curves_get: no curves are set (cosim_scenario_curves_set)");
  HIP_TRY(hipSetDevice(e->device));
  hipStream_t cs = (hipStream_t)stream;
  RC_TRY(join_ranges(e, cs));
  HIP_TRY(hipMemcpyAsync(cells_dev, e->cur.cells.get(), (size_t)(e->cur.groups > 0 ? e->cur.groups : 1) * e->cur.words * sizeof(unsigned), hipMemcpyDeviceToDevice, cs));
  return COSIM_OK;
}

__global__ void push_kernel(float* state, Layout lay, const float* v, const uint8_t* mask, int n) {
  int env = blockIdx.x * blockDim.x + threadIdx.x;
  if (env >= n || (mask && !mask[env])) return;
  float* rec = state + (size_t)env * lay.s_stride;
  // qvel[:2] = (R^T v_world)[:2], qvel[2] = v_world[2]   (reference flamingo_light_v1.py:234-243; quaternion used raw)
  float w = rec[lay.s_qpos + 3], x = rec[lay.s_qpos + 4], y = rec[lay.s_qpos + 5], z = rec[lay.s_qpos + 6];
  float R00 = 1 - 2 * y * y - 2 * z * z, R01 = 2 * x * y - 2 * z * w, R10 = 2 * x * y + 2 * z * w, R11 = 1 - 2 * x * x - 2 * z * z,
        R20 = 2 * x * z - 2 * y * w, R21 = 2 * y * z + 2 * x * w;
  const float* vw = v + (size_t)env * 3;
  rec[lay.s_qvel + 0] = R00 * vw[0] + R10 * vw[1] + R20 * vw[2];
  rec[lay.s_qvel + 1] = R01 * vw[0] + R11 * vw[1] + R21 * vw[2];
  rec[lay.s_qvel + 2] = vw[2];
}

int cosim_event_push(cosim_engine_t* e, const float* v_dev, const uint8_t* mask_dev, void* stream) {
  if (!e || !v_dev) return fail(COSIM_EINVAL, "cosim_event_push: null argument");
  HIP_TRY(hipSetDevice(e->device));
  { int rc = join_ranges(e, (hipStream_t)stream); if (rc) return rc; }
  hipLaunchKernelGGL(push_kernel, dim3((e->n_envs + 255) / 256), dim3(256), 0, (hipStream_t)stream, e->d_state.get(), e->lay, v_dev, mask_dev, e->n_envs);
  HIP_TRY(hipGetLastError());
  return COSIM_OK;
}

static int debug_cholesky(cosim_engine_t* e, int nv, float* io, int capacity);
static int debug_ldsbatch(cosim_engine_t* e, int nv, float* io, int capacity);
int cosim_debug_forward(cosim_engine_t* e, int env, const char* name, float* host_out, int capacity) {
  if (e && host_out && name && !strcmp(name, "cholesky")) return debug_cholesky(e, env, host_out, capacity);   // no env, no launch of a step kernel
  if (e && host_out && name && !strcmp(name, "ldsbatch")) return debug_ldsbatch(e, env, host_out, capacity);   // likewise
  if (!e || !host_out || env < 0 || env >= e->n_envs) return fail(COSIM_EINVAL, "cosim_debug_forward: bad argument");
  HIP_TRY(hipSetDevice(e->device));
  int rc = upload_params(e);
  if (rc) return rc;
  rc = join_ranges(e, 0);
  if (rc) return rc;
  HIP_TRY(hipMemset(e->d_dbg.get(), 0, 8192 * sizeof(float)));
  KArgs a = base_args(e);
  a.mode = MODE_DEBUG; a.dbg = e->d_dbg.get(); a.dbg_env = env;
  // split: the product's own pair of kernels; with the heightfield fix-up on, every contact the fix-up kernel would keep (where the
  // fleet kernel exists at that capacity); else the kernel that resets (two-per-wave: both groups replay env `env`, same dump twice)
  if (e->plan.split) e->plan.narrow.launch(e, a, e->narrow_waves, 0);
  e->plan.debug.launch(e, a, 1, 0);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipDeviceSynchronize());
  int n = capacity < 8192 ? capacity : 8192;
  HIP_TRY(hipMemcpy(host_out, e->d_dbg.get(), (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
  return COSIM_OK;
}

int cosim_profile_step(cosim_engine_t* e, const float* actions_dev, const float* commands_dev, float* state_out_dev, uint8_t* terminated_dev,
                       uint8_t* truncated_dev, double* cycles_out16) {
  if (!e || !actions_dev || !state_out_dev || !terminated_dev || !truncated_dev || !cycles_out16) return fail(COSIM_EINVAL, "cosim_profile_step: null argument");
  if (!has(e->plan.prof)) return fail(COSIM_EINVAL, "cosim_profile_step: no diagnostic kernel for this model");
  if (e->lat.tab.n_act + e->lat.tab.n_obs > 0)
    return fail(COSIM_EINVAL, "cosim_profile_step: latency is set (cosim_set_param \"latency\"): the diagnostic step advances the clocks without writing the delay lines, so a later step would deliver a stale slot; clear the latency first");
  HIP_TRY(hipSetDevice(e->device));
  int rc = upload_params(e);
  if (rc) return rc;
  rc = join_ranges(e, 0);
  if (rc) return rc;
  HIP_TRY(hipMemset(e->d_dbg.get(), 0, 8192 * sizeof(float)));
  KArgs a = base_args(e);
  a.mode = MODE_STEP; a.actions = actions_dev; a.commands = commands_dev; a.state_out = state_out_dev;
  a.terminated = terminated_dev; a.truncated = truncated_dev; a.dbg = e->d_dbg.get();
  e->stepped = true;
  e->plan.prof.launch(e, a, e->n_envs, 0);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipDeviceSynchronize());
  unsigned long long raw[32];
  HIP_TRY(hipMemcpy(raw, e->d_dbg.get(), sizeof raw, hipMemcpyDeviceToHost));
  for (int i = 0; i < 32; i++) cycles_out16[i] = (double)raw[i] / (double)(e->n_envs / e->sw.epw);   // per wave
  return COSIM_OK;
}

// Test hook: support points of mesh geom `geom` at identity pose for n_dirs directions, from the device's own support routines:
// out [n_dirs][6] = the lane-parallel routine's point, then the wave-cooperative routine's.  use_map 0: full scans of the hull.
int cosim_debug_support(cosim_engine_t* e, int geom, const float* dirs_host, int n_dirs, float* out_host, int use_map) {
  if (!e || !dirs_host || !out_host || n_dirs < 1 || geom < 0 || geom >= e->hm.ngeom) return fail(COSIM_EINVAL, "cosim_debug_support: bad argument");
  if (e->hm.rec[geom].g_type != CS_GEOM_MESH) return fail(COSIM_EINVAL, "cosim_debug_support: not a mesh geom");
  HIP_TRY(hipSetDevice(e->device));
  const char* const fn = "cosim_debug_support";
  Dev<float> d_dirs, d_out;   // scratch of this call
  HIP_TRY_AS(fn, d_dirs.upload(dirs_host, (size_t)n_dirs * 3));
  HIP_TRY_AS(fn, d_out.alloc((size_t)n_dirs * 6));
  const HullGraph H{e->d_hull_vert.get(), e->d_hull_adr.get(), e->d_hull_nbr.get(), e->d_hull_cell.get(), e->d_hull_cand.get()};
  hipLaunchKernelGGL(support_probe_kernel, dim3((n_dirs + 63) / 64), dim3(64), 0, 0, e->d_model.get(), H, geom, d_dirs.get(), n_dirs, d_out.get(), use_map);
  HIP_TRY_AS(fn, hipGetLastError());
  HIP_TRY_AS(fn, hipDeviceSynchronize());
  HIP_TRY_AS(fn, d_out.download(out_host, (size_t)n_dirs * 6));
  return COSIM_OK;
}

// Test hooks: the device's pair routines (MPR on primitives, MPR prism - primitive, box-box) on pairs given in host arrays; the engine
// handle names the device only.  Kinds without an O(1) support in these kernels are rejected (no silent zero-size geom).
namespace {
bool prim_kind(int k) { return k == CS_GEOM_SPHERE || k == CS_GEOM_CYLINDER || k == CS_GEOM_BOX; }
hipError_t dbg_finish() {
  const hipError_t r = hipGetLastError();
  return r != hipSuccess ? r : hipDeviceSynchronize();
}
}  // namespace

int cosim_debug_mpr_prims(cosim_engine_t* e, const int* kinds_host, const float* geo_host, int n, int coop, int* irec_host, float* frec_host) {
  if (!e || !kinds_host || !geo_host || !irec_host || !frec_host || n < 1) return fail(COSIM_EINVAL, "cosim_debug_mpr_prims: bad argument");
  for (int i = 0; i < 2 * n; i++)
    if (!prim_kind(kinds_host[i])) return fail(COSIM_EINVAL, "cosim_debug_mpr_prims: geom kind is not sphere / cylinder / box");
  HIP_TRY(hipSetDevice(e->device));
  const char* const fn = "cosim_debug_mpr_prims";
  Dev<int> kinds, irec;   // device buffers that live for this call
  Dev<float> geo, frec;
  HIP_TRY_AS(fn, kinds.upload(kinds_host, (size_t)n * 2));
  HIP_TRY_AS(fn, geo.upload(geo_host, (size_t)n * 20));
  HIP_TRY_AS(fn, irec.alloc((size_t)n * 3));
  HIP_TRY_AS(fn, frec.alloc((size_t)n * 7));
  if (coop) hipLaunchKernelGGL(mpr_prims_probe_kernel<true>, dim3(n), dim3(64), 0, 0, (const int*)kinds.get(), (const float*)geo.get(), n, irec.get(), frec.get());
  else hipLaunchKernelGGL(mpr_prims_probe_kernel<false>, dim3((n + 63) / 64), dim3(64), 0, 0, (const int*)kinds.get(), (const float*)geo.get(), n, irec.get(), frec.get());
  HIP_TRY_AS(fn, dbg_finish());
  HIP_TRY_AS(fn, irec.download(irec_host, (size_t)n * 3));
  HIP_TRY_AS(fn, frec.download(frec_host, (size_t)n * 7));
  return COSIM_OK;
}

int cosim_debug_mpr_prism(cosim_engine_t* e, const float* prism_host, const int* kinds_host, const float* geo_host, int n, int* irec_host, float* frec_host) {
  if (!e || !prism_host || !kinds_host || !geo_host || !irec_host || !frec_host || n < 1) return fail(COSIM_EINVAL, "cosim_debug_mpr_prism: bad argument");
  for (int i = 0; i < n; i++)
    if (!prim_kind(kinds_host[i])) return fail(COSIM_EINVAL, "cosim_debug_mpr_prism: geom kind is not sphere / cylinder / box");
  HIP_TRY(hipSetDevice(e->device));
  const char* const fn = "cosim_debug_mpr_prism";
  Dev<int> kinds, irec;
  Dev<float> prism, geo, frec;
  HIP_TRY_AS(fn, prism.upload(prism_host, (size_t)n * 10));
  HIP_TRY_AS(fn, kinds.upload(kinds_host, (size_t)n));
  HIP_TRY_AS(fn, geo.upload(geo_host, (size_t)n * 10));
  HIP_TRY_AS(fn, irec.alloc((size_t)n * 3));
  HIP_TRY_AS(fn, frec.alloc((size_t)n * 7));
  hipLaunchKernelGGL(mpr_prism_probe_kernel, dim3((n + 63) / 64), dim3(64), 0, 0, (const float*)prism.get(), (const int*)kinds.get(), (const float*)geo.get(), n, irec.get(),
                     frec.get());
  HIP_TRY_AS(fn, dbg_finish());
  HIP_TRY_AS(fn, irec.download(irec_host, (size_t)n * 3));
  HIP_TRY_AS(fn, frec.download(frec_host, (size_t)n * 7));
  return COSIM_OK;
}

int cosim_debug_box_box(cosim_engine_t* e, const float* geo_host, const float* margin_host, int n, int* count_host, float* out_host) {
  if (!e || !geo_host || !margin_host || !count_host || !out_host || n < 1) return fail(COSIM_EINVAL, "cosim_debug_box_box: bad argument");
  HIP_TRY(hipSetDevice(e->device));
  const char* const fn = "cosim_debug_box_box";
  Dev<float> geo, margin, out;
  Dev<int> cnt;
  HIP_TRY_AS(fn, geo.upload(geo_host, (size_t)n * 20));
  HIP_TRY_AS(fn, margin.upload(margin_host, (size_t)n));
  HIP_TRY_AS(fn, cnt.alloc((size_t)n));
  HIP_TRY_AS(fn, out.alloc_zeroed((size_t)n * 35));
  hipLaunchKernelGGL(box_box_probe_kernel, dim3(n), dim3(64), 0, 0, (const float*)geo.get(), (const float*)margin.get(), n, cnt.get(), out.get());
  HIP_TRY_AS(fn, dbg_finish());
  HIP_TRY_AS(fn, cnt.download(count_host, (size_t)n));
  HIP_TRY_AS(fn, out.download(out_host, (size_t)n * 35));
  return COSIM_OK;
}

// cosim_debug_forward "cholesky": both forms of the step kernels' in-register Cholesky and its solve on n matrices of order nv, one per
// wave.  io holds rows [n][64][nv] and rhs [n][64] on entry, fac [n][2][nv][nv], dinv [n][2][nv] and sol [n][2][nv] on return.
static int debug_cholesky(cosim_engine_t* e, int nv, float* io, int capacity) {
  if (nv != 18 && nv != 10 && nv != 7) return fail(COSIM_EINVAL, "cosim_debug_forward cholesky: the order is not 18, 10 or 7");
  const int per = 64 * (nv + 1), n = capacity / per;
  if (capacity < per || capacity % per) return fail(COSIM_EINVAL, "cosim_debug_forward cholesky: capacity is not n * 64 * (order + 1)");
  HIP_TRY(hipSetDevice(e->device));
  const char* const fn = "cosim_debug_forward cholesky";
  Dev<float> in, out;
  const size_t nfac = (size_t)n * 2 * nv * nv, nvec = (size_t)n * 2 * nv;   // nfac + 2 nvec < capacity: the answer fits the caller's block
  HIP_TRY_AS(fn, in.upload(io, (size_t)capacity));
  HIP_TRY_AS(fn, out.alloc_zeroed(nfac + 2 * nvec));
  const float *rows = in.get(), *rhs = rows + (size_t)n * 64 * nv;
  float *fac = out.get(), *dinv = fac + nfac, *sol = dinv + nvec;
  auto launch = [&](auto kern) { hipLaunchKernelGGL(kern, dim3(n), dim3(64), 0, 0, rows, rhs, n, fac, dinv, sol); };
  if (nv == 18) launch(chol_probe_kernel<18>); else if (nv == 10) launch(chol_probe_kernel<10>); else launch(chol_probe_kernel<7>);
  HIP_TRY_AS(fn, dbg_finish());
  HIP_TRY_AS(fn, out.download(io, nfac + 2 * nvec));
  return COSIM_OK;
}

// cosim_debug_forward "ldsbatch": both forms of the solver primitives with batched LDS reads on n problems of order nv, one per wave
// (ldsbatch_probe_kernel says what a problem holds).  io holds n blocks of 64 nv + nv nv + 3 nv floats on entry and n blocks of
// 2 (64 + 2 nv) on return.
static int debug_ldsbatch(cosim_engine_t* e, int nv, float* io, int capacity) {
  if (nv != 18 && nv != 10 && nv != 7) return fail(COSIM_EINVAL, "cosim_debug_forward ldsbatch: the order is not 18, 10 or 7");
  const int per = 64 * nv + nv * nv + 3 * nv, n = capacity / per;
  if (capacity < per || capacity % per) return fail(COSIM_EINVAL, "cosim_debug_forward ldsbatch: capacity is not n * (64 nv + nv nv + 3 nv)");
  HIP_TRY(hipSetDevice(e->device));
  const char* const fn = "cosim_debug_forward ldsbatch";
  Dev<float> in, out;
  const size_t nout = (size_t)n * 2 * (64 + 2 * nv);   // < capacity: the answer fits the caller's block
  HIP_TRY_AS(fn, in.upload(io, (size_t)capacity));
  HIP_TRY_AS(fn, out.alloc_zeroed(nout));
  auto launch = [&](auto kern) { hipLaunchKernelGGL(kern, dim3(n), dim3(64), 0, 0, (const float*)in.get(), n, out.get()); };
  if (nv == 18) launch(ldsbatch_probe_kernel<18>); else if (nv == 10) launch(ldsbatch_probe_kernel<10>); else launch(ldsbatch_probe_kernel<7>);
  HIP_TRY_AS(fn, dbg_finish());
  HIP_TRY_AS(fn, out.download(io, nout));
  return COSIM_OK;
}

int cosim_debug_counters(cosim_engine_t* e, unsigned long long* out32, int clear) {   // the 32 64-bit words diagnostic kernels accumulate into
  if (!e || !out32) return fail(COSIM_EINVAL, "cosim_debug_counters: null argument");
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(out32, e->d_dbg.get(), 32 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  if (clear) HIP_TRY(hipMemset(e->d_dbg.get(), 0, 8192 * sizeof(float)));
  return COSIM_OK;
}

int cosim_set_timing(cosim_engine_t* e, int enabled) {
  if (!e) return fail(COSIM_EINVAL, "cosim_set_timing: null engine");
  HIP_TRY(hipSetDevice(e->device));
  int rc = drain_events(e);
  if (rc) return rc;
  e->timing = enabled != 0;
  if (e->timing)   // event pool up front: creating events inside a timed loop costs host time per launch
    while (e->ev.size() < 4096) { hipEvent_t x; HIP_TRY(hipEventCreate(&x)); e->ev.push_back(x); }
  e->t_accum_ms = 0.0;
  e->t_launches = 0;
  return COSIM_OK;
}

int cosim_kernel_time(cosim_engine_t* e, float* avg_ms, int* launches) {
  if (!e || !avg_ms || !launches) return fail(COSIM_EINVAL, "cosim_kernel_time: null argument");
  HIP_TRY(hipSetDevice(e->device));
  int rc = drain_events(e);
  if (rc) return rc;
  *launches = e->t_launches;
  *avg_ms = e->t_launches ? (float)(e->t_accum_ms / e->t_launches) : 0.f;
  e->t_accum_ms = 0.0;
  e->t_launches = 0;
  return COSIM_OK;
}

}  // extern "C"
