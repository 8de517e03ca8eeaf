"""ctypes binding of ``libcosim_hip.so`` (the C ABI of ``include/cosim.h``).

PyTorch is used here only as plumbing: device buffers, streams and (in ``distributed.py``)
``torch.distributed``.  All arithmetic of the hot path happens in the HIP kernels.  There is no
CPU fallback: if the shared library is missing or no GPU is present, construction fails loudly.
"""
from __future__ import annotations

import ctypes
import os
import subprocess
from typing import Dict, Optional

import numpy as np

from .model import CosimModel

_DIR = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_DIR, "libcosim_hip.so")
CSRC = os.path.join(_DIR, "csrc")

CS_MAXFIELD = 16
CS_MAXCMD = 6
OBS_IDS = {"dof_pos": 0, "dof_vel": 1, "ang_vel": 2, "lin_vel": 3, "projected_gravity": 4, "last_action": 5,
           "height_map": 6, "command": 7}


class ObsConfig(ctypes.Structure):
    """``cosim_obs_config_t`` (include/cosim.h)."""
    _fields_ = [
        ("stack_size", ctypes.c_int), ("command_dim", ctypes.c_int),
        ("n_stacked", ctypes.c_int), ("n_non_stacked", ctypes.c_int),
        ("stacked_field", ctypes.c_int * CS_MAXFIELD), ("non_stacked_field", ctypes.c_int * CS_MAXFIELD),
        ("field_dim", ctypes.c_int * 8), ("field_interval", ctypes.c_int * 8), ("field_scale", ctypes.c_float * 8),
        ("noise_mean", ctypes.c_float * 8), ("noise_std", ctypes.c_float * 8),
        ("noise_lower", ctypes.c_float * 8), ("noise_upper", ctypes.c_float * 8),
        ("noise_enabled", ctypes.c_int), ("position_command", ctypes.c_int),
        ("command_scales", ctypes.c_float * CS_MAXCMD),
        ("max_sim_step", ctypes.c_int), ("action_delay_prob", ctypes.c_float), ("init_noise", ctypes.c_float),
        ("auto_reset", ctypes.c_int),
        ("hm_res_x", ctypes.c_int), ("hm_res_y", ctypes.c_int), ("hm_size_x", ctypes.c_float), ("hm_size_y", ctypes.c_float),
    ]


# Packed fp32 (v_pk_fma_f32) pays in the solver's long FMA chains, but the SLP vectoriser's default cost model also packs the
# quaternion / cross-product code, where the v_mov shuffles around each packed op cost more than the op saves (kinematics: 243
# moves for 237 packed ops).  Measured on MI355X, 1000-step benches, threshold 0 (default) / 1 / 2 / 3 / 4 / off: headline
# 13.00 / 13.17 / 13.23 / 13.36 / 11.87 / 11.5 M env-steps/s, p_v3_flat 7.9 / 8.3 / 8.8 / 8.3 / 7.4, w4_rocky 2.73 / 2.76 / 2.86 / 2.87 / 2.85.
HIPCC_TUNING = ["-mllvm", "-slp-threshold=2"]


def build_library(force: bool = False, verbose: bool = False) -> str:
    """Compile the HIP engine for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    # every file the translation unit pulls in (cosim_engine.hip includes the other .hip / .h files of csrc/)
    inc = os.path.join(_DIR, "..", "include")
    deps = [os.path.join(CSRC, f) for f in sorted(os.listdir(CSRC)) if f.endswith((".hip", ".h"))]
    deps += [os.path.join(inc, f) for f in sorted(os.listdir(inc)) if f.endswith(".h")]
    if not force and os.path.isfile(LIB_PATH):
        newest = max(os.path.getmtime(p) for p in deps)
        if os.path.getmtime(LIB_PATH) >= newest:
            return LIB_PATH
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-Wno-unused-value", *HIPCC_TUNING,
           "-o", LIB_PATH, os.path.join(CSRC, "cosim_engine.hip")]
    if verbose:
        cmd.append("-Rpass-analysis=kernel-resource-usage")
    subprocess.check_call(cmd)
    return LIB_PATH


_vp, _ci, _cf, _cs = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_char_p
_pci, _pvp = ctypes.POINTER(_ci), ctypes.POINTER(_vp)

# The C ABI of include/cosim.h, one row per entry point: (name, restype, argtypes).  The only place a signature is written;
# load_library applies it, EXPORTS lists its names, tests/test_python_core_host.py holds every arity against the header.
_ABI_ROWS = (
    ("cosim_create", _ci, [_vp, _vp, _vp, _vp, _vp, _vp, _ci, _ci, ctypes.c_uint64, ctypes.c_int64, _pvp]),
    ("cosim_destroy", _ci, [_vp]),
    ("cosim_query", _ci, [_vp, _cs]),
    ("cosim_set_param", _ci, [_vp, _cs, _vp, _ci]),      # also the word tables "obs_faults", "action_faults" and "search": no entry point of their own
    ("cosim_reset", _ci, [_vp] * 5),
    ("cosim_step", _ci, [_vp] * 8),
    ("cosim_step_range", _ci, [_vp, _ci, _ci] + [_vp] * 7),
    ("cosim_join", _ci, [_vp, _vp]),
    ("cosim_rollout", _ci, [_vp, _ci] + [_vp] * 7),
    ("cosim_range", _ci, [_vp, _ci, _pci, _pci, _pvp]),
    ("cosim_range_mark", _ci, [_vp, _ci]),
    ("cosim_get", _ci, [_vp, _cs, _vp, _vp]),
    ("cosim_set", _ci, [_vp, _cs, _vp, _vp]),
    ("cosim_event_push", _ci, [_vp] * 4),
    ("cosim_spawn_set", _ci, [_vp, _vp, _ci, _vp, _ci, _cf, _ci, _vp]),
    ("cosim_spawn_get", _ci, [_vp, _vp, _ci]),
    ("cosim_snapshot", _ci, [_vp] * 3),
    ("cosim_restore", _ci, [_vp, _vp, _ci, _vp, _vp, _ci, _vp]),
    ("cosim_history_set", _ci, [_vp, _ci, _ci]),
    ("cosim_history_get", _ci, [_vp, _ci, _vp, _pci, _vp]),
    ("cosim_ledger_set", _ci, [_vp, _ci]),
    ("cosim_ledger_get", _ci, [_vp] * 5),
    ("cosim_ftrace_set", _ci, [_vp, _ci, _ci, _ci]),
    ("cosim_ftrace_get", _ci, [_vp] * 5),
    ("cosim_scenario_set", _ci, [_vp, _ci] + [_vp] * 6 + [_ci, _vp, _vp, _vp]),
    ("cosim_scenario_params_set", _ci, [_vp, _ci] + [_vp] * 6),
    ("cosim_scenario_params_get", _ci, [_vp, _vp, _ci]),
    ("cosim_scenario_checks_set", _ci, [_vp, _ci] + [_vp] * 7 + [_ci]),
    ("cosim_scenario_checks_get", _ci, [_vp] * 5),
    ("cosim_scenario_curves_set", _ci, [_vp, _ci] + [_vp] * 7),
    ("cosim_scenario_curves_get", _ci, [_vp] * 3),
    ("cosim_scenario_curves_clear", _ci, [_vp]),
    ("cosim_scenario_curves_groups", _ci, [_vp, _ci, _vp]),
    ("cosim_fall_set", _ci, [_vp, _cf, _cf, _ci, _vp, _ci]),
    ("cosim_debug_forward", _ci, [_vp, _ci, _cs, _vp, _ci]),   # also the test hook "cholesky" (both forms of the in-register Cholesky): no entry point of its own
    ("cosim_debug_counters", _ci, [_vp, _vp, _ci]),
    ("cosim_debug_support", _ci, [_vp, _ci, _vp, _ci, _vp, _ci]),
    ("cosim_debug_mpr_prims", _ci, [_vp, _vp, _vp, _ci, _ci, _vp, _vp]),
    ("cosim_debug_mpr_prism", _ci, [_vp, _vp, _vp, _vp, _ci, _vp, _vp]),
    ("cosim_debug_box_box", _ci, [_vp, _vp, _vp, _ci, _vp, _vp]),
    ("cosim_hull_support_check", _ci, [_vp, _ci, _vp, _vp, _vp, _ci, _vp, _vp, _vp]),
    ("cosim_kernel_time", _ci, [_vp, ctypes.POINTER(_cf), _pci]),
    ("cosim_set_timing", _ci, [_vp, _ci]),
    ("cosim_profile_step", _ci, [_vp] * 7),
    ("cosim_policy_table_create", _ci, [_ci] + [_vp] * 6 + [_ci, _vp, _ci, _vp, _pvp]),
    ("cosim_policy_table_forward", _ci, [_vp, _vp, _vp, _ci, _cf, _vp]),
    ("cosim_policy_table_destroy", _ci, [_vp]),
    ("cosim_policy_table_rotate", _ci, [_vp, _ci]),
    ("cosim_policy_table_forward_rotating", _ci, [_vp] * 7 + [_ci, _cf, _vp]),
    ("cosim_policy_table_lists", _ci, [_vp, _ci, _vp, _vp, _pci]),
    ("cosim_recurrent_table_create", _ci, [_ci] + [_vp] * 17 + [_ci, _vp, _ci, _vp, _pvp]),
    ("cosim_recurrent_table_forward", _ci, [_vp] * 7 + [_ci, _cf, _vp]),
    ("cosim_recurrent_table_destroy", _ci, [_vp]),
    ("cosim_recurrent_table_rotate", _ci, [_vp, _ci]),
    ("cosim_recurrent_table_forward_rotating", _ci, [_vp] * 9 + [_ci, _cf, _vp]),
    ("cosim_recurrent_table_lists", _ci, [_vp, _ci, _vp, _vp, _pci]),
    ("cosim_mlp_forward", _ci, [_vp, _ci, _ci] + [_vp] * 5 + [_cf, _vp, _vp]),
    ("cosim_lstm_cell", _ci, [_vp] * 3 + [_ci] * 3 + [_vp] * 6),
    ("cosim_fleet_stats", _ci, [_vp, _ci, _ci, _ci, _vp, _ci, _ci, _vp, _vp]),
    ("cosim_fleet_hist", _ci, [_vp, _ci, _ci, _ci, _vp, _ci, _ci, _vp, _ci, _vp, _vp]),
    ("cosim_last_error", _cs, []),
    ("cosim_model_sizeof", _ci, []),
    ("cosim_obs_config_sizeof", _ci, []),
)
ABI = {name: (restype, argtypes) for name, restype, argtypes in _ABI_ROWS}
EXPORTS = list(ABI)
# include/cosim_actor.h, the same way (tests/test_actor_graph_host.py holds it against that header)
ABI_ACTOR = {
    "cosim_mlp_forward_ex": (_ci, [_vp, _ci, _ci] + [_vp] * 6 + [_cf, _vp, _vp]),
    "cosim_policy_table_create_ex": (_ci, [_ci] + [_vp] * 7 + [_ci, _vp, _ci, _vp, _pvp]),
}

_lib = None


def load_library():
    """Load ``libcosim_hip.so`` and type every entry point from ``ABI``; raises if it has not been built (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    # torch first: libcosim_hip.so must bind to the HIP runtime torch has loaded (torch ships its own libamdhip64);
    # two HIP runtimes in one process do not see each other's devices, streams or allocations.
    import torch  # noqa: F401
    if not os.path.isfile(LIB_PATH):
        raise RuntimeError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(the HIP engine has no CPU fallback)")
    L = ctypes.CDLL(LIB_PATH)
    for name, (restype, argtypes) in {**ABI, **ABI_ACTOR}.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = restype, argtypes
    if L.cosim_model_sizeof() != ctypes.sizeof(CosimModel):
        raise RuntimeError("cosim_model_t layout mismatch between include/cosim_model.h and libcosim_hip.so: rebuild")
    if L.cosim_obs_config_sizeof() != ctypes.sizeof(ObsConfig):
        raise RuntimeError("cosim_obs_config_t layout mismatch: rebuild libcosim_hip.so")
    _lib = L
    return L


def make_obs_config(config: dict, obs_to_dim: Dict[str, int], control_freq: float, auto_reset: bool) -> ObsConfig:
    """Flatten config["observation"/"env"/"random"] into ``cosim_obs_config_t``.

    Mirrors the constructor-time checks of the reference wrappers: unknown observation names raise ``KeyError``
    (wrappers.py:116-117), non-positive frequencies raise ``ValueError`` (:186-187).
    """
    ob = config["observation"]
    c = ObsConfig()
    c.stack_size = int(ob["stack_size"])
    c.command_dim = int(ob["command_dim"])
    if c.command_dim < 0:
        raise AssertionError("command_dim must be equal or greater than 0.")
    if c.command_dim > CS_MAXCMD:
        raise ValueError(f"Invalid 'command_dim': expected 0> or <7; but got {c.command_dim}.")
    stacked, non_stacked = list(ob["stacked_obs_order"]), list(ob["non_stacked_obs_order"])
    if len(stacked) > CS_MAXFIELD or len(non_stacked) > CS_MAXFIELD:
        raise ValueError("too many observation fields")
    c.n_stacked, c.n_non_stacked = len(stacked), len(non_stacked)
    for i, n in enumerate(stacked):
        c.stacked_field[i] = OBS_IDS[n] if n in OBS_IDS else _unknown(n, obs_to_dim)
    for i, n in enumerate(non_stacked):
        c.non_stacked_field[i] = OBS_IDS[n] if n in OBS_IDS else _unknown(n, obs_to_dim)
    level = config["random"]["sensor_noise"]
    noise = config["random_table"]["sensor_noise"][level]
    for name, fid in OBS_IDS.items():
        c.field_dim[fid] = int(obs_to_dim[name])
        c.field_interval[fid] = 1
        c.field_scale[fid] = 1.0
        c.noise_std[fid] = 1.0
        if name in stacked + non_stacked and name != "command":
            n_cfg = ob[name]
            freq, scale = float(n_cfg["freq"]), float(n_cfg["scale"])
            if freq <= 0:
                raise ValueError(f"Invalid observation update frequency for '{name}': {freq}. Must be > 0.")
            c.field_interval[fid] = max(1, int(round(control_freq / freq)))
            c.field_scale[fid] = scale
        if name in noise:
            c.noise_mean[fid], c.noise_std[fid] = float(noise[name]["mean"]), float(noise[name]["std"])
            c.noise_lower[fid], c.noise_upper[fid] = float(noise[name]["lower"]), float(noise[name]["upper"])
    # level "none" perturbs by <= 1e-8 in the reference (random_table.yaml:25-55): below fp32 resolution, skipped
    c.noise_enabled = int(level != "none")
    c.position_command = int(bool(config["env"]["position_command"]))
    for i in range(c.command_dim):
        c.command_scales[i] = float(ob["command_scales"][str(i)])
    c.max_sim_step = int(config["env"]["max_duration"] * control_freq)
    c.action_delay_prob = float(config["random"]["action_delay_prob"])
    c.init_noise = float(config["random"]["init_noise"])
    c.auto_reset = int(auto_reset)
    hm = ob.get("height_map")
    if hm is not None:
        if config["env"]["terrain"] == "flat" and ("height_map" in list(ob["stacked_obs_order"]) + list(ob["non_stacked_obs_order"])):
            # the reference samples the map with mj_rayHfield on the ground geom (utils/mujoco_utils.py:169), which is an error
            # on the plane that terrain "flat" turns the ground into (xml_manager.py:24-28)
            raise ValueError("the height_map observation needs a heightfield terrain (mj_rayHfield rejects the plane of terrain 'flat')")
        c.hm_res_x, c.hm_res_y = int(hm["res_x"]), int(hm["res_y"])
        c.hm_size_x, c.hm_size_y = float(hm["size_x"]), float(hm["size_y"])
    return c


def _unknown(name, obs_to_dim):
    return obs_to_dim[name]  # raises KeyError like wrappers.py:116 does for names no env provides


def _columns(arrays, dtypes):
    """The host arrays of a CSR table, each contiguous in the dtype its column has in the C ABI."""
    arrays = tuple(arrays)
    if len(arrays) != len(dtypes):
        raise ValueError(f"expected {len(dtypes)} table arrays, got {len(arrays)}")
    return [np.ascontiguousarray(x, dtype=dt) for x, dt in zip(arrays, dtypes)]


class Engine:
    """Owning handle of one ``cosim_engine_t``; thin, typed wrappers over the C entry points."""

    def __init__(self, compiled, obs_cfg: ObsConfig, num_envs: int, device: int = 0, seed: int = 0, env_id0: int = 0):
        self.L = load_library()
        self.compiled = compiled
        self._keep = (np.ascontiguousarray(compiled.hull_vert, dtype=np.float32),
                      np.ascontiguousarray(compiled.hull_adr, dtype=np.int32),
                      np.ascontiguousarray(compiled.hull_nbr, dtype=np.int32),
                      np.ascontiguousarray(compiled.hfield, dtype=np.float32))
        h = ctypes.c_void_p()
        rc = self.L.cosim_create(ctypes.addressof(compiled.blob), self._keep[0].ctypes.data, self._keep[1].ctypes.data,
                                 self._keep[2].ctypes.data, self._keep[3].ctypes.data, ctypes.addressof(obs_cfg),
                                 int(num_envs), int(device), ctypes.c_uint64(seed & (2 ** 64 - 1)), ctypes.c_int64(env_id0),
                                 ctypes.byref(h))
        self._check(rc)
        self.h = h
        self.num_envs = num_envs
        self.device = device

    def _check(self, rc: int):
        if rc < 0:
            msg = self.L.cosim_last_error().decode()
            if rc == -1:
                raise ValueError(msg)
            raise RuntimeError(msg)
        return rc

    def close(self):
        if getattr(self, "h", None):
            self.L.cosim_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def query(self, name: str) -> int:
        return self._check(self.L.cosim_query(self.h, name.encode()))

    def set_param(self, name: str, values: np.ndarray):
        v = np.ascontiguousarray(values, dtype=np.float32)
        self._check(self.L.cosim_set_param(self.h, name.encode(), v.ctypes.data, int(v.size)))

    def reset(self, mask_ptr, commands_ptr, state_out_ptr, stream=None):
        self._check(self.L.cosim_reset(self.h, mask_ptr, commands_ptr, state_out_ptr, stream))

    def step(self, actions_ptr, commands_ptr, state_out_ptr, term_ptr, trunc_ptr, info_ptr, stream=None):
        self._check(self.L.cosim_step(self.h, actions_ptr, commands_ptr, state_out_ptr, term_ptr, trunc_ptr, info_ptr, stream))

    def step_range(self, first, count, actions_ptr, commands_ptr, state_out_ptr, term_ptr, trunc_ptr, info_ptr, stream=None):
        self._check(self.L.cosim_step_range(self.h, int(first), int(count), actions_ptr, commands_ptr, state_out_ptr, term_ptr, trunc_ptr,
                                            info_ptr, stream))

    def rollout(self, steps, actions_ptr, commands_ptr, state_out_ptr, term_ptr, trunc_ptr, info_ptr, stream=None):
        self._check(self.L.cosim_rollout(self.h, int(steps), actions_ptr, commands_ptr, state_out_ptr, term_ptr, trunc_ptr, info_ptr, stream))

    def join(self, stream=None):
        self._check(self.L.cosim_join(self.h, stream))

    def range(self, i: int):
        """(first env, env count, hipStream_t or None) of range ``i`` (``cosim_range``)."""
        first, count, st = ctypes.c_int(), ctypes.c_int(), ctypes.c_void_p()
        self._check(self.L.cosim_range(self.h, int(i), ctypes.byref(first), ctypes.byref(count), ctypes.byref(st)))
        return first.value, count.value, st.value

    def range_mark(self, i: int):
        self._check(self.L.cosim_range_mark(self.h, int(i)))

    def get(self, name: str, out_ptr, stream=None):
        self._check(self.L.cosim_get(self.h, name.encode(), out_ptr, stream))

    def set(self, name: str, in_ptr, stream=None):
        self._check(self.L.cosim_set(self.h, name.encode(), in_ptr, stream))

    def push(self, v_ptr, mask_ptr, stream=None):
        self._check(self.L.cosim_event_push(self.h, v_ptr, mask_ptr, stream))

    def spawn_set(self, xyyaw: np.ndarray, footprint: np.ndarray, clearance: float, per_episode: bool, stream=None):
        """``cosim_spawn_set``: ``xyyaw`` [M, 3] (M = 0 clears the table), ``footprint`` [G, 4] = (ox, oy, r, free) per ground geom."""
        xy = np.ascontiguousarray(xyyaw, dtype=np.float32).reshape(-1, 3)
        fp = np.ascontiguousarray(footprint, dtype=np.float32).reshape(-1, 4)
        self._check(self.L.cosim_spawn_set(self.h, xy.ctypes.data, int(xy.shape[0]), fp.ctypes.data, int(fp.shape[0]),
                                           ctypes.c_float(clearance), int(bool(per_episode)), stream))

    def spawn_get(self) -> np.ndarray:
        """``cosim_spawn_get``: the placed poses, host float32 [M, 7] = x, y, z, qw, qx, qy, qz."""
        out = np.zeros((self.query("spawn_rows"), 7), dtype=np.float32)
        self._check(self.L.cosim_spawn_get(self.h, out.ctypes.data, int(out.shape[0])))
        return out

    def snapshot(self, out_ptr, stream=None):
        """``cosim_snapshot``: every env's row into ``out_ptr`` ``[N, snapshot_floats]``."""
        self._check(self.L.cosim_snapshot(self.h, out_ptr, stream))

    def restore(self, snap_ptr, snap_rows: int, src_ptr=None, mask_ptr=None, with_params: bool = False, stream=None):
        """``cosim_restore``: env ``d`` takes row ``src[d]`` (``None``: row ``d``) of a ``[snap_rows, snapshot_floats]`` buffer."""
        self._check(self.L.cosim_restore(self.h, snap_ptr, int(snap_rows), src_ptr, mask_ptr, int(bool(with_params)), stream))

    def history_set(self, slots: int, every: int):
        self._check(self.L.cosim_history_set(self.h, int(slots), int(every)))

    def history_get(self, age: int, out_ptr, stream=None) -> int:
        """``cosim_history_get``: capture ``age`` (0 = newest) into ``out_ptr``; returns how many ``step`` calls ago it was taken."""
        ago = ctypes.c_int()
        self._check(self.L.cosim_history_get(self.h, int(age), out_ptr, ctypes.byref(ago), stream))
        return ago.value

    def ledger_set(self, slots: int):
        """``cosim_ledger_set``: a ring of ``slots`` episode records per env (0: off)."""
        self._check(self.L.cosim_ledger_set(self.h, int(slots)))

    def ledger_get(self, records_ptr, counts_ptr, open_ptr=None, stream=None):
        """``cosim_ledger_get``: rings ``[N, slots, 16]``, ended-episode counts ``[N]`` and (or ``None``) open rows ``[N, 16]``, int32."""
        self._check(self.L.cosim_ledger_get(self.h, records_ptr, counts_ptr, open_ptr, stream))

    def ftrace_set(self, frames: int, keep: int, on_mask: int):
        """``cosim_ftrace_set``: a window of ``frames`` control steps and ``keep`` frozen traces per env (``frames`` 0: off)."""
        self._check(self.L.cosim_ftrace_set(self.h, int(frames), int(keep), int(on_mask)))

    def ftrace_get(self, buffers_ptr, counts_ptr, open_ptr=None, stream=None):
        """``cosim_ftrace_get``: buffers ``[N, keep + 1, 16 + frames * F]``, counters ``[N, 3]`` (working buffer, triggered, lost) and
        (or ``None``) open headers ``[N, 16]``, int32."""
        self._check(self.L.cosim_ftrace_get(self.h, buffers_ptr, counts_ptr, open_ptr, stream))

    def _csr_set(self, who: str, csr, dtypes, t_width: int, tail=()):
        """The body the ``scenario_*_set`` wrappers share: ``csr`` = ``(adr [S + 1], t [n, t_width], one column [n] per entry of
        dtypes)`` goes to entry point ``cosim_<who>`` as contiguous host arrays, followed by the integers ``tail``; ``None`` clears
        (S = 0, null arrays, zeros for ``tail``).  ``who`` is also the word the two refusals begin with."""
        fn = getattr(self.L, "cosim_" + who)
        if csr is None:
            self._check(fn(self.h, 0, *[None] * (2 + len(dtypes)), *[0] * len(tail)))
            return
        adr, t, *cols = _columns(csr, (np.int32, np.int32, *dtypes))
        if adr.ndim != 1 or adr.size < 1:
            raise ValueError(f"{who}: adr must be [S + 1]")
        n = int(max(adr.max(), 0))
        if t.size < t_width * n or min(c.size for c in cols) < n:   # (the engine reads the arrays up to the addresses)
            raise ValueError(f"{who}: the item arrays are shorter than their row addresses ({n} items)")
        self._check(fn(self.h, int(adr.size) - 1, adr.ctypes.data, t.ctypes.data, *[c.ctypes.data for c in cols], *tail))

    def scenario_set(self, csr, mode: int, cmd_out_ptr, row_out_ptr, stream=None):
        """``cosim_scenario_set``: ``csr`` = the six host arrays ``(key_adr, key_t, key_cmd, push_adr, push_t, push_v)`` of
        ``ScenarioTable.pack`` (``None``: clear the table); ``cmd_out_ptr`` ``[N, command_dim]`` float32 and ``row_out_ptr`` ``[N]``
        int32 are persistent device buffers the caller keeps alive."""
        if csr is None:
            self._check(self.L.cosim_scenario_set(self.h, 0, None, None, None, None, None, None, 0, None, None, stream))
            return
        ka, kt, kc, pa, pt, pv = _columns(csr, (np.int32, np.int32, np.float32, np.int32, np.int32, np.float32))
        if ka.shape != pa.shape or ka.ndim != 1 or ka.size < 1:
            raise ValueError("scenario_set: key_adr and push_adr must both be [S + 1]")
        nk, npw, cd = int(max(ka.max(), 0)), int(max(pa.max(), 0)), self.query("command_dim")
        if kt.size < nk or kc.size < nk * cd or pt.size < 2 * npw or pv.size < 3 * npw:   # (the engine reads the arrays up to the addresses)
            raise ValueError(f"scenario_set: the table arrays are shorter than their row addresses ({nk} keyframes, {npw} push windows)")
        self._check(self.L.cosim_scenario_set(self.h, int(ka.size) - 1, ka.ctypes.data, kt.ctypes.data, kc.ctypes.data, pa.ctypes.data,
                                              pt.ctypes.data, pv.ctypes.data, int(mode), cmd_out_ptr, row_out_ptr, stream))

    def scenario_params_set(self, csr):
        """``cosim_scenario_params_set``: ``csr`` = the six host arrays ``(adr, t, field, index, op, value)`` of
        ``ScenarioTable.pack_params`` (``None``: clear the windows)."""
        self._csr_set("scenario_params_set", csr, (np.int32, np.int32, np.int32, np.float32), 2)

    def _word_table_set(self, who: str, param: bytes, csr):
        """The body of the two setters that have no entry point of their own: ``csr`` = the six host arrays ``(adr, t, elem, op, ord,
        value)`` (``None``: clear), sent through ``cosim_set_param`` ``param`` as one table of 32-bit words ``S | adr | t | elem | op |
        ord | value`` (include/cosim.h)."""
        if csr is None:
            words = np.zeros(1, dtype=np.int32)
        else:
            adr, t, *cols = _columns(csr, (np.int32, np.int32, np.int32, np.int32, np.int32, np.float32))
            if adr.ndim != 1 or adr.size < 1:
                raise ValueError(f"{who}: adr must be [S + 1]")
            n = int(max(adr[-1], 0))
            if t.size != 2 * n or any(c.size != n for c in cols):  # (the engine reads the arrays by the last address)
                raise ValueError(f"{who}: the item arrays are shorter than their row addresses ({n} items)"
                                 if t.size < 2 * n or min(c.size for c in cols) < n else
                                 f"{who}: the item arrays are longer than their row addresses ({n} items)")
            words = np.concatenate([np.array([adr.size - 1], dtype=np.int32), adr, t.reshape(-1), *[c.view(np.int32).reshape(-1) for c in cols]])
        words = np.ascontiguousarray(words, dtype=np.int32)
        self._check(self.L.cosim_set_param(self.h, param, words.ctypes.data, int(words.size)))

    def scenario_faults_set(self, csr):
        """Observation faults, through ``cosim_set_param "obs_faults"`` (they have no entry point of their own): ``csr`` = the six host
        arrays ``(adr, t, elem, op, ord, value)`` of ``ScenarioTable.pack_faults`` (``None``: clear the faults), sent as one table of
        32-bit words ``S | adr | t | elem | op | ord | value`` (include/cosim.h)."""
        self._word_table_set("scenario_faults_set", b"obs_faults", csr)

    def scenario_action_faults_set(self, csr):
        """Action faults, through ``cosim_set_param "action_faults"``: ``csr`` = the six host arrays ``(adr, t, actuator, op, ord,
        value)`` of ``ScenarioTable.pack_action_faults`` (``None``: clear the faults), the word table of the observation faults."""
        self._word_table_set("scenario_action_faults_set", b"action_faults", csr)

    def latency_set(self, words):
        """Latency lines, through ``cosim_set_param "latency"``: ``words`` = the int32 word table of ``ScenarioTable.pack_latency`` (``S |
        act_adr | obs_adr | act[na][6] | obs[no][6]``, an item being ``(t0, t1, element, ord, steps, jitter)``; ``None``: clear the
        latency)."""
        words = np.zeros(1, dtype=np.int32) if words is None else np.ascontiguousarray(words, dtype=np.int32).reshape(-1)
        self._check(self.L.cosim_set_param(self.h, b"latency", words.ctypes.data, int(words.size)))

    def search_set(self, words):
        """Limit search, through ``cosim_set_param "search"``: ``words`` = the int32 word table of ``ScenarioTable.pack_search`` (``S |
        slots | has | lo | hi | x0 | d0 | d_min | rule | trials | targets | fail_mask | rev_skip``, in its long form ``| harder | chk_lo |
        chk_hi``; ``None``: clear the search)."""
        words = np.zeros(1, dtype=np.int32) if words is None else np.ascontiguousarray(words, dtype=np.int32).reshape(-1)
        self._check(self.L.cosim_set_param(self.h, b"search", words.ctypes.data, int(words.size)))

    def scenario_checks_set(self, csr, slots: int = 0):
        """``cosim_scenario_checks_set``: ``csr`` = the seven host arrays ``(adr, t, signal, index, mode, cmp, bound)`` of
        ``ScenarioTable.pack_checks`` (``None``: clear the checks); ``slots`` verdict records per env."""
        self._csr_set("scenario_checks_set", csr, (np.int32, np.int32, np.int32, np.int32, np.float32), 2, (int(slots),))

    def scenario_checks_get(self, records_ptr, counts_ptr, open_ptr=None, stream=None):
        """``cosim_scenario_checks_get``: rings ``[N, slots, words]``, ended-episode counts ``[N]`` and (or ``None``) open rows ``[N,
        words]``, int32."""
        self._check(self.L.cosim_scenario_checks_get(self.h, records_ptr, counts_ptr, open_ptr, stream))

    def scenario_curves_set(self, csr):
        """``cosim_scenario_curves_set``: ``csr`` = the seven host arrays ``(adr, t [n, 3], signal, index, lo, hi, bins)`` of
        ``ScenarioTable.pack_curves`` (``None``: clear the curves)."""
        self._csr_set("scenario_curves_set", csr, (np.int32, np.int32, np.float32, np.float32, np.int32), 3)

    def scenario_curves_groups(self, n_groups: int, group_ptr=None):
        """``cosim_scenario_curves_groups``: the cells become ``n_groups`` planes keyed by the int32 ``[N]`` device words at ``group_ptr``
        (the caller keeps them alive); ``n_groups = 0``: no groups.  Every call empties the cells."""
        self._check(self.L.cosim_scenario_curves_groups(self.h, int(n_groups), group_ptr))

    def scenario_curves_get(self, cells_ptr, stream=None):
        """``cosim_scenario_curves_get``: the cells, uint32 ``[max(scenario_curve_groups, 1) * scenario_curve_words]``."""
        self._check(self.L.cosim_scenario_curves_get(self.h, cells_ptr, stream))

    def scenario_curves_clear(self):
        """``cosim_scenario_curves_clear``: empty cells, every env's episode begun anew."""
        self._check(self.L.cosim_scenario_curves_clear(self.h))

    def scenario_params_get(self) -> np.ndarray:
        """``cosim_scenario_params_get``: the effective parameter records, host float32 ``[N, param_stride]``."""
        out = np.zeros((self.num_envs, self.query("param_stride")), dtype=np.float32)
        self._check(self.L.cosim_scenario_params_get(self.h, out.ctypes.data, int(out.size)))
        return out

    def fall_set(self, min_up: float, min_height: float, grace_steps: int, body_ids=None):
        """``cosim_fall_set``: ``min_up <= -1`` / ``min_height <= 0`` switch the tilt / height rule off; ``body_ids`` ``None`` leaves the
        model's own ``_is_done`` list alone, an int array (possibly empty) replaces it."""
        if body_ids is None:
            self._check(self.L.cosim_fall_set(self.h, ctypes.c_float(min_up), ctypes.c_float(min_height), int(grace_steps), None, -1))
            return
        ids = np.ascontiguousarray(body_ids, dtype=np.int32).reshape(-1)
        self._check(self.L.cosim_fall_set(self.h, ctypes.c_float(min_up), ctypes.c_float(min_height), int(grace_steps),
                                          ids.ctypes.data if ids.size else None, int(ids.size)))

    def debug_forward(self, env: int) -> np.ndarray:
        out = np.zeros(8192, dtype=np.float32)
        self._check(self.L.cosim_debug_forward(self.h, int(env), b"all", out.ctypes.data, out.size))
        return out

    def profile_step(self, actions_ptr, commands_ptr, state_out_ptr, term_ptr, trunc_ptr) -> np.ndarray:
        out = np.zeros(32, dtype=np.float64)
        self._check(self.L.cosim_profile_step(self.h, actions_ptr, commands_ptr, state_out_ptr, term_ptr, trunc_ptr, out.ctypes.data))
        return out

    def debug_counters(self, clear: bool = True) -> np.ndarray:
        out = np.zeros(32, dtype=np.uint64)
        self._check(self.L.cosim_debug_counters(self.h, out.ctypes.data, int(clear)))
        return out

    def set_timing(self, enabled: bool):
        self._check(self.L.cosim_set_timing(self.h, int(enabled)))

    def kernel_time(self):
        ms, n = ctypes.c_float(), ctypes.c_int()
        self._check(self.L.cosim_kernel_time(self.h, ctypes.byref(ms), ctypes.byref(n)))
        return ms.value, n.value
