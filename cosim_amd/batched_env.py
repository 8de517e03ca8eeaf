"""``BatchedEnv`` — N environment instances on one MI355X behind the reference's env API.

Host-side mirror of the reference's wrapper stack for the batched case: one object plays
``CommandWrapper(TimeLimitWrapper(StateBuildWrapper(<Robot>(config))))`` (reference
``envs/build.py:8-24``) for ``num_envs`` instances at once.  Method names, argument meaning
and error behaviour follow ``envs/wrappers.py``; tensors carry a leading ``[N]`` dimension and
live on the GPU (torch is used for device memory and streams only).  All per-step arithmetic —
command transform, delay filter, PD law, physics substeps, observation build — runs inside
``cosim_step`` (one HIP kernel launch per control step).
"""
from __future__ import annotations

from typing import Dict, Optional

import os

import numpy as np

from . import rng as crng
from .compile import CompiledModel, compile_model, env_constants
from .engine import Engine, make_obs_config
from .model import get_field
from .robots import ROBOTS, obs_to_dim as robot_obs_to_dim
from .scenario import FAULT_KINDS


def _cmd_slices(stacked, non_stacked, dims, stack_size, command_dim):
    """``StateBuildWrapper._get_cmd_index_cache`` (wrappers.py:129-158)."""
    out = []
    if command_dim <= 0:
        return out
    stacked_dim = sum(dims[n] for n in stacked)
    off, starts = 0, []
    for n in stacked:
        if n == "command":
            starts.append(off)
        off += dims[n]
    for k in range(stack_size):
        for s in starts:
            out.append(slice(k * stacked_dim + s, k * stacked_dim + s + command_dim))
    base, off = stack_size * stacked_dim, 0
    for n in non_stacked:
        if n == "command":
            out.append(slice(base + off, base + off + command_dim))
        off += dims[n]
    return out


def draw_env_params(config: dict, cm: CompiledModel, seed: int, gids, gain_noise: float = 0.0) -> Dict[str, np.ndarray]:
    """Per-env domain randomisation as pure functions of (seed, global env id): body masses (XMLManager step 3, reference
    manager/xml_manager.py:43-55: ``mass += U(-m k, +m k)`` on the listed bodies, ``+ load`` on the base) and PD gains
    (table value x U(1 - g, 1 + g)).  Shared by ``BatchedEnv`` and by the CPU twin of a fleet env (oracle/fleet.py)."""
    blob = cm.blob
    gids = np.asarray(gids, dtype=np.uint64)
    N, nb, nu = len(gids), blob.nbody, blob.nu
    mass = np.tile(np.array(get_field(blob, "body_mass")[:nb]), (N, 1))
    k, load = config["random"]["mass_noise"], config["random"]["load"]
    robot = ROBOTS[config["env"]["id"]]
    for name in robot["mass_bodies"]:
        b = cm.body_names.index(name)
        m0 = mass[:, b].copy()
        u = crng.uniform(seed, gids, 0, crng.PURPOSE_MASS, b).astype(np.float64)
        mass[:, b] = m0 + (2.0 * u - 1.0) * m0 * k
        if name == robot["base_body"]:
            mass[:, b] += load
    kp = np.tile(np.array(get_field(blob, "ctl_kp")[:nu]), (N, 1))
    kd = np.tile(np.array(get_field(blob, "ctl_kd")[:nu]), (N, 1))
    if gain_noise > 0:
        idx = np.arange(nu)[None, :]
        up = crng.uniform(seed, gids[:, None], 0, crng.PURPOSE_GAIN, idx)
        ud = crng.uniform(seed, gids[:, None], 1, crng.PURPOSE_GAIN, idx)
        kp = kp * (1.0 + gain_noise * (2.0 * up - 1.0))
        kd = kd * (1.0 + gain_noise * (2.0 * ud - 1.0))
    return {"body_mass": mass, "kp": kp, "kd": kd}


# COSIM_* overrides of engine parameters for A/B and tuning runs, applied by the constructor in this order: (variable, parameter,
# tolerate-refusal -- the engine may refuse a variant the model's kernels do not have, and the run goes on without it)
_ENV_OVERRIDES = (
    ("COSIM_WAVE_PRIORITY", "wave_priority", False),       # "base,t1,t2,t3"
    ("COSIM_CONTACT_TWIST", "contact_twist", True),        # "1": dense-row kernel -> its contact-twist variant
    ("COSIM_LS_SCALE", "ls_tolerance_scale", False),       # line-search gradient tolerance multiplier
    ("COSIM_PAIR_MODE", "pair_mode", False),               # "1": hull pairs wave-cooperative
    ("COSIM_SPLIT", "split", True),                        # split pipeline of the heightfield humanoid kernels
    ("COSIM_NARROW_WAVES", "narrow_waves", True),
    ("COSIM_NARROW_OCC", "narrow_occupancy", True),
    ("COSIM_ENVS_PER_WAVE", "envs_per_wave", True),        # 1 | 2: overrides the engine's choice where the variant exists
)


class _Data:
    """What ``get_data()`` hands out: batched ``qpos`` / ``qvel`` views (reference: the MjData object)."""

    def __init__(self, qpos, qvel):
        self.qpos, self.qvel = qpos, qvel


class BatchedEnv:
    def __init__(self, config: dict, num_envs: Optional[int] = None, device: Optional[int] = None, seed: Optional[int] = None,
                 auto_reset: bool = True, env_id0: int = 0, gain_noise: float = 0.0, compiled: Optional[CompiledModel] = None,
                 ranges: Optional[int] = None, deferred_join: Optional[bool] = None, hfield_fixup: Optional[bool] = None,
                 spawn=None, history=None, ledger: Optional[int] = None, scenarios=None, scenario_mode: Optional[str] = None,
                 fall=None, failure_traces=None, streams: Optional[int] = None, check_slots: Optional[int] = None,
                 curves: Optional[bool] = None, search: Optional[int] = None):
        """``ranges`` > 1: ``step()`` issues the fleet as that many launches over contiguous env ranges on engine-owned HIP streams
        (``cosim_set_param "ranges"``).  With ``deferred_join`` the caller's stream is NOT made to wait for them inside ``step()``:
        call ``join()`` before consuming ``state`` / ``terminated`` / ``info`` on the current stream (``get_data``, ``reset``,
        ``event``, ``set_state`` and ``solver_stats`` join by themselves).  That is what lets a range's next control step overlap
        the tail of the others' current one; it fits callers whose next action does not need the whole fleet's last state (an
        action table; a policy evaluated per range on ``range_streams``).  With a deferred join the ``action`` tensor of a step must
        stay untouched until that step has run (at most two steps are in flight: an action table or three rotating buffers), and
        ``receive_user_command`` joins first.  Defaults: ``config["engine"]`` / 1 / False.

        ``streams``: how many engine-owned streams carry the ranges (``cosim_set_param "range_streams"``).  Default (``None`` / 0): as
        many as the process has hardware queues for -- half of ``GPU_MAX_HW_QUEUES`` (4 when unset), at most one per range.  With
        fewer streams than ranges, consecutive ranges form a group that is stepped as one launch sequence over their union:
        ``range_list`` keeps the ``ranges`` entries, the ``range_streams`` of a group are one and the same stream, and the results
        are the same bit for bit.  ``engine.query("range_streams")`` reports the number in use.

        ``hfield_fixup`` (heightfield terrain, opt-in): a control step -- on the split pipeline of humanoid_p_v0 a substep -- whose
        ground contacts exceed the fleet kernel's slots is redone by a kernel with 50 slots per ground geom (the most the narrowphase
        emits) instead of being cut off and counted in ``dropped_contacts`` (``cosim_set_param "hfield_fixup"``).  Raises
        ``ValueError`` where the engine has no such kernel (the plane).  Default: ``config["engine"]`` / False.

        ``spawn``: a spawn table -- an ``[M, 3]`` array of ``(x, y, yaw)`` or a dict ``{"pattern": "grid" | "uniform" | "poses",
        "count", "extent", "yaw", "per_episode", "clearance", "poses"}`` (``cosim_amd/spawn.py``) -- see ``set_spawn``.  Default:
        ``config["engine"].get("spawn")`` / none: every reset goes to the model's ``init_qpos``.

        ``history``: ``(slots, every)`` -- the engine keeps a ring of ``slots`` full-state captures, one after every ``every``-th
        ``step()`` (``cosim_history_set``), see ``history()``.  Default: ``config["engine"].get("history")`` / none.

        ``ledger``: slots -- the engine keeps the last ``slots`` (1..4096) episode records of every env on the device
        (``cosim_ledger_set``), see ``ledger()``.  Default: ``config["engine"].get("ledger")`` / none.

        ``scenarios``: a scenario table -- a ``ScenarioTable``, a list of scenarios, ``{"scenarios": [...]}`` or a YAML file
        (``cosim_amd/scenario.py``) -- with ``scenario_mode`` ``"env"`` (default) or ``"cycle"``, see ``set_scenarios``.  Default:
        ``config["engine"].get("scenarios")`` / ``config["engine"].get("scenario_mode")`` / none.

        ``check_slots``: arm the checks the scenario table holds (a scenario's ``"checks"``, ``cosim_amd/scenario.py``): the engine
        judges them on the device and keeps the last ``check_slots`` (1..64) verdict records of every env, see ``set_scenarios`` /
        ``verdicts()``.  Default: ``config["engine"].get("check_slots")`` / none: a table's checks are carried but not evaluated,
        and no launch, pointer or byte differs from a table without checks.

        ``curves``: arm the response curves the scenario table holds (a scenario's ``"curves"``, ``cosim_amd/scenario.py``): the engine
        keeps per-scenario ensemble time series on the device, see ``set_scenarios`` / ``curves()``.  Default:
        ``config["engine"].get("curves")`` / off: a table's curves are carried but not armed, and no launch, pointer or byte differs
        from a table without curves.

        ``search``: arm the limit search the scenario table holds (a scenario's ``"search"``, ``cosim_amd/scenario.py``): every env of
        such a row keeps a level that scales the row's pushes / commands and moves when its episodes end, and the engine keeps the
        last ``search`` (1..64) trial records of every env, see ``set_scenarios`` / ``search()``.  Needs ``auto_reset`` and mode
        ``"env"``.  Default: ``config["engine"].get("search")`` / none: a table's items are carried but not armed, and no launch,
        pointer or byte differs from a table without them.

        ``fall``: a fall rule -- a ``FallRule`` or a dict ``{"tilt", "height", "grace", "bodies"}`` (``cosim_amd/fall.py``) -- see
        ``set_fall``.  Default: ``config["engine"].get("fall")`` / none: an episode ends early only through the robot's own
        ``_is_done``.

        ``failure_traces``: ``(frames, keep)`` or ``{"frames", "keep", "on"}`` -- the engine keeps every env's last ``frames``
        control steps and freezes them as a trace when an episode ends with a selected cause (``cosim_ftrace_set``), see
        ``set_failure_traces`` / ``failure_traces()``.  Default: ``config["engine"].get("failure_traces")`` / none; ``False``: none
        whatever the config says."""
        import torch  # plumbing only

        eng_cfg = config.get("engine", {})
        self.config = config
        self.id = config["env"]["id"]
        if self.id not in ROBOTS:
            raise NameError(f"Please select a valid environment id. Received '{self.id}'.")
        self.num_envs = int(num_envs if num_envs is not None else eng_cfg.get("num_envs", 1))
        self.seed = int(seed if seed is not None else eng_cfg.get("seed", 0))
        dev = int(device if device is not None else eng_cfg.get("device", 0))
        if not torch.cuda.is_available():
            raise RuntimeError("BatchedEnv needs an AMD GPU (torch.cuda.is_available() is False); there is no CPU fallback")
        self.torch = torch
        self.device = torch.device(f"cuda:{dev}")
        self.env_id0 = int(env_id0)

        # robot-env constructor checks (flamingo_light_v1.py:36-42)
        level = config["random"]["precision"]
        ptab = config["random_table"]["precision"][level]
        self.dt_ = ptab["timestep"]
        self.frame_skip = ptab["frame_skip"]
        self.control_freq = 1 / (self.dt_ * self.frame_skip)
        assert self.control_freq == 50, "Currently, only control frequency of 50 is supported."

        self.cm = compiled if compiled is not None else compile_model(config)
        blob = self.cm.blob
        self.action_dim = blob.nu
        self.nq, self.nv = blob.nq, blob.nv
        self.obs_to_dim = robot_obs_to_dim(self.id, config)
        ob = config["observation"]
        self.command_dim = ob["command_dim"]
        assert self.command_dim >= 0, "command_dim must be equal or greater than 0."
        self.stack_size = int(ob["stack_size"])
        self.stacked_obs_order = list(ob["stacked_obs_order"])
        self.non_stacked_obs_order = list(ob["non_stacked_obs_order"])
        self._stacked_obs_dim = sum(self.obs_to_dim[n] for n in self.stacked_obs_order)
        self._non_stacked_obs_dim = sum(self.obs_to_dim[n] for n in self.non_stacked_obs_order)
        self.state_dim = self.stack_size * self._stacked_obs_dim + self._non_stacked_obs_dim
        self.cmd_slices = _cmd_slices(self.stacked_obs_order, self.non_stacked_obs_order, self.obs_to_dim,
                                      self.stack_size, self.command_dim)
        self.max_sim_step = int(config["env"]["max_duration"] * self.control_freq)
        self.auto_reset = bool(auto_reset)

        obs_cfg = make_obs_config(config, self.obs_to_dim, self.control_freq, self.auto_reset)
        self.engine = Engine(self.cm, obs_cfg, self.num_envs, dev, self.seed, self.env_id0)
        assert self.engine.query("state_dim") == self.state_dim
        self.info_dim = self.engine.query("info_dim")
        for var, name, tolerant in _ENV_OVERRIDES:
            if os.environ.get(var):
                try:
                    self.engine.set_param(name, np.array([float(x) for x in os.environ[var].split(",")]))
                except (ValueError, RuntimeError):
                    if not tolerant:
                        raise

        self.hfield_fixup = bool(hfield_fixup if hfield_fixup is not None else eng_cfg.get("hfield_fixup", False))
        if self.hfield_fixup:
            self.engine.set_param("hfield_fixup", np.array([1.0]))

        self.ranges = int(ranges if ranges is not None else os.environ.get("COSIM_RANGES", eng_cfg.get("ranges", 1)))
        self.ranges = max(1, min(self.ranges, self.num_envs, 16))
        self.deferred_join = bool(deferred_join if deferred_join is not None else eng_cfg.get("deferred_join", False))
        self.range_list = [(0, self.num_envs)]
        self.range_streams = [None]
        if self.ranges > 1:
            streams = streams if streams is not None else os.environ.get("COSIM_RANGE_STREAMS")   # (the variable: A/B runs of unchanged callers)
            if streams:
                self.engine.set_param("range_streams", np.array([float(streams)]))
            self.engine.set_param("ranges", np.array([float(self.ranges)]))
            self.engine.set_param("deferred_join", np.array([float(self.deferred_join)]))
            if os.environ.get("COSIM_INFLIGHT"):               # steps the host may run ahead of each range stream (tuning runs)
                self.engine.set_param("inflight", np.array([float(os.environ["COSIM_INFLIGHT"])]))
            rl = [self.engine.range(i) for i in range(self.ranges)]
            self.range_list = [(f, c) for f, c, _ in rl]
            self.range_streams = [torch.cuda.ExternalStream(st, device=self.device) for _, _, st in rl]

        self.fall_rule = None
        fall = fall if fall is not None else eng_cfg.get("fall")
        if fall is not None:
            self.set_fall(fall)

        self._randomise(gain_noise)
        spawn = spawn if spawn is not None else eng_cfg.get("spawn")
        if spawn is not None:
            self.set_spawn(spawn)

        N, t = self.num_envs, torch
        f32 = dict(dtype=t.float32, device=self.device)
        self.state = t.zeros((N, self.state_dim), **f32)
        self.terminated = t.zeros((N,), dtype=t.uint8, device=self.device)
        self.truncated = t.zeros((N,), dtype=t.uint8, device=self.device)
        self.info_buf = t.zeros((N, self.info_dim), **f32)
        self.user_command = t.zeros((N, max(self.command_dim, 1)), **f32)
        self._qpos = t.zeros((N, self.nq), **f32)
        self._qvel = t.zeros((N, self.nv), **f32)
        self.reset_flag = False
        self.control_steps = 0          # control steps since the last whole-fleet reset (a restore sets it to the snapshot's)
        self.history_cfg = None
        history = history if history is not None else eng_cfg.get("history")
        if history is not None and int(history[0]) > 0:
            self.history_cfg = (int(history[0]), int(history[1]))
            self.engine.history_set(*self.history_cfg)
        self.ledger_slots = 0
        ledger = ledger if ledger is not None else eng_cfg.get("ledger")
        if ledger is not None and int(ledger) != 0:
            self.set_ledger(int(ledger))
        self.failure_traces_cfg = None
        failure_traces = failure_traces if failure_traces is not None else eng_cfg.get("failure_traces")
        if failure_traces is not None and failure_traces is not False:   # False: off whatever the config says
            self.set_failure_traces(failure_traces)
        self.scenario_table, self.scenario_mode = None, "env"
        self._cmd_out = self._row_out = None
        self.check_slots = 0
        self.curves_armed = False
        self.search_slots = 0
        self._search_marked, self._search_checks = (), False   # fault kinds whose items the armed search marks; it fails on a check
        self._curve_groups = None                                   # (tensor, G, names) of set_curve_groups: the tensor is kept alive here
        scenarios = scenarios if scenarios is not None else eng_cfg.get("scenarios")
        if scenarios is not None:
            self.set_scenarios(scenarios, scenario_mode if scenario_mode is not None else eng_cfg.get("scenario_mode", "env"),
                               check_slots=check_slots if check_slots is not None else eng_cfg.get("check_slots"),
                               curves=curves if curves is not None else eng_cfg.get("curves"),
                               search=search if search is not None else eng_cfg.get("search"))

    # ------------------------------------------------------------------ domain randomisation (XMLManager step 3)
    def _randomise(self, gain_noise: float):
        gids = np.arange(self.env_id0, self.env_id0 + self.num_envs, dtype=np.uint64)
        p = draw_env_params(self.config, self.cm, self.seed, gids, gain_noise)
        self.body_mass, self.kp, self.kd = p["body_mass"], p["kp"], p["kd"]
        c = env_constants(self.cm, self.body_mass)
        self.engine.set_param("body_mass", self.body_mass)
        self.engine.set_param("body_invweight0", c["body_invweight0"][:, :, 0])
        self.engine.set_param("dof_invweight0", c["dof_invweight0"])
        self.engine.set_param("meaninertia", c["meaninertia"])
        if gain_noise > 0:
            self.engine.set_param("kp", self.kp)
            self.engine.set_param("kd", self.kd)

    # ------------------------------------------------------------------ BaseEnv API (wrappers.py:8-85), batched
    def _stream(self):
        return self.torch.cuda.current_stream(self.device).cuda_stream

    def _cmd_ptr(self):
        return self.user_command.data_ptr() if self.command_dim > 0 else None

    def _mask_ptr(self, mask):
        """``(mask as a contiguous uint8 device tensor, its pointer)`` of an env mask, ``(None, None)`` for none."""
        if mask is None:
            return None, None
        mask = self.torch.as_tensor(mask, device=self.device).to(self.torch.uint8).contiguous()
        return mask, mask.data_ptr()

    def receive_user_command(self, user_command):
        """Store the raw user command(s); scaling / position-mode transform happen in the next kernel launch
        from the pre-step pose, exactly where ``CommandWrapper.receive_user_command`` reads ``get_data()``."""
        t = self.torch
        if not t.is_tensor(user_command):
            # the same command as last time (the reference's loop re-sends it every step, core/tester.py:68): nothing to write
            host = np.ascontiguousarray(user_command, dtype=np.float32)
            last = getattr(self, "_last_cmd_host", None)
            if last is not None and last.shape == host.shape and np.array_equal(last, host):
                return
            self._last_cmd_host = host.copy()
        else:
            self._last_cmd_host = None
        uc = t.as_tensor(user_command, dtype=t.float32, device=self.device)
        if uc.ndim == 1:
            uc = uc[None, :].expand(self.num_envs, -1)
        if self.config["env"]["position_command"] is not False:
            assert self.command_dim == 2, f"Currently, position command only support 2 dimenstion, but got {self.command_dim}."
        if self.ranges > 1 and self.deferred_join:
            self.engine.join(self._stream())          # steps in flight still read the command buffer: write it behind them
        self.user_command[:, :self.command_dim] = uc[:, :self.command_dim]

    def reset(self, mask=None):
        mask, mptr = self._mask_ptr(mask)
        self.engine.reset(mptr, self._cmd_ptr(), self.state.data_ptr(), self._stream())
        self.reset_flag = True
        if mask is None:
            self.control_steps = 0
        return self.state, {}

    def step(self, action):
        assert self.reset_flag is True, "Call 'reset()' before calling 'step()'."
        t = self.torch
        a = t.as_tensor(action, dtype=t.float32, device=self.device)
        if a.shape != (self.num_envs, self.action_dim):
            raise ValueError(f"Action dimension mismatch. Expected {(self.num_envs, self.action_dim)}, found {tuple(a.shape)}")
        a = a.contiguous()
        self.engine.step(a.data_ptr(), self._cmd_ptr(), self.state.data_ptr(), self.terminated.data_ptr(),
                         self.truncated.data_ptr(), self.info_buf.data_ptr(), self._stream())
        self.control_steps += 1
        if self.command_dim < 0 or self.command_dim > 6:
            raise ValueError(f"Invalid 'command_dim': expected 0> or <7; but got {self.command_dim}.")
        return self.state, self.terminated, self.truncated, self._info(a)

    def rollout(self, actions, info: bool = True):
        """``len(actions)`` control steps of the whole fleet under an action table ``[K, N, action_dim]`` in one launch per range
        (``cosim_rollout``: the reference's ``Tester.test`` loop, core/tester.py:66-97, with the policy replaced by a lookup).
        Returns ``(states [K, N, state_dim], terminated [K, N], truncated [K, N], info_buf [K, N, info_dim] or None)``: row k is what
        ``step(actions[k])`` would have returned (auto-reset included).  ``self.state`` etc. keep the last row."""
        assert self.reset_flag is True, "Call 'reset()' before calling 'step()'."
        if self.scenario_table is not None and self.scenario_table.has_latency:
            raise ValueError("rollout(): latency is set and the delay lines are written between steps, which one rollout launch does not leave; "
                             "step() or set a table without 'latency'")
        if self.scenario_table is not None:
            raise ValueError("rollout(): a scenario table is set and one rollout launch reads one command row; step() or set_scenarios(None)")
        if self.failure_traces_cfg is not None:
            raise ValueError("rollout(): failure traces are set and one rollout launch leaves one state record for all its steps; step() or set_failure_traces(None)")
        if self.ledger_slots > 0 and not info:
            raise ValueError("rollout(info=False): a ledger is set and is built from the info rows; pass info=True or set_ledger(0)")
        t = self.torch
        a = t.as_tensor(actions, dtype=t.float32, device=self.device).contiguous()
        if a.ndim != 3 or tuple(a.shape[1:]) != (self.num_envs, self.action_dim):
            raise ValueError(f"Action table mismatch. Expected [K, {self.num_envs}, {self.action_dim}], found {tuple(a.shape)}")
        K = a.shape[0]
        states = t.empty((K, self.num_envs, self.state_dim), dtype=t.float32, device=self.device)
        term = t.empty((K, self.num_envs), dtype=t.uint8, device=self.device)
        trunc = t.empty((K, self.num_envs), dtype=t.uint8, device=self.device)
        inf = t.empty((K, self.num_envs, self.info_dim), dtype=t.float32, device=self.device) if info else None
        self.engine.rollout(K, a.data_ptr(), self._cmd_ptr(), states.data_ptr(), term.data_ptr(), trunc.data_ptr(),
                            inf.data_ptr() if info else None, self._stream())
        self.control_steps += K
        self.state.copy_(states[-1]); self.terminated.copy_(term[-1]); self.truncated.copy_(trunc[-1])
        if info:
            self.info_buf.copy_(inf[-1])
        return states, term, trunc, inf

    def step_range(self, first: int, count: int, action):
        """One control step of envs ``[first, first + count)`` on the current stream (``cosim_step_range``): ``action`` is the
        whole fleet's ``[N, action_dim]`` tensor; outputs land in the fleet's ``state`` / ``terminated`` / ``truncated`` /
        ``info_buf`` rows of that range.  Stepping the fleet as S such shards on S streams pipelines control steps across shards."""
        assert self.reset_flag is True, "Call 'reset()' before calling 'step()'."
        if tuple(action.shape) != (self.num_envs, self.action_dim) or not action.is_contiguous():
            raise ValueError(f"Action dimension mismatch. Expected contiguous {(self.num_envs, self.action_dim)}, found {tuple(action.shape)}")
        self.engine.step_range(first, count, action.data_ptr(), self._cmd_ptr(), self.state.data_ptr(), self.terminated.data_ptr(),
                               self.truncated.data_ptr(), self.info_buf.data_ptr(), self._stream())
        if first + count == self.num_envs:
            self.control_steps += 1

    def join(self):
        """Deferred join: make the current stream wait for every range stream's work so far (``cosim_join``)."""
        self.engine.join(self._stream())

    def range_mark(self, i: int):
        """After enqueuing work of your own on ``range_streams[i]``: the next ``join()`` waits for it too (``cosim_range_mark``)."""
        self.engine.range_mark(i)

    def _info(self, action) -> Dict[str, object]:
        """Batched ``_get_info`` + ``user_command_i`` (flamingo_light_v1.py:166-183; wrappers.py:399-400)."""
        info = getattr(self, "_info_views", None)
        if info is None:   # views of the fleet's fixed buffers: built once, handed out every step (only "action" changes)
            nu, b = self.action_dim, self.info_buf
            info = {
                "dt": self.dt_ * self.frame_skip,
                "action": action,
                "action_diff_RMSE": b[:, 0],
                "lin_vel_x": b[:, 1],
                "lin_vel_y": b[:, 2],
                "ang_vel_yaw": b[:, 3],
                "torque": b[:, 4:4 + nu],
                "set_points": b[:, 4 + nu:4 + 2 * nu],
                "state": b[:, 4 + 2 * nu:],
            }
            for i in range(self.command_dim):
                info[f"user_command_{i}"] = self.applied_command[:, i]
            self._info_views = info
        info = dict(info)
        info["action"] = action
        return info

    def event(self, event: str, value, mask=None):
        if event == "push":
            t = self.torch
            v = t.as_tensor(value, dtype=t.float32, device=self.device).reshape(-1, 3)
            if v.shape[0] == 1:
                v = v.expand(self.num_envs, 3)
            v = v.contiguous()
            mask, mptr = self._mask_ptr(mask)
            self.engine.push(v.data_ptr(), mptr, self._stream())
        else:
            raise NotImplementedError(f"event:{event} is not supported.")

    def get_data(self):
        self.engine.get("qpos", self._qpos.data_ptr(), self._stream())
        self.engine.get("qvel", self._qvel.data_ptr(), self._stream())
        return _Data(self._qpos, self._qvel)

    def set_state(self, qpos=None, qvel=None, qacc_warmstart=None):
        """Test / checkpoint hook: overwrite the physics state of all envs."""
        t = self.torch
        for name, v in (("qpos", qpos), ("qvel", qvel), ("qacc_warmstart", qacc_warmstart)):
            if v is not None:
                x = t.as_tensor(v, dtype=t.float32, device=self.device).contiguous()
                self.engine.set(name, x.data_ptr(), self._stream())
                t.cuda.synchronize(self.device)

    # ------------------------------------------------------------------ snapshots (cosim_snapshot / cosim_restore / history ring)
    def snapshot_meta(self) -> dict:
        """What a snapshot of this env records about where it came from, and what ``restore`` compares (``snapshot.META_FIELDS``).
        Neither the scenario table nor the fall rule is part of it: set them again on the env you restore into."""
        return {"env_id": self.id, "terrain": self.config["env"]["terrain"], "precision": self.config["random"]["precision"],
                "snapshot_floats": self.engine.query("snapshot_floats"), "state_stride": self.engine.query("state_stride"),
                "param_stride": self.engine.query("param_stride"), "state_dim": self.state_dim, "n_envs": self.num_envs,
                "env_id0": self.env_id0, "seed": self.seed}

    def snapshot(self, policy=None):
        """The whole fleet's state, bit for bit: engine rows (state record + parameter record of every env, ``cosim_snapshot``), the
        last observation, the command buffer and the control-step count; with ``policy`` also ``policy.state()``.  Joins the range
        streams; asynchronous on the current stream otherwise.  ``restore`` of it into this env -- or, through ``Snapshot.save`` /
        ``load``, into an env built the same way in another process -- continues with the same bits."""
        from .snapshot import Snapshot
        t = self.torch
        meta = self.snapshot_meta()
        rows = t.empty((self.num_envs, meta["snapshot_floats"]), dtype=t.float32, device=self.device)
        self.engine.snapshot(rows.data_ptr(), self._stream())      # (joins: state / user_command below are the newest step's)
        return Snapshot(rows, self.state.clone(), self.user_command.clone(), self.control_steps, meta,
                        policy.state() if policy is not None else None)

    def restore(self, snap, src=None, mask=None, params: bool = False):
        """Env ``d`` takes row ``src[d]`` of ``snap`` (``None``: row ``d``; the snapshot must then have ``num_envs`` rows); envs with
        ``mask[d] == 0`` are left untouched.  ``params=False`` keeps every env's own parameter record (the robot in slot ``d`` keeps
        its masses and gains); ``True`` restores it with the state.  One gather launch (``cosim_restore``).  Raises ``ValueError``
        naming the first metadata field that disagrees with this env, or the first ``src`` entry outside the snapshot (those envs are
        left untouched).  Returns the restored observation rows ``[N, state_dim]`` -- ``self.state``, which is what the interrupted
        loop would feed its policy next -- or ``None`` for a snapshot without observation rows (``history()``): the engine keeps no
        observation per ring slot and does not rebuild it (the applied command of the last step is not in the record), so a
        policy that needs the observation gets it from the first ``step()`` after the restore.
        A restored env in slot ``d`` draws from slot ``d``'s random streams (they are keyed by the global env id).  The diagnostic
        counters (``solver_stats()``) are part of the rows and go back with them."""
        from .snapshot import check_compatible
        t = self.torch
        check_compatible(snap.meta, self.snapshot_meta(), need_n_envs=src is None)
        rows = t.as_tensor(snap.rows, dtype=t.float32, device=self.device).contiguous()
        if rows.ndim != 2 or rows.shape[1] != snap.meta["snapshot_floats"]:
            raise ValueError(f"snapshot rows have shape {tuple(rows.shape)}, expected [M, {snap.meta['snapshot_floats']}]")
        if src is None and rows.shape[0] != self.num_envs:
            raise ValueError(f"snapshot holds {rows.shape[0]} rows, this env has {self.num_envs} (give src to pick rows)")
        sptr = None
        if src is not None:
            src = t.as_tensor(src, device=self.device).to(t.int32).contiguous()
            if tuple(src.shape) != (self.num_envs,):
                raise ValueError(f"src must have shape ({self.num_envs},), found {tuple(src.shape)}")
            sptr = src.data_ptr()
        mask, mptr = self._mask_ptr(mask)
        if mask is not None and tuple(mask.shape) != (self.num_envs,):
            raise ValueError(f"mask must have shape ({self.num_envs},), found {tuple(mask.shape)}")
        # (the engine validates src before anything below indexes with it)
        self.engine.restore(rows.data_ptr(), rows.shape[0], sptr, mptr, params, self._stream())
        self.reset_flag = True
        if mask is None:
            self.control_steps = snap.steps

        def put(dst, rows_):
            x = t.as_tensor(rows_, dtype=t.float32, device=self.device)
            if src is not None:
                x = x[src.long()]
            if mask is not None:
                x = t.where(mask.bool()[:, None], x, dst)
            dst.copy_(x)
        if snap.command is not None:
            self._last_cmd_host = None
            put(self.user_command, snap.command)
        if snap.obs is None:
            return None
        put(self.state, snap.obs)
        return self.state

    def fork(self, snap, row: int, params: bool = True):
        """Every env starts from row ``row`` of ``snap`` (``restore`` with a constant ``src``), by default with that env's parameter
        record.  The forks share no random streams with their source or each other: every stream is keyed by the global id of the
        slot an env runs in, so they differ exactly where the randomisation says they should (noise, action delay, spawn draws)."""
        row = int(row)
        if not 0 <= row < snap.num_rows:
            raise ValueError(f"fork: row {row} outside the snapshot's {snap.num_rows} rows")
        return self.restore(snap, src=self.torch.full((self.num_envs,), row, dtype=self.torch.int32, device=self.device), params=params)

    def history(self, age: int = 0):
        """Capture ``age`` of the history ring (0 = newest; ``history=(slots, every)``) as a ``Snapshot`` whose ``steps`` is the
        control step it was taken after.  It carries the engine rows only (``obs`` / ``command`` are ``None``): see ``restore``.
        Raises ``ValueError`` if ``age >= slots`` or that capture does not exist yet.  Joins the range streams."""
        from .snapshot import Snapshot
        t = self.torch
        meta = self.snapshot_meta()
        rows = t.empty((self.num_envs, meta["snapshot_floats"]), dtype=t.float32, device=self.device)
        ago = self.engine.history_get(age, rows.data_ptr(), self._stream())
        snap = Snapshot(rows, None, None, self.control_steps - ago, meta)
        snap.steps_ago = ago
        return snap

    def _read_records(self, get, ring_shape, count_shape, open_shape, include_open: bool):
        """The reader under ``ledger()`` / ``failure_traces()`` / ``verdicts()``: one ``get(rings, counts, open rows or None, stream)``
        into fresh int32 device tensors of the given per-env shapes, one synchronisation, then the three as host arrays (the
        ``from_raw`` arguments; the open rows ``None`` unless ``include_open``)."""
        t = self.torch
        rec = t.empty((self.num_envs, *ring_shape), dtype=t.int32, device=self.device)
        cnt = t.empty((self.num_envs, *count_shape), dtype=t.int32, device=self.device)
        opn = t.empty((self.num_envs, *open_shape), dtype=t.int32, device=self.device) if include_open else None
        get(rec.data_ptr(), cnt.data_ptr(), opn.data_ptr() if include_open else None, self._stream())
        t.cuda.current_stream(self.device).synchronize()
        return rec.cpu().numpy(), cnt.cpu().numpy(), opn.cpu().numpy() if include_open else None

    def _meta_words(self):
        """The engine's 16 meta words of every env as an int32 device tensor ``[N, 16]``.  Joins and synchronises."""
        t = self.torch
        buf = t.zeros((self.num_envs, 16), dtype=t.float32, device=self.device)
        self.engine.get("meta", buf.data_ptr(), self._stream())
        t.cuda.synchronize(self.device)
        return buf.view(t.int32)

    # ------------------------------------------------------------------ episode ledger (cosim_ledger_set / cosim_ledger_get)
    def set_ledger(self, slots: int):
        """Keep the last ``slots`` episode records of every env on the device (0: switch the ledger off and free it).  Every env
        starts an open episode at length 0; a later ``reset()`` starts it again.  Raises ``ValueError`` outside 0..4096.  Blocks
        until the device is idle (it allocates)."""
        self.engine.ledger_set(int(slots))
        self.ledger_slots = int(slots)

    def ledger(self, include_open: bool = False):
        """The fleet's episodes so far as an ``EpisodeLedger`` (``cosim_amd/ledger.py``): one row per ended episode still in the
        ring, sorted by (global env id, episode), each with its length, how it ended (terminated / truncated / after a non-finite
        state / not begun at a reset), the spawn row it started from and the episode's mean and peak tracking error, torque and
        action change.  ``include_open``: also the episodes still running (flag 16).  An episode the host cut -- ``reset()`` of its
        env, ``restore``, ``set_state`` -- is discarded, not recorded.  Joins the range streams and reads the device once; nothing is
        read per step.  The ledger is not part of a ``snapshot()``.  Raises ``ValueError`` if no ledger is set."""
        from .ledger import WORDS, EpisodeLedger
        if self.ledger_slots <= 0:
            raise ValueError("ledger(): no ledger is set (BatchedEnv(ledger=SLOTS) or set_ledger)")
        return EpisodeLedger.from_raw(*self._read_records(self.engine.ledger_get, (self.ledger_slots, WORDS), (), (WORDS,), include_open),
                                      self.env_id0)

    # ------------------------------------------------------------------ failure traces (cosim_ftrace_set / cosim_ftrace_get)
    def set_failure_traces(self, spec, on=None):
        """Keep every env's last ``frames`` control steps on the device and freeze them as a trace when an episode ends with a
        selected cause: ``spec`` is ``(frames, keep)`` or ``{"frames", "keep", "on"}`` (frames 1..1024, the ``keep`` 1..64 newest
        traces per env stay), ``None`` switches the feature off and frees its buffers.  ``on``: names out of ``"terminated"``,
        ``"truncated"``, ``"nonfinite"``, ``"tilt"``, ``"height"``, ``"contact"`` -- default ``("terminated", "nonfinite")``:
        everything but a plain time limit.  A frame is one control step: the state it started from, the action, the applied command,
        the info row and the flags (``cosim_amd/ftrace.py``); the engine copies it on every range's own stream, inside a captured
        graph, under a deferred join, with no host read.  The ``action`` tensor of a step must stay untouched until that step has run
        (it is read behind the step).  Every env starts in an empty window; ``reset()``, ``restore`` and ``set_state`` empty the
        windows of the envs they touch.  Set traces and the ledger together (both in the constructor) and their episode ordinals
        agree.  Limits: a scenario push applied ahead of a step shows in the next frame's state and in the info row, not in the
        frame's own state; the pose a terminal step ends in is not captured (the last frame holds the pose one control step earlier
        and the terminal info row); traces are not part of a ``snapshot()``; ``rollout()`` raises while traces are set.  Raises
        ``ValueError`` naming the value out of range or the unknown name.  Blocks until the device is idle (it allocates)."""
        from .ftrace import resolve
        if spec is None:
            self.engine.ftrace_set(0, 0, 0)
            self.failure_traces_cfg = None
            return
        frames, keep, mask = resolve(spec, on)
        self.failure_traces_cfg = None
        self.engine.ftrace_set(frames, keep, mask)
        self.failure_traces_cfg = (frames, keep, mask)

    def failure_traces(self, include_open: bool = False):
        """The fleet's kept traces as a ``FailureTraces`` (``cosim_amd/ftrace.py``): one row per trace, sorted by (global env id,
        episode), with the frames in time order.  ``include_open``: also the windows still running (flag 16).  Joins the range
        streams and reads the device once.  Raises ``ValueError`` if no traces are set."""
        from .ftrace import HDR, FailureTraces
        if self.failure_traces_cfg is None:
            raise ValueError("failure_traces(): no failure traces are set (BatchedEnv(failure_traces=(FRAMES, KEEP)) or set_failure_traces)")
        frames, keep, mask = self.failure_traces_cfg
        F = self.engine.query("ftrace_frame_words")
        dims = {"nq": self.nq, "nv": self.nv, "nu": self.action_dim, "command_dim": self.command_dim, "info_dim": self.info_dim}
        return FailureTraces.from_raw(*self._read_records(self.engine.ftrace_get, (keep + 1, HDR + frames * F), (3,), (HDR,), include_open),
                                      dims, mask, self.env_id0)

    # ------------------------------------------------------------------ fall rules (cosim_fall_set)
    def set_fall(self, rule):
        """End episodes on the robot's posture: ``rule`` is a ``FallRule``, a dict of its arguments (``tilt`` radians, ``height``
        metres, ``grace`` control steps, ``bodies`` names) or ``None`` to clear it (``cosim_amd/fall.py``).  The step kernel tests
        the pose every control step ends in -- inside ``step()``, every step of a ``rollout()``, the fix-up kernels, the split
        pipeline -- and a rule that fires ends the episode there like any other end: ``terminated``, the info row of the fallen
        step, the auto-reset and its observation, ``episodes_ended``, the ledger record (flags 32 tilt / 64 height / 128 body
        contact), the next scenario in mode ``"cycle"``.  ``end_cause()`` tells why.  ``bodies`` replaces the robot's own
        ``_is_done`` body list (``[]``: no body rule) until the rule is cleared.  Limits: tilt and height are tested on single
        steps, from episode step ``grace + 1`` on; the body rule knows no grace; the thresholds are kernel arguments, so a captured
        graph keeps the rule it was captured with -- set the rule before capturing; the rule is not part of a ``snapshot()`` (set
        it again on the env you restore into).  Raises ``ValueError`` naming the field or the body the model does not have.  Blocks
        until the device is idle when the body list changes."""
        from .fall import FallRule
        rule = FallRule.build(rule)
        if rule is not None and rule.is_off():
            rule = None
        if rule is None:
            self.engine.fall_set(-1.0, 0.0, 0, None)
            self.fall_rule = None
            return
        ids = rule.body_ids(self.cm.body_names)
        self.engine.fall_set(rule.min_up, rule.min_height, rule.grace, ids)
        self.fall_rule = rule

    def end_cause(self):
        """Per env: why its latest episode ended while a fall rule was set -- int32 tensor ``[N]``, engine meta word 15: bit 1 tilt,
        2 height, 4 body contact, 0 for a time limit, a non-finite state or no end yet.  Joins and synchronises."""
        return self._meta_words()[:, 15].clone()

    # ------------------------------------------------------------------ scenario table (cosim_scenario_set)
    def set_scenarios(self, scenarios, mode: str = "env", check_slots: Optional[int] = None, curves: Optional[bool] = None,
                      search: Optional[int] = None):
        """Give every env its own test: a table of S scenarios, each a command schedule and a push schedule keyed by the env's own
        episode step (``cosim_amd/scenario.py``; ``None`` clears the table).  Env with global id ``g`` runs row ``g mod S`` (mode
        ``"env"``) or, in mode ``"cycle"`` (needs ``auto_reset``), row ``(g + episodes it has ended) mod S``: one scenario per
        episode.  The engine applies the schedule on the device ahead of every control step -- on every range's own stream, inside a
        captured graph, under a deferred join -- with no host read: a keyframe replaces the env's whole command row
        (``applied_command``; before a scenario's first keyframe ``user_command`` passes through), a push window sets ``qvel[0:3]``
        before every step it covers, bit for bit as ``event("push")`` does.  A table of the sizes of the one that is set is rewritten in
        place (captured graphs pick it up).  The schedule is a function of the state record alone: ``restore`` continues it, a fork
        follows its slot's id, shards with the same table give one fleet's results.  Limits: the table is not part of a
        ``snapshot()``; host commands and pushes still work, a scenario keyframe / push due in the same step overrides them;
        ``rollout()`` raises while a table is set.  Raises ``ValueError`` naming the scenario and the row for a malformed table.
        Joins the range streams and blocks until the device is idle.

        Observation faults ride with the table (a scenario's ``"faults"``, ``cosim_set_param "obs_faults"``): behind every control step
        and reset one small kernel changes what the policy SEES of the envs whose scenario holds an item at the observation's own
        clock -- the newest frame of ``state`` and of the record's observation stack, so the next step's roll carries the faulted
        frame on -- and nothing else; ``obs_faults()`` returns the expanded items.  They act from the next ``step()`` / ``reset()`` on.

        Action faults ride with the table too (a scenario's ``"action_faults"``, ``cosim_set_param "action_faults"``): ahead of every
        control step one small kernel writes the EFFECTIVE action of every env -- the caller's action with the items applied that hold
        at the env's pre-step episode clock -- and the step kernels are handed that buffer instead of ``actions``; ``last_action`` in
        the observation stays the policy's own output.  ``action_faults()`` returns the expanded items, ``effective_action()`` what the
        last step's kernels were handed.  They act from the next ``step()`` on.  Limits: set before capturing a graph; not part of a
        ``snapshot()`` (nothing is kept per env: the same table set again continues bit for bit).

        Latency rides with the table too (a scenario's ``"latency"``, ``cosim_set_param "latency"``): k-step delays of the command
        channel and of observation elements, served by per-env delay lines on the device ahead of the fault kernels at the same two
        sites; ``latency()`` returns the expanded items.  A table with the same items per scenario whose delays fit the lines' depth
        is rewritten in place and keeps the lines; any other restarts them.  Limits: set before capturing a graph; the lines are not
        part of a ``snapshot()``: ``restore`` / ``fork`` / ``set_state`` restart the lines of the envs they touch.

        ``check_slots`` (1..64) arms the table's checks (``cosim_scenario_checks_set``): behind every control step the engine samples
        every item of the env's scenario whose window holds at the step's pre-step episode clock -- the clock this step's keyframes
        and pushes were keyed on -- and closes the items into one verdict record when the episode ends, on the device, with no host
        read; ``verdicts()`` reads them.  Every call begins every env's episode anew for the checks (flag 8 on a stepped fleet);
        ``reset()``, ``restore`` and ``set_state`` do so for the envs they touch, and an episode the host cuts leaves no record.
        Items of the same counts are rewritten in place (captured graphs pick them up).  ``None`` / 0: the checks are not
        evaluated (what an earlier call armed is cleared).  Set the ledger, the traces and the checks together and their episode
        ordinals agree.  Limits: state signals take no sample on a step that ends the episode; checks are not part of a
        ``snapshot()``.

        ``curves=True`` arms the table's response curves (``cosim_scenario_curves_set``): behind every control step the engine stages
        one sample of every curve item of the env's scenario that is due at the step's pre-step episode clock, and when the episode
        ends folds its samples into the cells of (scenario, item, outcome) with integer atomics, on the device, with no host read;
        ``curves()`` reads them.  Every call empties the cells and begins every env's episode anew for the curves; ``reset()``,
        ``restore`` and ``set_state`` discard what the envs they touch had staged, so an episode the host cuts is in no cell.  Items
        of the same counts and sizes are rewritten in place (captured graphs pick them up; groups set by ``set_curve_groups`` stay).
        Any other call FORGETS the groups of ``set_curve_groups`` -- the cells they split are freed -- so set them again.  ``None`` /
        ``False``: the curves are not armed (what an earlier call armed is cleared).  Limits: state signals take no sample on a step that ends the episode; open
        episodes are not in the cells; curves are not part of a ``snapshot()``.

        ``search`` (1..64) arms the table's limit search (``cosim_set_param "search"``): every env whose scenario holds a
        ``"search"`` item keeps a level -- ``search_levels()`` -- that the scenario kernel multiplies into the row's push vectors
        and / or command keyframes; behind the step that ends an episode of the env a small rule on the device judges it by the
        ledger's flags (``fail_on``) and moves the level: down after a failure, up after a pass, by a step that halves.  An episode is
        a counted trial only if it began at a reset (one that began at ``restore`` / ``set_state`` may have missed its push window);
        after ``trials`` counted trials the env is done and its level frozen.  The last ``search`` trial records of every env are kept;
        ``search()`` reads records and trials, ``search_remaining()`` one word.  A call with the same scenarios holding items and the
        same ``search`` rewrites the items in place and KEEPS the records (captured graphs pick the new bounds up); any other call
        begins every search anew.  ``None`` / 0: the search is not armed (what an earlier call armed is cleared).  Set the ledger and
        the search together and their episode ordinals agree.  Needs ``auto_reset`` and mode ``"env"``.  A ``"tilt"`` / ``"height"`` /
        ``"contact"`` in ``fail_on`` while no fall rule is set is accepted and never fires.  An item whose ``targets`` name
        ``"params"`` / ``"faults"`` / ``"action_faults"`` (or ``"kind:i,j"``) has the level multiplied into the values of those listed items (the items
        are sent marked, behind the search: the engine takes them only while it is armed); ``"harder": "down"`` moves the level up
        after a failure; a ``"checks"`` / ``"check:NAME"`` / ``"check:I"`` in ``fail_on`` fails a trial whose selected check did not
        pass and needs ``check_slots``.  Limits: the records are not part of a ``snapshot()``; per-rank thresholds are not merged."""
        from .scenario import MODES, ScenarioTable
        t = self.torch
        if scenarios is None:
            self.engine.scenario_set(None, 0, None, None, self._stream())
            self._drop_scenarios()
            return
        if mode not in MODES:
            raise ValueError(f"set_scenarios: mode must be 'env' or 'cycle', got {mode!r}")
        table = ScenarioTable.build(scenarios, self.command_dim)
        if table.params is None:                                    # parameter windows: names and "*" against this env's model
            table.resolve(self.param_names())
        elif table.has_params:
            self._check_param_items(table)
        if table.has_faults:                                        # observation names, "*" and ranges against this env's observation config
            table.resolve_faults(self.fault_names())
        if table.has_action_faults:                                 # actuator names, "*" and ranges against this env's model
            table.resolve_action_faults(self.actuator_names())
        if table.has_latency:                                       # channels, names and "*" against this env's observation config and model
            table.resolve_latency(self.fault_names(), self.actuator_names())
        check_slots = int(check_slots or 0)
        if check_slots and table.has_checks:                        # names and ranges against this env's model
            table.resolve_checks(self.check_names())
        if curves and table.has_curves:
            table.resolve_curves(self.check_names())
        will_search = bool(search) and table.has_search
        if will_search:
            for s_, it in enumerate(table.search):
                if it is not None and it["check_mask"] and not (check_slots and table.has_checks):
                    raise ValueError(f"set_scenarios: scenario {s_}, search: fail_on {it['fail_on']!r} names a check and the checks are not armed "
                                     "(pass check_slots)")
        old_table, old_marked = self.scenario_table, self._search_marked
        try:
            # What the armed search holds in place comes off first: marked fault items are rewritten unmarked (in place: same items), and a
            # search that fails on a check is disarmed where the next one does not.
            for key in self._search_marked:
                self._send_items(self.scenario_table, key, False)
            self._search_marked = ()
            if self._search_checks and not (will_search and any(it is not None and it["check_mask"] for it in table.search)):
                self.engine.search_set(None)
                self.search_slots, self._search_checks = 0, False
            if self._cmd_out is None:                                   # persistent: captured graphs hold these pointers
                self._cmd_out = t.zeros_like(self.user_command)
                self._row_out = t.zeros((self.num_envs,), dtype=t.int32, device=self.device)
            try:
                self.engine.scenario_set(table.pack(), MODES[mode], self._cmd_out.data_ptr() if self.command_dim > 0 else None,
                                         self._row_out.data_ptr(), self._stream())
            except Exception:
                if self.engine.query("scenario_rows") == 0:             # the engine dropped its table (a failed upload): so does the env
                    self._drop_scenarios()
                raise
            self.scenario_table, self.scenario_mode = table, mode
            self._info_views = None
            # parameter windows ride with the table: set the ones it holds, clear what an earlier table left
            if table.has_params:
                self.engine.scenario_params_set(table.pack_params())
            elif self.engine.query("scenario_param_items") > 0:
                self.engine.scenario_params_set(None)
            for kind in FAULT_KINDS:                                    # so do the observation and the action faults
                if any(getattr(table, kind.rows)):
                    getattr(self.engine, kind.setter)(table._pack_fault_items(kind))
                elif self.engine.query(kind.param) > 0:
                    getattr(self.engine, kind.setter)(None)
            if table.has_latency:                                       # and the latency lines
                try:
                    self.engine.latency_set(table.pack_latency())
                except Exception:                                       # refused (the lines' size cap): the engine has none, and neither has the env's table
                    if self.engine.query("latency") == 0:
                        table.latency_rows, table.latency = [[] for _ in table.latency_rows], [[] for _ in table.latency_rows]
                    raise
            elif self.engine.query("latency") > 0:
                self.engine.latency_set(None)
            # so do the checks, once they are armed
            self.check_slots = 0
            if check_slots and table.has_checks:
                self.engine.scenario_checks_set(table.pack_checks(), check_slots)
                self.check_slots = check_slots
            elif self.engine.query("scenario_check_items") > 0:
                self.engine.scenario_checks_set(None)
            # and the curves
            self.curves_armed = False
            if curves and table.has_curves:
                self.engine.scenario_curves_set(table.pack_curves())
                self.curves_armed = True
            elif self.engine.query("scenario_curve_items") > 0:
                self.engine.scenario_curves_set(None)
            if not self.curves_armed or self.engine.query("scenario_curve_groups") == 0:   # the engine dropped the groups with the cells they split
                self._curve_groups = None
            # and the limit search
            armed, self.search_slots = self.search_slots, 0
            if will_search:
                self.engine.search_set(table.pack_search(int(search)))
                self.search_slots = int(search)
                self._search_checks = any(it is not None and it["check_mask"] for it in table.search)
                # the items the search scales carry their mark only now: the engine takes a marked table while that search is armed
                marked = tuple(key for key in ("params", *(k.key for k in FAULT_KINDS)) if table.has_search_marks(key))
                for key in marked:
                    self._send_items(table, key, True)
                    self._search_marked += (key,)
            elif armed > 0:
                self.engine.search_set(None)
                self._search_checks = False
        except Exception as exc:
            # A refusal part-way: where the earlier table and its search still stand, its items get their marks back -- the env would
            # otherwise go on searching without scaling them.  If that is refused too, the exception that leaves says so.
            if old_table is not None and self.scenario_table is old_table and self.engine.query("search") > 0:
                self.search_slots = self.engine.query("search_slots")
                self._search_checks = self.engine.query("search_checks") > 0
                try:
                    for key in old_marked:
                        if key not in self._search_marked:
                            self._send_items(old_table, key, True)
                            self._search_marked += (key,)
                except ValueError as again:
                    left = [key for key in old_marked if key not in self._search_marked]
                    note = (f"set_scenarios: the earlier table stays, but the marks of its {', '.join(left)} items could not be put back ({again}): "
                            "the search that is armed does not scale them until set_scenarios is called again")
                    exc.args = (f"{exc.args[0]}\n{note}" if exc.args and isinstance(exc.args[0], str) else note,) + tuple(exc.args[1:])
            raise

    def _send_items(self, table, key: str, marks: bool):
        """The parameter windows (``"params"``) or the faults of kind ``key`` of ``table`` to the engine, with or without the marks of
        the table's search items."""
        if key == "params":
            self.engine.scenario_params_set(table.pack_params(marks=marks))
        else:
            kind = next(k for k in FAULT_KINDS if k.key == key)
            getattr(self.engine, kind.setter)(table._pack_fault_items(kind, marks=marks))

    def _drop_scenarios(self):
        """The env forgets its scenario table and what rode with it (checks, curves, curve groups)."""
        self.scenario_table, self.scenario_mode = None, "env"
        self._info_views = None
        self.check_slots = 0
        self.curves_armed = False
        self.search_slots = 0
        self._search_marked, self._search_checks = (), False
        self._curve_groups = None

    def set_curve_groups(self, groups, n_groups: Optional[int] = None, names=None):
        """Split the armed response curves by one device word per env (``cosim_scenario_curves_groups``): the cells become ``n_groups``
        planes, and an episode is folded into the plane its env's word names WHEN THE FOLD READS IT -- behind the step that ended the
        episode, on the range's own stream, ahead of whatever is enqueued there next.  ``groups``: a ``PolicyTable`` /
        ``RecurrentPolicyTable`` (its ``curve_groups()``: curves by policy, under rotation too, since a rotating table rewrites
        ``policy_now`` only in its forward; the table must drive the env from its first step), or an int32 device tensor ``[N]``
        (then ``n_groups``, 1..64, is required; ``names``: one string per group), or ``None`` to go back to ungrouped curves.  The env
        holds a reference to the tensor; its contents may change between steps and between replays of a captured graph, but the
        pointer and ``n_groups`` are kernel arguments: set the groups before capturing.  A word outside ``[0, n_groups)`` leaves its
        episode in no plane (``curve_groups_lost()`` counts those).  Every call empties the cells and begins every env's episode anew
        for the curves.  ``curves()`` then returns grouped ``Curves``.  An in-place rewrite of the items by ``set_scenarios`` (same
        counts and sizes) keeps the groups; any other ``set_scenarios`` forgets them, as does disarming the curves: call this again.
        Any other per-env key works the same way -- the per-spawn-row view is a tensor of ``spawn_rows()``.  Raises ``ValueError`` if no
        curves are armed."""
        t = self.torch
        if not self.curves_armed:
            raise ValueError("set_curve_groups(): no curves are armed (BatchedEnv(scenarios=TABLE, curves=True) or set_scenarios(..., curves=True)): "
                             "groups split the cells of armed curves")
        if groups is None:
            self.engine.scenario_curves_groups(0, None)
            self._curve_groups = None
            return
        if hasattr(groups, "curve_groups"):
            if n_groups is not None:
                raise ValueError("set_curve_groups(): a policy table brings its own n_groups (its policy count); pass n_groups with a tensor only")
            if getattr(groups, "num_envs", self.num_envs) != self.num_envs:
                raise ValueError(f"set_curve_groups(): the table was built for {groups.num_envs} envs, the env has {self.num_envs}")
            words, n_groups, tab_names = groups.curve_groups()
            names = tab_names if names is None else names
        else:
            words = groups
            if n_groups is None:
                raise ValueError("set_curve_groups(): a group tensor needs n_groups (the words that count are 0 .. n_groups - 1)")
        if not isinstance(words, t.Tensor) or words.dtype != t.int32 or tuple(words.shape) != (self.num_envs,) or not words.is_contiguous() \
                or words.device != self.device:
            what = f"{type(words).__name__}" if not isinstance(words, t.Tensor) else f"{words.dtype} {tuple(words.shape)} on {words.device}"
            raise ValueError(f"set_curve_groups(): groups must be a contiguous int32 tensor [{self.num_envs}] on {self.device}, got {what}")
        if isinstance(n_groups, bool) or not isinstance(n_groups, (int, np.integer)) or not 1 <= int(n_groups) <= 64:
            raise ValueError(f"set_curve_groups(): n_groups {n_groups!r}: an integer 1..64 (None as groups clears them)")
        n_groups = int(n_groups)
        names = [str(g) for g in range(n_groups)] if names is None else [str(x) for x in names]
        if len(names) != n_groups or len(set(names)) != n_groups:
            raise ValueError(f"set_curve_groups(): names must be {n_groups} different strings, got {names}")
        self.engine.scenario_curves_groups(n_groups, words.data_ptr())
        self._curve_groups = (words, n_groups, names)

    def curve_groups_lost(self) -> int:
        """Ended episodes whose group word was outside ``[0, n_groups)`` since the cells were last emptied: they are in no plane.  Joins
        the range streams and reads one device word (a synchronising call); 0 with no groups set."""
        return self.engine.query("scenario_curve_ungrouped") if self.curves_armed else 0

    def curves(self):
        """The response curves of the fleet's ended episodes so far as a ``Curves`` (``cosim_amd/curves.py``): per (scenario, item)
        the sample times and, per outcome class and time bin, count, mean, min, max, histogram and quantiles; with groups set
        (``set_curve_groups``) the grouped ``Curves``, one plane per group.  Joins the range streams and reads the device once; nothing is
        read per step.  Raises ``ValueError`` if no curves are armed."""
        from .curves import Curves
        if not self.curves_armed:
            raise ValueError("curves(): no curves are armed (BatchedEnv(scenarios=TABLE, curves=True) or set_scenarios(..., curves=True))")
        t = self.torch
        G = self.engine.query("scenario_curve_groups")
        cells = t.empty((max(G, 1) * self.engine.query("scenario_curve_words"),), dtype=t.int32, device=self.device)
        self.engine.scenario_curves_get(cells.data_ptr(), self._stream())
        t.cuda.current_stream(self.device).synchronize()
        if G == 0:
            return Curves.from_raw(cells.cpu().numpy().view(np.uint32), self.scenario_table)
        return Curves.from_raw(cells.cpu().numpy().view(np.uint32), self.scenario_table, groups=G, group_names=self._curve_groups[2],
                               ungrouped=self.engine.query("scenario_curve_ungrouped"))

    def clear_curves(self):
        """Empty the cells and begin every env's episode anew for the curves (what was staged is discarded).  Joins the range streams
        and blocks until the device is idle."""
        if not self.curves_armed:
            raise ValueError("clear_curves(): no curves are armed")
        self.engine.scenario_curves_clear()

    # ------------------------------------------------------------------ limit search (cosim_set_param "search")
    def _search_words(self, name: str, shape):
        t = self.torch
        buf = t.empty((self.num_envs, *shape), dtype=t.int32, device=self.device)
        self.engine.get(name, buf.data_ptr(), self._stream())
        return buf

    def search(self, include_trials: bool = True):
        """The fleet's limit search so far as a ``SearchResult`` (``cosim_amd/search.py``): per env its level, step, counted trials,
        fails, reversals, bracket and threshold; with ``include_trials`` one row per ended episode still in the rings, sorted by
        (global env id, episode), with the level it ran at and its outcome.  Joins the range streams and reads the device once;
        nothing is read per step.  Raises ``ValueError`` if no search is armed."""
        from .search import NCNT, TRIAL_WORDS, SearchResult, search_rows
        if self.search_slots <= 0:
            raise ValueError("search(): no search is armed (BatchedEnv(scenarios=TABLE, search=SLOTS) or set_scenarios(..., search=SLOTS))")
        state = self._search_words("search_state", (NCNT,))
        ring = self._search_words("search_trials", (self.search_slots, TRIAL_WORDS)) if include_trials else None
        self.torch.cuda.current_stream(self.device).synchronize()
        rows = search_rows(self.scenario_table, self.scenario_mode, np.arange(self.env_id0, self.env_id0 + self.num_envs))
        return SearchResult.from_raw(state.cpu().numpy(), ring.cpu().numpy() if include_trials else None, rows, self.env_id0, self.scenario_table)

    def search_remaining(self) -> int:
        """Envs with a search item that still have trials left.  Joins the range streams and reads one device word (a synchronising
        call).  Raises ``ValueError`` if no search is armed."""
        if self.search_slots <= 0:
            raise ValueError("search_remaining(): no search is armed (BatchedEnv(scenarios=TABLE, search=SLOTS) or set_scenarios(..., search=SLOTS))")
        return self.engine.query("search_remaining")

    def search_levels(self):
        """The level each env's next step will run at: a float32 tensor ``[N]`` (a copy; 0 for an env whose scenario has no item).
        Joins the ranges.  Raises ``ValueError`` if no search is armed."""
        from .search import LEVEL, NCNT
        if self.search_slots <= 0:
            raise ValueError("search_levels(): no search is armed (BatchedEnv(scenarios=TABLE, search=SLOTS) or set_scenarios(..., search=SLOTS))")
        return self._search_words("search_state", (NCNT,))[:, LEVEL].contiguous().view(self.torch.float32)

    def check_names(self) -> dict:
        """What a check's ``index`` is resolved against on this env (``scenario.check_names``)."""
        from .scenario import check_names
        return check_names(self.cm, self.info_dim, self.command_dim)

    def verdicts(self, include_open: bool = False):
        """The verdicts of the fleet's episodes so far as a ``Verdicts`` (``cosim_amd/checks.py``): one row per ended episode still in
        the ring, sorted by (global env id, episode), with the fail / incomplete / passed flag, the value and the step of every item
        of its scenario.  ``include_open``: also the episodes still running (flag 16).  Joins the range streams and reads the device
        once; nothing is read per step.  Raises ``ValueError`` if no checks are armed."""
        from .checks import Verdicts
        if self.check_slots <= 0:
            raise ValueError("verdicts(): no checks are armed (BatchedEnv(scenarios=TABLE, check_slots=SLOTS) or set_scenarios(..., check_slots=))")
        W = self.engine.query("scenario_check_words")
        return Verdicts.from_raw(*self._read_records(self.engine.scenario_checks_get, (self.check_slots, W), (), (W,), include_open),
                                 self.scenario_table, self.env_id0)

    def fault_names(self) -> dict:
        """What an observation fault's ``obs`` / ``index`` are resolved against on this env (``scenario.fault_names``)."""
        from .scenario import fault_names
        return fault_names(self.stacked_obs_order, self.non_stacked_obs_order, self.obs_to_dim, self.stack_size)

    def _fault_items(self, kind) -> list:
        if self.scenario_table is None:
            return []
        items = [list(f) for f in getattr(self.scenario_table, kind.key)]
        assert sum(len(f) for f in items) == self.engine.query(kind.param)
        return items

    def obs_faults(self) -> list:
        """The expanded observation-fault items of the scenario table that is set, per scenario: ``(t0, t1, frame element, op id,
        ordinal of the listed item, float32 value)`` (``ScenarioTable.faults``); an empty list per scenario without any, ``[]`` with
        no table.  ``cosim_query "obs_faults"`` counts them."""
        return self._fault_items(FAULT_KINDS[0])

    def actuator_names(self) -> list:
        """The model's actuator names in order: what an action fault's ``index`` is resolved against."""
        return list(self.param_names()["kp"])

    def action_faults(self) -> list:
        """The expanded action-fault items of the scenario table that is set, per scenario: ``(t0, t1, actuator, op id, ordinal of the
        listed item, float32 value)`` (``ScenarioTable.action_faults``); an empty list per scenario without any, ``[]`` with no table.
        ``cosim_query "action_faults"`` counts them."""
        return self._fault_items(FAULT_KINDS[1])

    def latency(self) -> list:
        """The expanded latency items of the scenario table that is set, per scenario: ``(t0, t1, channel kind (0 action, 1
        observation), element, ordinal of the listed item, steps, jitter)`` (``ScenarioTable.latency``); an empty list per scenario
        without any, ``[]`` with no table.  ``cosim_query "latency"`` counts them, ``"latency_depth"`` is the depth of the lines."""
        if self.scenario_table is None:
            return []
        items = [list(f) for f in self.scenario_table.latency or [[] for _ in range(len(self.scenario_table))]]
        if sum(len(f) for f in items) != self.engine.query("latency"):
            raise RuntimeError(f"latency(): the table holds {sum(len(f) for f in items)} items and the engine {self.engine.query('latency')}: "
                               "the latency was set or cleared behind the env (Engine.latency_set); call set_scenarios again")
        return items

    def effective_action(self):
        """What the last ``step()``'s kernels were handed as the action while action faults or a latency of the command channel are
        set: a float32 tensor ``[N, nu]`` (a copy; zeros before the first step), ``None`` when neither is set.  Joins the ranges."""
        if self.engine.query("action_faults") == 0 and self.engine.query("latency_action_items") == 0:
            return None
        out = self.torch.empty((self.num_envs, self.action_dim), dtype=self.torch.float32, device=self.device)
        self.engine.get("action_effective", out.data_ptr(), self._stream())
        return out

    def param_names(self) -> dict:
        """The names a parameter window's ``index`` may use on this env, per field (``scenario.param_names``)."""
        from .scenario import param_names
        return param_names(self.cm)

    def param_layout(self) -> dict:
        """Word offsets of ``kp``, ``kd``, ``geom_friction`` and ``dof_frictionloss`` in a parameter record, and its ``stride``."""
        from .scenario import param_layout
        q = self.engine.query
        lay = param_layout(q("nbody"), q("nv"), q("ngeom"), q("action_dim"))
        assert lay["stride"] == q("param_stride")
        return lay

    def _check_param_items(self, table):
        """A table resolved elsewhere: its items must fit this env's model (the engine checks again, this names the window)."""
        width = {f: len(n) for f, n in self.param_names().items()}
        from .scenario import _FIELD_NAMES
        for s, items in enumerate(table.params):
            for k, (_, _, field, index, _, _) in enumerate(items):
                if not 0 <= index < width[_FIELD_NAMES[field]]:
                    raise ValueError(f"set_scenarios: scenario {s}, parameter item {k}: index {index} out of range: "
                                     f"'{_FIELD_NAMES[field]}' has {width[_FIELD_NAMES[field]]} entries")

    def effective_params(self) -> np.ndarray:
        """The parameter records the step kernels read, host float32 ``[N, param_stride]``: while the scenario table holds parameter
        windows the EFFECTIVE records as the last ``step()`` / ``reset()`` / ``set_scenarios`` wrote them (base values with every
        window applied that held at the env's clock before that step), otherwise the base records.  ``set_param``, ``snapshot()``
        and the history ring always hold the base.  Joins and synchronises."""
        return self.engine.scenario_params_get()

    @property
    def applied_command(self):
        """The raw command rows ``[N, command_dim]`` the engine steps with: the scenario kernel's output while a table is set,
        ``user_command`` itself otherwise."""
        return self._cmd_out if self.scenario_table is not None else self.user_command

    def scenario_rows(self) -> np.ndarray:
        """Per env: the table row the last ``step()`` / ``reset()`` applied (int64 ``[N]``; ``-1`` with no table).  Joins and
        synchronises."""
        if self.scenario_table is None:
            return np.full(self.num_envs, -1, dtype=np.int64)
        self.join()
        self.torch.cuda.current_stream(self.device).synchronize()
        return self._row_out.cpu().numpy().astype(np.int64)

    # ------------------------------------------------------------------ spawn table (cosim_spawn_set)
    def set_spawn(self, spawn, clearance: Optional[float] = None, per_episode: Optional[bool] = None):
        """Spread the fleet's resets over the terrain.  ``spawn``: ``[M, 3]`` rows ``(x, y, yaw)``, or the dict that
        ``spawn.resolve`` documents (pose generators ``grid`` / ``uniform`` use the env's seed), or ``None`` / an empty array to
        clear the table.  The engine lifts every row onto the heightfield on the device (no penetration, ``clearance`` metres of
        extra height) and every later reset of an env -- ``reset()``, the auto-reset inside ``step()`` / ``rollout()``, the reset
        after a non-finite state -- takes its base pose ``qpos[0:7]`` from row ``global env id mod M``, or with ``per_episode`` from
        a row drawn anew for each episode.  Joint angles, init noise and velocities are as without a table.  Ranks of a distributed
        run that set the same table give the results of one fleet.  Limits: yaw orientations only (others raise ``ValueError``);
        position-mode commands stay world-frame targets; rows that are not finite or reach off the field raise ``ValueError``."""
        from . import spawn as sp
        if spawn is None or (not isinstance(spawn, dict) and np.asarray(spawn).size == 0):
            self.engine.spawn_set(np.zeros((0, 3), dtype=np.float32), np.zeros((0, 4), dtype=np.float32), 0.0, False, self._stream())
            return
        xy, clr, per = sp.resolve(self.cm, spawn, self.seed)
        clr = float(clearance) if clearance is not None else clr
        per = bool(per_episode) if per_episode is not None else per
        self.engine.spawn_set(xy, sp.footprint(self.cm), clr, per, self._stream())

    def spawn_poses(self) -> np.ndarray:
        """The placed table, host float32 ``[M, 7]`` = ``x, y, z, qw, qx, qy, qz`` (``[0, 7]`` with no table)."""
        return self.engine.spawn_get()

    def spawn_rows(self) -> np.ndarray:
        """Per env: the table row its last reset took (int64 ``[N]``, engine meta word 14; meaningful once a table is set)."""
        return self._meta_words()[:, 14].cpu().numpy().astype(np.int64)

    def solver_stats(self):
        """Cumulative solver counters since creation (fleet sums): control steps, constraint rows (summed over
        substeps), Newton iterations, line-search evaluations, Hessian factorisations, non-finite resets.  The counters live in the
        state record, so ``restore`` / ``fork`` put them back with the rest: afterwards they describe the restored history (a fork
        copies its source's)."""
        mi = self._meta_words().to(self.torch.int64)
        m = mi.sum(dim=0).cpu().numpy()
        # dropped_*: contacts / limit rows that found no slot (0 unless an env was stepped with a truncated constraint set);
        # max_contacts: most contacts detected in one substep by any env of the fleet
        return {"step_count": int(m[1]), "rows": int(m[3]), "nan_resets": int(m[4]), "newton_iters": int(m[5]),
                "ls_evals": int(m[6]), "factorisations": int(m[7]), "dropped_contacts": int(m[8]), "dropped_limit_rows": int(m[9]),
                "max_contacts": int(mi[:, 10].max().item()), "episodes_ended": int(m[11]),
                # control steps redone by the large-capacity kernel because their contacts did not fit the fleet kernel's slots
                # (heightfield fix-up on the split pipeline: substeps, the unit that pipeline redoes)
                "fixup_steps": int(m[12]),
                # heightfield: geoms whose prism walk hit the 32768-prism bound (counted in dropped_contacts too)
                "truncated_walks": int(m[13])}

    def render(self):
        pass  # headless

    def close(self):
        self.engine.close()
