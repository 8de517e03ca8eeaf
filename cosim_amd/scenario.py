"""Scenario tables: per-env command and push schedules kept on the device (``cosim_scenario_set``, csrc/cosim_scenario.hip).

The reference's tester gives its one robot a test while it runs: the operator changes the command and holds the push button
(core/tester.py:41-53,68,80-81).  A ``ScenarioTable`` is S such tests; the engine gives every env of a fleet its own -- row
``global env id mod S`` (mode ``env``), advanced by one per episode of the env in mode ``cycle`` -- keyed by the env's own episode
clock, with no host read per step.  ``reference_schedule`` is the numpy twin of the kernel's rule (rows and commands exact),
``push_reference`` a float64 statement of the push arithmetic, ``sweep`` a generator of scenario grids.  No torch, no GPU here.

A scenario is a mapping ``{"commands": [[t, c0, c1, ...], ...], "pushes": [[t0, t1, vx, vy, vz], ...]}``: from episode step ``t`` on
the command is that row (whole row; before the first keyframe the caller's command passes through); a push is held for
``t0 <= t < t1`` (the last LISTED window that holds wins).  Either list may be missing or empty.

Parameter windows (``cosim_scenario_params_set``, csrc/cosim_scnparams.hip): a scenario may also hold ``"params": [[t0, t1, field,
index, op, value], ...]``.  While ``t0 <= t < t1`` word ``field[index]`` of the env's EFFECTIVE parameter record is ``base * value``
(``op`` ``"scale"``, one float32 multiply) or ``value`` (``"set"``); the last LISTED window that holds wins, per word; outside every
window the word is the base value.  Fields: ``"kp"`` / ``"kd"`` (index = actuator), ``"geom_friction"`` (index = geom; the mixed
ground-contact friction) and ``"dof_frictionloss"`` (index = dof).  ``index`` is an int, a name of the model (actuator, geom or joint
name; needs ``names``, see ``param_names``) or ``"*"`` for every entry of the field; names and ``"*"`` are expanded here, on the host.
The mass fields are refused.  ``reference_params`` is the numpy twin of the kernel's rule, exact.

Checks (``cosim_scenario_checks_set``, csrc/cosim_checks.hip): a scenario may hold ``"checks": [[t0, t1, signal, index, mode, op, bound],
...]`` (an optional eighth entry names the item; or a dict with those keys and ``"name"``): a timed pass / fail criterion on a signal of
the step, judged on the device.  ``signal``: ``"info"`` / ``"abs_info"`` (index = column of the info row: an int, a column name
``action_diff_RMSE``, ``lin_vel_x``, ``lin_vel_y``, ``ang_vel_yaw``, or ``torque[k]`` / ``set_points[k]`` / ``state[k]``),
``"tracking_error"`` (index = command entry), ``"torque_max"``, ``"up"`` (index 0), ``"qpos"`` / ``"qvel"`` / ``"abs_qvel"`` (index = an
int or a joint name: the joint's first qpos / dof address).  ``mode`` ``"always"`` / ``"settle"`` / ``"mean"``, ``op`` ``"<"`` / ``">"``.
``cosim_amd/checks.py`` has the verdict container and the numpy twin.

Response curves (``cosim_scenario_curves_set``, csrc/cosim_curves.hip): a scenario may hold ``"curves": [[t0, t1, every, signal, index,
lo, hi, bins], ...]`` (an optional ninth entry names the item; or a dict with those keys and ``"name"``), at most 8: the signal --
``signal`` / ``index`` exactly as in a check -- is sampled at every control step whose pre-step episode clock ``t`` holds ``t0 <= t <
t1`` and ``(t - t0) % every == 0``, into time bin ``(t - t0) // every`` of ``ceil((t1 - t0) / every) <= 1024``; when the episode ends
its samples go into per-(scenario, item, outcome) cells on the device: count, fixed-point sum, min, max and a histogram of ``bins``
(0..64; 0: none) equal bins over ``[lo, hi)`` plus an underflow and an overflow row.  ``cosim_amd/curves.py`` has the container and the
numpy twin.

Observation faults (``cosim_set_param "obs_faults"``, csrc/cosim_obsfault.hip): a scenario may hold ``"faults": [[t0, t1, obs, index, op,
value], ...]`` (an optional seventh entry names the item; or a dict with those keys and ``"name"``): a timed change of what the POLICY
SEES.  ``obs`` is a name of the env's ``stacked_obs_order`` / ``non_stacked_obs_order`` (``dof_pos``, ``dof_vel``, ``ang_vel``,
``lin_vel``, ``projected_gravity``, ``last_action``, ``height_map``; ``command`` is refused: the command words are the scenario's
keyframes), ``index`` an int in ``[0, dim)`` or ``"*"``, ``value`` in the units the policy sees (after the observation's ``scale``).
The window is keyed on the observation's OWN clock ``t_obs``: 0 for a reset's observation, k after the k-th step of the episode -- the
``t`` the commands and pushes of the NEXT step are keyed on, so a push over ``[150, 155)`` and a fault over ``[150, 200)`` start on the
same policy decision.  Ops, applied to the newest frame's value ``x`` in listed order, composing (float32): ``"scale"`` ``x * value``,
``"bias"`` ``x + value``, ``"set"`` ``value``, ``"noise"`` ``x + value * u`` with ``u`` uniform in ``[-1, 1)`` (``value >= 0``),
``"hold"`` the element's value in the previous frame (what the policy saw one step earlier, faults included: a frozen sensor),
``"drop"`` with probability ``value`` in ``[0, 1]`` per step and listed item as ``"hold"`` (all elements of the item together: a lost
packet).  ``"hold"`` / ``"drop"`` need a stacked observation and ``stack_size >= 2``; at ``t_obs = 0`` they change nothing.  At most 256
items per scenario after expansion.  ``reference_obs_faults`` is the numpy twin of the kernel's rule, exact.

Action faults (``cosim_set_param "action_faults"``, csrc/cosim_actfault.hip): a scenario may hold ``"action_faults": [[t0, t1, index, op,
value], ...]`` (an optional sixth entry names the item; or a dict with those keys and ``"name"``): a timed change of what the MOTORS
ARE TOLD, the channel from the policy to the drives.  ``index`` is an actuator index, an actuator name of the model or ``"*"``,
``value`` in the units of the policy's output (the raw action, before ``a_scale``).  The window is keyed on the env's PRE-STEP episode
clock ``t`` (the clock keyframes, pushes and parameter windows use).  Ops, applied to the caller's action word ``x`` in listed order,
composing (float32): ``"scale"``, ``"bias"``, ``"set"``, ``"noise"`` as for an observation fault (Philox purpose 8), ``"hold"`` the action the
step kernel was given one step earlier (the effective one: a held channel stays frozen through the window), ``"drop"`` with probability
``value`` per step and listed item as ``"hold"`` (all actuators of the item together: a lost packet, the drive keeps its last set point),
``"clip"`` ``x > value ? value : (x < -value ? -value : x)`` (a saturating output; NaN stays NaN).  At episode step 0 ``"hold"`` / ``"drop"``
change nothing.  ``last_action`` in the observation stays the policy's own output.  At most 256 items per scenario after expansion.
``reference_action_faults`` is the numpy twin of one step of the kernel's rule, exact.

Limit search (``cosim_set_param "search"``, csrc/cosim_search.hip): a scenario may hold ONE ``"search": {"lo", "hi", "start" = the
middle, "step" = (hi - lo) / 4, "min_step" = (hi - lo) / 256, "rule": "bisect" | "staircase", "trials", "targets": ["pushes" |
"commands", ...], "fail_on": ["terminated" | "nonfinite" | "tilt" | "height" | "contact", ...], "rev_skip" = 0}``: every env of the row
keeps a level in ``[lo, hi]`` that is multiplied into the row's push vectors and / or command keyframes and moved when an episode of
the env ends -- down after a failure (an ended episode with one of the ``fail_on`` ledger flags), up after a pass.  ``cosim_amd/search.py``
has the result container and the numpy twin; ``reference_schedule(level=...)`` is the twin of the scaled schedule.
``targets`` also takes ``"params"``, ``"faults"`` and ``"action_faults"`` (every listed item of that kind in the row) or ``"kind:i,j"``
(the listed items with the ordinals i, j, counted before ``"*"`` is expanded): a MARKED item uses ``float32(value * level)`` in the place
of its value (a window: ``scale`` becomes ``base * v``, ``set`` becomes ``v``; ``drop``: as its probability; a ``hold`` has no value and
cannot be marked), the row's other items are untouched; ``reference_params`` / ``reference_obs_faults`` / ``reference_action_faults``
``(level=...)`` are the twins.  Parameter windows and action faults take the level the open episode runs at, an observation fault the
level of the episode its observation belongs to.  ``"harder":
"up" | "down"`` (default up): with ``"down"`` a LOWER level is harder (a gain scale, a friction): a failure moves the level up, a pass
down.  ``fail_on`` also takes ``"checks"`` (any check of the row), ``"check:NAME"`` and ``"check:I"``: a trial fails too if a selected
check of the ended episode did not pass (failed or incomplete); the checks must be armed (``check_slots``).

Latency (``cosim_set_param "latency"``, csrc/cosim_latency.hip): a scenario may hold ``"latency": [[t0, t1, channel, index, steps], ...]``
(optional trailing entries: an int ``jitter``, default 0, and a string name; or a dict with the keys ``t0, t1, channel, index, steps,
jitter, name``): a timed TRANSPORT DELAY of ``steps`` control steps plus ``0..jitter`` drawn per step and listed item.  ``channel`` is
``"action"`` (what the drives are told arrives late; ``index`` an actuator index, an actuator name or ``"*"``; keyed on the pre-step
episode clock, as an action fault) or an observation name (what the policy sees arrives late; ``index`` an int or ``"*"``; ``command``
is refused; keyed on the observation's own clock, as an observation fault).  ``steps >= 0``, ``jitter >= 0``, ``steps + jitter <= 63``;
at most 256 expanded items per scenario and channel kind.  Per element the LAST listed item that holds gives the delay; delays do not
compose.  Every env whose row lists an item of a kind keeps a line of the channel's clean words on the device, written at every clock,
inside and outside the windows, so a window that opens in mid-episode delivers the history before it.  Before the line holds the
word asked for, an observation is the line's first reading and an action is 0 after a reset (nothing has arrived yet), the first
word after a host cut in mid-episode.  Latency comes ahead of the faults: they take the delivered word.  ``last_action`` in the
observation stays the policy's own output.  ``LatencyTwin`` is the numpy twin, exact; the lines are not part of a snapshot.
"""
from __future__ import annotations

import itertools
import math
from typing import Iterable, Iterator, NamedTuple, Sequence

import numpy as np

MODES = {"env": 0, "cycle": 1}
MAX_ROWS, MAX_ITEMS, MAX_TIME = 65536, 64, 1 << 30
PARAM_FIELDS = {"kp": 0, "kd": 1, "geom_friction": 2, "dof_frictionloss": 3}
PARAM_OPS = {"scale": 0, "set": 1}
MAX_PARAM_ITEMS = 256
CHECK_SIGNALS = {"info": 0, "abs_info": 1, "tracking_error": 2, "torque_max": 3, "up": 4, "qpos": 5, "qvel": 6, "abs_qvel": 7}
CHECK_MODES = {"always": 0, "settle": 1, "mean": 2}
CHECK_OPS = {"<": 0, ">": 1}
MAX_CHECK_ITEMS = 64
_CHECK_KEYS = ("t0", "t1", "signal", "index", "mode", "op", "bound")
MAX_CURVE_ITEMS, MAX_CURVE_T, MAX_CURVE_BINS = 8, 1024, 64
_CURVE_KEYS = ("t0", "t1", "every", "signal", "index", "lo", "hi", "bins")
# consistent only as a set that compile.env_constants computes in fp64 on the host
REFUSED_PARAM_FIELDS = ("body_mass", "body_invweight0", "dof_invweight0", "meaninertia")
FAULT_OPS = {"scale": 0, "bias": 1, "set": 2, "noise": 3, "hold": 4, "drop": 5}
ACTION_FAULT_OPS = dict(FAULT_OPS, clip=6)
MAX_FAULT_ITEMS = MAX_ACTION_FAULT_ITEMS = 256
SEARCH_RULES = {"bisect": 0, "staircase": 1}
SEARCH_TARGETS = {"pushes": 1, "commands": 2}
SEARCH_ITEM_TARGETS = {"params": 4, "faults": 8, "action_faults": 16}   # kinds whose MARKED items the level scales ("kind" or "kind:i,j")
PARAM_MARK = 0x100                             # of a packed parameter item's op word: a search scales its value
SEARCH_HARDER = {"up": 0, "down": 1}
FAULT_MARK = 0x8000                            # of a packed fault item's element: a search scales its value
SEARCH_FAIL_ON = {"terminated": 1, "nonfinite": 4, "tilt": 32, "height": 64, "contact": 128}   # the ledger's flag values
MAX_SEARCH_SLOTS, MAX_SEARCH_TRIALS, MAX_SEARCH_REV_SKIP = 64, 1 << 20, 255
_SEARCH_KEYS = ("lo", "hi", "start", "step", "min_step", "rule", "trials", "targets", "fail_on", "rev_skip")
_SEARCH_OPT_KEYS = ("harder",)                 # emitted only when not the default
MAX_LATENCY_ITEMS, MAX_LATENCY_DELAY = 256, 63 # expanded items per scenario and channel kind; steps + jitter
_LATENCY_KEYS = ("t0", "t1", "channel", "index", "steps", "jitter")
LATENCY_ACTION, LATENCY_OBS = 0, 1             # the channel kind of an expanded item


class _FaultKind(NamedTuple):
    """What the two kinds of fault differ in but for their resolvers and twins.  ``key`` is the scenario key and the attribute of the
    expanded items, ``rows`` the attribute of the rows as written."""
    key: str
    rows: str
    param: str           # the engine's name of the word table (cosim_set_param / cosim_query) ...
    setter: str          # ... and the Engine method that sends it
    what: str            # "faults": how the messages name the kind ...
    noun: str            # ... and one item of it
    keys: tuple          # the columns of a row
    ops: dict
    cap: int
    index: str           # what an index may be, in the message ...
    named: bool          # ... and whether a name is one
    unresolved: str

    @property
    def op_names(self) -> dict:
        return {v: k for k, v in self.ops.items()}


_OBS_FAULTS = _FaultKind("faults", "fault_rows", "obs_faults", "scenario_faults_set", "faults", "fault item", ("t0", "t1", "obs", "index", "op", "value"), FAULT_OPS, MAX_FAULT_ITEMS,
                         "an int or '*'", False, "pass names={'faults': fault_names(...)} or call resolve_faults")
_ACTION_FAULTS = _FaultKind("action_faults", "action_fault_rows", "action_faults", "scenario_action_faults_set", "action faults", "action-fault item",
                            ("t0", "t1", "index", "op", "value"), ACTION_FAULT_OPS, MAX_ACTION_FAULT_ITEMS, "an int, an actuator name or '*'", True,
                            "pass names={'action_faults': [actuator names]} or call resolve_action_faults")
FAULT_KINDS = (_OBS_FAULTS, _ACTION_FAULTS)
_FIELD_NAMES = {v: k for k, v in PARAM_FIELDS.items()}
_OP_NAMES = {v: k for k, v in PARAM_OPS.items()}


def param_names(cm) -> dict:
    """The names an ``index`` of a parameter window may use, per field, from a compiled model: actuator names for ``kp`` / ``kd``,
    geom names for ``geom_friction``, and for ``dof_frictionloss`` the name of the joint each dof belongs to (a free joint's name
    expands to its six dofs).  The length of a list is the field's width."""
    from .model import get_field
    acts = [a["name"] for a in cm.spec["actuators"]]
    jid = np.asarray(get_field(cm.blob, "dof_jntid"))[:cm.blob.nv]
    return {"kp": acts, "kd": acts, "geom_friction": list(cm.geom_names), "dof_frictionloss": [cm.joint_names[int(j)] for j in jid]}


def fault_names(stacked_obs_order, non_stacked_obs_order, obs_to_dim: dict, stack_size: int) -> dict:
    """What a fault's ``obs`` / ``index`` are resolved against: ``{"stacked": [(name, dim), ...], "non_stacked": [(name, dim), ...],
    "stack_size"}`` in the order of the observation frame (frame element ``e`` counts through the stacked names, then the others)."""
    return {"stacked": [(n, int(obs_to_dim[n])) for n in stacked_obs_order],
            "non_stacked": [(n, int(obs_to_dim[n])) for n in non_stacked_obs_order], "stack_size": int(stack_size)}


def fault_layout(names: dict) -> dict:
    """The frame layout ``reference_obs_faults`` takes, from ``fault_names``: ``stacked_dim``, ``frame_dim``, ``stack_size``,
    ``state_dim`` and ``command`` (the frame elements of the command field)."""
    sd = sum(d for _, d in names["stacked"])
    fd = sd + sum(d for _, d in names["non_stacked"])
    cmd, e = [], 0
    for n, d in list(names["stacked"]) + list(names["non_stacked"]):
        cmd += list(range(e, e + d)) if n == "command" else []
        e += d
    S = int(names["stack_size"])
    return {"stacked_dim": sd, "frame_dim": fd, "stack_size": S, "state_dim": S * sd + fd - sd, "command": cmd}


def info_columns(nu: int, info_dim: int) -> dict:
    """Column name -> ``(first column, width)`` of an info row: ``action_diff_RMSE``, ``lin_vel_x``, ``lin_vel_y``, ``ang_vel_yaw``,
    ``torque [nu]``, ``set_points [nu]``, ``state [the rest]`` (``BatchedEnv._info``)."""
    nu, info_dim = int(nu), int(info_dim)
    return {"action_diff_RMSE": (0, 1), "lin_vel_x": (1, 1), "lin_vel_y": (2, 1), "ang_vel_yaw": (3, 1), "torque": (4, nu),
            "set_points": (4 + nu, nu), "state": (4 + 2 * nu, max(info_dim - 4 - 2 * nu, 0))}


def check_names(cm, info_dim: int, command_dim: int) -> dict:
    """What the ``index`` of a check is resolved against, from a compiled model: ``{"info": info_columns, "info_dim", "command_dim",
    "nq", "nv", "qpos": {joint: first qpos address}, "qvel": {joint: first dof address}}``."""
    from .model import get_field
    b = cm.blob
    nj = len(cm.joint_names)
    qadr, dadr = np.asarray(get_field(b, "jnt_qposadr"))[:nj], np.asarray(get_field(b, "jnt_dofadr"))[:nj]
    return {"info": info_columns(b.nu, info_dim), "info_dim": int(info_dim), "command_dim": int(command_dim), "nq": int(b.nq), "nv": int(b.nv),
            "qpos": {n: int(qadr[j]) for j, n in enumerate(cm.joint_names)}, "qvel": {n: int(dadr[j]) for j, n in enumerate(cm.joint_names)}}


def param_layout(nbody: int, nv: int, ngeom: int, nu: int) -> dict:
    """Word offsets of the fields a window may name in a parameter record, and the record's ``stride`` (the engine's build_layout:
    body_mass, body_invweight0 [nbody] | dof_invweight0, dof_frictionloss [nv] | geom_friction [ngeom] | kp, kd [nu] | meaninertia,
    rounded up to 32 words)."""
    floss = 2 * nbody + nv
    gmu = floss + nv
    kp = gmu + ngeom
    return {"dof_frictionloss": floss, "geom_friction": gmu, "kp": kp, "kd": kp + nu, "stride": -(-(kp + 2 * nu + 1) // 32) * 32}


class ScenarioTable:
    """S scenarios, validated.  ``keys[s]`` is a list of ``(t, command float32[command_dim])``, ``pushes[s]`` a list of
    ``(t0, t1, v float32[3])``.  ``pack()`` gives the CSR arrays of the C ABI, ``from_csr`` reads them back."""

    def __init__(self, scenarios: Sequence, command_dim: int, names: dict = None):
        """``names`` (``param_names(compiled_model)``, or any mapping field -> list of entry names) is what parameter windows are
        resolved against: it gives every field its width and the names an ``index`` may use.  Without it windows are kept as
        written and ``resolve(names)`` expands them later (``BatchedEnv.set_scenarios`` does)."""
        self.command_dim = int(command_dim)
        if self.command_dim < 0:
            raise ValueError("ScenarioTable: command_dim must be >= 0")
        scenarios = list(scenarios)
        if not 1 <= len(scenarios) <= MAX_ROWS:
            raise ValueError(f"ScenarioTable: {len(scenarios)} scenarios: must be 1..{MAX_ROWS}")
        self.keys, self.pushes, self.param_windows, self.params = [], [], [], None
        self.check_rows, self.checks = [], None
        self.curve_rows, self.curves = [], None
        self.fault_rows, self.faults = [], None                   # (the attributes the two _FaultKind name)
        self.action_fault_rows, self.action_faults = [], None
        self.search = []                                          # per scenario: None or the item as a dict of _SEARCH_KEYS
        self.latency_rows, self.latency = [], None                # the rows as written; per scenario the expanded items (resolve_latency)
        for s, sc in enumerate(scenarios):
            sc = sc or {}
            if not isinstance(sc, dict) or set(sc) - {"commands", "pushes", "params", "checks", "curves", "faults", "action_faults", "search", "latency", "name"}:
                raise ValueError(f"ScenarioTable: scenario {s}: a mapping with the keys 'commands' and 'pushes' is expected, got {sc!r}")
            keys, pushes = [], []
            for r, row in enumerate(sc.get("commands") or []):
                who = f"ScenarioTable: scenario {s}, keyframe {r}"
                row = [float(x) for x in row]
                if len(row) != 1 + self.command_dim:
                    raise ValueError(f"{who}: {len(row)} values, expected [t, c0 .. c{self.command_dim - 1}]")
                if not all(math.isfinite(x) for x in row):
                    raise ValueError(f"{who}: non-finite value")
                if row[0] != int(row[0]) or not 0 <= row[0] < MAX_TIME:
                    raise ValueError(f"{who}: time {row[0]} must be a control step in [0, 2^30)")
                if keys and int(row[0]) <= keys[-1][0]:
                    raise ValueError(f"{who}: time {int(row[0])} does not increase (previous {keys[-1][0]})")
                keys.append((int(row[0]), np.asarray(row[1:], dtype=np.float32)))
            for r, row in enumerate(sc.get("pushes") or []):
                who = f"ScenarioTable: scenario {s}, push window {r}"
                row = [float(x) for x in row]
                if len(row) != 5:
                    raise ValueError(f"{who}: {len(row)} values, expected [t0, t1, vx, vy, vz]")
                if not all(math.isfinite(x) for x in row):
                    raise ValueError(f"{who}: non-finite value")
                if row[0] != int(row[0]) or row[1] != int(row[1]) or not 0 <= row[0] < MAX_TIME or not 0 <= row[1] <= MAX_TIME:
                    raise ValueError(f"{who}: times must be control steps in [0, 2^30)")
                if row[1] <= row[0]:
                    raise ValueError(f"{who}: t1 {int(row[1])} is not after t0 {int(row[0])}")
                pushes.append((int(row[0]), int(row[1]), np.asarray(row[2:], dtype=np.float32)))
            for what, lst in (("keyframes", keys), ("push windows", pushes)):
                if len(lst) > MAX_ITEMS:
                    raise ValueError(f"ScenarioTable: scenario {s}: {len(lst)} {what}, at most {MAX_ITEMS}")
            self.keys.append(keys)
            self.pushes.append(pushes)
            self.param_windows.append(_param_windows(s, sc.get("params") or []))
            self.check_rows.append(_check_rows(s, sc.get("checks") or []))
            self.curve_rows.append(_curve_rows(s, sc.get("curves") or []))
            for kind in FAULT_KINDS:
                getattr(self, kind.rows).append(_fault_kind_rows(kind, s, sc.get(kind.key) or []))
            self.latency_rows.append(_latency_rows(s, sc.get("latency") or []))
            self.search.append(_search_item(s, sc.get("search"), bool(pushes), bool(keys),
                                            {"params": self.param_windows[s], **{k.key: getattr(self, k.rows)[s] for k in FAULT_KINDS}}, self.check_rows[s]))
        if names is not None or not self.has_params:
            self.resolve(names or {})
        cn = (names or {}).get("checks")
        if cn is not None or not any(isinstance(r[3], str) for rows in self.check_rows for r in rows):
            self.resolve_checks(cn)
        if cn is not None or not any(isinstance(r[4], str) for rows in self.curve_rows for r in rows):
            self.resolve_curves(cn)
        fn = (names or {}).get("faults")
        if fn is not None or not self.has_faults:
            self.resolve_faults(fn or {"stacked": [], "non_stacked": [], "stack_size": 1})
        an = (names or {}).get("action_faults")
        if an is not None or not self.has_action_faults:
            self.resolve_action_faults(an or [])
        ln = (names or {}).get("latency")
        if ln is not None or not self.has_latency:
            self.resolve_latency(*(ln or ({"stacked": [], "non_stacked": [], "stack_size": 1}, [])))

    # ---- latency: the rows as written, their expansion, packing and the way back
    @property
    def has_latency(self) -> bool:
        return any(self.latency_rows)

    def resolve_latency(self, names: dict, actuators) -> "ScenarioTable":
        """Expand the latency rows against ``names`` (``fault_names(...)``, ``BatchedEnv.fault_names()``) and ``actuators`` (the model's
        actuator names in order): ``self.latency[s]`` becomes the list of items ``(t0, t1, channel kind, element, ord, steps, jitter)`` in
        listed order, ``"*"`` expanded in index order -- kind ``LATENCY_ACTION`` with an actuator, ``LATENCY_OBS`` with a frame element;
        ``ord`` is the ordinal of the listed item (its elements share one jitter draw).  Raises ``ValueError`` naming the scenario and
        the item: unknown channel or actuator, index out of range, more than 256 items of a kind."""
        actuators = list(actuators)
        nu = len(actuators)
        first, e = {}, 0
        for lst in (names["stacked"], names["non_stacked"]):
            for n, d in lst:
                first.setdefault(n, (e, int(d)))
                e += int(d)
        out = []
        for s, rows in enumerate(self.latency_rows):
            items = []
            for r, (t0, t1, channel, index, steps, jitter, _) in enumerate(rows):
                who = f"ScenarioTable: scenario {s}, latency item {r}"
                if channel == "action":
                    if index == "*":
                        els = list(range(nu))
                    elif isinstance(index, str):
                        els = [i for i, n in enumerate(actuators) if n == index]
                        if not els:
                            raise ValueError(f"{who}: unknown actuator '{index}' (the model has {', '.join(map(str, actuators)) or 'none'})")
                    elif not 0 <= index < nu:
                        raise ValueError(f"{who}: index {index} out of range: the model has {nu} actuators")
                    else:
                        els = [index]
                    kind = LATENCY_ACTION
                else:
                    if channel not in first:
                        raise ValueError(f"{who}: unknown channel '{channel}' ('action' or an observation: the env observes {', '.join(first) or 'nothing'})")
                    e0, dim = first[channel]
                    if isinstance(index, str) and index != "*":
                        raise ValueError(f"{who}: index must be an int or '*' on an observation, got {index!r}")
                    if index != "*" and not 0 <= index < dim:
                        raise ValueError(f"{who}: index {index} out of range: '{channel}' has {dim} entries")
                    els = [e0 + i for i in (range(dim) if index == "*" else [index])]
                    kind = LATENCY_OBS
                items += [(t0, t1, kind, el, r, steps, jitter) for el in els]
            for kind, what in ((LATENCY_ACTION, "action"), (LATENCY_OBS, "observation")):
                n = sum(1 for it in items if it[2] == kind)
                if n > MAX_LATENCY_ITEMS:
                    raise ValueError(f"ScenarioTable: scenario {s}: {n} {what} latency items after expansion, at most {MAX_LATENCY_ITEMS}")
            out.append(items)
        self.latency = out
        return self

    def _carry_latency(self, new: "ScenarioTable") -> "ScenarioTable":
        """``new``, a table rebuilt from this one's ``to_list()`` (the ``*_from_csr`` helpers), with this one's expanded latency
        items: its latency rows are this one's, so the expansion is too."""
        if new.latency is None and self.latency is not None:
            new.latency = [list(f) for f in self.latency]
        return new

    def _resolved_latency(self) -> list:
        if self.latency is None:
            raise ValueError("ScenarioTable: the latency items are not resolved yet: pass names={'latency': (fault_names(...), [actuator names])} "
                             "or call resolve_latency")
        return self.latency

    @property
    def n_latency_items(self) -> int:
        return sum(len(f) for f in self._resolved_latency())

    @property
    def latency_depth(self) -> int:
        """The depth D of the lines a fresh allocation gets: the largest ``steps + jitter``, plus 1."""
        return 1 + max((it[5] + it[6] for f in self._resolved_latency() for it in f), default=0)

    def pack_latency(self) -> np.ndarray:
        """The expanded items as the int32 word table ``Engine.latency_set`` sends through ``cosim_set_param "latency"``: ``S |
        act_adr[S + 1] | obs_adr[S + 1] | act[na][6] | obs[no][6]``, an item being ``(t0, t1, element, ord, steps, jitter)``."""
        adr, items = ([0], [0]), ([], [])
        for f in self._resolved_latency():
            for kind in (LATENCY_ACTION, LATENCY_OBS):
                items[kind].extend([t0, t1, el, r, steps, jitter] for t0, t1, k, el, r, steps, jitter in f if k == kind)
                adr[kind].append(len(items[kind]))
        flat = [w for kind in (LATENCY_ACTION, LATENCY_OBS) for it in items[kind] for w in it]
        return np.array([len(self)] + adr[0] + adr[1] + flat, dtype=np.int32)

    def latency_from_words(self, words, names: dict, actuators) -> "ScenarioTable":
        """A table with everything of this one but the latency, which is what the word table of ``pack_latency`` holds: the items of
        one ``ord`` become one listed item again (``"*"`` if they cover the channel, else one item per element), resolved against
        ``names`` and ``actuators``."""
        words = np.asarray(words, dtype=np.int64).reshape(-1)
        S = int(words[0])
        scn = self.to_list()
        if S != len(scn):
            raise ValueError(f"ScenarioTable: latency for {S} scenarios, the table has {len(scn)}")
        adr = (words[1:S + 2], words[S + 2:2 * S + 3])
        na, no = int(adr[0][-1]), int(adr[1][-1])
        body = words[2 * S + 3:]
        if len(body) != 6 * (na + no):
            raise ValueError(f"ScenarioTable: latency words: {len(body)} item words, {na} + {no} items take {6 * (na + no)}")
        recs = (body[:6 * na].reshape(-1, 6), body[6 * na:].reshape(-1, 6))
        actuators = list(actuators)
        spans, e = [], 0
        for n, d in list(names["stacked"]) + list(names["non_stacked"]):
            spans.append((n, e, int(d)))
            e += int(d)
        for s, sc in enumerate(scn):
            sc.pop("latency", None)
            groups = {}                                             # ord -> (kind, head, [elements])
            for kind in (LATENCY_ACTION, LATENCY_OBS):
                for t0, t1, el, r, steps, jitter in recs[kind][int(adr[kind][s]):int(adr[kind][s + 1])].tolist():
                    groups.setdefault(r, (kind, (t0, t1, steps, jitter), []))[2].append(el)
            rows = []
            for r in sorted(groups):
                kind, (t0, t1, steps, jitter), els = groups[r]
                if kind == LATENCY_ACTION:
                    channel, idx, whole = "action", els, len(actuators) > 1 and els == list(range(len(actuators)))
                else:
                    span = [sp for sp in spans if sp[1] <= els[0] < sp[1] + sp[2]]
                    if not span:
                        raise ValueError(f"ScenarioTable: scenario {s}, latency item {r}: element {els[0]} outside the frame")
                    channel, e0, d = span[0]
                    idx, whole = [k - e0 for k in els], d > 1 and els == list(range(e0, e0 + d))
                rows += [[t0, t1, channel, "*" if whole else k, steps, jitter] for k in (["*"] if whole else idx)]
            if rows:
                sc["latency"] = rows
        return type(self)(scn, self.command_dim).resolve_latency(names, actuators)

    # ---- faults, both kinds: the rows as written, their expansion, packing and the way back
    def _expand_faults(self, kind: _FaultKind, elements) -> "ScenarioTable":
        """``getattr(self, kind.key)[s]`` becomes the list of items ``(t0, t1, element, op id, ord, float32 value)`` in listed order:
        ``elements(who, row)`` gives the elements a row names, in order; ``ord`` is the ordinal of the listed item (its elements
        share one ``drop`` draw)."""
        out = []
        for s, rows in enumerate(getattr(self, kind.rows)):
            items = []
            for r, row in enumerate(rows):
                items += [(row[0], row[1], e, kind.ops[row[-3]], r, np.float32(row[-2]))
                          for e in elements(f"ScenarioTable: scenario {s}, {kind.noun} {r}", row)]
            if len(items) > kind.cap:
                raise ValueError(f"ScenarioTable: scenario {s}: {len(items)} {kind.noun}s after expansion, at most {kind.cap}")
            out.append(items)
        setattr(self, kind.key, out)
        return self

    def _resolved_items(self, kind: _FaultKind) -> list:
        if getattr(self, kind.key) is None:
            raise ValueError(f"ScenarioTable: the {kind.what} are not resolved yet: {kind.unresolved}")
        return getattr(self, kind.key)

    def _pack_fault_items(self, kind: _FaultKind, marks: bool = False):
        """The CSR form of the kind's items; ``marks``: the items a search item of their row marks carry ``FAULT_MARK`` in their
        element (the engine takes such a table only while that search is armed)."""
        adr, t, elem, op, ord_, value = _pack_items(self._resolved_items(kind), 2, (np.int32, np.int32, np.int32, np.float32))
        if marks:
            for s in range(len(self)):
                m = self.search_marks(kind.key, s)
                if m:
                    sl = slice(int(adr[s]), int(adr[s + 1]))
                    elem[sl] |= np.where(np.isin(ord_[sl], m), FAULT_MARK, 0).astype(np.int32)
        return adr, t, elem, op, ord_, value

    def search_marks(self, key: str, s: int) -> list:
        """The ordinals of the listed items of kind ``key`` (``"params"``, ``"faults"``, ``"action_faults"``) that scenario ``s``'s
        search item marks, ascending."""
        it = self.search[s]
        return list(it["marks"].get(key, ())) if it is not None else []

    def has_search_marks(self, key: str) -> bool:
        return any(self.search_marks(key, s) for s in range(len(self)))

    def _faults_from_csr(self, kind: _FaultKind, adr, t, elem, op, ord, value, listed) -> "ScenarioTable":
        """A table with everything of this one but the faults of ``kind``, which are those the CSR arrays hold, not resolved yet: the
        items of one ``ord`` become one listed item again.  ``listed(s, i, elements)`` says how: ``(the columns between the times and
        the index, the elements as indices, whether they are the whole "*")``."""
        t = np.asarray(t).reshape(-1, 2)
        scn = self.to_list()
        if len(adr) != len(scn) + 1:
            raise ValueError(f"ScenarioTable: {kind.what} for {len(adr) - 1} scenarios, the table has {len(scn)}")
        for s, sc in enumerate(scn):
            sc.pop(kind.key, None)
            rows, i, i1 = [], int(adr[s]), int(adr[s + 1])
            while i < i1:
                j = i
                while j < i1 and int(ord[j]) == int(ord[i]):
                    j += 1
                cols, idx, whole = listed(s, i - int(adr[s]), [int(x) for x in elem[i:j]])
                head = [int(t[i, 0]), int(t[i, 1])] + cols
                tail = [kind.op_names.get(int(op[i]), int(op[i])), float(np.float32(value[i]))]
                rows += [head + ["*"] + tail] if whole else [head + [k] + tail for k in idx]
                i = j
            if rows:
                sc[kind.key] = rows
        return self._carry_latency(type(self)(scn, self.command_dim))

    @property
    def has_action_faults(self) -> bool:
        return any(self.action_fault_rows)

    def resolve_action_faults(self, actuators) -> "ScenarioTable":
        """Expand the action faults against ``actuators`` (the model's actuator names in order, ``BatchedEnv.actuator_names()``):
        ``self.action_faults[s]`` becomes the list of items ``(t0, t1, actuator j, op id, ord, float32 value)`` in listed order, ``"*"``
        expanded in index order; ``ord`` is the ordinal of the listed item (its actuators share one ``drop`` draw).  Raises
        ``ValueError`` naming the scenario and the item: unknown actuator, index out of range, more than 256 items."""
        actuators = list(actuators)
        nu = len(actuators)

        def elements(who, row):
            index = row[2]
            if index == "*":
                return list(range(nu))
            if isinstance(index, str):
                idx = [i for i, n in enumerate(actuators) if n == index]
                if not idx:
                    raise ValueError(f"{who}: unknown actuator '{index}' (the model has {', '.join(map(str, actuators)) or 'none'})")
                return idx
            if not 0 <= index < nu:
                raise ValueError(f"{who}: index {index} out of range: the model has {nu} actuators")
            return [index]
        return self._expand_faults(_ACTION_FAULTS, elements)

    @property
    def n_action_fault_items(self) -> int:
        return sum(len(f) for f in self._resolved_items(_ACTION_FAULTS))

    def pack_action_faults(self):
        """``(adr int32[S + 1], t int32[n, 2], actuator int32[n], op int32[n], ord int32[n], value float32[n])``: the expanded items in
        the CSR form ``Engine.scenario_action_faults_set`` sends through ``cosim_set_param "action_faults"``."""
        return self._pack_fault_items(_ACTION_FAULTS)

    def action_faults_from_csr(self, adr, t, elem, op, ord, value, actuators) -> "ScenarioTable":
        """A table with everything of this one but the action faults, which are those the CSR arrays of ``pack_action_faults`` hold:
        the items of one ``ord`` become one listed item again (``"*"`` if they cover every actuator, else one item per actuator),
        resolved against ``actuators``."""
        nu = len(list(actuators))
        listed = lambda s, i, elems: ([], elems, nu > 1 and elems == list(range(nu)))   # noqa: E731
        return self._faults_from_csr(_ACTION_FAULTS, adr, t, elem, op, ord, value, listed).resolve_action_faults(actuators)

    @property
    def has_faults(self) -> bool:
        return any(self.fault_rows)

    def resolve_faults(self, names: dict) -> "ScenarioTable":
        """Expand the faults against ``names`` (``fault_names(...)``, ``BatchedEnv.fault_names()``): ``self.faults[s]`` becomes the list
        of items ``(t0, t1, frame element e, op id, ord, float32 value)`` in listed order, ``"*"`` expanded in index order; ``ord`` is
        the ordinal of the listed item (its elements share one ``drop`` draw).  Raises ``ValueError`` naming the scenario and the item:
        unknown name, index out of range, ``hold`` / ``drop`` without a previous frame, more than 256 items."""
        first, e = {}, 0
        for stacked, lst in ((True, names["stacked"]), (False, names["non_stacked"])):
            for n, d in lst:
                first.setdefault(n, (e, int(d), stacked))
                e += int(d)

        def elements(who, row):
            obs, index, op = row[2:5]
            if obs not in first:
                raise ValueError(f"{who}: unknown observation '{obs}' (the env observes {', '.join(first) or 'nothing'})")
            e0, dim, stacked = first[obs]
            if op in ("hold", "drop") and (not stacked or int(names["stack_size"]) < 2):
                raise ValueError(f"{who}: op '{op}' on '{obs}' needs a stacked observation and stack_size >= 2: there is no previous "
                                 "frame in the record")
            if index != "*" and not 0 <= index < dim:
                raise ValueError(f"{who}: index {index} out of range: '{obs}' has {dim} entries")
            return [e0 + i for i in (range(dim) if index == "*" else [index])]
        return self._expand_faults(_OBS_FAULTS, elements)

    @property
    def n_fault_items(self) -> int:
        return sum(len(f) for f in self._resolved_items(_OBS_FAULTS))

    def pack_faults(self):
        """``(adr int32[S + 1], t int32[n, 2], elem int32[n], op int32[n], ord int32[n], value float32[n])``: the expanded items in
        the CSR form ``Engine.scenario_faults_set`` sends through ``cosim_set_param "obs_faults"``."""
        return self._pack_fault_items(_OBS_FAULTS)

    def faults_from_csr(self, adr, t, elem, op, ord, value, names: dict) -> "ScenarioTable":
        """A table with everything of this one but the faults, which are those the CSR arrays of ``pack_faults`` hold: the items of
        one ``ord`` become one listed item again (``"*"`` if they cover the observation, else one item per element), resolved
        against ``names`` (``fault_names``)."""
        spans, e = [], 0
        for n, d in list(names["stacked"]) + list(names["non_stacked"]):
            spans.append((n, e, int(d)))
            e += int(d)

        def listed(s, i, elems):
            span = [sp for sp in spans if sp[1] <= elems[0] < sp[1] + sp[2]]
            if not span:
                raise ValueError(f"ScenarioTable: scenario {s}, fault item {i}: element {elems[0]} outside the frame")
            n, first, d = span[0]
            return [n], [k - first for k in elems], d > 1 and elems == list(range(first, first + d))
        return self._faults_from_csr(_OBS_FAULTS, adr, t, elem, op, ord, value, listed).resolve_faults(names)

    @property
    def has_curves(self) -> bool:
        return any(self.curve_rows)

    def resolve_curves(self, names: dict = None) -> "ScenarioTable":
        """Resolve the curves against ``names`` (``check_names(compiled_model, info_dim, command_dim)``: the checks' name tables):
        ``self.curves[s]`` becomes the list of items ``(t0, t1, every, signal id, index, float32 lo, float32 hi, bins, name)``.  With
        ``names`` ``None`` only int indices resolve and no range is checked (the engine checks them).  Raises ``ValueError`` naming
        the scenario and the item."""
        def item(row, index):
            t0, t1, every, signal, _, lo, hi, bins, name = row
            return (t0, t1, every, CHECK_SIGNALS[signal], index, np.float32(lo), np.float32(hi), bins,
                    name if name is not None else f"{signal}[{index}] @{t0}:{t1}:{every}")
        self.curves = _resolve_items(self.curve_rows, "curve", 3, item, names)
        return self

    def _resolved_curves(self):
        if self.curves is None:
            raise ValueError("ScenarioTable: the curves are not resolved yet: call resolve_curves(check_names(model, info_dim, command_dim))")
        return self.curves

    @property
    def n_curve_items(self) -> int:
        return sum(len(c) for c in self.curve_rows)

    def pack_curves(self):
        """``(adr int32[S + 1], t int32[n, 3] (t0, t1, every), signal int32[n], index int32[n], lo float32[n], hi float32[n], bins
        int32[n])``: the items in the CSR form of ``cosim_scenario_curves_set``."""
        return _pack_items(self._resolved_curves(), 3, (np.int32, np.int32, np.float32, np.float32, np.int32))

    def curve_item_names(self) -> list:
        """Per scenario, the names of its curve items (the given name, or one made from the item's fields)."""
        return [[it[8] for it in c] for c in self._resolved_curves()]

    # ---- limit search: at most one item per scenario
    @property
    def has_search(self) -> bool:
        return any(it is not None for it in self.search)

    def pack_search(self, slots: int) -> np.ndarray:
        """The int32 word table ``cosim_set_param "search"`` takes: ``S | slots | has[S] | lo | hi | x0 | d0 | d_min | rule | trials |
        targets | fail_mask | rev_skip`` (``[S]`` each, floats as their bits; zeros for a scenario without an item), ``2 + 11 S`` words.
        Only when an item uses ``harder="down"`` or fails on a check, three more columns follow: ``harder | chk_lo | chk_hi`` (the
        64-bit mask of the selected checks of the row), ``2 + 14 S`` words."""
        if isinstance(slots, bool) or not isinstance(slots, (int, np.integer)) or not 1 <= int(slots) <= MAX_SEARCH_SLOTS:
            raise ValueError(f"ScenarioTable: search slots {slots!r}: an integer 1..{MAX_SEARCH_SLOTS}")
        S = len(self)
        f, i = np.zeros((5, S), dtype=np.float32), np.zeros((5, S), dtype=np.int32)
        has = np.zeros(S, dtype=np.int32)
        for s, it in enumerate(self.search):
            if it is None:
                continue
            has[s] = 1
            f[:, s] = [it["lo"], it["hi"], it["start"], it["step"], it["min_step"]]
            i[:, s] = [SEARCH_RULES[it["rule"]], it["trials"], search_target_bits(it), search_fail_mask(it), it["rev_skip"]]
        words = [np.array([S, int(slots)], dtype=np.int32), has, f.view(np.int32).reshape(-1), i.reshape(-1)]
        if any(it is not None and (it["harder"] != "up" or it["check_mask"]) for it in self.search):
            x = np.zeros((3, S), dtype=np.uint32)
            for s, it in enumerate(self.search):
                if it is not None:
                    x[:, s] = [SEARCH_HARDER[it["harder"]], it["check_mask"] & 0xFFFFFFFF, it["check_mask"] >> 32]
            words.append(x.view(np.int32).reshape(-1))
        return np.concatenate(words)

    def search_from_words(self, words) -> "ScenarioTable":
        """A table with everything of this one but the search items, which are those the word table of ``pack_search`` holds.  The
        words say WHICH KINDS an item marks (targets 4, 8, 16), not which ordinals: those travel as mark bits in the kinds' own item
        tables.  Where this table's own item of the row names the kind, its ordinals are kept; else the whole kind is marked -- and
        if that would mark a ``hold`` the item is refused like any other (``ValueError``): pass the ordinals in the table instead."""
        words = np.ascontiguousarray(words, dtype=np.int32).reshape(-1)
        scn = self.to_list()
        S = len(scn)
        if len(words) not in (2 + 11 * S, 2 + 14 * S) or int(words[0]) != S:
            raise ValueError(f"ScenarioTable: a search table of {int(words[0]) if len(words) else 0} scenarios in {len(words)} words, the table has {S}")
        cols = words[2:].reshape(-1, S)
        fl = np.ascontiguousarray(cols[1:6]).view(np.float32)
        for s, sc in enumerate(scn):
            sc.pop("search", None)
            if cols[0, s]:
                sc["search"] = {"lo": float(fl[0, s]), "hi": float(fl[1, s]), "start": float(fl[2, s]), "step": float(fl[3, s]), "min_step": float(fl[4, s]),
                                "rule": {v: k for k, v in SEARCH_RULES.items()}.get(int(cols[6, s]), int(cols[6, s])), "trials": int(cols[7, s]),
                                "targets": [k for k, v in SEARCH_TARGETS.items() if int(cols[8, s]) & v],
                                "fail_on": [k for k, v in SEARCH_FAIL_ON.items() if int(cols[9, s]) & v], "rev_skip": int(cols[10, s])}
                # which listed items a kind's bit marks travels in that kind's item table: this table's own item says it, else all are
                old = self.search[s]["targets"] if self.search[s] is not None else []
                for k, v in SEARCH_ITEM_TARGETS.items():
                    if int(cols[8, s]) & v:
                        sc["search"]["targets"] += [n for n in old if n.partition(":")[0] == k] or [k]
                if len(cols) > 11:
                    if int(cols[11, s]):
                        sc["search"]["harder"] = {v: k for k, v in SEARCH_HARDER.items()}.get(int(cols[11, s]), int(cols[11, s]))
                    mask = (int(cols[12, s]) & 0xFFFFFFFF) | (int(cols[13, s]) & 0xFFFFFFFF) << 32
                    nc = len(self.check_rows[s])
                    if mask and nc and mask == (1 << nc) - 1:
                        sc["search"]["fail_on"].append("checks")
                    else:
                        sc["search"]["fail_on"] += [f"check:{i}" for i in range(64) if mask >> i & 1]
        return self._carry_latency(type(self)(scn, self.command_dim))

    @property
    def has_checks(self) -> bool:
        return any(self.check_rows)

    def resolve_checks(self, names: dict = None) -> "ScenarioTable":
        """Resolve the checks against ``names`` (``check_names(compiled_model, info_dim, command_dim)``): ``self.checks[s]`` becomes the
        list of items ``(t0, t1, signal id, index, mode id, op id, float32 bound, name)``.  With ``names`` ``None`` only int indices
        resolve and no range is checked (the engine checks them).  Raises ``ValueError`` naming the scenario and the item."""
        def item(row, index):
            t0, t1, signal, _, mode, op, bound, name = row
            return (t0, t1, CHECK_SIGNALS[signal], index, CHECK_MODES[mode], CHECK_OPS[op], np.float32(bound),
                    name if name is not None else f"{signal}[{index}] {mode} {op} {float(np.float32(bound))!r} @{t0}:{t1}")
        self.checks = _resolve_items(self.check_rows, "check", 2, item, names)
        return self

    def _resolved_checks(self):
        if self.checks is None:
            raise ValueError("ScenarioTable: the checks are not resolved yet: call resolve_checks(check_names(model, info_dim, command_dim))")
        return self.checks

    @property
    def n_check_items(self) -> int:
        return sum(len(c) for c in self.check_rows)

    def pack_checks(self):
        """``(adr int32[S + 1], t int32[n, 2], signal int32[n], index int32[n], mode int32[n], cmp int32[n], bound float32[n])``: the items
        in the CSR form of ``cosim_scenario_checks_set``."""
        return _pack_items(self._resolved_checks(), 2, (np.int32, np.int32, np.int32, np.int32, np.float32))

    def check_item_names(self) -> list:
        """Per scenario, the names of its items (the given name, or one made from the item's fields)."""
        return [[it[7] for it in c] for c in self._resolved_checks()]

    @property
    def has_params(self) -> bool:
        return any(self.param_windows)

    def resolve(self, names: dict) -> "ScenarioTable":
        """Expand the windows against ``names`` (field -> list of entry names): ``self.params[s]`` becomes the list of items ``(t0, t1,
        field id, index, op id, float32 value)`` in listed order, ``"*"`` and names that several entries share expanded in index
        order.  Raises ``ValueError`` naming the scenario and the row: unknown name, index out of range, more than 256 items."""
        out, out_ords = [], []
        for s, wins in enumerate(self.param_windows):
            items, ords = [], []
            for r, (t0, t1, field, index, op, value) in enumerate(wins):
                who = f"ScenarioTable: scenario {s}, parameter window {r}"
                if field not in names:
                    raise ValueError(f"{who}: field '{field}' needs the model's names to be resolved (param_names)")
                entries = list(names[field])
                if isinstance(index, str):
                    idx = list(range(len(entries))) if index == "*" else [i for i, n in enumerate(entries) if n == index]
                    if not idx:
                        raise ValueError(f"{who}: unknown name '{index}' for field '{field}'")
                else:
                    if not 0 <= index < len(entries):
                        raise ValueError(f"{who}: index {index} out of range: '{field}' has {len(entries)} entries")
                    idx = [index]
                items += [(t0, t1, PARAM_FIELDS[field], i, PARAM_OPS[op], value) for i in idx]
                ords += [r] * len(idx)
            if len(items) > MAX_PARAM_ITEMS:
                raise ValueError(f"ScenarioTable: scenario {s}: {len(items)} parameter items after expansion, at most {MAX_PARAM_ITEMS}")
            out.append(items)
            out_ords.append(ords)
        self.params, self.param_ords = out, out_ords                # param_ords[s][k]: the listed window item k was expanded from
        return self

    @property
    def n_param_items(self) -> int:
        return sum(len(p) for p in self._resolved())

    def _resolved(self):
        if self.params is None:
            raise ValueError("ScenarioTable: the parameter windows are not resolved yet: pass names= or call resolve(param_names(model))")
        return self.params

    def __len__(self):
        return len(self.keys)

    @property
    def has_push(self) -> bool:
        return any(self.pushes)

    @classmethod
    def build(cls, spec, command_dim: int) -> "ScenarioTable":
        """From a ``ScenarioTable`` (returned as is), a list of scenarios, a mapping ``{"scenarios": [...]}`` or the path of a YAML
        file holding either."""
        if isinstance(spec, cls):
            if spec.command_dim != int(command_dim):
                raise ValueError(f"ScenarioTable: built for command_dim {spec.command_dim}, the env has {command_dim}")
            return spec
        if isinstance(spec, (str, bytes)) or hasattr(spec, "__fspath__"):
            import yaml
            with open(spec) as f:
                spec = yaml.safe_load(f)
        if isinstance(spec, dict):
            if "scenarios" not in spec:
                raise ValueError("ScenarioTable: a mapping must hold the key 'scenarios'")
            spec = spec["scenarios"]
        if not isinstance(spec, (list, tuple)):
            raise ValueError(f"ScenarioTable: expected a list of scenarios, got {type(spec).__name__}")
        return cls(spec, command_dim)

    def to_list(self) -> list:
        out = [{"commands": [[t] + [float(x) for x in c] for t, c in keys], "pushes": [[t0, t1] + [float(x) for x in v] for t0, t1, v in pushes]}
               for keys, pushes in zip(self.keys, self.pushes)]
        for sc, wins in zip(out, self.param_windows):
            if wins:
                sc["params"] = [[t0, t1, field, index, op, float(value)] for t0, t1, field, index, op, value in wins]
        for sc, rows in zip(out, self.check_rows):
            if rows:
                sc["checks"] = [[t0, t1, signal, index, mode, op, float(bound)] + ([name] if name is not None else [])
                                for t0, t1, signal, index, mode, op, bound, name in rows]
        for sc, rows in zip(out, self.curve_rows):
            if rows:
                sc["curves"] = [[t0, t1, every, signal, index, float(lo), float(hi), bins] + ([name] if name is not None else [])
                                for t0, t1, every, signal, index, lo, hi, bins, name in rows]
        for kind in FAULT_KINDS:
            for sc, rows in zip(out, getattr(self, kind.rows)):
                if rows:
                    sc[kind.key] = [[*row[:-2], float(row[-2])] + ([row[-1]] if row[-1] is not None else []) for row in rows]
        for sc, it in zip(out, self.search):
            if it is not None:
                sc["search"] = {k: (list(it[k]) if isinstance(it[k], list) else it[k]) for k in _SEARCH_KEYS}
                sc["search"].update({k: it[k] for k in _SEARCH_OPT_KEYS if it[k] != "up"})
        for sc, rows in zip(out, self.latency_rows):
            if rows:
                sc["latency"] = [[*row[:-1]] + ([row[-1]] if row[-1] is not None else []) for row in rows]
        return out

    def pack(self):
        """``(key_adr int32[S + 1], key_t int32[nk], key_cmd float32[nk, command_dim], push_adr int32[S + 1], push_t int32[np, 2],
        push_v float32[np, 3])``."""
        key_adr, key_t, key_cmd = _pack_items(self.keys, 1, (np.float32,))
        push_adr, push_t, push_v = _pack_items(self.pushes, 2, (np.float32,))
        return key_adr, key_t.reshape(-1), key_cmd.reshape(len(key_t), self.command_dim), push_adr, push_t, push_v.reshape(-1, 3)

    def pack_params(self, marks: bool = False):
        """``(adr int32[S + 1], t int32[n, 2], field int32[n], index int32[n], op int32[n], value float32[n])``: the expanded items
        in the CSR form of ``cosim_scenario_params_set``.  ``marks``: the items a search item of their row marks carry ``PARAM_MARK``
        in their op word (the engine takes such a table only while that search is armed)."""
        adr, t, field, index, op, value = _pack_items(self._resolved(), 2, (np.int32, np.int32, np.int32, np.float32))
        if marks:
            for s in range(len(self)):
                m = self.search_marks("params", s)
                if m:
                    sl = slice(int(adr[s]), int(adr[s + 1]))
                    op[sl] |= np.where(np.isin(self.param_ords[s], m), PARAM_MARK, 0).astype(np.int32)
        return adr, t, field, index, op, value

    def params_from_csr(self, adr, t, field, index, op, value, names: dict = None) -> "ScenarioTable":
        """A table with this one's commands and pushes and the windows that the CSR arrays of ``pack_params`` hold (one window per
        item, int indices), resolved against ``names`` if given."""
        t = np.asarray(t).reshape(-1, 2)
        scn = self.to_list()
        if len(adr) != len(scn) + 1:
            raise ValueError(f"ScenarioTable: parameter windows for {len(adr) - 1} scenarios, the table has {len(scn)}")
        for s, sc in enumerate(scn):
            sc.pop("params", None)
            rows = [[int(t[i, 0]), int(t[i, 1]), _FIELD_NAMES.get(int(field[i]), int(field[i])), int(index[i]), _OP_NAMES.get(int(op[i]), int(op[i])),
                     float(np.float32(value[i]))] for i in range(int(adr[s]), int(adr[s + 1]))]
            if rows:
                sc["params"] = rows
        return self._carry_latency(type(self)(scn, self.command_dim, names=names))

    @classmethod
    def from_csr(cls, key_adr, key_t, key_cmd, push_adr, push_t, push_v, command_dim: int) -> "ScenarioTable":
        key_cmd = np.asarray(key_cmd, dtype=np.float32).reshape(-1, int(command_dim))
        push_t, push_v = np.asarray(push_t).reshape(-1, 2), np.asarray(push_v, dtype=np.float32).reshape(-1, 3)
        out = []
        for s in range(len(key_adr) - 1):
            out.append({"commands": [[int(key_t[k])] + key_cmd[k].tolist() for k in range(int(key_adr[s]), int(key_adr[s + 1]))],
                        "pushes": [[int(push_t[p, 0]), int(push_t[p, 1])] + push_v[p].tolist()
                                   for p in range(int(push_adr[s]), int(push_adr[s + 1]))]})
        return cls(out, command_dim)


def _param_windows(s: int, rows) -> list:
    """The ``"params"`` rows of scenario ``s``, checked for everything that needs no model."""
    out = []
    for r, row in enumerate(rows):
        who = f"ScenarioTable: scenario {s}, parameter window {r}"
        if not isinstance(row, (list, tuple)) or len(row) != 6:
            raise ValueError(f"{who}: expected [t0, t1, field, index, op, value], got {row!r}")
        t0, t1, field, index, op, value = row
        try:
            t0f, t1f, value = float(t0), float(t1), float(value)
        except (TypeError, ValueError):
            raise ValueError(f"{who}: times and value must be numbers, got {row!r}") from None
        if not math.isfinite(value) or abs(value) > float(np.finfo(np.float32).max):   # (finite as float32 too)
            raise ValueError(f"{who}: non-finite value")
        if not (math.isfinite(t0f) and math.isfinite(t1f)) or t0f != int(t0f) or t1f != int(t1f) or not 0 <= t0f < MAX_TIME or not 0 <= t1f <= MAX_TIME:
            raise ValueError(f"{who}: times must be control steps in [0, 2^30)")
        if t1f <= t0f:
            raise ValueError(f"{who}: t1 {int(t1f)} is not after t0 {int(t0f)}")
        if field in REFUSED_PARAM_FIELDS:
            raise ValueError(f"{who}: field '{field}' is refused: body_mass, body_invweight0, dof_invweight0 and meaninertia are consistent only "
                             "as a set that compile.env_constants computes in fp64 on the host; a payload change in mid-episode is out of scope")
        if field not in PARAM_FIELDS:
            raise ValueError(f"{who}: unknown field {field!r} (one of {', '.join(PARAM_FIELDS)})")
        if op not in PARAM_OPS:
            raise ValueError(f"{who}: unknown op {op!r} ('scale' or 'set')")
        if isinstance(index, (bool, float)) or not isinstance(index, (int, np.integer, str)):
            raise ValueError(f"{who}: index must be an int, a name or '*', got {index!r}")
        out.append((int(t0f), int(t1f), field, index if isinstance(index, str) else int(index), op, value))
    return out


def _fault_kind_rows(kind: _FaultKind, s: int, rows) -> list:
    """The rows of ``kind`` of scenario ``s``, checked for everything that needs no observation config and no model: the columns of
    ``kind.keys`` and ``name or None``.  The messages are those of ``_param_windows``."""
    out, keys = [], kind.keys
    if not isinstance(rows, (list, tuple)):
        raise ValueError(f"ScenarioTable: scenario {s}: '{kind.key}' must be a list of items, got {rows!r}")
    for r, row in enumerate(rows):
        who = f"ScenarioTable: scenario {s}, {kind.noun} {r}"
        name = None
        if isinstance(row, dict):
            if set(row) - set(keys) - {"name"} or any(k not in row for k in keys if k not in ("index", "value")):
                raise ValueError(f"{who}: a mapping with the keys {', '.join(keys)} (and 'name') is expected, got {row!r}")
            name = row.get("name")
            row = [row.get(k, {"index": "*"}.get(k, 0.0)) for k in keys]
        elif isinstance(row, (list, tuple)) and len(row) == len(keys) + 1:
            row, name = list(row[:-1]), row[-1]
        if not isinstance(row, (list, tuple)) or len(row) != len(keys):
            raise ValueError(f"{who}: expected [{', '.join(keys)}] and an optional name, got {row!r}")
        (t0, t1), (index, op, value) = row[:2], row[-3:]
        try:
            t0f, t1f, value = float(t0), float(t1), float(value)
        except (TypeError, ValueError):
            raise ValueError(f"{who}: times and value must be numbers, got {row!r}") from None
        if not math.isfinite(value) or abs(value) > float(np.finfo(np.float32).max):   # (finite as float32 too)
            raise ValueError(f"{who}: non-finite value")
        if not (math.isfinite(t0f) and math.isfinite(t1f)) or t0f != int(t0f) or t1f != int(t1f) or not 0 <= t0f < MAX_TIME or not 0 <= t1f <= MAX_TIME:
            raise ValueError(f"{who}: times must be control steps in [0, 2^30)")
        if t1f <= t0f:
            raise ValueError(f"{who}: t1 {int(t1f)} is not after t0 {int(t0f)}")
        if "obs" in keys and row[2] == "command":
            raise ValueError(f"{who}: observation 'command' is refused: the command words are the scenario's keyframes ('commands')")
        if "obs" in keys and not isinstance(row[2], str):
            raise ValueError(f"{who}: obs must be the name of an observation, got {row[2]!r}")
        if not isinstance(op, str) or op not in kind.ops:
            raise ValueError(f"{who}: unknown op {op!r} (one of {', '.join(kind.ops)})")
        if op == "noise" and value < 0:
            raise ValueError(f"{who}: a noise amplitude must be >= 0, got {value!r}")
        if op == "clip" and value < 0:
            raise ValueError(f"{who}: a clip bound must be >= 0, got {value!r}")
        if op == "drop" and not 0.0 <= value <= 1.0:
            raise ValueError(f"{who}: a drop probability must lie in [0, 1], got {value!r}")
        if isinstance(index, (bool, float)) or not (isinstance(index, (int, np.integer)) or (isinstance(index, str) and (kind.named or index == "*"))):
            raise ValueError(f"{who}: index must be {kind.index}, got {index!r}")
        if name is not None and not isinstance(name, str):
            raise ValueError(f"{who}: the name must be a string, got {name!r}")
        out.append((int(t0f), int(t1f), *row[2:-3], index if isinstance(index, str) else int(index), op, value, name))
    return out


def _latency_rows(s: int, rows) -> list:
    """The ``"latency"`` rows of scenario ``s``, checked for everything that needs no observation config and no model: ``(t0, t1,
    channel, index, steps, jitter, name or None)``."""
    out = []
    if not isinstance(rows, (list, tuple)):
        raise ValueError(f"ScenarioTable: scenario {s}: 'latency' must be a list of items, got {rows!r}")
    is_int = lambda x: isinstance(x, (int, np.integer)) and not isinstance(x, bool)   # noqa: E731
    for r, row in enumerate(rows):
        who = f"ScenarioTable: scenario {s}, latency item {r}"
        name, jitter = None, 0
        if isinstance(row, dict):
            if set(row) - set(_LATENCY_KEYS) - {"name"} or any(k not in row for k in _LATENCY_KEYS if k not in ("index", "jitter")):
                raise ValueError(f"{who}: a mapping with the keys {', '.join(_LATENCY_KEYS)} (and 'name') is expected, got {row!r}")
            name, jitter = row.get("name"), row.get("jitter", 0)
            row = [row["t0"], row["t1"], row["channel"], row.get("index", "*"), row["steps"]]
        elif isinstance(row, (list, tuple)) and len(row) in (6, 7):
            tail = list(row[5:])
            if len(tail) == 2:
                jitter, name = tail
            elif isinstance(tail[0], str):
                name = tail[0]
            else:
                jitter = tail[0]
            row = list(row[:5])
        if not isinstance(row, (list, tuple)) or len(row) != 5:
            raise ValueError(f"{who}: expected [t0, t1, channel, index, steps] with an optional jitter and an optional name, got {row!r}")
        t0, t1, channel, index, steps = row
        try:
            t0f, t1f = float(t0), float(t1)
        except (TypeError, ValueError):
            raise ValueError(f"{who}: times must be numbers, got {row!r}") from None
        if not (math.isfinite(t0f) and math.isfinite(t1f)) or t0f != int(t0f) or t1f != int(t1f) or not 0 <= t0f < MAX_TIME or not 0 <= t1f <= MAX_TIME:
            raise ValueError(f"{who}: times must be control steps in [0, 2^30)")
        if t1f <= t0f:
            raise ValueError(f"{who}: t1 {int(t1f)} is not after t0 {int(t0f)}")
        if channel == "command":
            raise ValueError(f"{who}: channel 'command' is refused: the command words are the scenario's keyframes ('commands')")
        if not isinstance(channel, str):
            raise ValueError(f"{who}: channel must be 'action' or the name of an observation, got {channel!r}")
        for what, x in (("steps", steps), ("jitter", jitter)):
            if not is_int(x):
                raise ValueError(f"{who}: {what} must be an int, got {x!r}")
            if x < 0:
                raise ValueError(f"{who}: {what} {int(x)} is negative")
        if steps + jitter > MAX_LATENCY_DELAY:
            raise ValueError(f"{who}: steps {int(steps)} + jitter {int(jitter)} is more than {MAX_LATENCY_DELAY}")
        if not (is_int(index) or (isinstance(index, str) and (channel == "action" or index == "*"))):
            raise ValueError(f"{who}: index must be an int or '*' (on 'action' also an actuator name), got {index!r}")
        if name is not None and not isinstance(name, str):
            raise ValueError(f"{who}: the name must be a string, got {name!r}")
        out.append((int(t0f), int(t1f), channel, index if isinstance(index, str) else int(index), int(steps), int(jitter), name))
    return out


def _check_index(who: str, signal: str, index: str, names: dict) -> int:
    """A check's index given as a name: an info column (``name`` or ``name[k]``) or a joint."""
    if signal in ("info", "abs_info"):
        base, k = index, 0
        if index.endswith("]") and "[" in index:
            base, _, rest = index[:-1].partition("[")
            try:
                k = int(rest)
            except ValueError:
                raise ValueError(f"{who}: unknown info column '{index}'") from None
        if base not in names["info"]:
            raise ValueError(f"{who}: unknown info column '{index}' (one of {', '.join(names['info'])})")
        first, width = names["info"][base]
        if not 0 <= k < width:
            raise ValueError(f"{who}: '{index}' out of range: '{base}' has {width} entries")
        return first + k
    if signal in ("qpos", "qvel", "abs_qvel"):
        table = names["qpos" if signal == "qpos" else "qvel"]
        if index not in table:
            raise ValueError(f"{who}: unknown joint '{index}' for signal '{signal}'")
        return table[index]
    raise ValueError(f"{who}: signal '{signal}' takes an int index, got '{index}'")


def _signal_width(signal: str, names: dict) -> int:
    """How many entries a signal's ``index`` may name on the model behind ``names``."""
    return {"info": names["info_dim"], "abs_info": names["info_dim"], "tracking_error": min(names["command_dim"], 3), "torque_max": 1,
            "up": 1 if names["nq"] >= 7 else 0, "qpos": names["nq"], "qvel": names["nv"], "abs_qvel": names["nv"]}[signal]


def _resolve_items(rows_per_scenario, kind: str, at: int, item, names) -> list:
    """The resolver under ``resolve_checks`` / ``resolve_curves``: per scenario the list ``item(row, index)`` of its rows, ``index``
    being the row's ``index`` (entry ``at + 1``; ``at``: its ``signal``) as an int -- a name looked up in ``names``, and with
    ``names`` held against the signal's width."""
    out = []
    for s, rows in enumerate(rows_per_scenario):
        items = []
        for r, row in enumerate(rows):
            who = f"ScenarioTable: scenario {s}, {kind} item {r}"
            signal, index = row[at], row[at + 1]
            if isinstance(index, str):
                if names is None:
                    raise ValueError(f"{who}: index '{index}' needs the model's names to be resolved (check_names)")
                index = _check_index(who, signal, index, names)
            if names is not None:
                width = _signal_width(signal, names)
                if not 0 <= index < width:
                    raise ValueError(f"{who}: index {index} out of range: '{signal}' has {width} entries")
            items.append(item(row, int(index)))
        out.append(items)
    return out


def _pack_items(per_scenario, n_t: int, dtypes) -> tuple:
    """The packer under the ``pack*`` methods: ``(adr int32[S + 1], t int32[n, n_t], one array [n] per entry of dtypes)`` from
    per-scenario lists of items that begin with ``n_t`` times, followed by the columns."""
    adr = np.cumsum([0] + [len(c) for c in per_scenario]).astype(np.int32)
    flat = [it for c in per_scenario for it in c]
    t = np.array([it[:n_t] for it in flat], dtype=np.int32).reshape(-1, n_t)
    return (adr, t, *(np.array([it[n_t + k] for it in flat], dtype=dt) for k, dt in enumerate(dtypes)))


def _curve_rows(s: int, rows) -> list:
    """The ``"curves"`` rows of scenario ``s``, checked for everything that needs no model: ``(t0, t1, every, signal, index, lo, hi,
    bins, name or None)``."""
    out = []
    if not isinstance(rows, (list, tuple)):
        raise ValueError(f"ScenarioTable: scenario {s}: 'curves' must be a list of items, got {rows!r}")
    if len(rows) > MAX_CURVE_ITEMS:
        raise ValueError(f"ScenarioTable: scenario {s}: {len(rows)} curve items, at most {MAX_CURVE_ITEMS}")
    for r, row in enumerate(rows):
        who = f"ScenarioTable: scenario {s}, curve item {r}"
        name = None
        if isinstance(row, dict):
            if set(row) - set(_CURVE_KEYS) - {"name"} or any(k not in row for k in _CURVE_KEYS if k not in ("index", "every", "bins")):
                raise ValueError(f"{who}: a mapping with the keys {', '.join(_CURVE_KEYS)} (and 'name') is expected, got {row!r}")
            name = row.get("name")
            row = [row.get(k, {"every": 1}.get(k, 0)) for k in _CURVE_KEYS]
        elif isinstance(row, (list, tuple)) and len(row) == 9:
            row, name = list(row[:8]), row[8]
        if not isinstance(row, (list, tuple)) or len(row) != 8:
            raise ValueError(f"{who}: expected [t0, t1, every, signal, index, lo, hi, bins] and an optional name, got {row!r}")
        t0, t1, every, signal, index, lo, hi, bins = row
        try:
            t0f, t1f, evf, lo, hi, bf = float(t0), float(t1), float(every), float(lo), float(hi), float(bins)
        except (TypeError, ValueError):
            raise ValueError(f"{who}: times, every, lo, hi and bins must be numbers, got {row!r}") from None
        fmax = float(np.finfo(np.float32).max)
        if not (math.isfinite(lo) and math.isfinite(hi)) or abs(lo) > fmax or abs(hi) > fmax:
            raise ValueError(f"{who}: non-finite lo / hi")
        if not (math.isfinite(t0f) and math.isfinite(t1f)) or t0f != int(t0f) or t1f != int(t1f) or not 0 <= t0f < MAX_TIME or not 0 <= t1f <= MAX_TIME:
            raise ValueError(f"{who}: times must be control steps in [0, 2^30)")
        if t1f <= t0f:
            raise ValueError(f"{who}: t1 {int(t1f)} is not after t0 {int(t0f)}")
        if not math.isfinite(evf) or evf != int(evf) or evf < 1:
            raise ValueError(f"{who}: every must be a whole number of control steps >= 1, got {every!r}")
        T = -(-(int(t1f) - int(t0f)) // int(evf))
        if T > MAX_CURVE_T:
            raise ValueError(f"{who}: {T} time bins, at most {MAX_CURVE_T}")
        if not math.isfinite(bf) or bf != int(bf) or not 0 <= bf <= MAX_CURVE_BINS:
            raise ValueError(f"{who}: bins must be 0..{MAX_CURVE_BINS}, got {bins!r}")
        if int(bf) > 0 and not float(np.float32(hi)) > float(np.float32(lo)):
            raise ValueError(f"{who}: hi {hi!r} is not above lo {lo!r}")
        if signal not in CHECK_SIGNALS:
            raise ValueError(f"{who}: unknown signal {signal!r} (one of {', '.join(CHECK_SIGNALS)})")
        if isinstance(index, (bool, float)) or not isinstance(index, (int, np.integer, str)):
            raise ValueError(f"{who}: index must be an int or a name, got {index!r}")
        if name is not None and not isinstance(name, str):
            raise ValueError(f"{who}: the name must be a string, got {name!r}")
        out.append((int(t0f), int(t1f), int(evf), signal, index if isinstance(index, str) else int(index), lo, hi, int(bf), name))
    return out


def _check_rows(s: int, rows) -> list:
    """The ``"checks"`` rows of scenario ``s``, checked for everything that needs no model: ``(t0, t1, signal, index, mode, op, bound,
    name or None)``."""
    out = []
    if len(rows) > MAX_CHECK_ITEMS:
        raise ValueError(f"ScenarioTable: scenario {s}: {len(rows)} check items, at most {MAX_CHECK_ITEMS}")
    for r, row in enumerate(rows):
        who = f"ScenarioTable: scenario {s}, check item {r}"
        name = None
        if isinstance(row, dict):
            if set(row) - set(_CHECK_KEYS) - {"name"} or any(k not in row for k in _CHECK_KEYS if k != "index"):
                raise ValueError(f"{who}: a mapping with the keys {', '.join(_CHECK_KEYS)} (and 'name') is expected, got {row!r}")
            name = row.get("name")
            row = [row.get(k, 0) for k in _CHECK_KEYS]
        elif isinstance(row, (list, tuple)) and len(row) == 8:
            row, name = list(row[:7]), row[7]
        if not isinstance(row, (list, tuple)) or len(row) != 7:
            raise ValueError(f"{who}: expected [t0, t1, signal, index, mode, op, bound] and an optional name, got {row!r}")
        t0, t1, signal, index, mode, op, bound = row
        try:
            t0f, t1f, bound = float(t0), float(t1), float(bound)
        except (TypeError, ValueError):
            raise ValueError(f"{who}: times and bound must be numbers, got {row!r}") from None
        if not math.isfinite(bound) or abs(bound) > float(np.finfo(np.float32).max):
            raise ValueError(f"{who}: non-finite bound")
        if not (math.isfinite(t0f) and math.isfinite(t1f)) or t0f != int(t0f) or t1f != int(t1f) or not 0 <= t0f < MAX_TIME or not 0 <= t1f <= MAX_TIME:
            raise ValueError(f"{who}: times must be control steps in [0, 2^30)")
        if t1f <= t0f:
            raise ValueError(f"{who}: t1 {int(t1f)} is not after t0 {int(t0f)}")
        if signal not in CHECK_SIGNALS:
            raise ValueError(f"{who}: unknown signal {signal!r} (one of {', '.join(CHECK_SIGNALS)})")
        if mode not in CHECK_MODES:
            raise ValueError(f"{who}: unknown mode {mode!r} ('always', 'settle' or 'mean')")
        if op not in CHECK_OPS:
            raise ValueError(f"{who}: unknown op {op!r} ('<' or '>')")
        if isinstance(index, (bool, float)) or not isinstance(index, (int, np.integer, str)):
            raise ValueError(f"{who}: index must be an int or a name, got {index!r}")
        if name is not None and not isinstance(name, str):
            raise ValueError(f"{who}: the name must be a string, got {name!r}")
        out.append((int(t0f), int(t1f), signal, index if isinstance(index, str) else int(index), mode, op, bound, name))
    return out


def search_target_bits(it: dict) -> int:
    """The ``targets`` word of a search item (``_search_item``)."""
    return sum(SEARCH_TARGETS[t] for t in it["targets"] if t in SEARCH_TARGETS) | sum(SEARCH_ITEM_TARGETS[k] for k in it["marks"])


def search_fail_mask(it: dict) -> int:
    """The ledger flags a search item fails on (its checks are ``it["check_mask"]``)."""
    return sum(SEARCH_FAIL_ON[t] for t in it["fail_on"] if t in SEARCH_FAIL_ON)


class _ParamKind(NamedTuple):
    """Parameter windows as a kind a search may mark: what ``_search_marks`` reads of a ``_FaultKind``."""
    key: str = "params"
    noun: str = "parameter window"


def _search_marks(who: str, kind, name: str, rows, lo: float, hi: float) -> list:
    """The ordinals a target ``"kind"`` / ``"kind:i,j"`` marks among the listed ``rows`` of its kind, each held to the kind's value rule
    at both ends of the level's range."""
    _, colon, rest = name.partition(":")
    if not rows:
        raise ValueError(f"{who}: the target is '{name}' and the scenario lists no {kind.noun}")
    if colon:
        try:
            ords = sorted({int(x) for x in rest.split(",")})
        except ValueError:
            raise ValueError(f"{who}: target {name!r}: '{kind.key}:' is followed by ordinals, e.g. '{kind.key}:0,2'") from None
        bad = [o for o in ords if not 0 <= o < len(rows)]
        if bad or not ords:
            raise ValueError(f"{who}: target {name!r}: ordinal {bad[0] if bad else rest!r} outside the scenario's {len(rows)} listed {kind.noun}s")
    else:
        ords = list(range(len(rows)))
    for o in ords:
        op, value = (rows[o][-2], np.float32(rows[o][-1])) if kind.key == "params" else (rows[o][-3], np.float32(rows[o][-2]))
        if op == "hold":
            raise ValueError(f"{who}: target {name!r} would mark {kind.noun} {o}, a hold: a hold has no value to scale")
        with np.errstate(all="ignore"):
            ends = [float(value * np.float32(lo)), float(value * np.float32(hi))]
        for x in ends:
            if not math.isfinite(x):
                raise ValueError(f"{who}: target {name!r}, {kind.noun} {o}: value * level is not finite at an end of [lo, hi]")
            if op in ("noise", "clip") and x < 0:
                raise ValueError(f"{who}: target {name!r}, {kind.noun} {o}: a {op} value must stay >= 0 over [lo, hi], got {x!r}")
            if op == "drop" and not 0.0 <= x <= 1.0:
                raise ValueError(f"{who}: target {name!r}, {kind.noun} {o}: a drop probability must stay in [0, 1] over [lo, hi], got {x!r}")
    return ords


def _search_item(s: int, item, has_pushes: bool, has_keys: bool, fault_rows: dict = None, check_rows=()):
    """The ``"search"`` value of scenario ``s`` as a dict of ``_SEARCH_KEYS`` with the defaults filled in and the floats rounded to
    float32 (what the device holds), or ``None``; besides the keys: ``harder``, ``marks`` (kind -> the marked ordinals of the
    scenario's listed items ``fault_rows[kind]``) and ``check_mask`` (bit i: check i of ``check_rows`` is a failure criterion).  Raises
    ``ValueError`` naming the scenario."""
    if item is None:
        return None
    who = f"ScenarioTable: scenario {s}, search"
    if not isinstance(item, dict) or set(item) - set(_SEARCH_KEYS) - set(_SEARCH_OPT_KEYS):
        raise ValueError(f"{who}: a mapping with keys out of {_SEARCH_KEYS} is expected, got {item!r}")
    for k in ("lo", "hi", "rule", "trials", "targets", "fail_on"):
        if k not in item:
            raise ValueError(f"{who}: '{k}' is missing")
    try:
        lo, hi = float(item["lo"]), float(item["hi"])
        start = float(item["start"]) if item.get("start") is not None else (lo + hi) / 2
        step = float(item["step"]) if item.get("step") is not None else (hi - lo) / 4
        min_step = float(item["min_step"]) if item.get("min_step") is not None else (hi - lo) / 256
    except (TypeError, ValueError):
        raise ValueError(f"{who}: lo, hi, start, step and min_step must be numbers") from None
    lo, hi, start, step, min_step = (float(np.float32(x)) for x in (lo, hi, start, step, min_step))
    if not (math.isfinite(lo) and math.isfinite(hi)) or not lo < hi:
        raise ValueError(f"{who}: lo {lo} and hi {hi} must be finite with lo < hi")
    if not lo <= start <= hi:
        raise ValueError(f"{who}: start {start} lies outside [{lo}, {hi}]")
    if not (math.isfinite(step) and 0 < min_step <= step):
        raise ValueError(f"{who}: the steps must hold 0 < min_step <= step, got min_step {min_step}, step {step}")
    rule = item["rule"]
    if rule not in SEARCH_RULES:
        raise ValueError(f"{who}: unknown rule {rule!r} ({', '.join(SEARCH_RULES)})")
    trials, rev_skip = item["trials"], item.get("rev_skip", 0)
    if isinstance(trials, bool) or not isinstance(trials, (int, np.integer)) or not 1 <= int(trials) <= MAX_SEARCH_TRIALS:
        raise ValueError(f"{who}: trials {trials!r}: an integer 1..2^20")
    if isinstance(rev_skip, bool) or not isinstance(rev_skip, (int, np.integer)) or not 0 <= int(rev_skip) <= MAX_SEARCH_REV_SKIP:
        raise ValueError(f"{who}: rev_skip {rev_skip!r}: an integer 0..{MAX_SEARCH_REV_SKIP}")
    harder = item.get("harder", "up")
    if not isinstance(harder, str) or harder not in SEARCH_HARDER:
        raise ValueError(f"{who}: harder {harder!r}: 'up' or 'down'")
    out = {"lo": lo, "hi": hi, "start": start, "step": step, "min_step": min_step, "rule": rule, "trials": int(trials)}
    kinds = {"params": _ParamKind(), **{k.key: k for k in FAULT_KINDS}}
    check_names = [r[7] for r in check_rows]

    def extra(key, n):      # whether n is one of the forms beyond the plain names
        if not isinstance(n, str):
            return False
        if key == "targets":
            return n.partition(":")[0] in kinds
        return n == "checks" or n.startswith("check:")
    for key, known in (("targets", SEARCH_TARGETS), ("fail_on", SEARCH_FAIL_ON)):
        names = item[key]
        if (isinstance(names, str) or not isinstance(names, (list, tuple)) or not names or len(set(names)) != len(names)
                or any(n not in known and not extra(key, n) for n in names)):
            more = ", ".join(f"{k}[:i,j]" for k in kinds) if key == "targets" else "checks, check:NAME, check:I"
            raise ValueError(f"{who}: {key} {names!r}: a non-empty list of different names out of {', '.join(known)}, {more}")
        out[key] = [n for n in known if n in names] + [n for n in names if n not in known]
    out["marks"], out["check_mask"] = {}, 0
    for n in out["targets"]:
        kind = kinds.get(n.partition(":")[0])
        if kind is None:
            continue
        if kind.key in out["marks"]:
            raise ValueError(f"{who}: targets {item['targets']!r}: '{kind.key}' is named twice")
        out["marks"][kind.key] = _search_marks(who, kind, n, (fault_rows or {}).get(kind.key) or [], lo, hi)
    for n in out["fail_on"]:
        if n == "checks":
            if not check_rows:
                raise ValueError(f"{who}: fail_on 'checks' and the scenario has no check")
            out["check_mask"] |= (1 << len(check_rows)) - 1
        elif n.startswith("check:"):
            ref = n[len("check:"):]
            idx = [i for i, cn in enumerate(check_names) if cn == ref]
            if not idx and ref.isdigit() and int(ref) < len(check_rows):
                idx = [int(ref)]
            if not idx:
                raise ValueError(f"{who}: fail_on {n!r}: the scenario has no check of that name or ordinal (it has {len(check_rows)}: "
                                 f"{', '.join(str(c) for c in check_names) or 'none'})")
            out["check_mask"] |= sum(1 << i for i in idx)
    out["harder"] = harder
    if "pushes" in out["targets"] and not has_pushes:
        raise ValueError(f"{who}: the target is the pushes and the scenario has no push window")
    if "commands" in out["targets"] and not has_keys:
        raise ValueError(f"{who}: the target is the commands and the scenario has no keyframe")
    out["rev_skip"] = int(rev_skip)
    return out


def sweep(commands: Iterable, push_speeds: Iterable = (), directions: Iterable = (0.0,), push_times: Iterable = (),
          params: Iterable = (), checks: Iterable = (), curves: Iterable = (), faults: Iterable = (),
          action_faults: Iterable = (), search: Iterable = (), latency: Iterable = ()) -> Iterator[dict]:
    """The cartesian product command rows x push speeds x directions x push times as scenarios, commands outermost: each holds its
    command from episode step 0 and one push of ``speed`` m/s along the world direction ``angle`` (radians about z, 0 = +x) held over
    ``(t0, t1)``.  With no speeds or no times the product is over the commands alone (no push).
    ``len(list(sweep(C, V, D, T))) == len(C) * len(V) * len(D) * len(T)``.  ``params``: a list of window lists (each a scenario's
    ``"params"`` value, possibly empty) is one more cartesian axis, innermost: every scenario above is emitted once per window list,
    ``len(...) * len(P)`` scenarios in all.  ``checks``: a list of check lists (each a scenario's ``"checks"`` value, possibly empty)
    is one more axis, inside the parameters: ``len(...) * len(K)`` scenarios.  ``curves``: a list of curve lists (each a scenario's
    ``"curves"`` value, possibly empty) is one more axis, inside the checks.  ``faults``: a list of fault lists (each a scenario's
    ``"faults"`` value, possibly empty) is one more axis, inside the curves: ``len(...) * len(F)`` scenarios.  ``action_faults``: a list
    of action-fault lists (each a scenario's ``"action_faults"`` value, possibly empty) is one more axis, inside the faults and innermost
    of the tables: ``len(...) * len(A)`` scenarios.  ``search``: a list of search items (each a scenario's ``"search"`` value, or ``None``
    for a scenario without one) is one more axis, inside the action faults: ``len(...) * len(L)`` scenarios.  ``latency``: a list of
    latency lists (each a scenario's ``"latency"`` value, possibly empty) is one more axis, innermost of all: ``len(...) * len(Y)``
    scenarios -- ``latency=[[], [[0, 1000, "action", "*", 2]], [[0, 1000, "action", "*", 4]]]`` with ``by_scenario()`` is the latency
    a policy still tolerates."""
    latency = [list(f) for f in latency]
    if latency:
        for sc in sweep(commands, push_speeds, directions, push_times, params, checks, curves, faults, action_faults, search):
            for fl in latency:
                out = dict(sc)
                if fl:
                    out["latency"] = [dict(f) if isinstance(f, dict) else list(f) for f in fl]
                yield out
        return
    search = list(search)
    if search:
        for sc in sweep(commands, push_speeds, directions, push_times, params, checks, curves, faults, action_faults):
            for item in search:
                out = dict(sc)
                if item is not None:
                    out["search"] = dict(item)
                yield out
        return
    action_faults = [list(f) for f in action_faults]
    if action_faults:
        for sc in sweep(commands, push_speeds, directions, push_times, params, checks, curves, faults):
            for fl in action_faults:
                out = dict(sc)
                if fl:
                    out["action_faults"] = [dict(f) if isinstance(f, dict) else list(f) for f in fl]
                yield out
        return
    faults = [list(f) for f in faults]
    if faults:
        for sc in sweep(commands, push_speeds, directions, push_times, params, checks, curves):
            for fl in faults:
                out = dict(sc)
                if fl:
                    out["faults"] = [dict(f) if isinstance(f, dict) else list(f) for f in fl]
                yield out
        return
    curves = [list(c) for c in curves]
    if curves:
        for sc in sweep(commands, push_speeds, directions, push_times, params, checks):
            for cl in curves:
                out = dict(sc)
                if cl:
                    out["curves"] = [dict(c) if isinstance(c, dict) else list(c) for c in cl]
                yield out
        return
    checks = [list(c) for c in checks]
    if checks:
        for sc in sweep(commands, push_speeds, directions, push_times, params):
            for cl in checks:
                out = dict(sc)
                if cl:
                    out["checks"] = [dict(c) if isinstance(c, dict) else list(c) for c in cl]
                yield out
        return
    params = [[list(w) for w in wins] for wins in params]
    if params:
        for sc in sweep(commands, push_speeds, directions, push_times):
            for wins in params:
                out = dict(sc)
                if wins:
                    out["params"] = [list(w) for w in wins]
                yield out
        return
    commands = [[float(x) for x in c] for c in commands]
    speeds, directions, times = [float(v) for v in push_speeds], [float(a) for a in directions], [tuple(int(x) for x in w) for w in push_times]
    if not speeds or not times:
        for c in commands:
            yield {"commands": [[0] + c], "pushes": []}
        return
    for c, v, a, (t0, t1) in itertools.product(commands, speeds, directions, times):
        yield {"commands": [[0] + c], "pushes": [[t0, t1, v * math.cos(a), v * math.sin(a), 0.0]]}


def scenario_rows(n_scn: int, mode, gid, ep) -> np.ndarray:
    """The rule's row per env: ``gid mod S`` (mode ``env`` / 0) or ``(gid mod S + uint32(ep) mod S) mod S`` (``cycle`` / 1)."""
    S = int(n_scn)
    mode = MODES[mode] if isinstance(mode, str) else int(mode)
    gid = np.asarray(gid, dtype=np.int64)
    row = np.mod(gid, S)                                           # non-negative for negative ids too
    if mode == 1:
        ep32 = np.asarray(ep, dtype=np.int64) & 0xFFFFFFFF          # the meta word as uint32
        row = (row + ep32 % S) % S
    return row.astype(np.int32)


def reference_schedule(table: ScenarioTable, mode, gid, t, ep, base_cmd, level=None):
    """Numpy twin of ``scenario_step_kernel`` for N envs: global ids ``gid``, episode steps ``t`` (meta word 0), episodes ended ``ep``
    (meta word 11), the caller's commands ``base_cmd`` ``[N, >= command_dim]``.  Returns ``(row int32[N], cmd float32[N,
    command_dim], push_mask bool[N], push_v float32[N, 3])``: the command each env is given and the world velocity of the push that
    is due (zero rows where none is).  Rows and commands are exact.  ``level`` (float32 ``[N]``): the twin of
    ``scenario_search_step_kernel`` -- where the env's row has a search item, a selected keyframe row (target ``"commands"``) and the
    push that is due (target ``"pushes"``) are multiplied by the env's level, one float32 multiply per word; a passed-through caller's
    command and rows without an item are not scaled."""
    gid, t = np.asarray(gid, dtype=np.int64).reshape(-1), np.asarray(t, dtype=np.int64).reshape(-1)
    N, cd = len(gid), table.command_dim
    row = scenario_rows(len(table), mode, gid, np.asarray(ep).reshape(-1))
    cmd = np.array(np.asarray(base_cmd, dtype=np.float32).reshape(N, -1)[:, :cd], dtype=np.float32)
    mask, v = np.zeros(N, dtype=bool), np.zeros((N, 3), dtype=np.float32)
    level = None if level is None else np.asarray(level, dtype=np.float32).reshape(N)
    for i in range(N):
        item = table.search[row[i]] if level is not None else None
        targets = item["targets"] if item is not None else ()
        for kt, c in table.keys[row[i]]:
            if kt > t[i]:
                break
            cmd[i] = c * level[i] if "commands" in targets else c
        for t0, t1, pv in table.pushes[row[i]]:
            if t0 <= t[i] < t1:
                mask[i], v[i] = True, (pv * level[i] if "pushes" in targets else pv)
    return row, cmd, mask, v


def reference_params(table: ScenarioTable, mode, gid, t, ep, base_params, layout: dict, level=None) -> np.ndarray:
    """Numpy twin of ``scnparams_step_kernel`` for N envs: global ids ``gid``, episode steps ``t`` (meta word 0), episodes ended ``ep``
    (meta word 11), the base parameter records ``base_params`` ``[N, stride]`` and ``layout`` (``param_layout``: word offset per
    field).  Returns the effective records float32 ``[N, stride]``, exact: a word under no window that holds is the base word.
    ``level`` (float32 ``[N]``, ``None``: no search): the twin of ``scnparams_search_step_kernel`` -- an item its row's search item marks
    uses ``v = float32(value * level)`` of the env: ``scale`` gives ``base * v``, ``set`` gives ``v``."""
    gid, t = np.asarray(gid, dtype=np.int64).reshape(-1), np.asarray(t, dtype=np.int64).reshape(-1)
    base = np.ascontiguousarray(base_params, dtype=np.float32).reshape(len(gid), -1)
    eff = base.copy()
    row = scenario_rows(len(table), mode, gid, np.asarray(ep).reshape(-1))
    items = table._resolved()
    for i in range(len(gid)):
        marks = table.search_marks("params", row[i]) if level is not None else []
        for k, (t0, t1, field, index, op, value) in enumerate(items[row[i]]):
            if t0 <= t[i] < t1:
                w = layout[_FIELD_NAMES[field]] + index
                v = np.float32(value)
                if marks and table.param_ords[row[i]][k] in marks:
                    v = np.float32(v * np.float32(np.asarray(level, dtype=np.float32).reshape(-1)[i]))
                eff[i, w] = v if op == PARAM_OPS["set"] else np.float32(base[i, w] * v)
    return eff


def _level_value(table: ScenarioTable, key: str, r: int, ordinal: int, value, level):
    """The value word of item ``ordinal`` of row ``r`` for envs at ``level`` (``[M]`` float32 or ``None``): ``float32(value * level)``
    where the row's search item marks the item, else the value itself."""
    if level is None or ordinal not in table.search_marks(key, r):
        return np.float32(value)
    return (np.float32(value) * np.asarray(level, dtype=np.float32)).astype(np.float32)


def _fault_op(name: str, el: int, ordinal: int, value, x, prev, first, draw) -> np.ndarray:
    """One holding item ``name`` on the words ``x`` ``[M]`` of element ``el`` of M envs, float32, as ``fault_op`` / ``fault_walk``
    (csrc/cosim_fault.h) compute it: ``prev`` ``[M]`` the previous words, ``first`` ``[M]`` bool the envs at clock 0 (hold and drop are
    the identity there), ``draw(index)`` the envs' Philox words of the kind's purpose."""
    from . import rng
    v = np.asarray(value, dtype=np.float32)                         # one word, or one per env (a search's marked item)
    if name == "scale":
        x = x * v
    elif name == "bias":
        x = x + v
    elif name == "set":
        x = np.broadcast_to(v, x.shape).astype(np.float32)
    elif name == "noise":
        x = x + (v * rng.fault_noise_u(draw(el))).astype(np.float32)
    elif name == "clip":
        x = np.where(x > v, v, np.where(x < -v, -v, x))
    else:                                                           # hold / drop: one draw for the listed item
        lost = rng.fault_drop_u(draw(rng.FAULT_DROP_INDEX + ordinal)) < v if name == "drop" else True
        x = np.where(lost & ~first, prev, x)
    return x.astype(np.float32)


def reference_obs_faults(table: ScenarioTable, mode, gid, t_obs, ep, step_count, seed: int, frames, layout: dict, active=None, level=None) -> np.ndarray:
    """Numpy twin of ``obsfault_step_kernel`` over a run of K observations of N envs, exact.  ``gid`` ``[N]`` global ids; per
    observation k the POST-step meta words ``t_obs[k]`` (word 0), ``ep[k]`` (word 11) and ``step_count[k]`` (word 1), each ``[K, N]``;
    ``frames`` ``[K, N, frame_dim]`` float32, the CLEAN newest frame of every observation (the first ``stacked_dim`` words and the
    non-stacked tail of a fault-free run's ``state_out`` row); ``layout`` (``fault_layout``).  ``active`` ``[K, N]`` bool (default: all):
    observations an env did not take part in (a masked reset's other envs) leave its stack alone and repeat its row.  The twin
    emulates the roll and the fill -- an env's first observation must be a fill (``t_obs = 0``) -- and returns the faulted
    ``state_out`` rows ``[K, N, state_dim]``, stack rows included.  ``level`` (float32 ``[K, N]``, ``None``: no search): the twin of
    ``obsfault_search_step_kernel`` -- per observation the level of the episode it belongs to (behind a step that ended a counted
    trial: the level AFTER the move); an item its row's search item marks uses ``float32(value * level)``."""
    from . import rng
    gid = np.asarray(gid, dtype=np.int64).reshape(-1)
    N, sd, fd, S = len(gid), int(layout["stacked_dim"]), int(layout["frame_dim"]), int(layout["stack_size"])
    frames = np.ascontiguousarray(frames, dtype=np.float32).reshape(-1, N, fd)
    K = frames.shape[0]
    t_obs, ep, step_count = (np.asarray(a).reshape(K, N) for a in (t_obs, ep, step_count))
    active = np.ones((K, N), dtype=bool) if active is None else np.asarray(active, dtype=bool).reshape(K, N)
    cmd = np.zeros(sd, dtype=bool)
    cmd[[e for e in layout.get("command", []) if e < sd]] = True
    items = table._resolved_items(_OBS_FAULTS)
    stack = np.full((N, S, sd), np.nan, dtype=np.float32)
    out = np.full((K, N, S * sd + fd - sd), np.nan, dtype=np.float32)
    u32 = np.uint32
    for k in range(K):
        act, fill = active[k], active[k] & (t_obs[k] == 0)
        roll = act & ~fill
        if S > 1:
            stack[roll, 1:] = stack[roll, :-1]
        stack[roll, 0] = frames[k, roll, :sd]
        stack[fill] = frames[k, fill, None, :sd]
        tail = frames[k, :, sd:].copy()
        row = scenario_rows(len(table), mode, gid, ep[k])
        for r in np.unique(row[act]):
            for t0, t1, e, op, ordinal, value in items[r]:
                m = act & (row == r) & (t0 <= t_obs[k]) & (t_obs[k] < t1)
                if not m.any():
                    continue
                x = stack[m, 0, e] if e < sd else tail[m, e - sd]
                draw = lambda index: rng.first_word(seed, gid[m].astype(np.uint64), step_count[k, m].astype(u32), rng.PURPOSE_OBS_FAULT, index)   # noqa: E731
                v = _level_value(table, _OBS_FAULTS.key, r, ordinal, value, None if level is None else np.asarray(level, dtype=np.float32).reshape(K, N)[k, m])
                x = _fault_op(_OBS_FAULTS.op_names[op], e, ordinal, v, x, stack[m, 1, e] if e < sd and S > 1 else x, t_obs[k, m] == 0, draw)
                if e >= sd:
                    tail[m, e - sd] = x
                else:
                    stack[m, 0, e] = x
                    f = m & fill
                    stack[f, :, e] = stack[f, 0, e][:, None]        # a fill left the first frame in every row
        rows_out = stack.copy()
        rows_out[:, :, cmd] = frames[k, :, None, :sd][:, :, cmd]    # every stack row of state_out holds the applied command
        new = np.concatenate([rows_out.reshape(N, S * sd), tail], axis=1)
        out[k] = np.where(act[:, None], new, out[k - 1] if k > 0 else new)
    return out


def reference_action_faults(table: ScenarioTable, mode, gid, t, ep, step_count, seed: int, raw, prev_eff, level=None) -> np.ndarray:
    """Numpy twin of ONE step of ``actfault_step_kernel`` for N envs, exact.  ``gid`` ``[N]`` global ids; the PRE-STEP meta words ``t``
    (word 0), ``ep`` (word 11) and ``step_count`` (word 1), each ``[N]``; ``raw`` ``[N, nu]`` float32, the caller's actions; ``prev_eff``
    ``[N, nu]`` float32, the record's ``s_lastact``: the effective action of the env's previous step, zeros where that step ended the
    episode (or none was taken).  Returns the effective actions ``[N, nu]``: an actuator under no holding item keeps the caller's
    bits.  ``level`` (float32 ``[N]``, ``None``: no search): the twin of ``actfault_search_step_kernel`` -- an item its row's search item
    marks uses ``float32(value * level)`` of the env, the level its open episode runs at."""
    from . import rng
    gid = np.asarray(gid, dtype=np.int64).reshape(-1)
    N = len(gid)
    raw = np.ascontiguousarray(raw, dtype=np.float32).reshape(N, -1)
    prev = np.ascontiguousarray(prev_eff, dtype=np.float32).reshape(N, -1)
    t, ep, step_count = (np.asarray(a).reshape(N) for a in (t, ep, step_count))
    eff = raw.copy()
    items = table._resolved_items(_ACTION_FAULTS)
    row = scenario_rows(len(table), mode, gid, ep)
    u32 = np.uint32
    for r in np.unique(row):
        for t0, t1, j, op, ordinal, value in items[r]:
            m = (row == r) & (t0 <= t) & (t < t1)
            if not m.any():
                continue
            draw = lambda index: rng.first_word(seed, gid[m].astype(np.uint64), step_count[m].astype(u32), rng.PURPOSE_ACTION_FAULT, index)   # noqa: E731
            v = _level_value(table, _ACTION_FAULTS.key, r, ordinal, value, None if level is None else np.asarray(level, dtype=np.float32).reshape(N)[m])
            eff[m, j] = _fault_op(_ACTION_FAULTS.op_names[op], j, ordinal, v, eff[m, j], prev[m, j], t[m] == 0, draw)
    return eff


class LatencyTwin:
    """Numpy twin of ``latency_act_kernel`` / ``latency_obs_kernel`` (csrc/cosim_latency.hip) for N envs, exact.  It keeps what the
    engine keeps: per channel kind a line ``[N, D, width]`` of clean words (slot = clock mod D, D = ``depth`` or the table's
    ``latency_depth``) and per env the clock ``from`` its line is valid from (below 0: invalid).  ``gid`` ``[N]`` global env ids, ``nu``
    and ``frame_dim`` the widths.  A reset needs no call: clock 0 restarts a line."""

    def __init__(self, table: ScenarioTable, mode, gid, seed: int, nu: int, frame_dim: int, depth: int = None):
        self.table, self.mode, self.seed = table, mode, int(seed)
        self.gid = np.asarray(gid, dtype=np.int64).reshape(-1)
        self.N = len(self.gid)
        self.D = int(depth or table.latency_depth)
        if self.D < table.latency_depth:
            raise ValueError(f"LatencyTwin: depth {self.D} is below the table's {table.latency_depth}")
        self.width = (int(nu), int(frame_dim))
        self.line = [np.zeros((self.N, self.D, w), dtype=np.float32) for w in self.width]
        self.valid_from = [np.full(self.N, -1, dtype=np.int64) for _ in self.width]

    def cut(self, mask=None):
        """A host cut that is no reset (``restore``, ``fork``, ``set_state``) of the envs under ``mask`` (default: all): their lines are
        invalid and restart at the next clock their kernel finds."""
        m = np.ones(self.N, dtype=bool) if mask is None else np.asarray(mask, dtype=bool).reshape(self.N)
        for f in self.valid_from:
            f[m] = -1

    def _step(self, kind: int, words, t, ep, step_count, active):
        from . import rng
        N, D, W = self.N, self.D, self.width[kind]
        x = np.ascontiguousarray(words, dtype=np.float32).reshape(N, W)
        t, ep, step_count = (np.asarray(a).astype(np.int64).reshape(N) for a in (t, ep, step_count))
        act = np.ones(N, dtype=bool) if active is None else np.asarray(active, dtype=bool).reshape(N)
        row = scenario_rows(len(self.table), self.mode, self.gid, ep)
        items = self.table._resolved_latency()
        k, has = np.zeros((N, W), dtype=np.int64), np.zeros(N, dtype=bool)
        for r in np.unique(row[act]):
            its = [it for it in items[r] if it[2] == kind]
            if not its:
                continue
            in_row = act & (row == r)
            has |= in_row
            for t0, t1, _, el, ordinal, steps, jitter in its:      # the last listed item that holds wins
                m = in_row & (t0 <= t) & (t < t1)
                if not m.any():
                    continue
                kk = np.full(int(m.sum()), steps, dtype=np.int64)
                if jitter > 0:
                    w = rng.first_word(self.seed, self.gid[m].astype(np.uint64), step_count[m].astype(np.uint32), rng.PURPOSE_LATENCY, ordinal)
                    kk = kk + rng.latency_jitter(w, jitter)
                k[m, el] = np.minimum(kk, D - 1)
        f = self.valid_from[kind]
        restart = has & ((t == 0) | (f < 0) | (f > t))
        f[restart] = t[restart]
        line = self.line[kind]
        idx = np.nonzero(has)[0]
        line[idx, t[idx] % D] = x[idx]
        c = t[:, None] - k
        late = c >= f[:, None]
        src = np.where(late, c, f[:, None])
        got = line[np.arange(N)[:, None], np.mod(src, D), np.arange(W)[None, :]]
        if kind == LATENCY_ACTION:                                  # nothing has arrived yet after a reset
            got = np.where(~late & (f == 0)[:, None], np.float32(0.0), got)
        return np.where(has[:, None] & (k > 0), got, x).astype(np.float32)

    def step_actions(self, raw, t, ep, step_count) -> np.ndarray:
        """One control step: ``raw`` ``[N, nu]`` float32, the caller's actions; the PRE-STEP meta words ``t`` (word 0), ``ep`` (word 11)
        and ``step_count`` (word 1), each ``[N]``.  Returns the delivered actions ``[N, nu]``: what the step kernels (or the action
        faults) are handed."""
        return self._step(LATENCY_ACTION, raw, t, ep, step_count, None)

    def step_obs(self, frames, t_obs, ep, step_count, active=None) -> np.ndarray:
        """One observation: ``frames`` ``[N, frame_dim]`` float32, the CLEAN newest frame (the first ``stacked_dim`` words and the
        non-stacked tail of a latency-free run's ``state_out`` row); the POST-step meta words ``t_obs``, ``ep``, ``step_count``, each
        ``[N]``; ``active`` ``[N]`` bool (default: all): the envs a masked reset touched.  Returns the delivered newest frames ``[N,
        frame_dim]`` (an env that is not active gets its clean row back); ``reference_obs_faults`` over them emulates the stack's roll
        and fill, with or without faults on top."""
        return self._step(LATENCY_OBS, frames, t_obs, ep, step_count, active)


def push_reference(quat, v) -> np.ndarray:
    """``qvel[0:3]`` after a push of world velocity ``v`` at base quaternion ``quat = (w, x, y, z)`` (used raw, reference
    flamingo_light_v1.py:234-243), in float64: ``(R^T v)[0:2]`` and ``v[2]``."""
    w, x, y, z = (np.asarray(quat, dtype=np.float64)[..., k] for k in range(4))
    v = np.asarray(v, dtype=np.float64)
    R00, R01 = 1 - 2 * y * y - 2 * z * z, 2 * x * y - 2 * z * w
    R10, R11 = 2 * x * y + 2 * z * w, 1 - 2 * x * x - 2 * z * z
    R20, R21 = 2 * x * z - 2 * y * w, 2 * y * z + 2 * x * w
    return np.stack([R00 * v[..., 0] + R10 * v[..., 1] + R20 * v[..., 2], R01 * v[..., 0] + R11 * v[..., 1] + R21 * v[..., 2], v[..., 2]], axis=-1)
