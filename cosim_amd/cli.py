"""Headless runner: the reference's GUI + ``Tester`` session as one command.

    python -m cosim_amd.cli --env flamingo_light_v1 --num-envs 4096 --steps 1000 --command 0.5 0 0 0 \\
        --policy sinusoid | random-mlp | path/to/actor.onnx  [--terrain rocky_hard] [--push-at 200 --push 0.5 0 0] \\
        [--report report.json] [--trace-env 0] [--checkpoint snap.npz --checkpoint-at 500] [--resume snap.npz [--fork-row 7]] \
        [--history 8 10] [--ledger 4 [--ledger-out episodes.npz]] [--scenarios tests.yaml [--scenario-mode env|cycle]] \
        [--failure-traces 50 2 [--failure-traces-on terminated tilt] [--failure-traces-out traces.npz]] \
        [--fall-tilt 0.8 --fall-height 0.1 --fall-grace 5 --fall-bodies base_link,left_leg_link]
    python -m cosim_amd.cli --config session.yaml

One process per GPU: under ``torchrun`` every rank simulates its shard of ``--num-envs`` and rank 0 writes the report.

``--config`` (YAML in, report out) replaces a GUI session of the reference: what ``ui/main_window.py:709-788`` gathers from
widgets, plus the two things a user does WHILE the test runs -- key-driven commands (``ui/main_window.py:272-290`` ->
``Tester.update_command``, core/tester.py:41-46) as a time series, and the push button (held: ``core/tester.py:80-81`` applies
the push every loop iteration while ``_push_event`` is set) as a schedule:

    env:      {id: flamingo_p_v3, terrain: rocky_easy, max_duration: 120.0, position_command: false}
    engine:   {num_envs: 4096, seed: 1234}
    random:   {sensor_noise: low, action_delay_prob: 0.05, ...}        # overrides of the GUI defaults (config.make_config)
    observation: {stack_size: 3, ...}                                   # likewise
    policy:   {kind: sinusoid | random-mlp | onnx, onnx_file: actor.onnx, use_lstm: false, h_in_dim: 256, c_in_dim: 256}
    policy:   {onnx_files: [a.onnx, b.onnx], assign: interleave | cross, names: [base, tuned], rotate: 1}   # a policy table (policy.PolicyTable): every env
                                                                       # driven by one of the files; same as --policy a.onnx b.onnx
                                                                       # --policy-assign --policy-names --policy-rotate; the report gets episodes.by_policy.
                                                                       # Files with h_in / c_in inputs make a recurrent table
                                                                       # (policy.RecurrentPolicyTable): the kind is detected from the files,
                                                                       # all of one kind; use_lstm belongs to a single onnx_file
    steps:    1000
    commands: [[0, 0.5, 0, 0, 0], [200, 1.0, 0, 0.3, 0]]              # from control step t on: user_command = c0 .. c3
    pushes:   [[300, 310, 0.5, 0, 0]]                                   # held for steps t0 <= k < t1: event("push", [vx, vy, vz])
    report:   report.json
    trace_env: 0
    percentiles: true
    hfield_fixup: true                                                 # or engine: {hfield_fixup: true}; same as --hfield-fixup
    spawn:    {pattern: uniform, count: 256, extent: 100.0, per_episode: true, clearance: 0.01}   # or engine: {spawn: {...}}; same as --spawn*
    scenarios: [{commands: [[0, 0.5, 0, 0, 0], [100, 1.0, 0, 0, 0]], pushes: [[150, 155, 0.5, 0, 0]]}, {commands: [[0, 0.2, 0, 0, 0]]}]
    scenario_mode: cycle                                               # per-ENV schedules on the device, keyed by each env's own episode step
                                                                       # (cosim_amd/scenario.py; or a YAML file: --scenarios); unlike
                                                                       # commands: / pushes: they run under --graph and --pipelined too;
                                                                       # a scenario may also hold params:, faults:, action_faults:
                                                                       # ([[t0, t1, index, op, value], ...]: what the motors are told),
                                                                       # latency: ([[t0, t1, channel, index, steps, jitter], ...]: k-step delays), ...
    fall:     {tilt: 0.8, height: 0.1, grace: 5, bodies: [base_link]}  # fall rule (cosim_amd/fall.py): end an episode on tilt (rad), base
                                                                       # height (m) or contact of the listed bodies; or engine: {fall: {...}};
                                                                       # same as --fall-*; runs under --graph and --pipelined too
    search:   8                                                        # arm the scenarios' search: items (a scenario may hold search: {lo, hi,
                                                                       # rule, trials, targets, fail_on, ...}: a per-env level that scales its
                                                                       # pushes / commands and moves when an episode ends) and keep 8 trials per
                                                                       # env; or engine: {search: 8}; same as --search; needs scenario_mode env

Flags given on the command line override the file.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np


def session_opt(sess: dict):
    """``opt(flag_value, key, default)`` over a session mapping: the flag if given, else the session's top-level ``key``, else
    ``session["engine"][key]``, else ``default``.  Given means ``is not None``: a top-level ``0`` / ``False`` wins over the engine's."""
    s_eng = sess.get("engine", {}) or {}

    def opt(flag_value, key, default):
        return next((v for v in (flag_value, sess.get(key), s_eng.get(key)) if v is not None), default)
    return opt


def rank_path(path: str, rank: int, world: int) -> str:
    """Where a rank writes a per-rank output: ``path`` itself in a single process, else ``stem.rank<rank>.ext``."""
    if world == 1:
        return path
    stem, ext = os.path.splitext(path)
    return "%s.rank%d%s" % (stem, rank, ext)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="cosim_amd.cli", description=__doc__.split("\n")[0])
    ap.add_argument("--config", default="", help="YAML session file (see the module docstring); flags override it")
    ap.add_argument("--env", default=None)
    ap.add_argument("--terrain", default=None)
    ap.add_argument("--num-envs", type=int, default=None, help="total over all ranks")
    ap.add_argument("--steps", type=int, default=None, help="control steps (50 Hz)")
    ap.add_argument("--policy", default=None, nargs="+", metavar="POLICY",
                    help="sinusoid | random-mlp | <file.onnx>, or several ONNX actor files: a policy table, every env driven by one of them "
                         "(MLP actors, or recurrent ones with h_in / c_in inputs: the kind is detected from the files, all of one kind)")
    ap.add_argument("--policy-assign", choices=["interleave", "cross"], default=None,
                    help="several --policy files: env g runs policy g mod K (interleave, the default) or (g // S) mod K with S scenarios (cross)")
    ap.add_argument("--policy-rotate", type=int, default=None, metavar="EVERY",
                    help="several --policy files: every env moves to the next file after EVERY of its episodes (a paired design: every robot meets every "
                         "checkpoint); episodes.by_policy attributes each episode to the file that drove it")
    ap.add_argument("--policy-names", nargs="+", default=None, metavar="NAME", help="several --policy files: their names in the report (default: the file stems)")
    ap.add_argument("--lstm", action="store_true", help="the ONNX file is an LSTM policy with h_in / c_in inputs (a single --policy file; several recurrent files need no flag)")
    ap.add_argument("--hidden-dim", type=int, default=256, help="h_in_dim = c_in_dim of an LSTM policy")
    ap.add_argument("--command", type=float, nargs="*", default=None)
    ap.add_argument("--position-command", action="store_true")
    ap.add_argument("--max-duration", type=float, default=None)
    ap.add_argument("--seed", type=int, default=None)
    ap.add_argument("--push-at", type=int, default=-1, help="control step at which a push event fires")
    ap.add_argument("--push", type=float, nargs=3, default=[0.5, 0.0, 0.0])
    ap.add_argument("--report", default=None, help="write the fleet report (JSON) here")
    ap.add_argument("--trace-env", type=int, default=None, help="also keep the per-step info series of this local env")
    ap.add_argument("--percentiles", action="store_true", help="p5 / p50 / p95 of tracking error, |torque| and action-RMSE in the report")
    ap.add_argument("--graph", action="store_true", help="capture policy -> step -> report in a HIP graph and replay it (ONNX policies)")
    ap.add_argument("--pipelined", action="store_true",
                    help="policy -> step -> report per env range on the range's own stream, no fleet-wide barrier per step (an ONNX MLP policy, or a policy table of either kind)")
    ap.add_argument("--ranges", type=int, default=4, help="env ranges of --pipelined")
    ap.add_argument("--hfield-fixup", action="store_true",
                    help="heightfield terrain: redo steps whose ground contacts exceed the fleet kernel's slots instead of cutting them off")
    ap.add_argument("--spawn", choices=["grid", "uniform"], default=None,
                    help="spread resets over the terrain: a table of base poses on a grid / drawn uniformly, placed on the heightfield")
    ap.add_argument("--spawn-count", type=int, default=None, help="rows of the spawn table (default: --num-envs)")
    ap.add_argument("--spawn-extent", type=float, default=None, help="half-size (m) of the square the poses fill (default: the field minus the footprint)")
    ap.add_argument("--spawn-per-episode", action="store_true", help="draw a row anew at every reset instead of row = env id mod count")
    ap.add_argument("--spawn-clearance", type=float, default=None, help="extra height (m) above the no-penetration placement")
    ap.add_argument("--checkpoint", default=None, help="write a full-state snapshot (.npz) here after --checkpoint-at control steps, then go on")
    ap.add_argument("--checkpoint-at", type=int, default=None, help="control step (of the session's clock) after which --checkpoint is written")
    ap.add_argument("--resume", default=None, help="start from this snapshot instead of a reset; --steps more control steps are run")
    ap.add_argument("--fork-row", type=int, default=None, help="with --resume: every env starts from this row of the file, parameters included")
    ap.add_argument("--history", type=int, nargs=2, default=None, metavar=("SLOTS", "EVERY"),
                    help="keep a ring of SLOTS full-state captures on the device, one after every EVERY-th control step")
    ap.add_argument("--ledger", type=int, default=None, metavar="SLOTS",
                    help="keep the last SLOTS episode records of every env on the device; their summary goes into the report as \"episodes\"")
    ap.add_argument("--ledger-out", default=None, metavar="PATH.npz", help="with --ledger: write this rank's episode records here")
    ap.add_argument("--scenarios", default=None, metavar="FILE.yaml",
                    help="scenario table: per-env command and push schedules applied on the device (also under --graph / --pipelined)")
    ap.add_argument("--scenario-mode", choices=["env", "cycle"], default=None,
                    help="env: row = env id mod S; cycle: every env walks through the scenarios, one per episode")
    ap.add_argument("--fall-tilt", type=float, default=None, metavar="RAD", help="fall rule: end an episode when the base tilts further than this from upright")
    ap.add_argument("--fall-height", type=float, default=None, metavar="M", help="fall rule: end an episode when the base is lower than this above the ground under it")
    ap.add_argument("--fall-grace", type=int, default=None, metavar="STEPS", help="fall rule: control steps at the start of an episode without the tilt / height test")
    ap.add_argument("--fall-bodies", default=None, metavar="a,b,c", help="fall rule: bodies whose contact force ends the episode (replaces the robot's own list)")
    ap.add_argument("--failure-traces", type=int, nargs=2, default=None, metavar=("FRAMES", "KEEP"),
                    help="keep every env's last FRAMES control steps on the device and freeze them as a trace when an episode ends with a "
                         "selected cause; the KEEP newest traces per env stay (also under --graph / --pipelined)")
    ap.add_argument("--failure-traces-on", nargs="+", default=None, metavar="NAME",
                    help="causes that freeze a window: terminated truncated nonfinite tilt height contact (default: terminated nonfinite)")
    ap.add_argument("--failure-traces-out", default=None, metavar="PATH.npz", help="with --failure-traces: write this rank's traces here")
    ap.add_argument("--check-slots", type=int, default=None, metavar="SLOTS",
                    help="judge the checks of the scenario table on the device and keep the last SLOTS (1..64) verdict records of every env; "
                         "their summary goes into the report as \"episodes.checks\" (also under --graph / --pipelined)")
    ap.add_argument("--verdicts-out", default=None, metavar="PATH.npz", help="with --check-slots: write this rank's verdict records here")
    ap.add_argument("--require-pass", action="store_true",
                    help="with --check-slots: exit status 3 if any ended episode failed a check (a sweep can gate a CI job)")
    ap.add_argument("--search", type=int, default=None, metavar="SLOTS",
                    help="arm the limit search of the scenario table (a scenario's \"search\"): a per-env level that scales the row's pushes / "
                         "commands and moves when an episode ends; keeps the last SLOTS (1..64) trials of every env; its summary goes into the "
                         "report as \"episodes.search\" (also under --graph / --pipelined)")
    ap.add_argument("--search-out", default=None, metavar="PATH.npz", help="with --search: write this rank's search records and trials here")
    ap.add_argument("--until-searched", action="store_true", help="with --search: stop once every env has spent its trials (or after --steps)")
    ap.add_argument("--search-poll", type=int, default=50, metavar="STEPS",
                    help="with --until-searched: ask the device every STEPS control steps (one word; between graph replays under --graph)")
    ap.add_argument("--curves", action="store_true", default=None,
                    help="keep the response curves of the scenario table on the device (a scenario's \"curves\"): per-scenario ensemble time "
                         "series split by outcome; their summary goes into the report as \"episodes.curves\" (also under --graph / --pipelined)")
    ap.add_argument("--curves-out", default=None, metavar="PATH.npz",
                    help="with --curves: write the curves here (under torchrun: the whole fleet's, all-reduced, from rank 0)")
    ap.add_argument("--curves-by", default=None, choices=["policy"], metavar="KEY",
                    help="with --curves and several --policy files: split the curves by the policy that drove each ended episode (under "
                         "--policy-rotate too); the report gains \"episodes.curves.by_policy\" and --curves-out writes the grouped file")
    ap.add_argument("--backend", default="nccl")
    args = ap.parse_args(argv)

    # ---- session file: the GUI's config dict + the user's key / push input over time
    sess = {}
    if args.config:
        import yaml
        with open(args.config) as f:
            sess = yaml.safe_load(f) or {}
        if not isinstance(sess, dict):
            ap.error("--config: the YAML document must be a mapping")
        unknown = set(sess) - {"env", "engine", "random", "observation", "hardware", "policy", "steps", "commands", "pushes", "report",
                               "trace_env", "percentiles", "hfield_fixup", "spawn", "ledger", "scenarios", "scenario_mode", "fall", "failure_traces", "check_slots", "curves", "curves_by", "search"}
        if unknown:
            ap.error(f"--config: unknown top-level keys {sorted(unknown)}")
    s_env, s_eng, s_pol = sess.get("env", {}) or {}, sess.get("engine", {}) or {}, sess.get("policy", {}) or {}

    opt = session_opt(sess)

    def pick(flag, file_value, default):
        return flag if flag is not None else (file_value if file_value is not None else default)
    args.env = pick(args.env, s_env.get("id"), "flamingo_light_v1")
    args.terrain = pick(args.terrain, s_env.get("terrain"), "flat")
    args.max_duration = float(pick(args.max_duration, s_env.get("max_duration"), 120.0))
    args.position_command = bool(args.position_command or s_env.get("position_command", False))
    args.num_envs = int(pick(args.num_envs, s_eng.get("num_envs"), 1024))
    args.seed = int(pick(args.seed, s_eng.get("seed"), 1234))
    args.steps = int(pick(args.steps, sess.get("steps"), 500))
    kind = s_pol.get("kind")
    unknown = set(s_pol) - {"kind", "onnx_file", "onnx_files", "assign", "rotate", "names", "use_lstm", "h_in_dim", "c_in_dim"}
    if unknown:
        ap.error(f"--config: unknown keys policy.{sorted(unknown)}")
    # one policy, or several ONNX files: a policy table (policy.PolicyTable)
    policy_files = list(args.policy) if args.policy is not None else list(s_pol.get("onnx_files") or [])
    if len(policy_files) == 1:
        args.policy, policy_files = policy_files[0], []
    elif policy_files:
        args.policy = None
    args.policy = pick(args.policy, s_pol.get("onnx_file") if kind == "onnx" else kind, "sinusoid")
    policy_assign = pick(args.policy_assign, s_pol.get("assign"), "interleave")
    policy_names = args.policy_names if args.policy_names is not None else s_pol.get("names")
    policy_rotate = pick(args.policy_rotate, s_pol.get("rotate"), None)
    if policy_files:
        if policy_rotate is not None and (isinstance(policy_rotate, bool) or not isinstance(policy_rotate, int) or policy_rotate < 1):
            ap.error(f"--policy-rotate / policy.rotate: {policy_rotate!r} is not an integer >= 1")
        if args.lstm or s_pol.get("use_lstm", False):
            ap.error("--policy with several files: a policy table takes MLP actors only (no --lstm)")
        if any(p in ("sinusoid", "random-mlp") for p in policy_files):
            ap.error("--policy with several values: ONNX files only (sinusoid / random-mlp stand alone)")
        if policy_assign not in ("interleave", "cross"):
            ap.error("policy.assign: interleave or cross")
        if policy_names is not None and len(policy_names) != len(policy_files):
            ap.error("--policy-names: one name per --policy file")
    elif args.policy_assign is not None or args.policy_names is not None:
        ap.error("--policy-assign / --policy-names need several --policy files")
    elif policy_rotate is not None:
        ap.error("--policy-rotate needs several --policy files")
    args.lstm = bool(args.lstm or s_pol.get("use_lstm", False))
    if s_pol.get("h_in_dim") is not None:
        args.hidden_dim = int(s_pol["h_in_dim"])
    args.report = pick(args.report, sess.get("report"), "")
    args.trace_env = int(pick(args.trace_env, sess.get("trace_env"), -1))
    args.percentiles = bool(args.percentiles or sess.get("percentiles", False))
    args.hfield_fixup = bool(args.hfield_fixup or sess.get("hfield_fixup", False) or s_eng.get("hfield_fixup", False))
    # spawn table: the session's dict (top level or engine.spawn), overridden key by key by the flags; the table is built from the
    # TOTAL env count and the seed, so every rank sets the same one
    spawn = dict(sess.get("spawn") or s_eng.get("spawn") or {})
    if args.spawn is not None:
        spawn["pattern"] = args.spawn
    for key, val in (("count", args.spawn_count), ("extent", args.spawn_extent), ("clearance", args.spawn_clearance)):
        if val is not None:
            spawn[key] = val
    if args.spawn_per_episode:
        spawn["per_episode"] = True
    if spawn and "pattern" not in spawn and spawn.get("poses") is None:
        ap.error("--spawn-* / spawn: needs a pattern (--spawn grid|uniform) or poses")
    if spawn and spawn.get("pattern") in ("grid", "uniform"):
        spawn.setdefault("count", args.num_envs)
    # command time series: rows [t, c0, c1, ...]; --command is the row [0, c...]
    commands = [[float(x) for x in row] for row in (sess.get("commands") or [])]
    if args.command is not None:
        commands = [[0.0] + list(args.command)]
    if not commands:
        commands = [[0.0, 0.5, 0.0, 0.0, 0.0]]
    commands.sort(key=lambda r: r[0])
    pushes = [[float(x) for x in row] for row in (sess.get("pushes") or [])]
    if args.push_at >= 0:
        pushes.append([float(args.push_at), float(args.push_at + 1)] + [float(x) for x in args.push])
    for row in pushes:
        if len(row) != 5 or row[1] <= row[0]:
            ap.error("pushes: rows are [t0, t1, vx, vy, vz] with t1 > t0")
    if (args.checkpoint is None) != (args.checkpoint_at is None):
        ap.error("--checkpoint and --checkpoint-at go together")
    if args.fork_row is not None and not args.resume:
        ap.error("--fork-row needs --resume")
    if (args.checkpoint or args.resume) and (args.graph or args.pipelined):
        ap.error("--checkpoint / --resume run the eager loop (no --graph / --pipelined)")
    if args.history is not None and (args.history[0] < 1 or args.history[1] < 1):
        ap.error("--history SLOTS EVERY: both at least 1")
    args.ledger = int(opt(args.ledger, "ledger", 0))
    if not 0 <= args.ledger <= 4096:
        ap.error("--ledger SLOTS: 0..4096")
    if args.ledger_out and args.ledger < 1:
        ap.error("--ledger-out needs --ledger SLOTS")
    scenarios = opt(args.scenarios, "scenarios", None)
    scenario_mode = pick(args.scenario_mode, sess.get("scenario_mode", s_eng.get("scenario_mode")), "env")
    if scenario_mode not in ("env", "cycle"):
        ap.error("scenario_mode: env or cycle")
    args.check_slots = int(opt(args.check_slots, "check_slots", 0))
    if not 0 <= args.check_slots <= 64:
        ap.error("--check-slots SLOTS: 1..64")
    if (args.verdicts_out or args.require_pass) and args.check_slots < 1:
        ap.error("--verdicts-out / --require-pass need --check-slots SLOTS")
    if args.check_slots and scenarios is None:
        ap.error("--check-slots needs --scenarios: checks are rows of a scenario table")
    args.search = int(opt(args.search, "search", 0))
    if not 0 <= args.search <= 64:
        ap.error("--search SLOTS: 1..64")
    if (args.search_out or args.until_searched) and args.search < 1:
        ap.error("--search-out / --until-searched need --search SLOTS")
    if args.search and scenarios is None:
        ap.error("--search needs --scenarios: a search item is a row of a scenario table")
    if args.search and scenario_mode != "env":
        ap.error("--search needs scenario mode env: the search keeps one record per env")
    if args.search_poll < 1:
        ap.error("--search-poll STEPS: at least 1")
    args.curves = bool(opt(args.curves, "curves", False))
    if args.curves_out and not args.curves:
        ap.error("--curves-out needs --curves")
    if args.curves and scenarios is None:
        ap.error("--curves needs --scenarios: curves are rows of a scenario table")
    args.curves_by = pick(args.curves_by, sess.get("curves_by"), None)
    if args.curves_by is not None:
        if args.curves_by != "policy":
            ap.error(f"--curves-by / curves_by: {args.curves_by!r}: policy")
        if not args.curves:
            ap.error("--curves-by policy needs --curves: it splits the response curves")
        if not policy_files:
            ap.error("--curves-by policy needs a policy table: several --policy files (policy.onnx_files)")
    # fall rule: the session's dict (top level or engine.fall), overridden key by key by the flags
    fall = dict(sess.get("fall") or s_eng.get("fall") or {})
    for key, val in (("tilt", args.fall_tilt), ("height", args.fall_height), ("grace", args.fall_grace)):
        if val is not None:
            fall[key] = val
    if args.fall_bodies is not None:
        fall["bodies"] = [b for b in args.fall_bodies.split(",") if b]
    if fall:
        from .fall import FallRule
        try:
            FallRule.build(fall)
        except ValueError as e:
            ap.error(f"--fall-* / fall: {e}")
    # failure traces: the session's value (top level or engine.failure_traces: [frames, keep] or a mapping), overridden by the flags
    ftrace = opt(None, "failure_traces", None)
    if ftrace is not None and not isinstance(ftrace, dict):
        ftrace = {"frames": list(ftrace)[0], "keep": list(ftrace)[1]} if len(list(ftrace)) == 2 else ap.error("failure_traces: [FRAMES, KEEP] or a mapping")
    ftrace = dict(ftrace or {})
    if args.failure_traces is not None:
        ftrace["frames"], ftrace["keep"] = args.failure_traces
    if args.failure_traces_on is not None:
        ftrace["on"] = list(args.failure_traces_on)
    if (args.failure_traces_on is not None or args.failure_traces_out) and "frames" not in ftrace:
        ap.error("--failure-traces-on / --failure-traces-out need --failure-traces FRAMES KEEP")
    if ftrace:
        from .ftrace import resolve as ftrace_resolve
        try:
            ftrace_resolve(ftrace)
        except ValueError as e:
            ap.error(f"--failure-traces / failure_traces: {e}")
    if args.history is not None and args.graph:
        ap.error("--history cannot be combined with --graph: a replayed graph would repeat the captured step's parity")

    import torch
    from .batched_env import BatchedEnv
    from .config import make_config
    from .distributed import init_from_env, shard_range
    from .policy import build_policy, write_random_mlp
    from .reporter import FleetReporter
    from .runner import Runner, SinusoidPolicy
    from .scenario import FAULT_KINDS

    rank, world = init_from_env(args.backend)
    if world > 1 and (args.checkpoint or args.resume):
        ap.error("--checkpoint / --resume: one process (a snapshot file holds one rank's envs)")
    lo, hi = shard_range(args.num_envs, rank, world)
    dev = int(os.environ.get("LOCAL_RANK", "0"))
    cfg = make_config(args.env, terrain=args.terrain, max_duration=args.max_duration, position_command=args.position_command,
                      num_envs=hi - lo, seed=args.seed, device=dev)
    for section in ("random", "observation", "hardware"):          # the widgets' values (ui/main_window.py:750-787)
        for k, v in (sess.get(section) or {}).items():
            if k not in cfg[section]:
                ap.error(f"--config: unknown key {section}.{k}")
            if isinstance(cfg[section][k], dict) and isinstance(v, dict):
                cfg[section][k].update(v)
            else:
                cfg[section][k] = v
    env = BatchedEnv(cfg, num_envs=hi - lo, device=dev, seed=args.seed, auto_reset=True, env_id0=lo, hfield_fixup=args.hfield_fixup,
                     spawn=spawn or None, history=tuple(args.history) if args.history else None, ledger=args.ledger, scenarios=scenarios, scenario_mode=scenario_mode, fall=fall or None, failure_traces=ftrace or False, check_slots=args.check_slots or None, curves=args.curves or None, search=args.search or None, **({"ranges": args.ranges, "deferred_join": True} if args.pipelined else {}))
    if args.check_slots and env.check_slots < 1:
        ap.error("--check-slots: the scenario table holds no checks")
    if args.search and env.search_slots < 1:
        ap.error("--search: the scenario table holds no search item")
    if args.curves and not env.curves_armed:
        ap.error("--curves: the scenario table holds no curves")
    if policy_files:
        n_scn = len(env.scenario_table) if env.scenario_table is not None else 0
        if policy_assign == "cross" and n_scn < 1:
            ap.error("--policy-assign cross needs --scenarios")
        try:
            policy = build_policy({"policy": {"use_lstm": False, "onnx_files": policy_files, "assign": policy_assign, "rotate": policy_rotate}}, num_envs=env.num_envs,
                                  device=env.device, env_id0=lo, scenarios=n_scn, ranges=env.range_list, names=policy_names)
        except ValueError as e:
            ap.error(str(e))
    elif args.policy == "sinusoid":
        policy = SinusoidPolicy(env.num_envs, env.action_dim, env.device, env_id0=lo, seed=args.seed)
    else:
        path = args.policy
        if args.policy == "random-mlp":
            path = os.path.join(tempfile.mkdtemp(prefix="cosim_policy_"), "actor.onnx")
            write_random_mlp(path, env.state_dim, env.action_dim, seed=args.seed)
        pc = {"policy": {"use_lstm": bool(args.lstm), "h_in_dim": args.hidden_dim, "c_in_dim": args.hidden_dim}}
        policy = build_policy(pc, path, num_envs=env.num_envs, device=env.device)
    if args.curves_by == "policy":                                   # before the run, and so before the capture under --graph
        env.set_curve_groups(policy)
    if args.graph and not getattr(policy, "graph_safe", False):
        ap.error("--graph needs an ONNX policy (random-mlp or a file): the sinusoid drive keeps its clock on the host, a captured "
                 "graph would replay one frozen action")
    if args.graph and (pushes or len(commands) > 1 or args.trace_env >= 0):
        ap.error("--graph replays one captured control step: pushes, command changes and --trace-env need the eager loop")
    if args.pipelined and (not (hasattr(policy, "get_action_into") or hasattr(policy, "get_action_range")) or args.graph or args.trace_env >= 0):
        ap.error("--pipelined needs an ONNX MLP policy (random-mlp or a file) and excludes --graph / --trace-env")
    rep = FleetReporter(env, trace_env=args.trace_env if args.trace_env >= 0 else None, percentiles=args.percentiles)
    run = Runner(env, policy, reporter=rep)
    for i, v in enumerate(commands[0][1:1 + env.command_dim]):
        run.update_command(i, v)
    if args.until_searched:
        if world > 1:
            ap.error("--until-searched: one process (the ranks of a torchrun would stop at different steps)")
        run.stop_when(lambda: env.search_remaining() == 0, args.search_poll)

    def before_step(k):
        """What the reference's UI thread does between two loop iterations: key-driven command changes and the push button."""
        for row in commands:
            if int(row[0]) == k:
                for i, v in enumerate(row[1:1 + env.command_dim]):
                    run.update_command(i, v)                       # tester.py:41-46
        held = [row for row in pushes if row[0] <= k < row[1]]
        if held:
            run.activate_push_event(np.asarray(held[-1][2:5], dtype=np.float32))   # tester.py:48-50; applied while held (:80-81)
        else:
            run.deactivate_push_event()

    # episodes ended are counted on the device (engine meta word 11) and read once after the run: a per-step `.item()` on the done
    # flags would drain the GPU queue at every control step
    on_step = None
    resume = None
    used = {}                                                      # what the report records about snapshots
    if args.history:
        used["history"] = list(args.history)
    if args.resume:
        from .snapshot import Snapshot
        resume = Snapshot.load(args.resume, device=env.device)
        used.update({"resume": args.resume, "resume_step": resume.steps})
        if args.fork_row is not None:
            used["fork_row"] = args.fork_row
    if args.checkpoint:
        def on_step(k, state, terminated, truncated, info):
            if k + 1 == args.checkpoint_at:                        # after `checkpoint_at` control steps of the session's clock
                env.snapshot(policy if hasattr(policy, "state") else None).save(args.checkpoint)
                used.update({"checkpoint": args.checkpoint, "checkpoint_at": args.checkpoint_at})
    episodes0 = None
    torch.cuda.synchronize(env.device)
    episodes0 = env.solver_stats()["episodes_ended"]
    t0 = time.perf_counter()
    if args.pipelined:
        if pushes or len(commands) > 1:
            ap.error("--pipelined runs one command and no push schedule (use Runner.test_pipelined with update_command for more)")
        n = run.test_pipelined(args.steps)
    else:
        n = run.test_graphed(args.steps) if args.graph else run.test(max_steps=args.steps, on_step=on_step, before_step=before_step,
                                                                           resume=resume, fork_row=args.fork_row)
    torch.cuda.synchronize(env.device)
    dt = time.perf_counter() - t0
    rep.episodes_ended = env.solver_stats()["episodes_ended"] - episodes0
    if args.ledger_out:                                             # records stay per rank: one file each
        env.ledger().save(rank_path(args.ledger_out, rank, world))
    traces = env.failure_traces() if ftrace else None                # traces stay per rank, like the ledger's records
    if args.failure_traces_out:
        traces.save(rank_path(args.failure_traces_out, rank, world))
    verdicts = env.verdicts() if args.check_slots else None          # verdict records stay per rank too
    if args.verdicts_out:
        verdicts.save(rank_path(args.verdicts_out, rank, world))
    search = env.search() if args.search else None                   # search records and thresholds stay per rank too
    if args.search_out:
        search.save(rank_path(args.search_out, rank, world))
    if args.curves_out:                                              # the fleet's curves: the cells are all-reduced, every rank holds them
        fleet = rep.fleet_curves()
        if rank == 0:
            fleet.save(args.curves_out)
    if args.checkpoint and "checkpoint" not in used:
        print(f"warning: --checkpoint-at {args.checkpoint_at} was not reached, no snapshot written", file=sys.stderr)
    out = rep.save(args.report, extra={"snapshot": used} if used else None) if (args.report and rank == 0) else rep.summary()
    if rank == 0:
        print(json.dumps({"env": args.env, "terrain": args.terrain, "envs_total": args.num_envs, "ranks": world, "control_steps": n,
                          "env_steps_per_s_this_rank": env.num_envs * n / dt, "episodes_ended": out["episodes_ended"],
                          "metrics": {k: round(v["mean"], 5) for k, v in out["metrics"].items()},
                          **({"snapshot": used} if used else {}),
                          **({"policy_table": f"files={len(policy_files)} assign={policy_assign} rotate={policy_rotate}"} if policy_files and policy_rotate else {}),
                          **({"episodes": {k: out["episodes"][k] for k in ("episodes", "terminated", "truncated", "non_finite", "lost", "length") +
                                           (("fell", "fell_tilt", "fell_height", "fell_contact") if env.fall_rule is not None else ())}}
                             if "terminated" in out.get("episodes", {}) else {}),
                          **({"checks": {k: v for k, v in out["episodes"]["checks"].get("fleet", out["episodes"]["checks"]).items()
                                         if k not in ("checks", "by_scenario")}} if verdicts is not None else {}),
                          **({"curves": {k: ({name: {q: v[q] for q in ("episodes", "episodes_truncated", "episodes_terminated")} for name, v in x.items()}
                                             if k == "by_policy" else x) for k, x in out["episodes"]["curves"].items()}} if args.curves else {}),
                          **({"search": "{done}/{envs}".format(**out["episodes"]["search"].get("fleet", out["episodes"]["search"]))} if search is not None else {}),
                          **({"failure_traces": traces.summary()} if traces is not None else {}),
                          **({"by_scenario": {k: {q: v[q] for q in ("episodes", "terminated")} for k, v in out["episodes"]["by_scenario"].items()}}
                             if "by_scenario" in out.get("episodes", {}) else {}),
                          **({"by_policy": {k: {q: v.get("fleet", v)[q] for q in ("episodes", "terminated_share")} for k, v in out["episodes"]["by_policy"].items()}}
                             if "by_policy" in out.get("episodes", {}) else {}),
                          **({"param_windows": sum(len(w) for w in env.scenario_table.param_windows)}   # as listed in the table
                             if env.scenario_table is not None and env.scenario_table.has_params else {}),
                          **({kind.param: sum(len(f) for f in getattr(env.scenario_table, kind.key))     # expanded items, as the engine counts them
                              for kind in FAULT_KINDS if env.scenario_table is not None and any(getattr(env.scenario_table, kind.rows))}),
                          **({"latency": env.scenario_table.n_latency_items}                             # likewise
                             if env.scenario_table is not None and env.scenario_table.has_latency else {}),
                          **({"percentiles": {k: {q: round(x, 5) for q, x in v.items()} for k, v in out["percentiles"].items()}}
                             if "percentiles" in out else {})}))
    env.close()
    if args.require_pass:                                            # every rank judges the fleet's count (all-reduced in the report)
        c = out["episodes"]["checks"]
        if c.get("fleet", c)["episodes_failed"] > 0:
            return 3
    return 0


if __name__ == "__main__":
    sys.exit(main())
