"""Parameter windows of a scenario table on the device (cosim_scenario_params_set, csrc/cosim_scnparams.hip, and their BatchedEnv /
CLI surface) against the numpy twin (cosim_amd/scenario.py reference_params) and against a host-driven loop: an env whose table has
no windows and that is given, through engine.set_param before every step, the kp / kd / geom_friction / dof_frictionloss rows the
twin works out from the meta words read back from the device.

Every comparison is EXACT: float32 bits for floats (uint32 views), ints as ints.  Fleets are at most 24 envs, runs at most 60 steps;
max_duration = 0.5 puts the time limit in episode step 25; actions come from a fixed table.  Each test asserts that what it is about
-- an episode that ended, a window that opened and closed, a redone step -- happened.

Figures from the run this file was written against are in DESIGN.md section 4.18."""
import json

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_CACHE = {}
CD = 4
BASE = np.array([0.5, 0.0, 0.0, 0.0], dtype=np.float32)
N, K, RESET_AT = 24, 60, 30
RESET_MASK = (np.arange(N) % 4 == 1)
FIELDS = ("kp", "kd", "geom_friction", "dof_frictionloss")
WIDTH = {"kp": "action_dim", "kd": "action_dim", "geom_friction": "ngeom", "dof_frictionloss": "nv"}

# Three scenarios for flamingo_light_v1; an episode's pre-step clock runs 0 .. 24:
#   0  gains sag over [5, 12) ("*"), one actuator set and then scaled by 0 by overlapping windows (the last LISTED wins), and the floor
#      turns slippery across the time limit, [20, 30): held in 20 .. 24, gone after the auto-reset; a command and a push beside them
#   1  a joint binds over [3, 6); actuator 0 goes limp (kp = kd = 0) over [10, 18)
#   2  no window: these envs must run as if the feature did not exist
TABLE = [
    {"commands": [[0, 0.3, 0.1, 0.0, 0.0]], "pushes": [[6, 8, 0.3, 0.0, 0.0]],
     "params": [[5, 12, "kp", "*", "scale", 0.5], [8, 10, "kp", 1, "set", 7.0], [9, 11, "kp", 1, "scale", 0.0],
                [20, 30, "geom_friction", "*", "scale", 0.2]]},
    {"params": [[3, 6, "dof_frictionloss", "*", "set", 0.5], [10, 18, "kp", 0, "scale", 0.0], [10, 18, "kd", 0, "scale", 0.0]]},
    {"commands": [[4, 0.6, 0.0, 0.0, 0.0]]},
]


def _strip(scn):
    return [{k: v for k, v in s.items() if k != "params"} for s in scn]


def _variant(scn):
    """The same sizes with other values and times: what an in-place rewrite uploads."""
    out = [dict(s) for s in scn]
    out[1] = dict(out[1], params=[[2, 9, "dof_frictionloss", "*", "set", 0.25], [1, 20, "kp", 0, "scale", 0.5], [12, 14, "kd", 0, "scale", 2.0]])
    return out


def _model(robot, terrain="flat", **kw):
    from cosim_amd.compile import compile_model
    from cosim_amd.config import make_config
    key = (robot, terrain, json.dumps(kw, sort_keys=True))
    if key not in _CACHE:
        cfg = make_config(robot, terrain=terrain, **kw)
        if kw.get("position_command"):
            cfg["observation"]["command_dim"] = 2
        _CACHE[key] = (cfg, compile_model(cfg))
    return _CACHE[key]


def _light():
    return _model("flamingo_light_v1", "flat", max_duration=0.5)


def _env(cfg, cm, n, base=BASE, seed=3, **kw):
    from cosim_amd.batched_env import BatchedEnv
    kw.setdefault("auto_reset", True)
    env = BatchedEnv(cfg, num_envs=n, compiled=cm, seed=seed, **kw)
    env.receive_user_command(np.asarray(base, dtype=np.float32))
    return env


def _actions(n, steps, nu, seed=21):
    return np.random.default_rng(seed).uniform(-0.6, 0.6, size=(steps, n, nu)).astype(np.float32)


def _meta(env):
    t = env.torch
    buf = t.zeros((env.num_envs, 16), dtype=t.float32, device=env.device)
    env.engine.get("meta", buf.data_ptr(), env._stream())
    t.cuda.synchronize(env.device)
    return buf.view(t.int32).cpu().numpy().copy()


def _u(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


class _Run:
    """One run, recorded step by step.  ``device``: the env carries the windows and the host only checks ``effective_params()``
    against the twin; otherwise the host drives: twin -> engine.set_param of the four fields -> step."""

    def __init__(self, env, scenarios, mode, device=True, check=True):
        from cosim_amd.scenario import ScenarioTable
        self.env, self.mode, self.device, self.check = env, mode, device, check
        self.table = ScenarioTable(scenarios, env.command_dim, names=env.param_names())
        self.lay = env.param_layout()
        self.gid = env.env_id0 + np.arange(env.num_envs)
        self.base = env.effective_params() if not device else None  # no windows on a host-driven env: these are its base records
        self.state, self.te, self.tr, self.info, self.eff, self.clock, self.ep = [], [], [], [], [], [], []
        self.last = None

    def _base(self):
        if self.base is None:                                       # the base records: the parameter part of a snapshot row
            self.base = self.env.snapshot().rows.cpu().numpy()[:, self.env.engine.query("state_stride"):].copy()
        return self.base

    def twin(self, meta, reset=False):
        from cosim_amd.scenario import reference_params
        t = np.zeros(len(meta), dtype=np.int64) if reset else meta[:, 0]
        return reference_params(self.table, self.mode, self.gid, t, meta[:, 11], self._base(), self.lay)

    def _set(self, eff):
        q = self.env.engine.query
        for f in FIELDS:
            self.env.engine.set_param(f, eff[:, self.lay[f]:self.lay[f] + q(WIDTH[f])])

    def reset(self, mask):
        env, t = self.env, self.env.torch
        m = np.asarray(mask).astype(bool)
        want = self.twin(_meta(env), reset=True)
        before = env.effective_params() if self.device else self.last
        if not self.device:
            self._set(np.where(m[:, None], want, before))
        env.reset(mask=mask)
        t.cuda.synchronize(env.device)
        if self.device and self.check:                              # the masked envs' records restart at t = 0, the others stay
            got = env.effective_params()
            np.testing.assert_array_equal(_u(got[m]), _u(want[m]), err_msg="effective_params after a masked reset")
            np.testing.assert_array_equal(_u(got[~m]), _u(before[~m]))
        self.reset_state = env.state.cpu().numpy()[m].copy()

    def steps(self, actions, k0, k1):
        env, t = self.env, self.env.torch
        for k in range(k0, k1):
            meta = _meta(env)
            eff = self.twin(meta)
            self.clock.append(meta[:, 0].copy()); self.ep.append(meta[:, 11].copy()); self.eff.append(eff)
            if not self.device:
                self._set(eff)
                self.last = eff
            env.step(t.tensor(actions[k], device=env.device))
            env.join()
            t.cuda.synchronize(env.device)
            self.record()
            if self.device and self.check:
                np.testing.assert_array_equal(_u(env.effective_params()), _u(eff), err_msg=f"effective_params, step {k}")

    def record(self):
        env = self.env
        self.state.append(env.state.cpu().numpy().copy()); self.info.append(env.info_buf.cpu().numpy().copy())
        self.te.append(env.terminated.cpu().numpy().copy()); self.tr.append(env.truncated.cpu().numpy().copy())

    def final(self):
        """The complete STATE records after the run (the parameter rows are left out: a host-driven run has mutated its base)."""
        self.rows = self.env.snapshot().rows.cpu().numpy()[:, :self.env.engine.query("state_stride")].copy()
        return self

    def ended(self):
        return int((np.stack(self.te) | np.stack(self.tr)).astype(bool).sum())


def _same(a, b, what="", steps=None, envs=slice(None)):
    """State, flags and info of every step, and the final state records: bit-identical."""
    assert len(a.state) == len(b.state) > 0
    for k in range(len(a.state) if steps is None else steps):
        for name in ("state", "info"):
            x, y = _u(getattr(a, name)[k][envs]), _u(getattr(b, name)[k][envs])
            assert np.array_equal(x, y), f"{what}{name} differs in step {k}: envs {np.nonzero((x != y).any(axis=1))[0][:8]}"
        assert np.array_equal(a.te[k][envs], b.te[k][envs]) and np.array_equal(a.tr[k][envs], b.tr[k][envs]), f"{what}flags differ in step {k}"
    if steps is None and getattr(a, "rows", None) is not None and getattr(b, "rows", None) is not None:
        x, y = _u(a.rows[envs]), _u(b.rows[envs])
        assert np.array_equal(x, y), f"{what}final state records differ: envs {np.nonzero((x != y).any(axis=1))[0][:8]}"


def _reference(mode):
    """Test 1's device run, once per mode: flamingo_light_v1 flat, 24 envs, the three scenarios, 60 steps with a masked host reset
    before step 30, a ledger of 4 slots and failure traces alongside (they change no step output).  Shared, never modified."""
    key = ("reference", mode)
    if key not in _CACHE:
        cfg, cm = _light()
        env = _env(cfg, cm, N, scenarios=TABLE, scenario_mode=mode, ledger=4, failure_traces=(8, 2))
        assert env.engine.query("scenario_rows") == 3 and env.engine.query("scenario_param_items") == env.scenario_table.n_param_items > 0
        assert env.engine.query("param_stride") == 96
        actions = _actions(N, K, env.action_dim)
        env.reset()
        run = _Run(env, TABLE, mode)
        run.first_state = env.state.cpu().numpy().copy()
        run.steps(actions, 0, RESET_AT)
        run.reset(RESET_MASK)
        run.steps(actions, RESET_AT, K)
        run.final()
        run.ledger = env.ledger(include_open=True)
        run.traces = env.failure_traces(include_open=True)
        run.actions = actions
        run.base_rows = run._base().copy()
        env.close()
        run.env = None
        _CACHE[key] = run
    return _CACHE[key]


def _host_driven(mode):
    key = ("host", mode)
    if key not in _CACHE:
        a = _reference(mode)
        cfg, cm = _light()
        env = _env(cfg, cm, N, scenarios=_strip(TABLE), scenario_mode=mode, ledger=4, failure_traces=(8, 2))
        assert env.engine.query("scenario_param_items") == 0
        env.reset()
        b = _Run(env, TABLE, mode, device=False)
        b.first_state = env.state.cpu().numpy().copy()
        b.steps(a.actions, 0, RESET_AT)
        b.reset(RESET_MASK)
        b.steps(a.actions, RESET_AT, K)
        b.final()
        b.ledger = env.ledger(include_open=True)
        b.traces = env.failure_traces(include_open=True)
        env.close()
        b.env = None
        _CACHE[key] = b
    return _CACHE[key]


# ------------------------------------------------------------------------------------------------------------ 1: effective records = twin
@pytest.mark.parametrize("mode", ["env", "cycle"])
def test_effective_params_equal_the_twin(mode):
    a = _reference(mode)                                            # (asserts after every step and after the masked reset)
    eff, clock, ep = np.stack(a.eff), np.stack(a.clock), np.stack(a.ep)
    lay, base = a.lay, a.base_rows
    gid = np.arange(N)
    done = (np.stack(a.te) | np.stack(a.tr)).astype(bool)
    assert a.ended() >= N and done[24].all() and (clock[25][~RESET_MASK] == 0).all()
    for k in range(K):                                              # the clock: k mod 25 where the host did not reset, (k - 30) mod 25 after
        assert (clock[k][~RESET_MASK] == k % 25).all() and (clock[k][RESET_MASK] == (k % 25 if k < RESET_AT else (k - RESET_AT) % 25)).all()
    # windows opened and closed: scenario 0's kp[1] through base -> 0.5 base -> 7 -> 0 -> 0.5 base -> base in its first episode
    s0 = np.nonzero(gid % 3 == 0)[0]
    kp1 = lay["kp"] + 1
    b = base[s0, kp1]
    for k, want in ((4, b), (5, b * np.float32(0.5)), (8, np.full_like(b, 7.0)), (9, np.zeros_like(b)), (10, np.zeros_like(b)),
                    (11, b * np.float32(0.5)), (12, b)):
        assert np.array_equal(_u(eff[k][s0, kp1]), _u(want)), k
    g = slice(lay["geom_friction"], lay["geom_friction"] + 9)
    assert (eff[19][s0, g] == base[s0, g]).all() and (eff[20][s0, g] == base[s0, g] * np.float32(0.2)).all() and (eff[24][s0, g] != base[s0, g]).all()
    untouched = np.setdiff1d(np.arange(96), np.r_[lay["dof_frictionloss"]:lay["kd"] + 4])
    assert all(np.array_equal(_u(e[:, untouched]), _u(base[:, untouched])) for e in eff)   # masses, inverse weights, padding: base bits
    if mode == "env":
        s2 = gid % 3 == 2
        assert all(np.array_equal(_u(e[s2]), _u(base[s2])) for e in eff)                  # scenario 2 has no window
        assert (eff[25][s0, g] == base[s0, g]).all()                                       # [20, 30) ended with the episode
    else:   # one scenario per episode: after the first auto-reset env g runs row (g + 1) mod 3
        assert (ep[25] == 1).all() and (ep[0] == 0).all()
        was2 = np.nonzero(gid % 3 == 2)[0]                          # now scenario 0: the gains sag again at t = 5, step 30
        keep = was2[~RESET_MASK[was2]]
        assert len(keep) and (eff[30][keep, kp1] == base[keep, kp1] * np.float32(0.5)).all() and (eff[29][keep, kp1] == base[keep, kp1]).all()


# ------------------------------------------------------------------------------------------------------------ 2: device = host-driven
@pytest.mark.parametrize("mode", ["env", "cycle"])
def test_device_windows_equal_host_driven_set_param(mode):
    a, b = _reference(mode), _host_driven(mode)
    np.testing.assert_array_equal(_u(a.first_state), _u(b.first_state))
    _same(a, b, what="host-driven: ")
    np.testing.assert_array_equal(_u(a.reset_state), _u(b.reset_state))
    assert all(np.array_equal(_u(x), _u(y)) for x, y in zip(a.eff, b.eff)) and a.ended() >= N
    if mode == "cycle":
        return
    # a fleet that has no windows at all: the same bits until the first window opens (t = 3), for scenario 2 throughout; and the
    # limp-joint window of scenario 1 ([10, 18)) changes the trajectory after it opens, not before (its [3, 6) window did already:
    # compare against a fleet that has only that one)
    cfg, cm = _light()
    plain = _env(cfg, cm, N, scenarios=_strip(TABLE), scenario_mode=mode)
    only36 = [dict(s) for s in _strip(TABLE)]
    only36[1]["params"] = TABLE[1]["params"][:1]
    nolimp = _env(cfg, cm, N, scenarios=only36, scenario_mode=mode)
    runs = []
    for env in (plain, nolimp):
        env.reset()
        r = _Run(env, _strip(TABLE), mode, check=False)
        t = env.torch
        for k in range(25):
            env.step(t.tensor(a.actions[k], device=env.device))
            t.cuda.synchronize(env.device)
            r.record()
        env.close()
        runs.append(r)
    p, q = runs
    p.state, p.info, p.te, p.tr = p.state + a.state[25:], p.info + a.info[25:], p.te + a.te[25:], p.tr + a.tr[25:]   # (lengths for _same)
    q.state, q.info, q.te, q.tr = q.state + a.state[25:], q.info + a.info[25:], q.te + a.te[25:], q.tr + a.tr[25:]
    _same(a, p, what="no windows at all, steps 0 .. 2: ", steps=3)
    _same(a, p, what="scenario 2: ", steps=25, envs=np.arange(N) % 3 == 2)
    s1 = np.arange(N) % 3 == 1
    _same(a, q, what="before the limp window: ", steps=10, envs=s1)
    differs = [k for k in range(25) if not np.array_equal(_u(a.state[k][s1]), _u(q.state[k][s1]))]
    assert differs and differs[0] in (10, 11) and (_u(a.state[3][s1]) != _u(p.state[3][s1])).any()
    tq = np.stack(a.info)[:, :, 4]                                  # info[4 + u]: actuator u's torque; limp: exactly zero
    assert (tq[10:18][:, s1] == 0.0).all() and (tq[9][s1] != 0.0).all() and (tq[18][s1] != 0.0).all()


# ------------------------------------------------------------------------------------------------------------ 3: arrangements
def test_every_arrangement_gives_the_same_bits():
    """The cycle run of test 1 again: one launch (the reference), two uneven ranges through step_range chains, 4 ranges of 6 envs
    under a deferred join.  No host read between the steps of these runs."""
    import torch
    a = _reference("cycle")
    cfg, cm = _light()

    def drive(env, step):
        run = _Run(env, TABLE, "cycle", check=False)
        env.reset()
        for k in range(K):
            if k == RESET_AT:
                env.join()
                env.reset(mask=RESET_MASK)
            step(k)
            env.join()
            torch.cuda.synchronize(env.device)
            run.record()
        run.final()
        env.close()
        return run

    b = _env(cfg, cm, N, scenarios=TABLE, scenario_mode="cycle", ranges=4, deferred_join=True)
    assert b.engine.query("ranges") == 4 and [c for _, c in b.range_list] == [6] * 4 and b.engine.query("scenario_param_items") > 0
    tb = torch.tensor(a.actions, device=b.device)
    _same(a, drive(b, lambda k: b.step(tb[k])), what="4 ranges, deferred join: ")

    d = _env(cfg, cm, N, scenarios=TABLE, scenario_mode="cycle")
    streams = [torch.cuda.Stream(device=d.device) for _ in range(2)]

    def chains(k):
        torch.cuda.synchronize(d.device)
        for st, (first, count) in zip(streams, ((0, 10), (10, 14))):
            with torch.cuda.stream(st):
                d.step_range(first, count, tb[k])
    _same(a, drive(d, chains), what="step_range chains: ")


def test_captured_step_and_in_place_rewrite_between_replays():
    """A captured step carries the launch; items of the count of the ones that are set are rewritten in place: the graph keeps its
    pointers and picks the new values up.  Against an eager run that rewrites at the same step."""
    import torch
    cfg, cm = _light()
    n, steps, at = 12, 30, 7
    actions = _actions(n, steps, 4, seed=22)
    e = _env(cfg, cm, n, scenarios=TABLE, scenario_mode="env")
    e.reset()
    ref = _Run(e, TABLE, "env")
    ref.steps(actions, 0, at)
    items = e.engine.query("scenario_param_items")
    e.set_scenarios(_variant(TABLE), "env")
    assert e.engine.query("scenario_param_items") == items
    ref.table = type(ref.table)(_variant(TABLE), CD, names=e.param_names())
    ref.steps(actions, at, steps)
    ref.final()
    e.close()
    lay = ref.lay
    s1 = np.arange(n) % 3 == 1
    assert (ref.eff[at][s1, lay["kp"]] == ref.base[s1, lay["kp"]] * np.float32(0.5)).all() and ref.ended() >= n   # the variant's [1, 20) window

    g = _env(cfg, cm, n, scenarios=TABLE, scenario_mode="env")
    g.reset()
    run = _Run(g, TABLE, "env", check=False)
    tb = torch.tensor(actions, device=g.device)
    buf = torch.empty((n, g.action_dim), device=g.device)
    buf.copy_(tb[0])
    side = torch.cuda.Stream(device=g.device)
    torch.cuda.synchronize(g.device)
    side.wait_stream(torch.cuda.current_stream(g.device))
    with torch.cuda.stream(side):
        g.step(buf)
    torch.cuda.current_stream(g.device).wait_stream(side)
    torch.cuda.synchronize(g.device)
    run.record()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g.step(buf)                                                 # recorded, not run: the launch is part of the graph
    for k in range(1, steps):
        if k == at:
            g.set_scenarios(_variant(TABLE), "env")
        buf.copy_(tb[k])
        graph.replay()
        torch.cuda.synchronize(g.device)
        run.record()
    run.final()
    g.close()
    _same(ref, run, what="captured step, table rewritten in place: ")


# ------------------------------------------------------------------------------------------------------------ 4: abandon and redo
def test_abandoned_and_redone_steps_read_the_effective_records():
    """Drop poses with more than 14 contacts (the recipe of test_more_contacts_than_the_fleet_kernel_holds_are_redone_not_dropped):
    the fleet kernel gives such a step up and the 40-slot kernel redoes it -- under a friction window, from the effective records."""
    import torch
    from cosim_amd.compile import compile_model
    from cosim_amd.config import PARITY_RANDOM, make_config
    from cosim_amd.model import get_field
    from oracle.oracle import Oracle
    cfg = make_config("flamingo_light_v1", random=PARITY_RANDOM)
    cm = compile_model(cfg)
    q0 = np.array(get_field(cm.blob, "init_qpos")[:cm.blob.nq])
    o = Oracle(cm)
    rng = np.random.default_rng(3)
    poses = []
    for trial in range(60):
        q = q0.copy()
        quat = rng.normal(size=4)
        q[2] = rng.uniform(0.05, 0.25)
        q[3:7] = quat / np.linalg.norm(quat)
        q[7:] += rng.uniform(-0.3, 0.3, size=q.size - 7)
        o.reset(q)
        o.control_step(0.3 * np.sin(np.arange(4)))
        if o.ncon > 14:
            poses.append(q)
    assert len(poses) >= 8, len(poses)
    poses = np.array(poses[:16])
    n = len(poses)
    scn = [{"params": [[0, 2, "geom_friction", "*", "scale", 0.3]]}, {"params": [[1, 3, "geom_friction", "*", "set", 0.05]]}]
    act = np.tile((0.3 * np.sin(np.arange(4))).astype(np.float32), (4, n, 1))
    out = []
    for device in (True, False):
        env = _env(cfg, cm, n, auto_reset=False, scenarios=scn if device else _strip(scn))
        assert env.engine.query("contact_slots") == 14 and env.engine.query("fixup_contact_slots") == 40
        env.reset()
        env.set_state(poses, np.zeros((n, cm.blob.nv)), np.zeros((n, cm.blob.nv)))
        run = _Run(env, scn, "env", device=device)
        run.steps(act, 0, 4)
        run.final()
        run.stats = env.solver_stats()
        env.close()
        out.append(run)
    a, b = out
    assert a.stats["fixup_steps"] > 0 and a.stats["fixup_steps"] == b.stats["fixup_steps"] and a.stats["dropped_contacts"] == 0
    _same(a, b, what="redone steps: ")
    g = slice(a.lay["geom_friction"], a.lay["geom_friction"] + cm.blob.ngeom)
    late = a.clock[3] >= 3
    assert (a.clock[0] == 0).all() and (a.eff[0][0::2, g] != b.base[0::2, g]).all()                 # the windows opened ...
    assert late.any() and (a.eff[3][late][:, g] == b.base[late][:, g]).all()                         # ... and closed


# ------------------------------------------------------------------------------------------------------------ 5: split pipeline
@pytest.mark.parametrize("hfield_fixup", [False, True], ids=["split", "split+hfield_fixup"])
def test_split_pipeline(hfield_fixup):
    """humanoid_p_v0 on stairs_up_hard: a parameter record of 3 x 64 words (the word loop takes several passes),
    one launch ahead of every substep launch (and of the heightfield fix-ups) of the control step."""
    cfg, cm = _model("humanoid_p_v0", "stairs_up_hard", max_duration=0.5, position_command=True)
    base = np.array([1.0, 0.5], dtype=np.float32)
    n, steps = 4, 6
    actions = _actions(n, steps, cm.blob.nu, seed=23)
    out = []
    for device in (True, False):
        env = _env(cfg, cm, n, base=base, hfield_fixup=hfield_fixup,
                   scenarios=[{}, {}] if not device else None)
        joint = env.param_names()["kp"][3]
        scn = [{"params": [[1, 4, "geom_friction", "*", "scale", 0.4], [2, 5, "kp", joint, "scale", 0.5]]},
               {"params": [[0, 3, "dof_frictionloss", "*", "scale", 2.0]]}]
        if device:
            env.set_scenarios(scn)
        assert env.engine.query("split") > 0 and env.engine.query("param_stride") == 192   # three passes of the wave; 96 has the tail
        env.reset()
        run = _Run(env, scn, "env", device=device)
        if device:
            assert env.engine.query("scenario_param_items") == run.table.n_param_items == cm.blob.ngeom + 1 + cm.blob.nv
        run.steps(actions, 0, steps)
        run.final()
        env.close()
        out.append(run)
    a, b = out
    _same(a, b, what="split pipeline: ")
    lay = a.lay
    kp3 = lay["kp"] + 3
    assert (a.eff[1][0::2, kp3] == b.base[0::2, kp3]).all() and (a.eff[2][0::2, kp3] == b.base[0::2, kp3] * np.float32(0.5)).all()
    assert (a.eff[5][0::2, kp3] == b.base[0::2, kp3]).all() and (a.eff[0][1::2, lay["dof_frictionloss"] + 6] == 2 * b.base[1::2, lay["dof_frictionloss"] + 6]).all()


# ------------------------------------------------------------------------------------------------------------ 6: snapshot
def test_snapshot_inside_a_window_holds_base_rows_and_continues(tmp_path):
    from cosim_amd.snapshot import Snapshot
    cfg, cm = _light()
    n = 12
    actions = _actions(n, 40, 4, seed=24)
    env = _env(cfg, cm, n, scenarios=TABLE, scenario_mode="cycle")
    env.reset()
    base = env.snapshot().rows.cpu().numpy()[:, env.engine.query("state_stride"):].copy()
    t = env.torch
    for k in range(9):                                              # t = 9: inside scenario 0's kp windows
        env.step(t.tensor(actions[k], device=env.device))
    path = str(tmp_path / "snap.npz")
    snap = env.snapshot()
    snap.save(path)
    S = env.engine.query("state_stride")
    rows = snap.rows.cpu().numpy()
    eff = env.effective_params()
    assert np.array_equal(_u(rows[:, S:]), _u(base)) and not np.array_equal(_u(eff), _u(base))   # the snapshot holds BASE rows
    a = _Run(env, TABLE, "cycle")
    a.steps(actions, 9, 40)
    a.final()
    env.close()
    assert a.ended() >= n
    fresh = _env(cfg, cm, n, scenarios=TABLE, scenario_mode="cycle")   # the table is not part of the snapshot: set it again
    loaded = Snapshot.load(path, device=fresh.device)
    fresh.restore(loaded, params=True)
    b = _Run(fresh, TABLE, "cycle")
    b.steps(actions, 9, 40)
    b.final()
    _same(a, b, what="restored: ")
    # fork: every slot starts from row 0's state and base record and follows its OWN row of the table
    fresh.fork(loaded, 0)
    f = _Run(fresh, TABLE, "cycle")
    f.base = np.tile(base[0], (n, 1))
    f.steps(actions, 9, 12)
    lay = f.lay
    rows = (np.arange(n) + f.ep[0]) % 3
    assert (f.clock[0] == 9).all() and set(rows.tolist()) == {0, 1, 2}
    assert (f.eff[0][rows == 0, lay["kp"] + 1] == 0.0).all() and (f.eff[0][rows != 0, lay["kp"] + 1] == base[0, lay["kp"] + 1]).all()
    fresh.close()


# ------------------------------------------------------------------------------------------------------------ 7: ledger, failure traces
def test_ledger_and_failure_traces_equal_the_host_driven_run():
    from cosim_amd.ftrace import same_traces
    from cosim_amd.ledger import same_records
    a, b = _reference("cycle"), _host_driven("cycle")
    diff = same_records(a.ledger, b.ledger)
    assert diff is None, diff
    assert a.ledger.by_scenario() == b.ledger.by_scenario() and sorted(a.ledger.by_scenario()) == [0, 1, 2]
    assert int(a.ledger.ended().sum()) == a.ended() >= N
    diff = same_traces(a.traces, b.traces)
    assert diff is None, diff
    assert len(a.traces) > 0


# ------------------------------------------------------------------------------------------------------------ 8: off means off
def test_cleared_windows_leave_no_trace():
    cfg, cm = _light()
    n = 12
    actions = _actions(n, 32, 4, seed=25)
    y = _env(cfg, cm, n, scenarios=_strip(TABLE))
    y.reset()
    ref = _Run(y, _strip(TABLE), "env", check=False)
    x = _env(cfg, cm, n, scenarios=TABLE)                           # windows set; none opens before t = 3
    x.reset()
    run = _Run(x, _strip(TABLE), "env", check=False)
    t = x.torch
    assert x.engine.query("scenario_param_items") > 0
    for k in range(32):
        if k == 2:
            x.engine.scenario_params_set(None)
            assert x.engine.query("scenario_param_items") == 0 and x.engine.query("scenario_rows") == 3
            base = x.snapshot().rows.cpu().numpy()[:, x.engine.query("state_stride"):]
            assert np.array_equal(_u(x.effective_params()), _u(base))
        for env, r in ((x, run), (y, ref)):
            env.step(t.tensor(actions[k], device=env.device))
            t.cuda.synchronize(env.device)
            r.record()
    run.final(); ref.final()
    _same(ref, run, what="cleared: ")
    assert ref.ended() >= n
    # a scenario table of another S drops the windows; the same S keeps them; clearing the table drops them
    x.set_scenarios(TABLE)
    items = x.engine.query("scenario_param_items")
    assert items > 0
    T2 = x.scenario_table.pack()
    x.engine.scenario_set(T2, 0, x._cmd_out.data_ptr(), x._row_out.data_ptr(), x._stream())
    assert x.engine.query("scenario_param_items") == items
    x.set_scenarios(_strip(TABLE)[:2])
    assert x.engine.query("scenario_rows") == 2 and x.engine.query("scenario_param_items") == 0
    x.set_scenarios(TABLE)
    x.set_scenarios(None)
    assert x.engine.query("scenario_rows") == 0 and x.engine.query("scenario_param_items") == 0
    x.step(t.tensor(actions[0], device=x.device))
    t.cuda.synchronize(x.device)
    assert np.isfinite(x.state.cpu().numpy()).all()
    x.close(); y.close()


# ------------------------------------------------------------------------------------------------------------ 9: refusals
def test_refusals_through_the_c_abi_leave_the_env_stepping():
    cfg, cm = _light()
    n = 6
    actions = _actions(n, 4, 4, seed=26)
    env = _env(cfg, cm, n)
    t = env.torch
    tb = t.tensor(actions, device=env.device)
    env.reset()
    i32, f32 = np.int32, np.float32

    def raw(adr, tt, field, index, op, value):
        env.engine.scenario_params_set((np.array(adr, i32), np.array(tt, i32).reshape(-1, 2), np.array(field, i32), np.array(index, i32),
                                        np.array(op, i32), np.array(value, f32)))
    with pytest.raises(ValueError, match="no scenario table is set"):
        raw([0, 1, 1, 1], [[0, 5]], [0], [0], [0], [0.5])
    env.set_scenarios(_strip(TABLE))
    with pytest.raises(ValueError, match=r"2 scenarios, the table that is set has 3"):
        raw([0, 1, 1], [[0, 5]], [0], [0], [0], [0.5])
    for field in (4, 5, 6, 7):
        with pytest.raises(ValueError, match=r"scenario 1, parameter item 0: field %d .* is refused: .* fp64" % field):
            raw([0, 0, 1, 1], [[0, 5]], [field], [0], [0], [1.5])
    with pytest.raises(ValueError, match=r"scenario 0, parameter item 1: unknown field 9"):
        raw([0, 2, 2, 2], [[0, 5], [0, 5]], [0, 9], [0, 0], [0, 0], [0.5, 0.5])
    with pytest.raises(ValueError, match=r"scenario 2, parameter item 0: index 4 out of range: kp has 4 entries"):
        raw([0, 0, 0, 1], [[0, 5]], [0], [4], [0], [0.5])
    with pytest.raises(ValueError, match=r"parameter item 0: index -1 out of range"):
        raw([0, 1, 1, 1], [[0, 5]], [2], [-1], [0], [0.5])
    with pytest.raises(ValueError, match=r"parameter item 0: unknown op 2"):
        raw([0, 1, 1, 1], [[0, 5]], [0], [0], [2], [0.5])
    with pytest.raises(ValueError, match=r"parameter item 0: value is not finite"):
        raw([0, 1, 1, 1], [[0, 5]], [0], [0], [1], [np.inf])
    with pytest.raises(ValueError, match=r"parameter item 0: t1 5 is not after t0 5"):
        raw([0, 1, 1, 1], [[5, 5]], [0], [0], [1], [1.0])
    with pytest.raises(ValueError, match=r"parameter item 0: times outside \[0, 2\^30\)"):
        raw([0, 1, 1, 1], [[-1, 5]], [0], [0], [1], [1.0])
    with pytest.raises(ValueError, match=r"scenario 0: 257 parameter items, at most 256"):
        raw([0, 257, 257, 257], [[0, 5]] * 257, [0] * 257, [0] * 257, [0] * 257, [1.0] * 257)
    with pytest.raises(ValueError, match=r"shorter than their row addresses"):
        raw([0, 3, 3, 3], [[0, 5]], [0], [0], [0], [0.5])
    assert env.engine.query("scenario_param_items") == 0            # nothing was set by a refused call
    with pytest.raises(ValueError, match=r"scenario 0, parameter window 0: field 'body_mass' is refused"):
        env.set_scenarios([{"params": [[0, 5, "body_mass", 0, "scale", 2.0]]}])
    env.set_scenarios(TABLE)
    assert env.engine.query("scenario_param_items") > 0
    env.step(tb[0])
    with pytest.raises(ValueError, match="scenario table is set"):
        env.rollout(tb[1:3])
    with pytest.raises(ValueError, match="scenario table is set"):   # the C entry point refuses by itself while windows are set
        env.engine.rollout(1, tb[1:2].data_ptr(), env._cmd_ptr(), env.state.data_ptr(), env.terminated.data_ptr(), env.truncated.data_ptr(),
                           env.info_buf.data_ptr(), env._stream())
    env.step(tb[1])
    t.cuda.synchronize(env.device)
    assert np.isfinite(env.state.cpu().numpy()).all() and env.solver_stats()["step_count"] == n * 3   # the reset and two steps
    env.close()


# ------------------------------------------------------------------------------------------------------------ 10: CLI
def _cli(tmp_path, capsys, *extra):
    import yaml
    from cosim_amd import cli
    scn, report = tmp_path / "scn.yaml", tmp_path / ("r%d.json" % len(extra))
    scn.write_text(yaml.safe_dump({"scenarios": TABLE}))
    assert cli.main(["--env", "flamingo_light_v1", "--num-envs", "24", "--steps", "60", "--max-duration", "0.5", "--seed", "5", "--policy",
                     "random-mlp", "--scenarios", str(scn), "--scenario-mode", "cycle", *extra, "--ledger", "4", "--report", str(report)]) == 0
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    return json.loads(report.read_text()), line


@pytest.mark.parametrize("path", ["--graph", "--pipelined"])
def test_cli_windows_on_the_fast_paths(tmp_path, capsys, path):
    """The two closed-loop paths that cannot call set_param between steps run a scenario file that holds windows; the report's
    breakdown by scenario equals the eager run's."""
    if "eager" not in _CACHE:
        _CACHE["eager"] = _cli(tmp_path, capsys)
    eager, eline = _CACHE["eager"]
    r, line = _cli(tmp_path, capsys, path)
    by = r["episodes"]["by_scenario"]
    assert sorted(by) == ["0", "1", "2"] and sum(v["episodes"] for v in by.values()) == r["episodes"]["episodes"] >= 24
    assert by == eager["episodes"]["by_scenario"]
    assert line["param_windows"] == eline["param_windows"] == 7 and line["control_steps"] == 60
