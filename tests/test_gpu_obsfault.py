"""Observation faults of a scenario table on the device (cosim_set_param "obs_faults", csrc/cosim_obsfault.hip, and their BatchedEnv /
CLI surface) against the numpy twin (cosim_amd/scenario.py reference_obs_faults) fed with the frames of a fleet that runs the same
table WITHOUT the faults under the same seed and action table.

Every comparison is EXACT: float32 bits for floats (uint32 views), ints as ints.  The flat fleet is 128 flamingo_light_v1 envs over 40
steps; max_duration = 0.5 puts the time limit in episode step 25, so every env ends an episode inside the run; projected_gravity is
observed at half the control rate, so the table faults a frequency-gated element.  Each test asserts that what it is about -- a window that opened
and closed, a lost packet, a redone step -- happened."""
import copy
import json

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_CACHE = {}
CD = 4
BASE = np.array([0.5, 0.0, 0.0, 0.0], dtype=np.float32)
N, K, RESET_AT = 128, 40, 30
RESET_MASK = (np.arange(N) % 4 == 1)
FIRST_WINDOW = 2                                                    # no item of FAULTS holds before observation clock 2

# Three scenarios for flamingo_light_v1 (frame: dof_pos 0..1 | dof_vel 2..5 | ang_vel 6..8 | projected_gravity 9..11 | last_action
# 12..15 | command 16..19, three stack rows); an episode's observation clock runs 0 (the reset's) .. 24, then 0 again:
#   0  a gyro bias with a scale listed behind it, encoder noise, a frozen wheel encoder, lost IMU packets, a stuck gravity word
#   1  items that hold at the fill (t_obs = 0): every stack row; a hold and a drop there are the identity
#   2  no fault: these envs must see what the clean fleet sees
FAULTS = [
    {"commands": [[0, 0.3, 0.1, 0.0, 0.0]], "pushes": [[6, 8, 0.3, 0.0, 0.0]],
     "faults": [[4, 12, "ang_vel", "*", "bias", 0.05], [6, 9, "ang_vel", 2, "scale", -1.5], [2, 20, "dof_vel", "*", "noise", 0.02],
                [10, 18, "dof_pos", 1, "hold", 0.0], [5, 25, "ang_vel", "*", "drop", 0.2], [15, 17, "projected_gravity", 2, "set", -1.0],
                [20, 30, "last_action", 0, "scale", 0.0]]},
    {"faults": [[0, 3, "projected_gravity", "*", "bias", 0.125], [0, 2, "dof_pos", "*", "hold", 0.0], [0, 25, "dof_vel", 3, "drop", 1.0],
                [0, 1, "dof_vel", 0, "noise", 0.5], {"t0": 22, "t1": 26, "obs": "dof_pos", "index": 0, "op": "set", "value": 0.25, "name": "stuck"}]},
    {"commands": [[4, 0.6, 0.0, 0.0, 0.0]]},
]


def _strip(scn):
    return [{k: v for k, v in s.items() if k != "faults"} for s in scn]


def _variant(scn):
    """The same item counts with other values and times: what an in-place rewrite uploads."""
    out = [dict(s) for s in scn]
    out[0] = dict(out[0], faults=[[3, 9, "ang_vel", "*", "bias", -0.1], [1, 30, "ang_vel", 2, "scale", 0.5], [0, 20, "dof_vel", "*", "noise", 0.05],
                                  [8, 12, "dof_pos", 1, "hold", 0.0], [5, 25, "ang_vel", "*", "drop", 0.5], [1, 4, "projected_gravity", 2, "set", 1.0],
                                  [2, 3, "last_action", 0, "scale", 2.0]])
    return out


def _model(robot, terrain="flat", gate=None, **kw):
    from cosim_amd.compile import compile_model
    from cosim_amd.config import make_config
    key = (robot, terrain, gate, json.dumps(kw, sort_keys=True))
    if key not in _CACHE:
        cfg = make_config(robot, terrain=terrain, **kw)
        if kw.get("position_command"):
            cfg["observation"]["command_dim"] = 2
        if gate:
            cfg["observation"][gate]["freq"] = cfg["observation"][gate]["freq"] / 2   # refreshed every other control step
        _CACHE[key] = (cfg, compile_model(cfg))
    return _CACHE[key]


def _light():
    return _model("flamingo_light_v1", "flat", gate="projected_gravity", max_duration=0.5)


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


def _layout(env):
    from cosim_amd.scenario import fault_layout
    lay = fault_layout(env.fault_names())
    assert lay["state_dim"] == env.state_dim and lay["frame_dim"] == env.engine.query("frame_dim") and lay["stacked_dim"] == env.engine.query("stacked_dim")
    return lay


def _frames(state, lay):
    """The newest frame of state_out rows [..., state_dim]: the first stack row and the non-stacked tail."""
    sd, S = lay["stacked_dim"], lay["stack_size"]
    return np.concatenate([state[..., :sd], state[..., S * sd:]], axis=-1)


def _outside_stack(env, rows):
    """State records with the observation-stack words blanked: what faults must not touch."""
    q = env.engine.query
    s_stack = q("nq") + 2 * q("nv") + 2 * q("action_dim") + 16 + q("frame_dim")
    out = rows[:, :q("state_stride")].copy()
    out[:, s_stack:s_stack + env.stack_size * q("stacked_dim")] = 0.0
    return out


class _Run:
    """One run, recorded observation by observation: the reset's, then one per step (a masked reset's in between)."""

    def __init__(self, env):
        self.env = env
        self.state, self.te, self.tr, self.info, self.meta, self.active = [], [], [], [], [], []

    def observe(self, active=None, flags=True):
        env = self.env
        env.join()
        env.torch.cuda.synchronize(env.device)
        self.state.append(env.state.cpu().numpy().copy()); self.meta.append(_meta(env))
        self.active.append(np.ones(env.num_envs, dtype=bool) if active is None else np.asarray(active, dtype=bool))
        if flags:
            self.info.append(env.info_buf.cpu().numpy().copy())
            self.te.append(env.terminated.cpu().numpy().copy()); self.tr.append(env.truncated.cpu().numpy().copy())

    def drive(self, actions, step=None, reset_at=None, reset_mask=None, before=None):
        env, t = self.env, self.env.torch
        tb = t.tensor(actions, device=env.device)
        env.reset()
        self.observe(flags=False)
        for k in range(len(actions)):
            if k == reset_at:
                env.join()
                env.reset(mask=reset_mask)
                self.observe(active=reset_mask, flags=False)
            if before is not None:
                before(k)
            (step or (lambda k, a: env.step(a)))(k, tb[k])
            self.observe()
        self.rows = env.snapshot().rows.cpu().numpy().copy()
        self.qpos, self.qvel = env.get_data().qpos.cpu().numpy().copy(), env.get_data().qvel.cpu().numpy().copy()
        return self

    def ended(self):
        return int((np.stack(self.te) | np.stack(self.tr)).astype(bool).sum())

    def twin(self, table, mode, seed, clean=None):
        """The faulted state_out rows the twin works out from the frames of ``clean`` (default: this run's own meta words)."""
        from cosim_amd.scenario import reference_obs_faults
        env, src = self.env, clean or self
        meta = np.stack(src.meta)
        gid = env.env_id0 + np.arange(env.num_envs)
        return reference_obs_faults(table, mode, gid, meta[:, :, 0], meta[:, :, 11], meta[:, :, 1], seed, _frames(np.stack(src.state), self.lay), self.lay,
                                    active=np.stack(src.active))


def _same_physics(a, b, what=""):
    """qpos, qvel, info, flags of every step, the meta words of every observation and the final state records outside the stack."""
    assert len(a.info) == len(b.info) > 0 and len(a.meta) == len(b.meta)
    for k in range(len(a.info)):
        assert np.array_equal(_u(a.info[k]), _u(b.info[k])), f"{what}info differs in step {k}"
        assert np.array_equal(a.te[k], b.te[k]) and np.array_equal(a.tr[k], b.tr[k]), f"{what}flags differ in step {k}"
    for k in range(len(a.meta)):
        assert np.array_equal(a.meta[k], b.meta[k]), f"{what}meta words differ at observation {k}"
    assert np.array_equal(_u(a.qpos), _u(b.qpos)) and np.array_equal(_u(a.qvel), _u(b.qvel)), f"{what}final qpos / qvel differ"
    assert np.array_equal(_u(a.out_rows), _u(b.out_rows)), f"{what}final state records differ outside the stack words"


def _same_obs(a, b, what=""):
    assert len(a.state) == len(b.state) > 0
    for k in range(len(a.state)):
        x, y = _u(a.state[k]), _u(b.state[k])
        assert np.array_equal(x, y), f"{what}state differs at observation {k}: envs {np.nonzero((x != y).any(axis=1))[0][:8]}"
    assert np.array_equal(_u(a.rows), _u(b.rows)), f"{what}final state records differ"


def _pair(mode):
    """Test 1's two fleets, once per mode: FAULTS and the same table without faults, 128 envs, 40 steps with a masked host reset
    before step 30; all four observers armed on both (they change no step output).  Shared, never modified."""
    key = ("pair", mode)
    if key not in _CACHE:
        from cosim_amd.scenario import ScenarioTable
        cfg, cm = _light()
        checks = [[0, 25, "abs_info", "ang_vel_yaw", "always", "<", 50.0]]
        curves = [[0, 25, 1, "info", "lin_vel_x", -1.0, 1.0, 8]]
        runs = []
        for scn in (FAULTS, _strip(FAULTS)):
            scn = [dict(s, checks=checks, curves=curves) for s in scn]
            env = _env(cfg, cm, N, scenarios=scn, scenario_mode=mode, ledger=4, failure_traces=(8, 2), check_slots=4, curves=True)
            run = _Run(env)
            run.lay = _layout(env)
            actions = _actions(N, K, env.action_dim)
            run.items = env.engine.query("obs_faults")
            run.listed = env.obs_faults()
            run.drive(actions, reset_at=RESET_AT, reset_mask=RESET_MASK)
            run.out_rows = _outside_stack(env, run.rows)
            run.ledger, run.traces = env.ledger(include_open=True), env.failure_traces(include_open=True)
            run.verdicts, run.curves = env.verdicts(include_open=True), env.curves()
            run.seed, run.table, run.actions = env.seed, ScenarioTable(scn, CD, names={"faults": env.fault_names()}), actions
            run.names = env.fault_names()
            env.close()
            runs.append(run)
        _CACHE[key] = tuple(runs)
    return _CACHE[key]


# ------------------------------------------------------------------------------------------------------------ 1: open loop = twin
@pytest.mark.parametrize("mode", ["env", "cycle"])
def test_open_loop_equals_the_twin(mode):
    f, c = _pair(mode)
    assert f.items == f.table.n_fault_items == 3 + 1 + 4 + 1 + 3 + 1 + 1 + 3 + 2 + 1 + 1 + 1 and c.items == 0 and sum(map(len, f.listed)) == f.items
    assert [tuple(i[:5]) for i in f.listed[0][:3]] == [(4, 12, 6, 1, 0), (4, 12, 7, 1, 0), (4, 12, 8, 1, 0)] and c.listed == [[], [], []]
    _same_physics(f, c, what="faulted against clean: ")             # faults touch nothing but what the policy sees
    meta = np.stack(f.meta)
    t_obs = meta[:, :, 0]
    done = (np.stack(f.te) | np.stack(f.tr)).astype(bool)
    assert f.ended() >= N and done[24].all() and (t_obs[0] == 0).all() and (t_obs[25] == 0).all() and (t_obs[24] == 24).all()
    want = f.twin(f.table, mode, f.seed, clean=c)
    got, clean = np.stack(f.state), np.stack(c.state)
    for k in range(len(got)):
        act = f.active[k]
        x, y = _u(got[k][act]), _u(want[k][act])
        assert np.array_equal(x, y), f"observation {k} (t_obs {t_obs[k][:3]}): envs {np.nonzero((x != y).any(axis=1))[0][:8]}, words {np.nonzero((x != y).any(axis=0))[0][:12]}"
    assert not f.active[RESET_AT + 1].all() and np.array_equal(f.active[RESET_AT + 1], RESET_MASK)   # the masked reset's observation
    gid = np.arange(N)
    s0, s1, s2 = (gid % 3 == r for r in range(3))
    if mode == "env":
        # before the first window opens the two fleets see the same, scenario 2 throughout
        for k in range(FIRST_WINDOW):
            assert np.array_equal(_u(got[k][~s1]), _u(clean[k][~s1]))
        assert all(np.array_equal(_u(got[k][s2]), _u(clean[k][s2])) for k in range(len(got)))
        sd = f.lay["stacked_dim"]
        # windows opened and closed: the gyro bias of scenario 0 over [4, 12) on the newest frame ...
        assert np.array_equal(_u(got[3][s0, 6:9]), _u(clean[3][s0, 6:9])) and (got[4][s0, 6] != clean[4][s0, 6]).all()
        assert np.array_equal(_u(got[4][s0, 6]), _u(clean[4][s0, 6] + np.float32(0.05)))
        # ... which the roll carries to the second stack row one step on
        assert np.array_equal(_u(got[5][s0, sd + 6]), _u(got[4][s0, 6]))
        # scenario 1 at the fill: every stack row holds the biased gravity; the frozen encoder (drop 1.0) repeats the reset's value
        for r in range(3):
            assert np.array_equal(_u(got[0][s1, r * sd + 9:r * sd + 12]), _u(clean[0][s1, 9:12] + np.float32(0.125)))
        # the gated element is not refreshed at clock 1: it comes back clean from the cache and is biased again, once
        assert np.array_equal(_u(clean[1][:, 9:12]), _u(clean[0][:, 9:12])) and (clean[2][:, 9:12] != clean[1][:, 9:12]).any()
        assert np.array_equal(_u(got[1][s1, 9:12]), _u(got[0][s1, 9:12])) and np.array_equal(_u(got[3][s1, 9:12]), _u(clean[3][s1, 9:12]))
        assert all(np.array_equal(_u(got[k][s1, 5]), _u(got[0][s1, 5])) for k in range(1, 25)) and (clean[5][s1, 5] != clean[0][s1, 5]).any()
        # lost packets: all three gyro words of an env repeat the previous observation together, about one step in five
        lost = (got[6:25, :, 6:9] == got[5:24, :, 6:9])[:, s0]
        assert (lost.all(axis=2) | ~lost.any(axis=2)).mean() > 0.95 and 0.1 < lost.all(axis=2).mean() < 0.5
    else:
        assert (meta[26, :, 11] >= 1).all() and (got[28][s2] != clean[28][s2]).any()   # scenario 2's envs now run scenario 0: clock 3, encoder noise
        assert all(np.array_equal(_u(got[k][s2]), _u(clean[k][s2])) for k in range(25))


# ------------------------------------------------------------------------------------------------------------ 2: arrangements
def test_every_arrangement_gives_the_same_bits():
    """The cycle run of test 1 again: two uneven ranges through step_range chains, 4 ranges under a deferred join.  No host read
    between a step's launches."""
    import torch
    a, _ = _pair("cycle")
    cfg, cm = _light()
    scn = a.table.to_list()
    b = _env(cfg, cm, N, scenarios=scn, scenario_mode="cycle", ranges=4, deferred_join=True)
    assert b.engine.query("ranges") == 4 and [c for _, c in b.range_list] == [32] * 4 and b.engine.query("obs_faults") == a.items
    rb = _Run(b).drive(a.actions, reset_at=RESET_AT, reset_mask=RESET_MASK)
    _same_obs(a, rb, what="4 ranges, deferred join: ")
    b.close()

    d = _env(cfg, cm, N, scenarios=scn, scenario_mode="cycle")
    streams = [torch.cuda.Stream(device=d.device) for _ in range(2)]

    def chains(k, act):
        torch.cuda.synchronize(d.device)
        for st, (first, count) in zip(streams, ((0, 50), (50, 78))):
            with torch.cuda.stream(st):
                d.step_range(first, count, act)
        torch.cuda.synchronize(d.device)
    _same_obs(a, _Run(d).drive(a.actions, step=chains, reset_at=RESET_AT, reset_mask=RESET_MASK), what="step_range chains: ")
    d.close()


def test_captured_step_and_in_place_rewrite_between_replays():
    """A captured step carries the launch; items of the counts of the ones that are set are rewritten in place: the graph keeps its
    pointers and picks the new values up.  Against an eager run that rewrites at the same step."""
    import torch
    cfg, cm = _light()
    n, steps, at = 32, 30, 7
    actions = _actions(n, steps, 4, seed=22)
    e = _env(cfg, cm, n, scenarios=FAULTS, scenario_mode="env")
    items = e.engine.query("obs_faults")

    def rewrite(env):
        def before(k):
            if k == at:
                env.set_scenarios(_variant(FAULTS), "env")
                assert env.engine.query("obs_faults") == items
        return before
    ref = _Run(e).drive(actions, before=rewrite(e))
    e.close()
    plain = _env(cfg, cm, n, scenarios=FAULTS, scenario_mode="env")
    unre = _Run(plain).drive(actions)
    plain.close()
    assert np.array_equal(_u(ref.state[at]), _u(unre.state[at])) and not np.array_equal(_u(ref.state[at + 2]), _u(unre.state[at + 2]))

    g = _env(cfg, cm, n, scenarios=FAULTS, scenario_mode="env")
    run = _Run(g)
    tb = torch.tensor(actions, device=g.device)
    buf = torch.empty((n, g.action_dim), device=g.device)
    g.reset()
    run.observe(flags=False)
    buf.copy_(tb[0])
    side = torch.cuda.Stream(device=g.device)
    torch.cuda.synchronize(g.device)
    side.wait_stream(torch.cuda.current_stream(g.device))
    with torch.cuda.stream(side):
        g.step(buf)
    torch.cuda.current_stream(g.device).wait_stream(side)
    run.observe()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g.step(buf)                                                 # recorded, not run: the launch is part of the graph
    for k in range(1, steps):
        rewrite(g)(k)
        buf.copy_(tb[k])
        graph.replay()
        run.observe()
    run.rows = g.snapshot().rows.cpu().numpy().copy()
    g.close()
    _same_obs(ref, run, what="captured step, items rewritten in place: ")


# ------------------------------------------------------------------------------------------------------------ 3: abandon and redo
def test_redone_steps_are_faulted_once():
    """Drop poses with more than 14 contacts (the recipe of test_more_contacts_than_the_fleet_kernel_holds_are_redone_not_dropped):
    the fleet kernel gives such a step up and the 40-slot kernel redoes it; the fault kernel runs behind the redo, once."""
    from cosim_amd.compile import compile_model
    from cosim_amd.config import PARITY_RANDOM, make_config
    from cosim_amd.model import get_field
    from cosim_amd.scenario import ScenarioTable
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
    scn = [{"faults": [[1, 3, "dof_vel", "*", "scale", 2.0], [1, 5, "ang_vel", "*", "bias", 0.5], [2, 4, "dof_pos", "*", "hold", 0.0]]},
           {"faults": [[1, 2, "projected_gravity", "*", "scale", -1.0]]}]
    act = np.tile((0.3 * np.sin(np.arange(4))).astype(np.float32), (4, n, 1))
    out = []
    for faulted in (True, False):
        env = _env(cfg, cm, n, auto_reset=False, scenarios=scn if faulted else _strip(scn))
        assert env.engine.query("contact_slots") == 14 and env.engine.query("fixup_contact_slots") == 40
        run = _Run(env)
        run.lay = _layout(env)
        t = env.torch
        env.reset()
        run.observe(flags=False)
        env.set_state(poses, np.zeros((n, cm.blob.nv)), np.zeros((n, cm.blob.nv)))
        for k in range(4):
            env.step(t.tensor(act[k], device=env.device))
            run.observe()
        run.stats = env.solver_stats()
        run.table, run.seed = ScenarioTable(scn, CD, names={"faults": env.fault_names()}), env.seed
        env.close()
        out.append(run)
    a, b = out
    assert a.stats["fixup_steps"] > 0 and a.stats["fixup_steps"] == b.stats["fixup_steps"] and a.stats["dropped_contacts"] == 0
    want = a.twin(a.table, "env", a.seed, clean=b)
    for k in range(5):
        assert np.array_equal(_u(a.state[k]), _u(want[k])), k
    assert (np.stack(a.state)[1, 0::2, 2:6] == np.float32(2.0) * np.stack(b.state)[1, 0::2, 2:6]).all()   # scaled once, not twice
    assert not np.array_equal(_u(a.state[1]), _u(b.state[1])) and np.array_equal(_u(a.info[3]), _u(b.info[3]))


# ------------------------------------------------------------------------------------------------------------ heightfield, split pipeline
def test_non_stacked_height_map_takes_three_passes():
    """slope_easy with a non-stacked 15 x 9 height map behind the 20-element frame: 155 elements, three passes of the wave."""
    from cosim_amd.scenario import ScenarioTable
    cfg, cm = _model("flamingo_light_v1", "slope_easy", max_duration=0.2, height_map=True)
    n, steps = 64, 20
    scn = [{"faults": [[3, 8, "height_map", "*", "set", 0.0], [5, 12, "height_map", 134, "bias", 0.25], [0, 2, "height_map", 70, "noise", 0.1],
                       [4, 9, "ang_vel", "*", "hold", 0.0]]},
           {"faults": [[0, 10, "height_map", 0, "scale", 2.0], [2, 6, "dof_vel", "*", "drop", 0.5]]}, {}]
    out = []
    for faulted in (True, False):
        env = _env(cfg, cm, n, scenarios=scn if faulted else _strip(scn), scenario_mode="cycle")
        run = _Run(env)
        run.lay = _layout(env)
        assert run.lay["frame_dim"] == 155 and env.obs_to_dim["height_map"] == 135 and env.engine.query("obs_faults") == (135 + 1 + 1 + 3 + 1 + 4 if faulted else 0)
        run.drive(_actions(n, steps, env.action_dim, seed=27))
        run.out_rows = _outside_stack(env, run.rows)
        run.table, run.seed = ScenarioTable(scn, CD, names={"faults": env.fault_names()}), env.seed
        env.close()
        out.append(run)
    a, b = out
    _same_physics(a, b, what="height map: ")
    assert a.ended() >= n
    want = a.twin(a.table, "cycle", a.seed, clean=b)
    for k in range(steps + 1):
        assert np.array_equal(_u(a.state[k]), _u(want[k])), k
    tail = 3 * a.lay["stacked_dim"] + 4                             # the height map behind the command words
    s0 = np.arange(n) % 3 == 0
    assert (np.stack(a.state)[3, s0, tail:tail + 135] == 0.0).all() and (np.stack(b.state)[3, s0, tail:tail + 135] != 0.0).any()


def test_split_pipeline():
    """humanoid_p_v0 on stairs_up_hard: the launch behind the last substep's solver (and heightfield fix-up) launch, once per step."""
    from cosim_amd.scenario import ScenarioTable
    cfg, cm = _model("humanoid_p_v0", "stairs_up_hard", max_duration=0.5, position_command=True)
    base = np.array([1.0, 0.5], dtype=np.float32)
    n, steps = 16, 4
    scn = [{"faults": [[1, 3, "dof_pos", "*", "bias", 0.1], [2, 4, "lin_vel", "*", "hold", 0.0], [0, 5, "dof_vel", 22, "noise", 0.2]]},
           {"faults": [[0, 2, "last_action", "*", "scale", 0.5], [1, 5, "ang_vel", "*", "drop", 0.5]]}]
    for hfield_fixup in (False, True):
        out = []
        for faulted in (True, False):
            env = _env(cfg, cm, n, base=base, hfield_fixup=hfield_fixup, scenarios=scn if faulted else _strip(scn))
            assert env.engine.query("split") > 0
            run = _Run(env)
            run.lay = _layout(env)
            assert 64 < run.lay["frame_dim"] <= 128                     # two passes
            run.drive(_actions(n, steps, cm.blob.nu, seed=23))
            run.out_rows = _outside_stack(env, run.rows)
            run.table, run.seed = ScenarioTable(scn, 2, names={"faults": env.fault_names()}), env.seed
            env.close()
            out.append(run)
        a, b = out
        _same_physics(a, b, what="split pipeline: ")
        want = a.twin(a.table, "env", a.seed, clean=b)
        for k in range(steps + 1):
            assert np.array_equal(_u(a.state[k]), _u(want[k])), (hfield_fixup, k)
        assert not np.array_equal(_u(a.state[1]), _u(b.state[1]))


# ------------------------------------------------------------------------------------------------------------ 4: closed loop
def test_closed_loop_diverges_at_the_window_and_three_loops_agree(tmp_path):
    """A random-MLP policy over a fleet with a gyro bias from observation clock 10 on: the bits of the fleet without the fault
    through step 10's action, other bits afterwards; Runner.test, test_graphed and test_pipelined give the same bits."""
    import torch
    from cosim_amd.policy import MLPPolicy, write_random_mlp
    from cosim_amd.runner import Runner
    cfg, cm = _light()
    n, steps = 128, 30
    scn = [{"faults": [[10, 1000, "ang_vel", "*", "bias", 0.2]]}]
    f = str(tmp_path / "actor.onnx")
    write_random_mlp(f, 52, 4, hidden=(64, 64), seed=31)

    def loop(kind, scenarios):
        env = _env(cfg, cm, n, scenarios=scenarios, **({"ranges": 4, "deferred_join": True} if kind == "pipelined" else {}))
        assert env.state_dim == 52
        run = Runner(env, MLPPolicy(f, device=env.device, fused=True))
        run.update_command(0, 0.5)
        trace = []
        if kind == "eager":
            assert run.test(max_steps=steps, on_step=lambda k, s, te, tr, info: trace.append((s.cpu().numpy().copy(), env.get_data().qpos.cpu().numpy().copy()))) == steps
        else:
            assert (run.test_graphed(steps) if kind == "graphed" else run.test_pipelined(steps)) == steps
        torch.cuda.synchronize()
        out = (env.state.cpu().numpy().copy(), env.get_data().qpos.cpu().numpy().copy(), env.solver_stats()["episodes_ended"], trace)
        env.close()
        return out
    faulted, clean = loop("eager", scn), loop("eager", _strip(scn))
    # step k's action reads observation k (clock k): observations 0 .. 9 are clean, so steps 0 .. 9 and the physics of step 10's
    # observation are those of the clean fleet; observation 10 carries the bias, step 10 acts on it, step 11's physics differs
    for k in range(9):
        assert np.array_equal(_u(faulted[3][k][0]), _u(clean[3][k][0])) and np.array_equal(_u(faulted[3][k][1]), _u(clean[3][k][1])), k
    assert np.array_equal(_u(faulted[3][9][1]), _u(clean[3][9][1])) and not np.array_equal(_u(faulted[3][9][0]), _u(clean[3][9][0]))
    assert np.array_equal(_u(faulted[3][9][0][:, 6:9]), _u(clean[3][9][0][:, 6:9] + np.float32(0.2)))
    assert not np.array_equal(_u(faulted[3][10][1]), _u(clean[3][10][1]))
    assert faulted[2] >= n
    for kind in ("graphed", "pipelined"):
        other = loop(kind, scn)
        assert np.array_equal(_u(other[0]), _u(faulted[0])) and np.array_equal(_u(other[1]), _u(faulted[1])) and other[2] == faulted[2], kind


# ------------------------------------------------------------------------------------------------------------ 5: snapshot
def test_snapshot_inside_a_hold_window_continues_and_a_fork_follows_its_row(tmp_path):
    from cosim_amd.snapshot import Snapshot
    cfg, cm = _light()
    n = 24
    actions = _actions(n, 40, 4, seed=24)
    env = _env(cfg, cm, n, scenarios=FAULTS, scenario_mode="cycle")
    t = env.torch
    env.reset()
    for k in range(12):                                             # clock 12: inside scenario 0's hold [10, 18) and drop [5, 25) windows
        env.step(t.tensor(actions[k], device=env.device))
    path = str(tmp_path / "snap.npz")
    env.snapshot().save(path)

    def go(e, k0, k1):
        run = _Run(e)
        for k in range(k0, k1):
            e.step(t.tensor(actions[k], device=e.device))
            run.observe()
        run.rows = e.snapshot().rows.cpu().numpy().copy()
        return run
    a = go(env, 12, 40)
    env.close()
    assert a.ended() >= n
    fresh = _env(cfg, cm, n, scenarios=FAULTS, scenario_mode="cycle")   # the table is not part of the snapshot: set it again
    loaded = Snapshot.load(path, device=fresh.device)
    fresh.restore(loaded, params=True)
    b = go(fresh, 12, 40)
    _same_obs(a, b, what="restored: ")
    s0 = np.arange(n) % 3 == 0
    assert np.array_equal(_u(a.state[0][s0, 1]), _u(a.state[3][s0, 1]))                       # dof_pos[1] frozen over the restore
    # a fork: every slot starts from row 0's state and follows its OWN row of the table: the gyro bias [4, 12) is over, the frozen
    # encoder of scenario 0 and the one of scenario 1 (dof_vel[3], drop 1.0) go on in the slots that run them
    fresh.fork(loaded, 0)
    before = fresh.state.cpu().numpy().copy()
    f = go(fresh, 12, 14)
    rows = (np.arange(n) + f.meta[0][:, 11]) % 3
    assert (f.meta[0][:, 0] == 13).all() and set(rows.tolist()) == {0, 1, 2}
    assert np.array_equal(_u(f.state[0][rows == 0, 1]), _u(before[rows == 0, 1])) and (f.state[0][rows != 0, 1] != before[rows != 0, 1]).all()
    assert np.array_equal(_u(f.state[0][rows == 1, 5]), _u(before[rows == 1, 5])) and (f.state[0][rows == 2, 5] != before[rows == 2, 5]).all()
    fresh.close()


# ------------------------------------------------------------------------------------------------------------ 6: observers
def test_observers_see_the_same_open_loop_run():
    """Ledger, failure traces, verdicts and curves armed together with the faults: an open-loop run's physics does not depend on what
    the policy sees, so all four equal those of the clean fleet."""
    from cosim_amd.checks import same_verdicts
    from cosim_amd.curves import same_curves
    from cosim_amd.ftrace import same_traces
    from cosim_amd.ledger import same_records
    f, c = _pair("cycle")
    diff = same_records(f.ledger, c.ledger)
    assert diff is None, diff
    assert f.ledger.by_scenario() == c.ledger.by_scenario() and sorted(f.ledger.by_scenario()) == [0, 1, 2]
    assert int(f.ledger.ended().sum()) == f.ended() >= N
    diff = same_traces(f.traces, c.traces)
    assert diff is None, diff
    diff = same_verdicts(f.verdicts, c.verdicts)
    assert diff is None, diff
    diff = same_curves(f.curves, c.curves)
    assert diff is None, diff
    assert len(f.verdicts) > 0 and f.verdicts.summary() == c.verdicts.summary() and f.curves.summary() == c.curves.summary()


# ------------------------------------------------------------------------------------------------------------ 7: off means off, refusals, CLI
def test_cleared_faults_leave_no_trace():
    cfg, cm = _light()
    n = 32
    actions = _actions(n, 30, 4, seed=25)
    y = _env(cfg, cm, n, scenarios=_strip(FAULTS))
    ref = _Run(y).drive(actions)
    x = _env(cfg, cm, n, scenarios=[FAULTS[0], _strip(FAULTS)[1], FAULTS[2]])   # faults set; none holds before clock 2
    assert x.engine.query("obs_faults") > 0

    def before(k):
        if k == 1:
            x.engine.scenario_faults_set(None)
            assert x.engine.query("obs_faults") == 0 and x.engine.query("scenario_rows") == 3
    run = _Run(x).drive(actions, before=before)
    _same_obs(ref, run, what="cleared: ")
    assert ref.ended() >= n
    # a scenario table of another S drops the faults; the same S keeps them; clearing the table drops them
    x.set_scenarios(FAULTS)
    items = x.engine.query("obs_faults")
    assert items > 0
    x.engine.scenario_set(x.scenario_table.pack(), 0, x._cmd_out.data_ptr(), x._row_out.data_ptr(), x._stream())
    assert x.engine.query("obs_faults") == items
    x.set_scenarios(_strip(FAULTS))                                 # a table without faults clears what the earlier one left
    assert x.engine.query("obs_faults") == 0 and x.obs_faults() == [[], [], []]
    x.set_scenarios(FAULTS)
    x.set_scenarios(_strip(FAULTS)[:2])
    assert x.engine.query("scenario_rows") == 2 and x.engine.query("obs_faults") == 0
    x.set_scenarios(FAULTS)
    x.set_scenarios(None)
    assert x.engine.query("scenario_rows") == 0 and x.engine.query("obs_faults") == 0 and x.obs_faults() == []
    t = x.torch
    x.step(t.tensor(actions[0], device=x.device))
    t.cuda.synchronize(x.device)
    assert np.isfinite(x.state.cpu().numpy()).all()
    x.close(); y.close()


def test_refusals_through_the_c_abi_leave_the_env_stepping():
    cfg, cm = _light()
    n = 6
    actions = _actions(n, 4, 4, seed=26)
    env = _env(cfg, cm, n)
    t = env.torch
    tb = t.tensor(actions, device=env.device)
    env.reset()
    i32, f32 = np.int32, np.float32

    def raw(adr, tt, elem, op, ordinal, value):
        env.engine.scenario_faults_set((np.array(adr, i32), np.array(tt, i32).reshape(-1, 2), np.array(elem, i32), np.array(op, i32),
                                        np.array(ordinal, i32), np.array(value, f32)))
    with pytest.raises(ValueError, match="no scenario table is set"):
        raw([0, 1, 1, 1], [[0, 5]], [0], [0], [0], [0.5])
    env.set_scenarios(_strip(FAULTS))
    with pytest.raises(ValueError, match=r"2 scenarios, the table that is set has 3"):
        raw([0, 1, 1], [[0, 5]], [0], [0], [0], [0.5])
    with pytest.raises(ValueError, match=r"scenario 1, fault item 0: element 20 out of range: the frame has 20 elements"):
        raw([0, 0, 1, 1], [[0, 5]], [20], [0], [0], [0.5])
    with pytest.raises(ValueError, match=r"fault item 0: element -1 out of range"):
        raw([0, 1, 1, 1], [[0, 5]], [-1], [0], [0], [0.5])
    with pytest.raises(ValueError, match=r"scenario 0, fault item 1: element 17 is a command word and is refused: the command words are the scenario's keyframes"):
        raw([0, 2, 2, 2], [[0, 5], [0, 5]], [0, 17], [0, 0], [0, 1], [0.5, 0.5])
    with pytest.raises(ValueError, match=r"fault item 0: unknown op 6 \(0 scale, 1 bias, 2 set, 3 noise, 4 hold, 5 drop\)"):
        raw([0, 1, 1, 1], [[0, 5]], [0], [6], [0], [0.5])
    with pytest.raises(ValueError, match=r"fault item 0: value is not finite"):
        raw([0, 1, 1, 1], [[0, 5]], [0], [1], [0], [np.nan])
    with pytest.raises(ValueError, match=r"fault item 0: a noise amplitude must be >= 0"):
        raw([0, 1, 1, 1], [[0, 5]], [0], [3], [0], [-1.0])
    with pytest.raises(ValueError, match=r"fault item 0: a drop probability must lie in \[0, 1\]"):
        raw([0, 1, 1, 1], [[0, 5]], [0], [5], [0], [1.25])
    with pytest.raises(ValueError, match=r"fault item 0: ordinal 256 outside 0..255"):
        raw([0, 1, 1, 1], [[0, 5]], [0], [1], [256], [1.0])
    with pytest.raises(ValueError, match=r"fault item 0: t1 5 is not after t0 5"):
        raw([0, 1, 1, 1], [[5, 5]], [0], [1], [0], [1.0])
    with pytest.raises(ValueError, match=r"fault item 0: times outside \[0, 2\^30\)"):
        raw([0, 1, 1, 1], [[-1, 5]], [0], [1], [0], [1.0])
    with pytest.raises(ValueError, match=r"scenario 0: 257 fault items, at most 256"):
        raw([0, 257, 257, 257], [[0, 5]] * 257, [0] * 257, [0] * 257, [0] * 257, [1.0] * 257)
    with pytest.raises(ValueError, match=r"the table holds no fault item"):
        raw([0, 0, 0, 0], np.zeros((0, 2)), [], [], [], [])
    with pytest.raises(ValueError, match=r"shorter than their row addresses"):
        raw([0, 3, 3, 3], [[0, 5]], [0], [0], [0], [0.5])
    with pytest.raises(ValueError, match=r"scenario 1: row addresses must not decrease"):   # caught before anything is read by them
        raw([0, 2, 1, 1], [[0, 5]], [0], [0], [0], [0.5])
    # the table travels as 32-bit words through cosim_set_param "obs_faults": a count that does not fit its own addresses is refused
    words = np.array([3, 0, 1, 1, 1, 0, 5, 0, 1, 0], i32)              # one item needs 3 + 2 + 6 words, these are 10
    with pytest.raises(ValueError, match=r"10 words, a table of 3 scenarios and 1 items takes 11"):
        env.engine._check(env.engine.L.cosim_set_param(env.engine.h, b"obs_faults", words.ctypes.data, int(words.size)))
    with pytest.raises(ValueError, match=r"3 words do not hold the row addresses of 3 scenarios"):
        env.engine._check(env.engine.L.cosim_set_param(env.engine.h, b"obs_faults", words.ctypes.data, 3))
    assert env.engine.query("obs_faults") == 0                      # nothing was set by a refused call
    with pytest.raises(ValueError, match=r"scenario 0, fault item 0: observation 'command' is refused"):
        env.set_scenarios([{"faults": [[0, 5, "command", 0, "bias", 2.0]]}])
    with pytest.raises(ValueError, match=r"scenario 0, fault item 0: unknown observation 'height_map'"):
        env.set_scenarios([{"faults": [[0, 5, "height_map", 0, "bias", 2.0]]}])
    env.set_scenarios(FAULTS)
    assert env.engine.query("obs_faults") > 0
    env.step(tb[0])
    with pytest.raises(ValueError, match="scenario table is set"):
        env.rollout(tb[1:3])
    env.step(tb[1])
    t.cuda.synchronize(env.device)
    assert np.isfinite(env.state.cpu().numpy()).all() and env.solver_stats()["step_count"] == n * 3   # the reset and two steps
    env.close()
    # hold / drop without a previous frame in the record: a fleet with one stack row
    cfg1, cm1 = _model("flamingo_light_v1", "flat", max_duration=0.5)
    cfg1 = copy.deepcopy(cfg1)
    cfg1["observation"]["stack_size"] = 1
    one = _env(cfg1, cm1, n, scenarios=_strip(FAULTS))
    with pytest.raises(ValueError, match=r"fault item 0: hold / drop needs a stacked element and stack_size >= 2: there is no previous frame in the record"):
        one.engine.scenario_faults_set((np.array([0, 1, 1, 1], i32), np.array([[0, 5]], i32), np.array([0], i32), np.array([4], i32), np.array([0], i32),
                                        np.array([0.0], f32)))
    with pytest.raises(ValueError, match=r"op 'drop' on 'dof_pos' needs a stacked observation and stack_size >= 2"):
        one.set_scenarios([{"faults": [[0, 5, "dof_pos", 0, "drop", 0.5]]}])
    one.close()


def _cli(tmp_path, capsys, *extra):
    import yaml
    from cosim_amd import cli
    scn, report = tmp_path / "scn.yaml", tmp_path / ("r%d.json" % len(extra))
    scn.write_text(yaml.safe_dump({"scenarios": FAULTS}))
    assert cli.main(["--env", "flamingo_light_v1", "--num-envs", "24", "--steps", "60", "--max-duration", "0.5", "--seed", "5", "--policy",
                     "random-mlp", "--scenarios", str(scn), "--scenario-mode", "cycle", *extra, "--ledger", "4", "--report", str(report)]) == 0
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    return json.loads(report.read_text()), line


@pytest.mark.parametrize("path", ["--graph", "--pipelined"])
def test_cli_faults_on_the_fast_paths(tmp_path, capsys, path):
    """The two closed-loop paths that cannot edit the observation between steps run a scenario file that holds faults; the report
    equals the eager run's."""
    if "eager" not in _CACHE:
        _CACHE["eager"] = _cli(tmp_path, capsys)
    eager, eline = _CACHE["eager"]
    r, line = _cli(tmp_path, capsys, path)
    by = r["episodes"]["by_scenario"]
    assert sorted(by) == ["0", "1", "2"] and sum(v["episodes"] for v in by.values()) == r["episodes"]["episodes"] >= 24
    assert by == eager["episodes"]["by_scenario"]
    assert line["obs_faults"] == eline["obs_faults"] == 22 and line["control_steps"] == 60
