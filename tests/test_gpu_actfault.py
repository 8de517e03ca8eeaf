"""Action faults of a scenario table on the device (cosim_set_param "action_faults", csrc/cosim_actfault.hip, and their BatchedEnv / CLI
surface) against a HOST-DRIVEN fleet: fleet A runs a table with action faults, fleet B the same table without them, and at each step B
is handed reference_action_faults (cosim_amd/scenario.py, the numpy twin) of A's raw actions.

Every comparison is EXACT: float32 bits for floats (uint32 views), ints as ints.  The flat fleet is 70 flamingo_light_v1 envs (a tail
in the last 4-wave block, uneven when split into ranges) over 40 steps; max_duration = 0.24 puts the time limit in episode step 12, so
every env ends three episodes inside the run.  What A and B must share: info rows, flags, every state_out word that is not a
last_action element, and the state records -- but for the last_action words of the record's frequency cache and observation stack,
which on A hold the policy's own output (checked against the roll of raw * el_scale frames, zeros after a reset) and on B what B was
handed.  Each test asserts that what it is about -- a window that opened and closed, a lost packet, a redone step -- happened."""
import json

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_CACHE = {}
CD = 4
BASE = np.array([0.5, 0.0, 0.0, 0.0], dtype=np.float32)
N, K, LIMIT = 70, 40, 12

# Three scenarios for flamingo_light_v1 (actuators 0..3); an episode's pre-step clock runs 0 .. 11, then 0 again.  All seven ops,
# overlapping items and "*":
#   0  a saturating output with a bias listed behind it, jitter on every set point, a stuck channel, lost packets, a dead channel
#   1  items that hold at episode step 0, where hold and drop are the identity; a scale behind a hold
#   2  no fault: these envs must be handed the caller's bits
FAULTS = [
    {"commands": [[0, 0.3, 0.1, 0.0, 0.0]], "pushes": [[6, 8, 0.3, 0.0, 0.0]],
     "action_faults": [[1, 9, "*", "clip", 0.4], [3, 7, 0, "bias", 0.25], [2, 11, "*", "noise", 0.05], [4, 8, 1, "hold", 0.0],
                       [2, 12, "*", "drop", 0.2], [9, 11, 2, "set", 0.0], [5, 6, 0, "scale", -1.0]]},
    {"action_faults": [[0, 3, "*", "hold", 0.0], [0, 12, 3, "drop", 1.0], [1, 5, 3, "scale", 0.5], [0, 1, 1, "noise", 0.5],
                       {"t0": 10, "t1": 13, "index": 0, "op": "set", "value": 0.25, "name": "stuck"}]},
    {"commands": [[4, 0.6, 0.0, 0.0, 0.0]]},
]


def _strip(scn):
    return [{k: v for k, v in s.items() if k != "action_faults"} for s in scn]


def _variant(scn):
    """The same item counts with other values and times: what an in-place rewrite uploads."""
    out = [dict(s) for s in scn]
    out[0] = dict(out[0], action_faults=[[0, 12, "*", "clip", 0.2], [1, 9, 0, "bias", -0.5], [0, 12, "*", "noise", 0.1], [2, 5, 1, "hold", 0.0],
                                         [0, 12, "*", "drop", 0.5], [3, 4, 2, "set", 1.0], [5, 9, 0, "scale", 2.0]])
    return out


def _model(robot, terrain="flat", gate=False, **kw):
    from cosim_amd.compile import compile_model
    from cosim_amd.config import make_config
    key = (robot, terrain, gate, json.dumps(kw, sort_keys=True))
    if key not in _CACHE:
        cfg = make_config(robot, terrain=terrain, **kw)
        if kw.get("position_command"):
            cfg["observation"]["command_dim"] = 2
        if gate:                                                    # last_action refreshed every other control step, and scaled
            cfg["observation"]["last_action"]["freq"] = cfg["observation"]["last_action"]["freq"] / 2
            cfg["observation"]["last_action"]["scale"] = 0.5
        _CACHE[key] = (cfg, compile_model(cfg))
    return _CACHE[key]


def _light(gate=False):
    return _model("flamingo_light_v1", "flat", gate=gate, max_duration=0.24)


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


def _table(env, scn):
    from cosim_amd.scenario import ScenarioTable
    names = {"action_faults": env.actuator_names()}
    if any("faults" in s for s in scn):
        names["faults"] = env.fault_names()
    return ScenarioTable(scn, env.command_dim, names=names)


class _LastAction:
    """Where last_action lies in this env's frame, and the frames a policy that sees its own output is shown: the roll of
    raw * el_scale, refreshed at the clocks that are due, zeros after a reset."""

    def __init__(self, env, cfg):
        names = env.fault_names()
        self.sd = sum(d for _, d in names["stacked"])
        self.S = env.stack_size
        e, self.e0, self.stacked = 0, None, False
        for stacked, lst in ((True, names["stacked"]), (False, names["non_stacked"])):
            for n, d in lst:
                if n == "last_action":
                    self.e0, self.dim, self.stacked = e, d, stacked
                e += d
        self.fd = e
        q = env.engine.query
        self.s_cache = q("nq") + 2 * q("nv") + 2 * q("action_dim") + 16
        self.s_stack = self.s_cache + self.fd
        self.stride = q("state_stride")
        if self.e0 is None:
            return
        ob = cfg["observation"]["last_action"]
        self.scale = np.float32(ob["scale"])
        self.interval = max(int(round(50 / ob["freq"])), 1)        # control steps per refresh (the control rate is 50 Hz)
        n = env.num_envs
        self.rows = np.zeros((n, self.S if self.stacked else 1, self.dim), dtype=np.float32)
        self.cache = np.zeros((n, self.dim), dtype=np.float32)

    def state_words(self):
        """Indices of the last_action words in a state_out row, per stack row."""
        if self.e0 is None:
            return np.zeros((0, 0), dtype=int)
        if self.stacked:
            return np.array([[r * self.sd + self.e0 + j for j in range(self.dim)] for r in range(self.S)])
        return np.array([[self.S * self.sd + self.e0 - self.sd + j for j in range(self.dim)]])

    def record_words(self):
        """Indices of the last_action words in a state record: the frequency cache and the observation stack."""
        if self.e0 is None:
            return np.zeros(0, dtype=int)
        w = [self.s_cache + self.e0 + j for j in range(self.dim)]
        if self.stacked:
            w += [self.s_stack + r * self.sd + self.e0 + j for r in range(self.S) for j in range(self.dim)]
        return np.array(w)

    def step(self, raw, t_post):
        """After a step handed ``raw`` that left the clocks ``t_post``: the expected words, [n, rows, dim]."""
        reset = t_post == 0
        due = (t_post % self.interval == 0) & ~reset
        v = (raw[:, :self.dim] * self.scale).astype(np.float32)
        self.cache = np.where(due[:, None], v, self.cache)
        self.cache[reset] = 0.0
        if self.stacked:
            self.rows[~reset, 1:] = self.rows[~reset, :-1].copy()
        self.rows[:, 0] = self.cache
        self.rows[reset] = 0.0
        return self.rows


def _parity(cfg, cm, n, raw, scn, mode="env", scn_b=None, setup=None, prepare=None, check_records=True, **env_kw):
    """The host-driven pair: A runs ``scn``, B ``scn_b`` (default: ``scn`` without the action faults) and is handed the twin's
    effective actions.  Returns what the run recorded."""
    from cosim_amd.scenario import reference_action_faults
    a = _env(cfg, cm, n, scenarios=scn, scenario_mode=mode, **env_kw)
    b = _env(cfg, cm, n, scenarios=scn_b if scn_b is not None else _strip(scn), scenario_mode=mode, **env_kw)
    table = _table(a, scn)
    t = a.torch
    la = _LastAction(a, cfg)
    assert la.e0 is not None and a.engine.query("action_faults") == table.n_action_fault_items > 0 and b.engine.query("action_faults") == 0
    assert b.effective_action() is None and sum(map(len, a.action_faults())) == table.n_action_fault_items
    sw, rw = la.state_words(), la.record_words()
    other = np.setdiff1d(np.arange(a.state_dim), sw.reshape(-1))
    if setup is not None:
        setup(a); setup(b)
    a.reset(); b.reset()
    if prepare is not None:
        prepare(a); prepare(b)
    gid = a.env_id0 + np.arange(n)
    prev = np.zeros((n, a.action_dim), dtype=np.float32)
    out = {"eff": [], "state": [], "info": [], "done": [], "meta": [], "table": table, "seed": a.seed, "la": la}
    for k in range(len(raw)):
        ma, mb = _meta(a), _meta(b)
        assert np.array_equal(ma[:, [0, 1, 2, 11]], mb[:, [0, 1, 2, 11]]), f"meta words differ ahead of step {k}"
        eff = reference_action_faults(table, mode, gid, ma[:, 0], ma[:, 11], ma[:, 1], a.seed, raw[k], prev)
        a.step(t.tensor(raw[k], device=a.device)); b.step(t.tensor(eff, device=b.device))
        a.join(); b.join()
        t.cuda.synchronize(a.device)
        got = a.effective_action().cpu().numpy()
        x, y = _u(got), _u(eff)
        assert np.array_equal(x, y), f"step {k}: effective action, envs {np.nonzero((x != y).any(axis=1))[0][:8]} (clocks {ma[:3, 0]})"
        sa, sb = a.state.cpu().numpy().copy(), b.state.cpu().numpy().copy()
        assert np.array_equal(_u(a.info_buf.cpu().numpy()), _u(b.info_buf.cpu().numpy())), f"step {k}: info rows"
        te, tr = a.terminated.cpu().numpy().astype(bool), a.truncated.cpu().numpy().astype(bool)
        assert np.array_equal(te, b.terminated.cpu().numpy().astype(bool)) and np.array_equal(tr, b.truncated.cpu().numpy().astype(bool)), f"step {k}: flags"
        assert np.array_equal(_u(sa[:, other]), _u(sb[:, other])), f"step {k}: state_out outside last_action"
        post = _meta(a)
        want = la.step(raw[k], post[:, 0])
        for r in range(sw.shape[0]):
            x, y = _u(sa[:, sw[r]]), _u(want[:, r])
            assert np.array_equal(x, y), f"step {k}: last_action, stack row {r}, envs {np.nonzero((x != y).any(axis=1))[0][:8]}"
        if check_records:
            ra, rb = a.snapshot().rows.cpu().numpy()[:, :la.stride].copy(), b.snapshot().rows.cpu().numpy()[:, :la.stride].copy()
            assert np.array_equal(_u(ra[:, la.s_cache + la.e0:la.s_cache + la.e0 + la.dim]), _u(la.cache)), f"step {k}: the record's cache"
            ra[:, rw] = 0.0; rb[:, rw] = 0.0
            assert np.array_equal(_u(ra), _u(rb)), f"step {k}: state records"
        done = te | tr
        prev = eff.copy()
        if a.auto_reset:
            prev[done] = 0.0                                        # the step ended the episode: the record holds zeros
        out["eff"].append(eff); out["state"].append(sa); out["info"].append(a.info_buf.cpu().numpy().copy()); out["done"].append(done)
        out["meta"].append(ma)
    out["a"], out["b"] = a, b
    return out


def _close(run):
    run["a"].close(); run["b"].close()


# ------------------------------------------------------------------------------------------------------------ 1: the host-driven fleet
@pytest.mark.parametrize("mode, gate", [("env", False), ("cycle", True)])
def test_parity_with_a_host_driven_fleet(mode, gate):
    cfg, cm = _light(gate)
    raw = _actions(N, K, 4)
    run = _parity(cfg, cm, N, raw, FAULTS, mode)
    a = run["a"]
    assert a.engine.query("action_faults") == 4 + 1 + 4 + 1 + 4 + 1 + 1 + 4 + 1 + 1 + 1 + 1
    assert run["la"].interval == (2 if gate else 1) and run["la"].scale == np.float32(0.5 if gate else 1.0)
    done, eff, meta = np.stack(run["done"]), np.stack(run["eff"]), np.stack(run["meta"])
    assert done[LIMIT - 1].all() and done.sum() >= 3 * N and (meta[LIMIT, :, 0] == 0).all() and (meta[LIMIT - 1, :, 0] == LIMIT - 1).all()
    gid = np.arange(N)
    s0, s1, s2 = (gid % 3 == r for r in range(3))
    changed = (_u(eff) != _u(raw)).any(axis=2)
    if mode == "env":
        assert not changed[:, s2].any()                             # scenario 2: the caller's bits throughout
        assert not changed[0, s0].any() and changed[1, s0].any()    # scenario 0's first window opens at clock 1
        assert (np.abs(eff[1][s0]) <= np.float32(0.4)).all() and (np.abs(raw[1][s0]) > 0.4).any()
        # the stuck channel of scenario 0 over [4, 8): frozen at the effective action of clock 3
        assert all(np.array_equal(_u(eff[k][s0, 1]), _u(eff[3][s0, 1])) for k in range(4, 8))
        # scenario 1's channel 3 (drop 1.0, hold over [0, 3)): step 0 is the caller's (the identity at episode step 0), halved from 1 on
        assert np.array_equal(_u(eff[0][s1, 3]), _u(raw[0][s1, 3])) and np.array_equal(_u(eff[1][s1, 3]), _u(eff[0][s1, 3] * np.float32(0.5)))
        # lost packets: all four set points of an env repeat the previous step's together, about one step in five
        lost = (eff[3:9, :, :] == eff[2:8, :, :])[:, s0][:, :, [2, 3]]
        assert (lost.all(axis=2) | ~lost.any(axis=2)).all() and 0.05 < lost.all(axis=2).mean() < 0.5
    else:
        assert changed[LIMIT + 2, s2].any() and not changed[:LIMIT, s2].any()   # scenario 2's envs run scenario 0 in their second episode
    # the policy sees its own output: where the bus changed the action, last_action still shows the raw one
    la = run["la"]
    assert changed[K - 1].any() and la.stacked and la.dim == 4
    _close(run)


# ------------------------------------------------------------------------------------------------------------ 2: drivers
def _eager(cfg, cm, n, raw, scn, mode, rewrite_at=None, **kw):
    env = _env(cfg, cm, n, scenarios=scn, scenario_mode=mode, **kw)
    return env, _drive(env, raw, rewrite_at=rewrite_at)


def _drive(env, raw, step=None, rewrite_at=None):
    t = env.torch
    tb = t.tensor(raw, device=env.device)
    items = env.engine.query("action_faults")
    env.reset()
    out = []
    for k in range(len(raw)):
        if k == rewrite_at:
            env.set_scenarios(_variant(FAULTS), env.scenario_mode)
            assert env.engine.query("action_faults") == items
        (step or (lambda k, a: env.step(a)))(k, tb[k])
        out.append(_observe(env))
    out.append((env.snapshot().rows.cpu().numpy().copy(),))
    return out


def _observe(env):
    env.join()
    env.torch.cuda.synchronize(env.device)
    return tuple(x.cpu().numpy().copy() for x in (env.state, env.info_buf, env.terminated, env.truncated, env.effective_action()))


def _same_run(a, b, what):
    assert len(a) == len(b)
    for k, (x, y) in enumerate(zip(a, b)):
        for i, (p, q) in enumerate(zip(x, y)):
            p, q = (_u(p), _u(q)) if p.dtype == np.float32 else (p, q)
            assert np.array_equal(p, q), f"{what}: step {k}, buffer {i} differs"


def test_ranges_deferred_join_and_step_range_chains_give_the_same_buffers():
    import torch
    cfg, cm = _light(True)
    raw = _actions(N, K, 4, seed=22)
    one, ref = _eager(cfg, cm, N, raw, FAULTS, "cycle")
    one.close()
    two, r2 = _eager(cfg, cm, N, raw, FAULTS, "cycle", ranges=2)
    counts = [c for _, c in two.range_list]
    assert two.engine.query("ranges") == 2 and sum(counts) == N and all(c % 4 for c in counts)   # 35 + 35: a tail block in each
    two.close()
    _same_run(ref, r2, "two uneven ranges")
    four, r4 = _eager(cfg, cm, N, raw, FAULTS, "cycle", ranges=4, deferred_join=True)
    assert four.engine.query("ranges") == 4
    four.close()
    _same_run(ref, r4, "four ranges, deferred join")
    d = _env(cfg, cm, N, scenarios=FAULTS, scenario_mode="cycle")
    streams = [torch.cuda.Stream(device=d.device) for _ in range(2)]

    def chains(k, act):
        torch.cuda.synchronize(d.device)
        for st, (first, count) in zip(streams, ((0, 30), (30, 40))):
            with torch.cuda.stream(st):
                d.step_range(first, count, act)
        torch.cuda.synchronize(d.device)
    _same_run(ref, _drive(d, raw, step=chains), "step_range chains")
    d.close()


def test_captured_step_and_in_place_rewrite_between_replays():
    """A captured step carries both launches and the effective-action pointer; items of the counts of the ones that are set are
    rewritten in place: the graph keeps its pointers and picks the new values up.  Against an eager run that rewrites at the same
    step."""
    import torch
    cfg, cm = _light()
    n, steps, at = 32, 26, 7
    raw = _actions(n, steps, 4, seed=23)
    e, ref = _eager(cfg, cm, n, raw, FAULTS, "env", rewrite_at=at)
    e.close()
    p, unre = _eager(cfg, cm, n, raw, FAULTS, "env")
    p.close()
    assert np.array_equal(_u(ref[at - 1][4]), _u(unre[at - 1][4])) and not np.array_equal(_u(ref[at + 1][4]), _u(unre[at + 1][4]))
    g = _env(cfg, cm, n, scenarios=FAULTS, scenario_mode="env")
    items = g.engine.query("action_faults")
    tb = torch.tensor(raw, device=g.device)
    buf = torch.empty((n, g.action_dim), device=g.device)
    g.reset()
    out = []
    buf.copy_(tb[0])
    side = torch.cuda.Stream(device=g.device)
    torch.cuda.synchronize(g.device)
    side.wait_stream(torch.cuda.current_stream(g.device))
    with torch.cuda.stream(side):
        g.step(buf)
    torch.cuda.current_stream(g.device).wait_stream(side)
    out.append(_observe(g))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g.step(buf)                                                 # recorded, not run: the launches are part of the graph
    for k in range(1, steps):
        if k == at:
            g.set_scenarios(_variant(FAULTS), "env")
            assert g.engine.query("action_faults") == items
        buf.copy_(tb[k])
        graph.replay()
        out.append(_observe(g))
    out.append((g.snapshot().rows.cpu().numpy().copy(),))
    g.close()
    _same_run(ref, out, "captured step, items rewritten in place")


# ------------------------------------------------------------------------------------------------------------ 3: other kernel paths
SMALL = [{"action_faults": [[0, 9, "*", "clip", 0.2], [1, 3, 0, "bias", 0.1], [1, 4, 1, "hold", 0.0], [0, 9, "*", "noise", 0.05]]},
         {"action_faults": [[1, 9, "*", "drop", 0.5], [2, 3, 2, "set", 0.1], [0, 2, 3, "scale", -1.0]]}]


def test_redone_steps_read_the_effective_action():
    """Drop poses with more than 14 contacts (the recipe of test_more_contacts_than_the_fleet_kernel_holds_are_redone_not_dropped):
    the fleet kernel gives such a step up and the 40-slot kernel redoes it from the same effective-action buffer."""
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
    raw = np.tile((0.3 * np.sin(np.arange(4))).astype(np.float32), (4, n, 1)) + _actions(n, 4, 4, seed=24) * np.float32(0.1)
    run = _parity(cfg, cm, n, raw, SMALL, prepare=lambda env: env.set_state(poses, np.zeros((n, cm.blob.nv)), np.zeros((n, cm.blob.nv))), auto_reset=False)
    a, b = run["a"], run["b"]
    assert a.engine.query("contact_slots") == 14 and a.engine.query("fixup_contact_slots") == 40
    sa, sb = a.solver_stats(), b.solver_stats()
    assert sa["fixup_steps"] > 0 and sa["fixup_steps"] == sb["fixup_steps"] and sa["dropped_contacts"] == 0
    assert (_u(np.stack(run["eff"])) != _u(raw)).any()
    _close(run)


def test_split_pipeline_with_and_without_the_heightfield_fixup():
    """humanoid_p_v0 on stairs_up_hard: the first substep's launch reads the effective action, the later ones what it computed; the
    restore runs behind the last substep's solver (and heightfield fix-up) launch."""
    cfg, cm = _model("humanoid_p_v0", "stairs_up_hard", max_duration=0.5, position_command=True)
    base = np.array([1.0, 0.5], dtype=np.float32)
    n, steps, nu = 16, 4, cm.blob.nu
    scn = [{"action_faults": [[0, 9, "*", "clip", 0.3], [1, 3, nu - 1, "bias", 0.1], [1, 4, 5, "hold", 0.0], [0, 9, "*", "noise", 0.05]]},
           {"action_faults": [[1, 9, "*", "drop", 0.5], [2, 3, 2, "set", 0.1], [0, 2, 3, "scale", -1.0]]}]
    raw = _actions(n, steps, nu, seed=25)
    for hfield_fixup in (False, True):
        run = _parity(cfg, cm, n, raw, scn, base=base, hfield_fixup=hfield_fixup)
        assert run["a"].engine.query("split") > 0 and (_u(np.stack(run["eff"])) != _u(raw)).any()
        _close(run)


def test_two_envs_per_wave_kernel():
    from cosim_amd.config import PARITY_RANDOM
    cfg, cm = _model("flamingo_light_v1", "flat", max_duration=0.24, random=PARITY_RANDOM)
    n = 32
    raw = _actions(n, 16, 4, seed=26)
    run = _parity(cfg, cm, n, raw, SMALL, "cycle", setup=lambda env: env.engine.set_param("envs_per_wave", np.array([2.0])))   # (raises where the variant is missing)
    assert np.stack(run["done"]).sum() >= n and (_u(np.stack(run["eff"])) != _u(raw)).any()
    _close(run)


# ------------------------------------------------------------------------------------------------------------ 4: with observation faults
def test_a_hold_fault_on_last_action_composes_on_the_restored_value():
    """A: action faults and observation faults; C: the action faults alone (its frames are the restored ones, test 1's check); B: the
    observation faults alone, handed the action twin's output.  A's observation is the observation twin's over C's frames."""
    from cosim_amd.scenario import fault_layout, reference_obs_faults
    cfg, cm = _light()
    n, steps = 24, 16
    obs = [[3, 8, "last_action", "*", "hold", 0.0], [5, 12, "last_action", 1, "bias", 0.5], [2, 6, "ang_vel", "*", "bias", 0.05]]
    both = [dict(FAULTS[0], faults=obs), dict(FAULTS[1], faults=obs[:1]), FAULTS[2]]
    raw = _actions(n, steps, 4, seed=27)
    run = _parity(cfg, cm, n, raw, [{k: v for k, v in s.items() if k != "faults"} for s in both], "env", check_records=False)
    clean = [s.copy() for s in run["state"]]
    metas = run["meta"]
    _close(run)
    from cosim_amd.scenario import reference_action_faults
    a = _env(cfg, cm, n, scenarios=both)
    b = _env(cfg, cm, n, scenarios=_strip(both))
    table = _table(a, both)
    lay = fault_layout(a.fault_names())
    t = a.torch
    a.reset(); b.reset()
    first = a.state.cpu().numpy().copy()
    post, got, prev = [_meta(a)], [first], np.zeros((n, 4), dtype=np.float32)
    for k in range(steps):
        m = _meta(a)
        assert np.array_equal(m[:, [0, 1, 11]], metas[k][:, [0, 1, 11]])
        eff = reference_action_faults(table, "env", np.arange(n), m[:, 0], m[:, 11], m[:, 1], a.seed, raw[k], prev)
        a.step(t.tensor(raw[k], device=a.device)); b.step(t.tensor(eff, device=b.device))
        t.cuda.synchronize(a.device)
        assert np.array_equal(_u(a.effective_action().cpu().numpy()), _u(eff))
        assert np.array_equal(_u(a.info_buf.cpu().numpy()), _u(b.info_buf.cpu().numpy())), k
        prev = eff.copy()
        prev[(a.terminated | a.truncated).cpu().numpy().astype(bool)] = 0.0
        post.append(_meta(a)); got.append(a.state.cpu().numpy().copy())
    post = np.stack(post)
    sd, S = lay["stacked_dim"], lay["stack_size"]
    frames = np.stack([np.concatenate([s[:, :sd], s[:, S * sd:]], axis=1) for s in [first] + clean])
    want = reference_obs_faults(table, "env", np.arange(n), post[:, :, 0], post[:, :, 11], post[:, :, 1], a.seed, frames, lay)
    for k in range(steps + 1):
        x, y = _u(got[k]), _u(want[k])
        assert np.array_equal(x, y), f"observation {k}: envs {np.nonzero((x != y).any(axis=1))[0][:8]}, words {np.nonzero((x != y).any(axis=0))[0][:12]}"
    s0 = np.arange(n) % 3 == 0
    held = [12, 14, 15]                                             # frozen at what the policy put out at clock 2; element 1 carries the bias listed behind
    assert np.array_equal(_u(got[5][s0][:, held]), _u(got[2][s0][:, held])) and (clean[4][s0][:, held] != got[5][s0][:, held]).any()
    assert np.array_equal(_u(got[5][s0, 13]), _u(got[2][s0, 13] + np.float32(0.5)))
    a.close(); b.close()


# ------------------------------------------------------------------------------------------------------------ 4b: the shared walk's chunk edges
def test_chunk_edges_of_the_shared_walk_under_both_kinds():
    """Rows of 1, 4 and 5 expanded items of EACH kind (csrc/cosim_fault.h fetches FLT_CHUNK = 4 records at a time: one row is a
    chunk, one a part of one, one a chunk and a part, and that one lies last, so its second fetch reads the array's zero padding),
    6 envs in mode cycle from env_id0 = 7, 12 steps with the time limit in episode step 8: clock 0, a reset's fill and a changed row
    all occur.  C runs the action faults alone: its effective actions are the action twin's, its observations the frames the
    observation twin starts from.  Everything expected of A, which runs both kinds, is computed from them on the host before A takes
    a step; every item is in force somewhere in it."""
    from cosim_amd.scenario import fault_layout, reference_action_faults, reference_obs_faults, scenario_rows
    cfg, cm = _model("flamingo_light_v1", "flat", max_duration=0.16)
    n, steps, id0 = 6, 12, 7
    scn = [
        {"action_faults": [[2, 7, 2, "bias", 0.1]],
         "faults": [[1, 6, "ang_vel", 0, "bias", 0.05]]},
        {"action_faults": [[0, 8, 0, "noise", 0.1], [1, 8, 1, "drop", 0.6], [3, 8, 2, "hold", 0.0], [0, 5, 3, "scale", -1.0]],
         "faults": [[0, 9, "ang_vel", 0, "noise", 0.05], [3, 9, "ang_vel", 1, "hold", 0.0], [1, 5, "ang_vel", 2, "drop", 0.6],
                    [2, 4, "last_action", 1, "bias", 0.5]]},
        {"action_faults": [[1, 8, "*", "drop", 0.5], [0, 3, 0, "clip", 0.2]],
         "faults": [[0, 9, "ang_vel", 0, "scale", 2.0], [0, 2, "ang_vel", 1, "set", 0.25], [2, 9, "ang_vel", 2, "drop", 0.5],
                    [1, 9, "last_action", 0, "hold", 0.0], [4, 7, "last_action", 3, "noise", 0.1]]},
    ]
    raw = _actions(n, steps, 4, seed=31)
    gid = id0 + np.arange(n)
    only_act = [{k: v for k, v in s.items() if k != "faults"} for s in scn]
    c = _env(cfg, cm, n, scenarios=only_act, scenario_mode="cycle", env_id0=id0)
    table = _table(c, scn)
    assert [len(f) for f in table.action_faults] == [1, 4, 5] and [len(f) for f in table.faults] == [1, 4, 5]
    lay = fault_layout(c.fault_names())
    t = c.torch
    c.reset()
    pre, post, clean, eff_c = [], [_meta(c)], [c.state.cpu().numpy().copy()], []
    for k in range(steps):
        pre.append(_meta(c))
        c.step(t.tensor(raw[k], device=c.device))
        t.cuda.synchronize(c.device)
        eff_c.append(c.effective_action().cpu().numpy().copy()); post.append(_meta(c)); clean.append(c.state.cpu().numpy().copy())
    c.close()
    pre, post = np.stack(pre), np.stack(post)
    assert (post[1:, :, 0] == 0).any() and (pre[:, :, 11] > 0).any(), "no episode ended inside the run"
    # the action twin, step by step as the record's s_lastact goes
    prev, want_eff = np.zeros((n, 4), dtype=np.float32), []
    for k in range(steps):
        want_eff.append(reference_action_faults(table, "cycle", gid, pre[k, :, 0], pre[k, :, 11], pre[k, :, 1], c.seed, raw[k], prev))
        prev = want_eff[-1].copy()
        prev[post[k + 1, :, 0] == 0] = 0.0                          # the step ended the episode: the record holds zeros
    for k in range(steps):
        assert np.array_equal(_u(eff_c[k]), _u(want_eff[k])), f"step {k}: effective action of the fleet without observation faults"
    sd, S = lay["stacked_dim"], lay["stack_size"]
    frames = np.stack([np.concatenate([s[:, :sd], s[:, S * sd:]], axis=1) for s in clean])
    want_obs = reference_obs_faults(table, "cycle", gid, post[:, :, 0], post[:, :, 11], post[:, :, 1], c.seed, frames, lay)
    # every item of either kind is in force on some (env, step): the clocks are the pre-step ones for actions, the observations' own for faults
    for items, clock, ep in ((table.action_faults, pre[:, :, 0], pre[:, :, 11]), (table.faults, post[:, :, 0], post[:, :, 11])):
        rows = np.stack([scenario_rows(3, "cycle", gid, e) for e in ep])
        assert len(np.unique(rows[:, 0])) > 1, "no env changed its row"
        for r, its in enumerate(items):
            for i, (t0, t1, *_) in enumerate(its):
                assert ((rows == r) & (t0 <= clock) & (clock < t1)).any(), f"row {r}, item {i} never holds"
    assert any((np.stack(want_eff) != raw).any(axis=(1, 2))) and (_u(want_obs) != _u(np.stack(clean))).any()
    a = _env(cfg, cm, n, scenarios=scn, scenario_mode="cycle", env_id0=id0)
    assert a.engine.query("action_faults") == 10 and a.engine.query("obs_faults") == 10
    a.reset()
    assert np.array_equal(_u(a.state.cpu().numpy()), _u(want_obs[0])), "the reset's observation"
    for k in range(steps):
        assert np.array_equal(_meta(a)[:, [0, 1, 11]], pre[k][:, [0, 1, 11]])
        a.step(t.tensor(raw[k], device=a.device))
        t.cuda.synchronize(a.device)
        x, y = _u(a.effective_action().cpu().numpy()), _u(want_eff[k])
        assert np.array_equal(x, y), f"step {k}: effective action, envs {np.nonzero((x != y).any(axis=1))[0]}"
        x, y = _u(a.state.cpu().numpy()), _u(want_obs[k + 1])
        assert np.array_equal(x, y), f"observation {k + 1}: envs {np.nonzero((x != y).any(axis=1))[0]}, words {np.nonzero((x != y).any(axis=0))[0][:12]}"
    a.close()


# ------------------------------------------------------------------------------------------------------------ 5: snapshot
def test_snapshot_inside_a_hold_window_continues_and_a_fork_follows_its_slot(tmp_path):
    from cosim_amd.scenario import reference_action_faults
    from cosim_amd.snapshot import Snapshot
    cfg, cm = _light()
    n = 24
    raw = _actions(n, 30, 4, seed=28)
    env = _env(cfg, cm, n, scenarios=FAULTS, scenario_mode="cycle")
    t = env.torch
    env.reset()
    for k in range(6):                                              # clock 6: inside scenario 0's hold [4, 8) and drop [2, 12) windows
        env.step(t.tensor(raw[k], device=env.device))
    at_snap = env.effective_action().cpu().numpy().copy()
    path = str(tmp_path / "snap.npz")
    env.snapshot().save(path)

    def go(e, k0, k1):
        out = []
        for k in range(k0, k1):
            e.step(t.tensor(raw[k], device=e.device))
            out.append(_observe(e))
        out.append((e.snapshot().rows.cpu().numpy().copy(),))
        return out
    a = go(env, 6, 30)
    env.close()
    fresh = _env(cfg, cm, n, scenarios=FAULTS, scenario_mode="cycle")   # the table is not part of the snapshot: set it again
    loaded = Snapshot.load(path, device=fresh.device)
    fresh.restore(loaded, params=True)
    b = go(fresh, 6, 30)
    _same_run(a, b, "restored")
    s0 = np.arange(n) % 3 == 0
    assert np.array_equal(_u(a[0][4][s0, 1]), _u(at_snap[s0, 1])) and np.array_equal(_u(a[1][4][s0, 1]), _u(at_snap[s0, 1]))   # frozen over the restore
    assert sum(int((x[2] | x[3]).astype(bool).sum()) for x in a[:-1]) >= n
    # a fork: every slot starts from row 0's state record and follows its OWN row and random streams
    fresh.fork(loaded, 0)
    m = _meta(fresh)
    assert (m[:, 0] == 6).all()
    want = reference_action_faults(_table(fresh, FAULTS), "cycle", np.arange(n), m[:, 0], m[:, 11], m[:, 1], fresh.seed, raw[6], np.tile(at_snap[:1], (n, 1)))
    fresh.step(t.tensor(raw[6], device=fresh.device))
    got = fresh.effective_action().cpu().numpy()
    assert np.array_equal(_u(got), _u(want)) and (got[s0, 1] == at_snap[0, 1]).all() and not np.array_equal(_u(got[0]), _u(got[3]))
    fresh.close()


# ------------------------------------------------------------------------------------------------------------ 6: ledger and traces
def test_ledger_and_traces_hold_the_effective_set_point_and_the_raw_action():
    from cosim_amd.ledger import same_records
    cfg, cm = _light()
    n, steps = 24, 30
    raw = _actions(n, steps, 4, seed=29)
    run = _parity(cfg, cm, n, raw, FAULTS, "cycle", check_records=False, ledger=4, failure_traces={"frames": 8, "keep": 4, "on": ("truncated",)})
    a, b = run["a"], run["b"]
    la_, lb_ = a.ledger(include_open=True), b.ledger(include_open=True)
    diff = same_records(la_, lb_)                                   # B was handed the twin's effective actions: the same action_diff_RMSE means
    assert diff is None, diff
    assert int(la_.ended().sum()) >= 2 * n
    ta, tb = a.failure_traces(include_open=True), b.failure_traces(include_open=True)
    assert len(ta) == len(tb) > 0 and np.array_equal(ta.headers, tb.headers) and np.array_equal(ta.env, tb.env)
    v = ta.valid
    assert np.array_equal(_u(ta.info[v]), _u(tb.info[v])) and np.array_equal(_u(ta.qpos[v]), _u(tb.qpos[v]))
    eff = np.stack(run["eff"])
    differ = 0
    for m_ in range(len(ta)):
        i = int(ta.env[m_])
        for f in np.nonzero(v[m_])[0]:
            ks = np.nonzero((_u(raw[:, i]) == _u(ta.action[m_, f])).all(axis=1))[0]
            assert len(ks) == 1, (m_, f)                            # the trace's action is the policy's own, the row of that step
            assert np.array_equal(_u(tb.action[m_, f]), _u(eff[ks[0], i]))
            differ += int(not np.array_equal(_u(ta.action[m_, f]), _u(tb.action[m_, f])))
    assert differ > 0
    _close(run)


# ------------------------------------------------------------------------------------------------------------ 7: off means off
def test_cleared_or_absent_faults_leave_no_trace():
    cfg, cm = _light()
    n = 32
    raw = _actions(n, 26, 4, seed=30)

    def observe(env):
        env.join()
        env.torch.cuda.synchronize(env.device)
        return tuple(x.cpu().numpy().copy() for x in (env.state, env.info_buf, env.terminated, env.truncated))

    def drive(env):
        tb = env.torch.tensor(raw, device=env.device)
        env.reset()
        out = []
        for k in range(len(raw)):
            env.step(tb[k])
            assert env.effective_action() is None
            out.append(observe(env))
        out.append((env.snapshot().rows.cpu().numpy().copy(),))
        return out
    y = _env(cfg, cm, n, scenarios=_strip(FAULTS))
    assert y.engine.query("action_faults") == 0 and y.action_faults() == [[], [], []] and y.effective_action() is None
    ref = drive(y)
    x = _env(cfg, cm, n, scenarios=FAULTS)
    assert x.engine.query("action_faults") > 0 and x.effective_action() is not None
    x.engine.scenario_action_faults_set(None)
    assert x.engine.query("action_faults") == 0 and x.engine.query("scenario_rows") == 3
    _same_run(ref, drive(x), "cleared")
    # a scenario table of another S drops the faults; the same S keeps them; clearing the table drops them
    x.set_scenarios(FAULTS)
    items = x.engine.query("action_faults")
    assert items > 0
    x.engine.scenario_set(x.scenario_table.pack(), 0, x._cmd_out.data_ptr(), x._row_out.data_ptr(), x._stream())
    assert x.engine.query("action_faults") == items
    x.set_scenarios(_strip(FAULTS))                                 # a table without faults clears what the earlier one left
    assert x.engine.query("action_faults") == 0 and x.action_faults() == [[], [], []]
    x.set_scenarios(FAULTS)
    x.set_scenarios(_strip(FAULTS)[:2])
    assert x.engine.query("scenario_rows") == 2 and x.engine.query("action_faults") == 0
    x.set_scenarios(FAULTS)
    x.set_scenarios(None)
    assert x.engine.query("scenario_rows") == 0 and x.engine.query("action_faults") == 0 and x.action_faults() == [] and x.effective_action() is None
    with pytest.raises(ValueError, match="no action faults are set"):
        x.engine.get("action_effective", x.state.data_ptr(), x._stream())
    x.close(); y.close()


# ------------------------------------------------------------------------------------------------------------ 8: refusals
def test_refusals_by_message_leave_the_env_stepping():
    cfg, cm = _light()
    n = 6
    raw = _actions(n, 4, 4, seed=31)
    env = _env(cfg, cm, n)
    t = env.torch
    tb = t.tensor(raw, device=env.device)
    env.reset()
    i32, f32 = np.int32, np.float32

    def csr(adr, tt, elem, op, ordinal, value):
        env.engine.scenario_action_faults_set((np.array(adr, i32), np.array(tt, i32).reshape(-1, 2), np.array(elem, i32), np.array(op, i32),
                                               np.array(ordinal, i32), np.array(value, f32)))
    with pytest.raises(ValueError, match=r'cosim_set_param "action_faults": no scenario table is set'):
        csr([0, 1, 1, 1], [[0, 5]], [0], [0], [0], [0.5])
    env.set_scenarios(_strip(FAULTS))
    with pytest.raises(ValueError, match=r"2 scenarios, the table that is set has 3"):
        csr([0, 1, 1], [[0, 5]], [0], [0], [0], [0.5])
    with pytest.raises(ValueError, match=r"scenario 1, action-fault item 0: actuator 4 out of range: the model has 4 actuators"):
        csr([0, 0, 1, 1], [[0, 5]], [4], [0], [0], [0.5])
    with pytest.raises(ValueError, match=r"action-fault item 0: actuator -1 out of range"):
        csr([0, 1, 1, 1], [[0, 5]], [-1], [0], [0], [0.5])
    with pytest.raises(ValueError, match=r"action-fault item 0: unknown op 7 \(0 scale, 1 bias, 2 set, 3 noise, 4 hold, 5 drop, 6 clip\)"):
        csr([0, 1, 1, 1], [[0, 5]], [0], [7], [0], [0.5])
    with pytest.raises(ValueError, match=r"action-fault item 0: value is not finite"):
        csr([0, 1, 1, 1], [[0, 5]], [0], [1], [0], [np.nan])
    with pytest.raises(ValueError, match=r"action-fault item 0: value is not finite"):
        csr([0, 1, 1, 1], [[0, 5]], [0], [2], [0], [np.inf])
    with pytest.raises(ValueError, match=r"action-fault item 0: a noise amplitude must be >= 0"):
        csr([0, 1, 1, 1], [[0, 5]], [0], [3], [0], [-1.0])
    with pytest.raises(ValueError, match=r"action-fault item 0: a clip bound must be >= 0"):
        csr([0, 1, 1, 1], [[0, 5]], [0], [6], [0], [-1.0])
    with pytest.raises(ValueError, match=r"action-fault item 0: a drop probability must lie in \[0, 1\]"):
        csr([0, 1, 1, 1], [[0, 5]], [0], [5], [0], [1.25])
    with pytest.raises(ValueError, match=r"action-fault item 0: t1 5 is not after t0 5"):
        csr([0, 1, 1, 1], [[5, 5]], [0], [1], [0], [1.0])
    with pytest.raises(ValueError, match=r"scenario 0: 257 action-fault items, at most 256"):
        csr([0, 257, 257, 257], [[0, 5]] * 257, [0] * 257, [0] * 257, [0] * 257, [1.0] * 257)
    with pytest.raises(ValueError, match=r"the table holds no action-fault item"):
        csr([0, 0, 0, 0], np.zeros((0, 2)), [], [], [], [])
    words = np.array([3, 0, 1, 1, 1, 0, 5, 0, 1, 0], i32)           # one item needs 3 + 2 + 6 words, these are 10
    with pytest.raises(ValueError, match=r"10 words, a table of 3 scenarios and 1 items takes 11"):
        env.engine._check(env.engine.L.cosim_set_param(env.engine.h, b"action_faults", words.ctypes.data, int(words.size)))
    assert env.engine.query("action_faults") == 0                   # nothing was set by a refused call
    with pytest.raises(ValueError, match=r"scenario 0, action-fault item 0: unknown actuator 'elbow'"):
        env.set_scenarios([{"action_faults": [[0, 5, "elbow", "bias", 2.0]]}])
    with pytest.raises(ValueError, match=r"scenario 0, action-fault item 0: index 4 out of range: the model has 4 actuators"):
        env.set_scenarios([{"action_faults": [[0, 5, 4, "bias", 2.0]]}])
    with pytest.raises(ValueError, match=r"scenario 0, action-fault item 0: unknown op 'halve'"):
        env.set_scenarios([{"action_faults": [[0, 5, 0, "halve", 2.0]]}])
    with pytest.raises(ValueError, match=r"scenario 0, action-fault item 0: non-finite value"):
        env.set_scenarios([{"action_faults": [[0, 5, 0, "bias", float("inf")]]}])
    with pytest.raises(ValueError, match=r"scenario 0, action-fault item 0: a drop probability must lie in \[0, 1\]"):
        env.set_scenarios([{"action_faults": [[0, 5, 0, "drop", 1.5]]}])
    with pytest.raises(ValueError, match=r"scenario 0: 260 action-fault items after expansion, at most 256"):
        env.set_scenarios([{"action_faults": [[0, 5, "*", "bias", 0.1]] * 65}])
    name = env.actuator_names()[2]
    env.set_scenarios([{"action_faults": [[0, 5, name, "set", 0.125]]}])
    assert env.action_faults() == [[(0, 5, 2, 2, 0, np.float32(0.125))]]
    env.set_scenarios(FAULTS)
    assert env.engine.query("action_faults") > 0
    env.step(tb[0])
    with pytest.raises(ValueError, match="scenario table is set"):
        env.rollout(tb[1:3])
    env.step(tb[1])
    t.cuda.synchronize(env.device)
    assert np.isfinite(env.state.cpu().numpy()).all() and env.solver_stats()["step_count"] == n * 3   # the reset and two steps
    env.close()


# ------------------------------------------------------------------------------------------------------------ 9: CLI
def _cli(tmp_path, capsys, *extra):
    import yaml
    from cosim_amd import cli
    scn, report = tmp_path / "scn.yaml", tmp_path / ("r%d.json" % len(extra))
    scn.write_text(yaml.safe_dump({"scenarios": FAULTS}))
    assert cli.main(["--env", "flamingo_light_v1", "--num-envs", "24", "--steps", "40", "--max-duration", "0.24", "--seed", "5", "--policy",
                     "random-mlp", "--scenarios", str(scn), "--scenario-mode", "cycle", *extra, "--ledger", "4", "--report", str(report)]) == 0
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    return json.loads(report.read_text()), line


def test_cli_prints_the_count_and_three_loops_give_one_ledger(tmp_path, capsys):
    eager, eline = _cli(tmp_path, capsys)
    assert eline["action_faults"] == 24 and "obs_faults" not in eline
    by = eager["episodes"]["by_scenario"]
    assert sorted(by) == ["0", "1", "2"] and sum(v["episodes"] for v in by.values()) == eager["episodes"]["episodes"] >= 48
    for path in ("--graph", "--pipelined"):
        r, line = _cli(tmp_path, capsys, path)
        assert line["action_faults"] == 24, path
        assert r["episodes"]["by_scenario"] == by and r["episodes"]["episodes"] == eager["episodes"]["episodes"], path
