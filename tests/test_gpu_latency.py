"""Latency lines of a scenario table on the device (cosim_set_param "latency", csrc/cosim_latency.hip, and their BatchedEnv / CLI
surface) against LatencyTwin (cosim_amd/scenario.py, the numpy twin) and HOST-DRIVEN fleets: for the command channel fleet A runs the
latency table and is handed the raw actions, fleet B runs the same table without latency and is handed the twin's delivered actions;
for observations every word of A's state is the twin's over the frames of a fleet that runs without latency.

Every comparison is EXACT: float32 bits for floats (uint32 views), ints as ints.  The shapes are those of tests/test_gpu_actfault.py: 70
flamingo_light_v1 envs on the plane (a tail in the last 4-wave block, uneven when split into ranges) over 40 steps, max_duration = 0.24
puts the time limit in episode step 12, actions from a fixed random table, so the physics does not depend on the observation."""
import json

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_CACHE = {}
BASE = np.array([0.5, 0.0, 0.0, 0.0], dtype=np.float32)
N, K, LIMIT = 70, 40, 12

# Action latency, depth 4 (the line wraps three times per episode): overlapping items, jitter 2, a delay-0 item, a row with no item.
ACT4 = [
    {"commands": [[0, 0.3, 0.1, 0.0, 0.0]], "pushes": [[6, 8, 0.3, 0.0, 0.0]],
     "latency": [[0, 100, "action", "*", 1, 2], [3, 9, "action", 0, 3], [5, 7, "action", 0, 0], [2, 11, "action", 3, 2, "slow_wheel"]]},
    {"latency": [[0, 100, "action", 2, 2], {"t0": 4, "t1": 8, "channel": "action", "index": 1, "steps": 1, "jitter": 2}]},
    {"commands": [[4, 0.6, 0.0, 0.0, 0.0]]},
]
# depth 13: a delay of the episode's length is never delivered; the others wrap inside it
ACT13 = [
    {"latency": [[0, 100, "action", "*", 12], [2, 8, "action", 1, 1, 2]]},
    {},
    {"commands": [[4, 0.6, 0.0, 0.0, 0.0]], "latency": [[0, 6, "action", "*", 2]]},
]
# Observation latency: a whole stacked field with jitter, one element of another listed behind it, ang_vel (moved behind the stack
# in the variant below), projected_gravity (observed at half the control rate)
OBS = [
    {"latency": [[0, 100, "dof_vel", "*", 1, 2], [3, 9, "dof_vel", 1, 3], [0, 100, "ang_vel", "*", 2], [1, 100, "projected_gravity", "*", 1]]},
    {},
    {"commands": [[4, 0.6, 0.0, 0.0, 0.0]], "latency": [[2, 100, "dof_pos", 0, 3], [0, 100, "ang_vel", 1, 1, 1]]},
]


def _strip(scn, key="latency"):
    return [{k: v for k, v in s.items() if k != key} for s in scn]


def _model(robot="flamingo_light_v1", terrain="flat", obs=None, **kw):
    from cosim_amd.compile import compile_model
    from cosim_amd.config import make_config
    key = (robot, terrain, obs, json.dumps(kw, sort_keys=True, default=str))
    if key not in _CACHE:
        cfg = make_config(robot, terrain=terrain, **kw)
        if kw.get("position_command"):
            cfg["observation"]["command_dim"] = 2
        o = cfg["observation"]
        if obs == "gate":                                           # last_action refreshed every other control step, and scaled
            o["last_action"]["freq"] = o["last_action"]["freq"] / 2
            o["last_action"]["scale"] = 0.5
        if obs in ("tail", "single"):                               # ang_vel behind the stack rows, projected_gravity at half the rate
            o["stacked_obs_order"] = [n for n in o["stacked_obs_order"] if n != "ang_vel"]
            o["non_stacked_obs_order"] = list(o["non_stacked_obs_order"]) + ["ang_vel"]
            o["projected_gravity"]["freq"] = o["projected_gravity"]["freq"] / 2
        if obs == "single":
            o["stack_size"] = 1
        _CACHE[key] = (cfg, compile_model(cfg))
    return _CACHE[key]


def _light(obs=None):
    return _model(obs=obs, max_duration=0.24)


def _env(cfg, cm, n, base=BASE, seed=3, **kw):
    from cosim_amd.batched_env import BatchedEnv
    kw.setdefault("auto_reset", True)
    env = BatchedEnv(cfg, num_envs=n, compiled=cm, seed=seed, **kw)
    env.receive_user_command(np.asarray(base, dtype=np.float32))
    return env


def _actions(n, steps, nu, seed=41):
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
    return ScenarioTable(scn, env.command_dim, names={"latency": (env.fault_names(), env.actuator_names()), "action_faults": env.actuator_names(),
                                                      "faults": env.fault_names()})


def _twin(env, scn, mode="env"):
    from cosim_amd.scenario import LatencyTwin
    return LatencyTwin(_table(env, scn), mode, env.env_id0 + np.arange(env.num_envs), env.seed, env.action_dim, env.engine.query("frame_dim"))


def _layout(env):
    from cosim_amd.scenario import fault_layout
    return fault_layout(env.fault_names())


def _frames(state, lay):
    sd, S = lay["stacked_dim"], lay["stack_size"]
    return np.concatenate([state[..., :sd], state[..., S * sd:]], axis=-1)


class _LastAction:
    """Where last_action lies in this env's frame, and the frames a policy that sees its own output is shown: the roll of
    raw * el_scale, refreshed at the clocks that are due, zeros after a reset (tests/test_gpu_actfault.py has the same rule)."""

    def __init__(self, env, cfg):
        names = env.fault_names()
        self.sd, self.S = sum(d for _, d in names["stacked"]), env.stack_size
        e, self.e0, self.dim = 0, None, 0
        for n, d in names["stacked"]:
            if n == "last_action":
                self.e0, self.dim = e, d
            e += d
        self.fd = e + sum(d for _, d in names["non_stacked"])
        q = env.engine.query
        self.s_cache = q("nq") + 2 * q("nv") + 2 * q("action_dim") + 16
        self.s_stack, self.stride = self.s_cache + self.fd, q("state_stride")
        if self.e0 is None:
            return
        ob = cfg["observation"]["last_action"]
        self.scale, self.interval = np.float32(ob["scale"]), max(int(round(50 / ob["freq"])), 1)
        self.rows = np.zeros((env.num_envs, self.S, self.dim), dtype=np.float32)
        self.cache = np.zeros((env.num_envs, self.dim), dtype=np.float32)

    def state_words(self):
        if self.e0 is None:
            return np.zeros((0, 0), dtype=int)
        return np.array([[r * self.sd + self.e0 + j for j in range(self.dim)] for r in range(self.S)])

    def record_words(self):
        if self.e0 is None:
            return np.zeros(0, dtype=int)
        return np.array([self.s_cache + self.e0 + j for j in range(self.dim)] +
                        [self.s_stack + r * self.sd + self.e0 + j for r in range(self.S) for j in range(self.dim)])

    def step(self, raw, t_post):
        if self.e0 is None:
            return None
        reset = t_post == 0
        due = (t_post % self.interval == 0) & ~reset
        self.cache = np.where(due[:, None], (raw[:, :self.dim] * self.scale).astype(np.float32), self.cache)
        self.cache[reset] = 0.0
        self.rows[~reset, 1:] = self.rows[~reset, :-1].copy()
        self.rows[:, 0] = self.cache
        self.rows[reset] = 0.0
        return self.rows


def _parity(cfg, cm, n, raw, scn, mode="env", scn_b=None, deliver=None, setup=None, prepare=None, cut=None, **env_kw):
    """The host-driven pair: A runs ``scn`` and is handed ``raw``, B runs ``scn_b`` (default: ``scn`` without the latency) and is
    handed ``deliver(k, metaA, delivered)`` (default: the twin's delivered actions).  ``cut(k, a, b, twin)`` runs ahead of step k."""
    a = _env(cfg, cm, n, scenarios=scn, scenario_mode=mode, **env_kw)
    b = _env(cfg, cm, n, scenarios=scn_b if scn_b is not None else _strip(scn), scenario_mode=mode, **env_kw)
    tw = _twin(a, scn, mode)
    t = a.torch
    la = _LastAction(a, cfg)
    items = tw.table.n_latency_items
    assert a.engine.query("latency") == items > 0 and b.engine.query("latency") == 0 and sum(map(len, a.latency())) == items and b.latency() == [[]] * len(scn)
    assert a.engine.query("latency_depth") == tw.D
    sw, rw = la.state_words(), la.record_words()
    other = np.setdiff1d(np.arange(a.state_dim), sw.reshape(-1))
    if setup is not None:
        setup(a); setup(b)
    a.reset(); b.reset()
    if prepare is not None:
        prepare(a); prepare(b); tw.cut()
    out = {"eff": [], "done": [], "meta": [], "twin": tw, "la": la}
    for k in range(len(raw)):
        if cut is not None:
            cut(k, a, b, tw)
        ma, mb = _meta(a), _meta(b)
        assert np.array_equal(ma[:, [0, 1, 2, 11]], mb[:, [0, 1, 2, 11]]), f"meta words differ ahead of step {k}"
        eff = tw.step_actions(raw[k], ma[:, 0], ma[:, 11], ma[:, 1])
        fed = eff if deliver is None else deliver(k, ma, eff)
        a.step(t.tensor(raw[k], device=a.device)); b.step(t.tensor(fed, device=b.device))
        a.join(); b.join()
        t.cuda.synchronize(a.device)
        want = fed if b.effective_action() is None else b.effective_action().cpu().numpy()
        x, y = _u(a.effective_action().cpu().numpy()), _u(want)
        assert np.array_equal(x, y), f"step {k}: effective action, envs {np.nonzero((x != y).any(axis=1))[0][:8]} (clocks {ma[:3, 0]})"
        sa, sb = a.state.cpu().numpy().copy(), b.state.cpu().numpy().copy()
        assert np.array_equal(_u(a.info_buf.cpu().numpy()), _u(b.info_buf.cpu().numpy())), f"step {k}: info rows"
        te, tr = a.terminated.cpu().numpy().astype(bool), a.truncated.cpu().numpy().astype(bool)
        assert np.array_equal(te, b.terminated.cpu().numpy().astype(bool)) and np.array_equal(tr, b.truncated.cpu().numpy().astype(bool)), f"step {k}: flags"
        assert np.array_equal(_u(sa[:, other]), _u(sb[:, other])), f"step {k}: state_out outside last_action"
        rows = la.step(raw[k], _meta(a)[:, 0])
        if cut is None and prepare is None:                         # (a cut leaves the restored rows in the stack: not this rule's)
            for r in range(sw.shape[0]):
                x, y = _u(sa[:, sw[r]]), _u(rows[:, r])
                assert np.array_equal(x, y), f"step {k}: last_action, stack row {r}, envs {np.nonzero((x != y).any(axis=1))[0][:8]}"
        ra, rb = a.snapshot().rows.cpu().numpy()[:, :la.stride].copy(), b.snapshot().rows.cpu().numpy()[:, :la.stride].copy()
        ra[:, rw] = 0.0; rb[:, rw] = 0.0
        assert np.array_equal(_u(ra), _u(rb)), f"step {k}: state records"
        out["eff"].append(eff); out["done"].append(te | tr); out["meta"].append(ma)
    out["a"], out["b"] = a, b
    return out


def _close(run):
    run["a"].close(); run["b"].close()


# ------------------------------------------------------------------------------------------------------------ 1: action parity
@pytest.mark.parametrize("mode, obs, scn", [("env", None, ACT4), ("cycle", "gate", ACT13)], ids=["env-depth4", "cycle-depth13"])
def test_action_parity_with_a_host_driven_fleet(mode, obs, scn):
    cfg, cm = _light(obs)
    raw = _actions(N, K, 4)
    run = _parity(cfg, cm, N, raw, scn, mode)
    eff, done, meta = np.stack(run["eff"]), np.stack(run["done"]), np.stack(run["meta"])
    assert done[LIMIT - 1].all() and done.sum() >= 3 * N and (meta[LIMIT, :, 0] == 0).all()
    s0, s1, s2 = (np.arange(N) % 3 == r for r in range(3))
    changed = (_u(eff) != _u(raw)).any(axis=2)
    if mode == "env":
        assert run["twin"].D == 4 and not changed[:, s2].any() and changed[:, s0].all() and changed[:, s1].all()
        assert (eff[0][s0] == 0).all() and (eff[LIMIT][s0] == 0).all()           # nothing has arrived yet, after every reset
        assert np.array_equal(_u(eff[2][s1, 2]), _u(raw[0][s1, 2])) and np.array_equal(_u(eff[6][s0, 0]), _u(raw[6][s0, 0]))   # two steps late; the delay-0 item wins
        late = np.stack([(_u(eff[5][s0][:, 1:3]) == _u(raw[5 - d][s0][:, 1:3])).all(axis=1) for d in (1, 2, 3)])
        assert (late.sum(axis=0) >= 1).all() and (late.sum(axis=1) > 0).all()   # jitter: every env one of the three, every one somewhere
    else:
        assert run["twin"].D == 13 and run["la"].interval == 2
        assert (eff[:LIMIT, s0][:, :, [0, 2, 3]] == 0).all()        # a delay of the episode's length is never delivered
        assert changed[LIMIT + 3, s1].any() and not changed[:LIMIT, s1].any()   # scenario 1's envs run scenario 2 in their second episode
    _close(run)


# ------------------------------------------------------------------------------------------------------------ 2: observation parity
def _drive_obs(env, raw, reset_at=None, reset_mask=None, step=None):
    """The reset's observation and one per step: (state rows, post metas, active masks)."""
    t = env.torch
    tb = t.tensor(raw, device=env.device)
    env.reset()
    env.join(); t.cuda.synchronize(env.device)
    states, metas, active = [env.state.cpu().numpy().copy()], [_meta(env)], [np.ones(env.num_envs, dtype=bool)]
    extra = []
    for k in range(len(raw)):
        if k == reset_at:
            env.reset(mask=reset_mask)
            env.join(); t.cuda.synchronize(env.device)
            states.append(env.state.cpu().numpy().copy()); metas.append(_meta(env)); active.append(np.asarray(reset_mask, dtype=bool))
        (step or (lambda k, a: env.step(a)))(k, tb[k])
        env.join(); t.cuda.synchronize(env.device)
        states.append(env.state.cpu().numpy().copy()); metas.append(_meta(env)); active.append(np.ones(env.num_envs, dtype=bool))
        extra.append(tuple(x.cpu().numpy().copy() for x in (env.info_buf, env.terminated, env.truncated)))
    return np.stack(states), np.stack(metas), np.stack(active), extra


def _twin_states(env, scn, mode, clean_states, metas, active, cut_at=None, cut_mask=None):
    """The state_out rows the twins work out from a latency-free run's: LatencyTwin delivers the newest frames, reference_obs_faults
    (the table's faults, if any, on top) emulates the stack's roll and fill."""
    from cosim_amd.scenario import reference_obs_faults
    lay = _layout(env)
    tw = _twin(env, scn, mode)
    frames = _frames(clean_states, lay)
    out = []
    for k in range(len(frames)):
        if k == cut_at:
            tw.cut(cut_mask)
        out.append(tw.step_obs(frames[k], metas[k, :, 0], metas[k, :, 11], metas[k, :, 1], active=active[k]))
    gid = env.env_id0 + np.arange(env.num_envs)
    return reference_obs_faults(tw.table, mode, gid, metas[:, :, 0], metas[:, :, 11], metas[:, :, 1], env.seed, np.stack(out), lay, active=active)


def _same_words(got, want, what):
    for k in range(len(want)):
        x, y = _u(got[k]), _u(want[k])
        assert np.array_equal(x, y), f"{what}: observation {k}: envs {np.nonzero((x != y).any(axis=1))[0][:8]}, words {np.nonzero((x != y).any(axis=0))[0][:12]}"


@pytest.mark.parametrize("obs, mode", [("tail", "cycle"), ("single", "env")], ids=["stack3-cycle", "stack1-env"])
def test_observation_parity_with_the_twin(obs, mode):
    """ang_vel lies behind the stack rows (a non-stacked element), projected_gravity is observed at half the control rate, dof_vel
    and dof_pos are stacked; stack_size 3 and 1."""
    cfg, cm = _light(obs)
    raw = _actions(N, K, 4, seed=42)
    c = _env(cfg, cm, N, scenarios=_strip(OBS), scenario_mode=mode)
    lay = _layout(c)
    assert lay["stack_size"] == (1 if obs == "single" else 3) and c.fault_names()["non_stacked"][-1] == ("ang_vel", 3)
    clean, metas, active, extra_c = _drive_obs(c, raw)
    c.close()
    a = _env(cfg, cm, N, scenarios=OBS, scenario_mode=mode)
    assert a.engine.query("latency_obs_items") == a.engine.query("latency") == 4 + 1 + 3 + 3 + 1 + 1 and a.effective_action() is None
    want = _twin_states(a, OBS, mode, clean, metas, active)
    got, metas_a, _, extra_a = _drive_obs(a, raw)
    a.close()
    assert np.array_equal(metas_a, metas)
    for x, y in zip(extra_a, extra_c):
        assert all(np.array_equal(p.view(np.uint8), q.view(np.uint8)) for p, q in zip(x, y)), "the physics changed"
    _same_words(got, want, "state")
    differ = (_u(got) != _u(clean)).any(axis=2)
    assert not differ[metas[:, :, 0] == 0].any() and differ[metas[:, :, 0] > 1].mean() > 0.5   # a fill (the reset's, an episode's first) is untouched
    sd, S = lay["stacked_dim"], lay["stack_size"]
    s0 = np.arange(N) % 3 == 0
    tail = S * sd + 4                                               # ang_vel behind the command words
    assert np.array_equal(_u(got[5][s0, tail:tail + 3]), _u(clean[3][s0, tail:tail + 3]))   # two observations late
    assert np.array_equal(_u(got[1][s0, tail:tail + 3]), _u(clean[0][s0, tail:tail + 3]))   # the channel is full of its first reading


# ------------------------------------------------------------------------------------------------------------ 3: composition with faults
def test_latency_composes_under_action_faults_and_observation_faults():
    """Latency first: the action faults take the delivered action as their x (B runs the action faults alone and is handed the
    latency twin's output), the observation faults the delivered newest frame (twin of twin); last_action stays the policy's own."""
    cfg, cm = _light()
    n, steps = 24, 26
    af = [[1, 9, "*", "clip", 0.4], [4, 8, 1, "hold", 0.0], [2, 12, "*", "drop", 0.3]]
    both = [dict(ACT4[0], action_faults=af), dict(ACT4[1], action_faults=af[1:]), ACT4[2]]
    raw = _actions(n, steps, 4, seed=43)
    run = _parity(cfg, cm, n, raw, both, "env", scn_b=_strip(both))
    a, b = run["a"], run["b"]
    assert a.engine.query("action_faults") == b.engine.query("action_faults") > 0
    assert (_u(np.stack(run["eff"])) != _u(raw)).any()
    _close(run)
    # observations: latency and hold / noise faults over the same elements
    of = [[2, 9, "dof_vel", "*", "hold", 0.0], [0, 12, "ang_vel", "*", "noise", 0.05], [3, 6, "dof_vel", 1, "bias", 0.5]]
    scn = [dict(OBS[0], faults=of), dict(OBS[1], faults=of[1:]), dict(OBS[2], faults=of[:1])]
    c = _env(cfg, cm, n, scenarios=_strip(_strip(scn), "faults"))
    clean, metas, active, _ = _drive_obs(c, raw)
    c.close()
    a = _env(cfg, cm, n, scenarios=scn)
    assert a.engine.query("obs_faults") > 0 and a.engine.query("latency") > 0
    want = _twin_states(a, scn, "env", clean, metas, active)
    only_faults = _twin_states(a, _strip(scn), "env", clean, metas, active)
    got, _, _, _ = _drive_obs(a, raw)
    a.close()
    _same_words(got, want, "latency under faults")
    assert (_u(want) != _u(only_faults)).any()


# ------------------------------------------------------------------------------------------------------------ 4: launch shapes
BOTH = [dict(ACT4[0], latency=ACT4[0]["latency"] + OBS[0]["latency"]), dict(ACT4[1], latency=ACT4[1]["latency"]), dict(ACT4[2], latency=OBS[2]["latency"])]


def _variant(scn):
    """The same row addresses with other delays and windows, none above the depth: what an in-place rewrite uploads."""
    out = [dict(s) for s in scn]
    out[0] = dict(out[0], latency=[[0, 100, "action", "*", 2, 1], [1, 5, "action", 0, 1], [0, 100, "action", 0, 3], [0, 100, "action", 3, 0, "slow_wheel"],
                                   [0, 100, "dof_vel", "*", 3], [0, 100, "dof_vel", 1, 0], [2, 100, "ang_vel", "*", 1, 1], [0, 100, "projected_gravity", "*", 2]])
    return out


def _observe(env):
    env.join()
    env.torch.cuda.synchronize(env.device)
    return tuple(x.cpu().numpy().copy() for x in (env.state, env.info_buf, env.terminated, env.truncated, env.effective_action()))


def _drive(env, raw, step=None, rewrite_at=None, rewrite=None):
    tb = env.torch.tensor(raw, device=env.device)
    env.reset()
    out = []
    for k in range(len(raw)):
        if k == rewrite_at:
            rewrite(env)
        (step or (lambda k, a: env.step(a)))(k, tb[k])
        out.append(_observe(env))
    out.append((env.snapshot().rows.cpu().numpy().copy(),))
    return out


def _same_run(a, b, what):
    assert len(a) == len(b)
    for k, (x, y) in enumerate(zip(a, b)):
        for i, (p, q) in enumerate(zip(x, y)):
            p, q = (_u(p), _u(q)) if p.dtype == np.float32 else (p, q)
            assert np.array_equal(p, q), f"{what}: step {k}, buffer {i} differs"


def test_ranges_deferred_join_and_step_range_chains_give_the_same_buffers():
    import torch
    cfg, cm = _light("gate")
    raw = _actions(N, K, 4, seed=44)
    one = _env(cfg, cm, N, scenarios=BOTH, scenario_mode="cycle")
    ref = _drive(one, raw)
    one.close()
    two = _env(cfg, cm, N, scenarios=BOTH, scenario_mode="cycle", ranges=2)
    assert two.engine.query("ranges") == 2 and all(c % 4 for _, c in two.range_list)
    _same_run(ref, _drive(two, raw), "two uneven ranges")
    two.close()
    four = _env(cfg, cm, N, scenarios=BOTH, scenario_mode="cycle", ranges=4, deferred_join=True)
    _same_run(ref, _drive(four, raw), "four ranges, deferred join")
    four.close()
    d = _env(cfg, cm, N, scenarios=BOTH, scenario_mode="cycle")
    streams = [torch.cuda.Stream(device=d.device) for _ in range(2)]

    def chains(k, act):
        torch.cuda.synchronize(d.device)
        for st, (first, count) in zip(streams, ((0, 30), (30, 40))):
            with torch.cuda.stream(st):
                d.step_range(first, count, act)
        torch.cuda.synchronize(d.device)
    _same_run(ref, _drive(d, raw, step=chains), "step_range chains")
    d.close()


def test_captured_step_in_place_rewrite_and_a_deeper_table_outside_the_capture():
    """A captured step carries the latency launches and the pointers of the lines; a table with the row addresses of the one that is
    set whose delays fit the depth is rewritten in place, the lines kept: the graph picks it up.  A table that needs a deeper line
    is a fresh allocation: set outside a capture, it restarts every line."""
    import torch
    cfg, cm = _light()
    n, steps, at = 32, 26, 7
    raw = _actions(n, steps, 4, seed=45)
    rewrite = lambda env: env.set_scenarios(_variant(BOTH), "env")   # noqa: E731
    e = _env(cfg, cm, n, scenarios=BOTH, scenario_mode="env")
    ref = _drive(e, raw, rewrite_at=at, rewrite=rewrite)
    assert e.engine.query("latency_depth") == 4
    e.close()
    p = _env(cfg, cm, n, scenarios=BOTH, scenario_mode="env")
    unre = _drive(p, raw)
    p.close()
    assert np.array_equal(_u(ref[at - 1][4]), _u(unre[at - 1][4])) and not np.array_equal(_u(ref[at + 1][4]), _u(unre[at + 1][4]))
    g = _env(cfg, cm, n, scenarios=BOTH, scenario_mode="env")
    items = g.engine.query("latency")
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
            rewrite(g)
            assert g.engine.query("latency") == items and g.engine.query("latency_depth") == 4
        buf.copy_(tb[k])
        graph.replay()
        out.append(_observe(g))
    out.append((g.snapshot().rows.cpu().numpy().copy(),))
    _same_run(ref, out, "captured step, items rewritten in place")
    # the in-place rewrite kept the lines: the variant's three-step delay of actuator 0 delivers, at the step of the rewrite, a word
    # that was written to the line under the earlier table
    s0 = np.arange(n) % 3 == 0
    assert np.array_equal(_u(out[at][4][s0, 0]), _u(raw[at - 3][s0, 0])) and np.array_equal(_u(out[at + 1][4][s0, 0]), _u(raw[at - 2][s0, 0]))
    # a deeper table: a fresh allocation, every line restarts where it is set
    deeper = [dict(BOTH[0], latency=[[0, 100, "action", "*", 6]]), BOTH[1], BOTH[2]]
    g.set_scenarios(deeper, "env")
    assert g.engine.query("latency_depth") == 7
    mk = _meta(g)
    assert (mk[:, 0] == steps % LIMIT).all() and steps % LIMIT > 0
    g.step(tb[0])
    eff = g.effective_action().cpu().numpy()
    assert np.array_equal(_u(eff[s0]), _u(raw[0][s0]))            # restarted in mid-episode: the first word after the restart
    g.close()


# ------------------------------------------------------------------------------------------------------------ 5: other kernel paths
SMALL = [{"latency": [[1, 9, "action", "*", 1], [2, 4, "action", 0, 2, 1]]},{"latency": [[1, 9, "action", 2, 2], [0, 2, "action", 3, 0, 3]]}]


def test_redone_steps_read_the_delivered_action():
    """Drop poses with more than 14 contacts (the recipe of tests/test_gpu_actfault.py): the fleet kernel gives such a step up and
    the 40-slot kernel redoes it from the same delivered-action buffer."""
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
    raw = np.tile((0.3 * np.sin(np.arange(4))).astype(np.float32), (4, n, 1)) + _actions(n, 4, 4, seed=46) * np.float32(0.1)
    run = _parity(cfg, cm, n, raw, SMALL, prepare=lambda env: env.set_state(poses, np.zeros((n, cm.blob.nv)), np.zeros((n, cm.blob.nv))), auto_reset=False)
    a, b = run["a"], run["b"]
    sa, sb = a.solver_stats(), b.solver_stats()
    assert sa["fixup_steps"] > 0 and sa["fixup_steps"] == sb["fixup_steps"] and sa["dropped_contacts"] == 0
    assert (_u(np.stack(run["eff"])) != _u(raw)).any()
    _close(run)


def test_two_envs_per_wave_kernel():
    from cosim_amd.config import PARITY_RANDOM
    cfg, cm = _model(max_duration=0.24, random=PARITY_RANDOM)
    n = 32
    raw = _actions(n, 16, 4, seed=47)
    run = _parity(cfg, cm, n, raw, SMALL, "cycle", setup=lambda env: env.engine.set_param("envs_per_wave", np.array([2.0])))
    assert np.stack(run["done"]).sum() >= n and (_u(np.stack(run["eff"])) != _u(raw)).any()
    _close(run)


def test_split_pipeline():
    cfg, cm = _model("humanoid_p_v0", "stairs_up_hard", max_duration=0.5, position_command=True)
    n, steps, nu = 8, 4, cm.blob.nu
    scn = [{"latency": [[0, 9, "action", "*", 1], [1, 3, "action", nu - 1, 2, 1]]}, {"latency": [[1, 9, "action", 2, 2]]}]
    raw = _actions(n, steps, nu, seed=48)
    run = _parity(cfg, cm, n, raw, scn, base=np.array([1.0, 0.5], dtype=np.float32))
    assert run["a"].engine.query("split") > 0 and (_u(np.stack(run["eff"])) != _u(raw)).any()
    _close(run)


# ------------------------------------------------------------------------------------------------------------ 6: host cuts
def test_masked_reset_restore_and_fork_equal_the_twin_with_a_cut():
    cfg, cm = _light()
    n, steps = 24, 20
    raw = _actions(n, steps, 4, seed=49)
    mask = np.arange(n) % 4 == 1
    s0 = np.arange(n) % 3 == 0
    # a masked reset in mid-episode, observations: clock 0 restarts the masked envs' lines, the others are untouched
    c = _env(cfg, cm, n, scenarios=_strip(OBS))
    clean, metas, active, _ = _drive_obs(c, raw, reset_at=5, reset_mask=mask)
    c.close()
    a = _env(cfg, cm, n, scenarios=OBS)
    want = _twin_states(a, OBS, "env", clean, metas, active)
    got, metas_a, _, _ = _drive_obs(a, raw, reset_at=5, reset_mask=mask)
    a.close()
    assert np.array_equal(metas_a, metas) and (metas[6][mask, 0] == 0).all() and (metas[6][~mask, 0] == 5).all()
    _same_words(got, want, "masked reset")
    assert (_u(got[7]) != _u(clean[7])).any(axis=1)[~mask & s0].all()
    # ... and actions: nothing has arrived yet on the masked envs, the others go on
    def reset_at_5(k, x, y, tw):
        if k == 5:
            x.reset(mask=mask); y.reset(mask=mask)
    run = _parity(cfg, cm, n, raw, ACT4, cut=reset_at_5)
    eff = np.stack(run["eff"])
    assert (eff[5][mask & s0] == 0).all() and (eff[5][~mask & s0] != 0).any()
    _close(run)

    # restore and fork on fresh fleets, against a latency-free pair driven the same way
    def cut_run(do):
        c = _env(cfg, cm, n, scenarios=_strip(BOTH))
        x = _env(cfg, cm, n, scenarios=BOTH)
        twin = _twin(x, BOTH)
        tc, frames, mts, got_s, got_e, want_e = c.torch, [], [], [], [], []

        def both(fn):
            fn(c); fn(x)
        both(lambda e: e.reset())
        frames.append(c.state.cpu().numpy().copy()); mts.append(_meta(c)); got_s.append(x.state.cpu().numpy().copy())
        snaps = {}
        cuts = {}
        for k in range(steps):
            if k == 6:
                snaps["c"], snaps["x"] = c.snapshot(), x.snapshot()
            if k == 10:
                cm_ = do(c, snaps["c"]); do(x, snaps["x"])
                cm_, src_ = cm_
                twin.cut(cm_)
                cuts[len(frames)] = (cm_, src_)
            m = _meta(x)
            want_e.append(twin.step_actions(raw[k], m[:, 0], m[:, 11], m[:, 1]))
            c.step(tc.tensor(want_e[-1], device=c.device)); x.step(tc.tensor(raw[k], device=x.device))
            tc.cuda.synchronize(c.device)
            got_e.append(x.effective_action().cpu().numpy())
            frames.append(c.state.cpu().numpy().copy()); mts.append(_meta(c)); got_s.append(x.state.cpu().numpy().copy())
            assert np.array_equal(_meta(x)[:, [0, 1, 11]], mts[-1][:, [0, 1, 11]])
        c.close(); x.close()
        return np.stack(frames), np.stack(mts), np.stack(got_s), np.stack(got_e), np.stack(want_e), cuts

    def restore_masked(env, snap):
        env.restore(snap, mask=env.torch.tensor(mask, device=env.device))
        return mask, np.arange(n)

    def fork_row(env, snap):
        env.fork(snap, 3)
        return np.ones(n, dtype=bool), np.full(n, 3)
    for what, do in (("restore", restore_masked), ("fork", fork_row)):
        frames, mts, got_s, got_e, want_e, cuts = cut_run(do)
        assert np.array_equal(_u(got_e), _u(want_e)), f"{what}: delivered actions"
        (cut_at, (cut_mask, cut_src)), = cuts.items()
        a2 = _env(cfg, cm, n, scenarios=BOTH)
        lay = _layout(a2)
        tw3 = _twin(a2, BOTH)
        names = a2.fault_names()["stacked"]
        a2.close()
        # Every word of state outside last_action, stack rows included (the latency-free fleet was handed the delivered action: its
        # last_action differs).  The test plays the stack: a fill at clock 0, else a roll under the delivered newest frame; the snapshot
        # holds the stack of delivered words as it was taken, and the cut puts the source row's back.
        e0 = sum(d for nme, d in names[:[nme for nme, _ in names].index("last_action")])
        sd, S = lay["stacked_dim"], lay["stack_size"]
        keep = np.setdiff1d(np.arange(lay["state_dim"]), [r * sd + e0 + j for r in range(S) for j in range(4)])
        fr = _frames(frames, lay)
        stack, saved = np.zeros((n, S, sd), dtype=np.float32), None
        for k in range(len(fr)):
            if k == cut_at:
                tw3.cut(cut_mask)
                stack[cut_mask] = saved[cut_src][cut_mask]
            d = tw3.step_obs(fr[k], mts[k, :, 0], mts[k, :, 11], mts[k, :, 1])
            fill = mts[k, :, 0] == 0
            stack[~fill, 1:] = stack[~fill, :-1].copy()
            stack[:, 0] = d[:, :sd]
            stack[fill] = d[fill, None, :sd]
            if k == 6:                                              # the snapshot was taken ahead of step 6: behind observation 6
                saved = stack.copy()
            want_row = np.concatenate([stack.reshape(n, S * sd), d[:, sd:]], axis=1)
            x, y = _u(got_s[k][:, keep]), _u(want_row[:, keep])
            assert np.array_equal(x, y), f"{what}: observation {k}: envs {np.nonzero((x != y).any(axis=1))[0][:8]}, words {keep[np.nonzero((x != y).any(axis=0))[0][:12]]}"
        assert S == 3 and (_u(got_s[cut_at + 2][:, keep]) != _u(frames[cut_at + 2][:, keep])).any()
        if what == "restore":                                       # the uncut envs never noticed
            assert (mts[cut_at][mask, 0] == 7).all() and (mts[cut_at][~mask, 0] == 11).all()


# ------------------------------------------------------------------------------------------------------------ 7: off means off
def test_cleared_or_absent_latency_leaves_no_trace_and_refusals_leave_the_env_stepping():
    cfg, cm = _light()
    n = 32
    raw = _actions(n, 26, 4, seed=50)

    def observe(env):
        env.join()
        env.torch.cuda.synchronize(env.device)
        return tuple(x.cpu().numpy().copy() for x in (env.state, env.info_buf, env.terminated, env.truncated))

    launches = []

    def drive(env, off=True):
        """A reset, the steps and a snapshot; the kernel launches the engine issued for them go to ``launches``."""
        tb = env.torch.tensor(raw, device=env.device)
        before = env.engine.query("launches")
        env.reset()
        out = []
        for k in range(len(raw)):
            env.step(tb[k])
            assert (env.effective_action() is None) == off
            out.append(observe(env))
        out.append((env.snapshot().rows.cpu().numpy().copy(),))
        launches.append((env.engine.query("launches") - before) % (1 << 31))
        return out
    y = _env(cfg, cm, n, scenarios=_strip(BOTH))
    assert y.engine.query("latency") == 0 and y.engine.query("latency_depth") == 0 and y.latency() == [[], [], []] and y.effective_action() is None
    ref = drive(y)
    x = _env(cfg, cm, n, scenarios=BOTH)
    assert x.engine.query("latency") > 0 and x.effective_action() is not None
    x.engine.latency_set(None)
    assert x.engine.query("latency") == 0 and x.engine.query("scenario_rows") == 3
    _same_run(ref, drive(x), "cleared")
    assert launches[1] == launches[0] > len(raw), launches         # a cleared table launches what a table without the key does
    x.set_scenarios(BOTH)
    drive(x, off=False)
    # ... and the counter sees a launch: one range issues three more per step (latency_act_kernel, actfault_obs_kernel,
    # latency_obs_kernel) and one more per reset (latency_obs_kernel)
    assert launches[2] == launches[0] + 3 * len(raw) + 1, launches
    with pytest.raises(ValueError, match=r'cosim_profile_step: latency is set \(cosim_set_param "latency"\)'):
        x.engine.profile_step(x.state.data_ptr(), x._cmd_ptr(), x.state.data_ptr(), x.terminated.data_ptr(), x.truncated.data_ptr())
    x.set_scenarios(BOTH)
    assert x.engine.query("latency") > 0
    x.set_scenarios(_strip(BOTH))                                   # a table without the key clears what the earlier one left
    assert x.engine.query("latency") == 0 and x.latency() == [[], [], []]
    x.set_scenarios(BOTH)
    x.set_scenarios(_strip(BOTH)[:2])                               # another S drops it with the other tables
    assert x.engine.query("scenario_rows") == 2 and x.engine.query("latency") == 0
    x.set_scenarios(BOTH)
    x.set_scenarios(None)
    assert x.engine.query("latency") == 0 and x.latency() == [] and x.effective_action() is None
    # refusals by message
    t = x.torch
    tb = t.tensor(raw, device=x.device)
    with pytest.raises(ValueError, match=r'cosim_set_param "latency": no scenario table is set'):
        x.engine.latency_set(np.array([3, 0, 1, 1, 1, 0, 0, 0, 0, 0, 5, 0, 0, 1, 0], dtype=np.int32))
    x.set_scenarios(_strip(BOTH))
    with pytest.raises(ValueError, match=r"2 scenarios, the table that is set has 3"):
        x.engine.latency_set(np.array([2, 0, 1, 1, 0, 0, 0, 0, 5, 0, 0, 1, 0], dtype=np.int32))
    with pytest.raises(ValueError, match=r"scenario 0, action latency item 0: actuator 4 out of range: the model has 4 actuators"):
        x.engine.latency_set(np.array([3, 0, 1, 1, 1, 0, 0, 0, 0, 0, 5, 4, 0, 1, 0], dtype=np.int32))
    with pytest.raises(ValueError, match=r"scenario 0, action latency item 0: steps 60 \+ jitter 4 is more than 63"):
        x.engine.latency_set(np.array([3, 0, 1, 1, 1, 0, 0, 0, 0, 0, 5, 0, 0, 60, 4], dtype=np.int32))
    with pytest.raises(ValueError, match=r"14 words, a table of 3 scenarios and 1 \+ 0 items takes 15"):
        x.engine.latency_set(np.array([3, 0, 1, 1, 1, 0, 0, 0, 0, 0, 5, 0, 0, 1], dtype=np.int32))
    assert x.engine.query("latency") == 0                           # nothing was set by a refused call
    with pytest.raises(ValueError, match=r"scenario 0, latency item 0: channel 'command' is refused"):
        x.set_scenarios([{"latency": [[0, 5, "command", 0, 1]]}])
    with pytest.raises(ValueError, match=r"scenario 0, latency item 0: unknown channel 'gyro'"):
        x.set_scenarios([{"latency": [[0, 5, "gyro", 0, 1]]}])
    x.set_scenarios(BOTH)
    x.reset()
    x.step(tb[0])
    with pytest.raises(ValueError, match="latency is set"):
        x.rollout(tb[1:3])
    x.step(tb[1])
    t.cuda.synchronize(x.device)
    assert np.isfinite(x.state.cpu().numpy()).all()
    x.close(); y.close()
    # the 256 MiB cap names the sizes: the observation lines of 60000 envs at depth 64 would take more, the action lines fit
    big = _env(cfg, cm, 60000)
    fd = big.engine.query("frame_dim")
    assert 60000 * 64 * fd * 4 > 256 << 20 >= 60000 * 64 * 4 * 4
    with pytest.raises(ValueError, match=rf"the observation lines take 60000 envs x depth 64 x {fd} frame elements x 4 = {60000 * 64 * fd * 4} bytes, more than 256 MiB"):
        big.set_scenarios([{"latency": [[0, 5, "dof_pos", 0, 63]]}])
    assert big.engine.query("latency") == 0 and big.latency() == [[]] and not big.scenario_table.has_latency   # the env's table agrees with the engine
    with pytest.raises(ValueError, match=r'no action faults are set \(cosim_set_param "action_faults"\) and no latency of the command channel \(cosim_set_param "latency"\)'):
        big.engine.get("action_effective", big.state.data_ptr(), big._stream())
    big.set_scenarios([{"latency": [[0, 5, "action", 0, 63]]}])     # the action lines fit
    assert big.engine.query("latency_depth") == 64
    big.reset()
    big.step(t.zeros((60000, 4), device=big.device))
    t.cuda.synchronize(big.device)
    assert np.isfinite(big.state.cpu().numpy()).all()
    big.close()


# ------------------------------------------------------------------------------------------------------------ 8: CLI
def _cli(tmp_path, capsys, *extra):
    import yaml
    from cosim_amd import cli
    scn, report = tmp_path / "scn.yaml", tmp_path / ("r%d.json" % len(extra))
    scn.write_text(yaml.safe_dump({"scenarios": BOTH}))
    assert cli.main(["--env", "flamingo_light_v1", "--num-envs", "24", "--steps", "40", "--max-duration", "0.24", "--seed", "5", "--policy",
                     "random-mlp", "--scenarios", str(scn), "--scenario-mode", "cycle", *extra, "--ledger", "4", "--report", str(report)]) == 0
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    return json.loads(report.read_text()), line


def test_cli_prints_the_count_and_three_loops_give_one_ledger(tmp_path, capsys):
    eager, eline = _cli(tmp_path, capsys)
    want = 4 + 1 + 1 + 1 + 4 + 1 + 3 + 3 + 1 + 1 + 1 + 1
    assert eline["latency"] == want and "action_faults" not in eline
    by = eager["episodes"]["by_scenario"]
    assert sorted(by) == ["0", "1", "2"] and sum(v["episodes"] for v in by.values()) == eager["episodes"]["episodes"] >= 48
    for path in ("--graph", "--pipelined"):
        r, line = _cli(tmp_path, capsys, path)
        assert line["latency"] == want, path
        assert r["episodes"]["by_scenario"] == by and r["episodes"]["episodes"] == eager["episodes"]["episodes"], path
