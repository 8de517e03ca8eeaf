"""Full-state snapshots on the device (cosim_snapshot / cosim_restore / the history ring, csrc/cosim_snapshot.hip, and their
BatchedEnv / Runner / CLI surface): resume, rewind and fork of a fleet.

Every comparison is BITWISE (assert_array_equal on observation, terminated, truncated and info rows, qpos / qvel / meta at the end):
this is the engine against itself on identical inputs, so no tolerance applies.  Actions come from a fixed per-step table
(numpy.random.default_rng), so a step's action is a function of the step index alone.  Fleets are 16 envs, 8 for the humanoid; the
time limit (max_duration) is set so that an auto-reset falls inside every compared window, and each test asserts that it did."""
import json

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_CACHE = {}
CMD = np.array([0.5, 0.0, 0.0, 0.0, 0.0, 0.0], dtype=np.float32)


def _model(robot, terrain="flat", random=None, **kw):
    """(config, compiled model), compiled once per distinct request; random=None: the GUI-default randomisation (mass noise 0.05,
    action delay 0.05, sensor noise low, init noise 0.05)."""
    from cosim_amd.compile import compile_model
    from cosim_amd.config import make_config
    key = (robot, terrain, json.dumps(random, sort_keys=True), json.dumps(kw, sort_keys=True))
    if key not in _CACHE:
        cfg = make_config(robot, terrain=terrain, random=random, **kw)
        if kw.get("position_command"):
            cfg["observation"]["command_dim"] = 2
        _CACHE[key] = (cfg, compile_model(cfg))
    return _CACHE[key]


def _env(cfg, cm, n=16, seed=3, **kw):
    from cosim_amd.batched_env import BatchedEnv
    kw.setdefault("auto_reset", True)
    env = BatchedEnv(cfg, num_envs=n, compiled=cm, seed=seed, **kw)
    env.receive_user_command(CMD[:env.command_dim] if env.command_dim != 2 else np.array([1.0, 0.5], dtype=np.float32))
    return env


def _table(env, steps, seed=11, per_env=True):
    """[steps, N, nu] actions on the device; per_env=False: the same action for every env of a step."""
    import torch
    rng = np.random.default_rng(seed)
    a = rng.uniform(-0.6, 0.6, size=(steps, env.num_envs if per_env else 1, env.action_dim)).astype(np.float32)
    a = np.broadcast_to(a, (steps, env.num_envs, env.action_dim)).copy()
    return torch.tensor(a, device=env.device)


def _run(env, table, k0, k1):
    """Steps k0..k1-1 of the table; one (state, terminated, truncated, info) tuple of host arrays per step."""
    out = []
    for k in range(k0, k1):
        s, te, tr, _ = env.step(table[k])
        env.join()
        env.torch.cuda.synchronize(env.device)
        out.append((s.cpu().numpy().copy(), te.cpu().numpy().copy(), tr.cpu().numpy().copy(), env.info_buf.cpu().numpy().copy()))
    return out


def _final(env):
    t = env.torch
    d = env.get_data()
    buf = t.zeros((env.num_envs, 16), dtype=t.float32, device=env.device)
    env.engine.get("meta", buf.data_ptr(), env._stream())
    t.cuda.synchronize(env.device)
    return d.qpos.cpu().numpy().copy(), d.qvel.cpu().numpy().copy(), buf.view(t.int32).cpu().numpy().copy()


def _same(a, b, rows=None):
    """Bitwise equality of two step series (optionally of the given env rows), or of two _final() triples."""
    assert len(a) == len(b)
    for x, y in zip(a, b):
        if isinstance(x, tuple):
            for u, v in zip(x, y):
                np.testing.assert_array_equal(u if rows is None else u[rows], v if rows is None else v[rows])
        else:
            np.testing.assert_array_equal(x, y)


def _ended(series):
    return sum(int((te | tr).sum()) for _, te, tr, _ in series)


# ------------------------------------------------------------------------------------------------------------ 1, 2: resume
def _resume_case(tmp_path, robot, terrain, n, k_snap, k_total, max_duration, random=None, env_kw=None, **cfg_kw):
    from cosim_amd.snapshot import Snapshot
    cfg, cm = _model(robot, terrain, random=random, max_duration=max_duration, **cfg_kw)
    env_kw = env_kw or {}
    a = _env(cfg, cm, n, **env_kw)
    table = _table(a, k_total)
    a.reset()
    ref = _run(a, table, 0, k_total)
    ref_final = _final(a)
    tail = ref[k_snap:]
    assert _ended(tail) > 0, "no auto-reset inside the compared window"
    b = _env(cfg, cm, n, **env_kw)
    b.reset()
    _same(_run(b, table, 0, k_snap), ref[:k_snap])
    snap = b.snapshot()
    assert snap.steps == k_snap and snap.rows.shape == (n, b.engine.query("snapshot_floats"))
    assert b.engine.query("snapshot_floats") == b.engine.query("state_stride") + b.engine.query("param_stride")
    assert b.engine.query("snapshot_floats") % 32 == 0
    _same(_run(b, table, k_snap, k_total), tail)                           # taking the snapshot changed nothing
    obs = b.restore(snap)
    b.torch.cuda.synchronize(b.device)
    np.testing.assert_array_equal(obs.cpu().numpy(), ref[k_snap - 1][0])   # the observation the interrupted loop would act on
    assert b.control_steps == k_snap
    _same(_run(b, table, k_snap, k_total), tail)
    _same(_final(b), ref_final)
    # a fresh engine with the same seed, through a file, parameters included
    path = str(tmp_path / "snap.npz")
    snap.save(path)
    c = _env(cfg, cm, n, **env_kw)
    c.receive_user_command(np.zeros(c.command_dim, dtype=np.float32))      # the command comes back with the snapshot
    loaded = Snapshot.load(path, device=c.device)
    assert loaded.meta == snap.meta and loaded.steps == k_snap
    c.restore(loaded, params=True)
    _same(_run(c, table, k_snap, k_total), tail)
    _same(_final(c), ref_final)
    a.close(); b.close(); c.close()


def test_resume_fused_dense_kernel(tmp_path):
    """flamingo_light_v1 flat, GUI-default randomisation: steps 20..39 after a restore, and after a restore through a file into a
    fresh engine, equal the uninterrupted run's.  The 0.5 s time limit ends every episode in the 25th step."""
    _resume_case(tmp_path, "flamingo_light_v1", "flat", 16, 20, 40, max_duration=0.5)


@pytest.mark.parametrize("robot,terrain,kw", [
    ("humanoid_p_v0", "stairs_up_hard", dict(position_command=True)),                                   # split pipeline
    ("humanoid_p_v0", "stairs_up_hard", dict(position_command=True, env_kw=dict(hfield_fixup=True))),   # ... with the substep fix-up
    ("w4_p_v2", "rocky_hard", {}),                                                                       # fused contact-twist
    ("flamingo_light_v1", "flat", dict(precision="high")),
], ids=["humanoid_split", "humanoid_split_fixup", "w4_contact_twist", "light_high"])
def test_resume_other_paths(tmp_path, robot, terrain, kw):
    """6 + 6 steps; the 0.17 s time limit (8 control steps) resets every env inside the second half."""
    from cosim_amd.config import GUI_RANDOM_DEFAULTS
    kw = dict(kw)
    random = None
    if "precision" in kw:
        random = dict(GUI_RANDOM_DEFAULTS, precision=kw.pop("precision"))
    n = 8 if robot == "humanoid_p_v0" else 16
    if robot == "humanoid_p_v0":
        cfg, cm = _model(robot, terrain, random=random, max_duration=0.17, position_command=True)
        e = _env(cfg, cm, n, **kw.get("env_kw", {}))
        assert e.engine.query("split") > 0
        e.close()
    _resume_case(tmp_path, robot, terrain, n, 6, 12, max_duration=0.17, random=random, **kw)


# ------------------------------------------------------------------------------------------------------------ 3: rollout
def test_rollout_after_restore_repeats():
    cfg, cm = _model("flamingo_light_v1", "flat", max_duration=0.2)        # time limit: 10 control steps
    env = _env(cfg, cm)
    assert env.engine.query("rollout") == 1
    table = _table(env, 23)
    env.reset()
    _run(env, table, 0, 3)
    snap = env.snapshot()
    first = [x.cpu().numpy().copy() for x in env.rollout(table[3:23])]
    assert int((first[1] | first[2]).sum()) > 0                            # an auto-reset inside the rollout
    assert env.control_steps == 23
    env.restore(snap)
    assert env.control_steps == 3
    second = [x.cpu().numpy().copy() for x in env.rollout(table[3:23])]
    for u, v in zip(first, second):
        np.testing.assert_array_equal(u, v)
    env.close()


# ------------------------------------------------------------------------------------------------------------ 4: fork
def _fork_setup(random, gain_noise=0.0):
    cfg, cm = _model("flamingo_light_v1", "flat", random=random, max_duration=0.3)   # time limit: 15 control steps
    env = _env(cfg, cm, gain_noise=gain_noise)
    apart = _table(env, 10, seed=21)                  # per-env actions: the envs drift apart
    common = _table(env, 10, seed=22, per_env=False)  # then the same action for every env
    env.reset()
    _run(env, apart, 0, 10)
    snap = env.snapshot()
    src_run = _run(env, common, 0, 10)                # every env's own continuation
    assert _ended(src_run) > 0
    q = np.stack([s for s, _, _, _ in src_run])
    assert np.abs(q - q[:, 5:6]).max() > 0            # ... and they do differ from env 5's
    return env, snap, common, src_run


def _all_equal_row(series, ref, row):
    for (s, te, tr, inf), (rs, rte, rtr, rinf) in zip(series, ref):
        for u, v in ((s, rs), (te, rte), (tr, rtr), (inf, rinf)):
            np.testing.assert_array_equal(u, np.broadcast_to(v[row:row + 1], u.shape))


def test_fork_without_stochastic_knobs():
    from cosim_amd.config import PARITY_RANDOM
    env, snap, common, src_run = _fork_setup(PARITY_RANDOM)
    obs = env.fork(snap, row=5)
    env.torch.cuda.synchronize(env.device)
    np.testing.assert_array_equal(obs.cpu().numpy(), np.broadcast_to(snap.obs[5:6].cpu().numpy(), obs.shape))
    _all_equal_row(_run(env, common, 0, 10), src_run, 5)
    env.close()


def test_fork_params_flag():
    from cosim_amd.config import PARITY_RANDOM
    env, snap, common, src_run = _fork_setup(dict(PARITY_RANDOM, mass_noise=0.05))
    env.fork(snap, row=5, params=True)
    _all_equal_row(_run(env, common, 0, 10), src_run, 5)
    env.restore(snap, params=True)                    # every slot its own parameter record again (the fork above copied env 5's)
    env.fork(snap, row=5, params=False)               # every env keeps its own masses: not env 5's continuation any more
    own = _run(env, common, 0, 10)
    differs = [d for d in range(env.num_envs) if any(not np.array_equal(s[d], rs[5]) for (s, _, _, _), (rs, _, _, _) in zip(own, src_run))]
    assert differs, "params=False behaved like params=True"
    env.close()


def test_restore_permutation_with_mask():
    import torch
    from cosim_amd.config import PARITY_RANDOM
    cfg, cm = _model("flamingo_light_v1", "flat", random=dict(PARITY_RANDOM, mass_noise=0.05), max_duration=0.37)   # 18 control steps
    env = _env(cfg, cm)
    n = env.num_envs
    apart, more, common = _table(env, 10, seed=31), _table(env, 5, seed=32), _table(env, 5, seed=33, per_env=False)
    env.reset()
    _run(env, apart, 0, 10)
    snap10 = env.snapshot()
    _run(env, more, 0, 5)
    snap15 = env.snapshot()
    untouched = _run(env, common, 0, 5)
    assert _ended(untouched) > 0                      # the time limit ends every episode in the 18th step, the third of these
    env.restore(snap10, params=True)
    sources = _run(env, common, 0, 5)
    env.restore(snap15, params=True)
    src = torch.arange(n - 1, -1, -1, dtype=torch.int32, device=env.device)
    mask = (torch.arange(n, device=env.device) % 2).to(torch.uint8)       # odd envs are restored
    env.restore(snap10, src=src, mask=mask, params=True)
    mixed = _run(env, common, 0, 5)
    even, odd = np.arange(0, n, 2), np.arange(1, n, 2)
    _same(mixed, untouched, rows=even)
    for (s, te, tr, inf), (rs, rte, rtr, rinf) in zip(mixed, sources):
        for u, v in ((s, rs), (te, rte), (tr, rtr), (inf, rinf)):
            np.testing.assert_array_equal(u[odd], v[n - 1 - odd])
    env.close()


def test_set_param_after_restore_with_params_keeps_the_restored_table():
    """A restore with parameters leaves the engine's host mirror behind the device; a later set_param of one field rewrites the
    whole table from the mirror, so the mirror must have been brought up to date: re-sending the kp in force changes nothing."""
    from cosim_amd.config import PARITY_RANDOM
    env, snap, common, src_run = _fork_setup(dict(PARITY_RANDOM, mass_noise=0.05), gain_noise=0.1)
    env.fork(snap, row=5, params=True)
    _all_equal_row(_run(env, common, 0, 5), src_run[:5], 5)
    env.fork(snap, row=5, params=True)
    env.engine.set_param("kp", np.tile(env.kp[5:6], (env.num_envs, 1)))    # the kp every env runs with after the fork
    _all_equal_row(_run(env, common, 0, 5), src_run[:5], 5)
    env.close()


# ------------------------------------------------------------------------------------------------------------ 5: history
def test_history_ring():
    cfg, cm = _model("flamingo_light_v1", "flat", max_duration=0.61)      # time limit: 30 control steps
    plain = _env(cfg, cm)
    table = _table(plain, 40)
    plain.reset()
    ref = _run(plain, table, 0, 40)
    assert _ended(ref[25:]) > 0
    # history on, captures never read: the same bits
    g = _env(cfg, cm, history=(4, 5))
    assert g.engine.query("history_slots") == 4 and g.engine.query("history_every") == 5
    g.reset()
    got = _run(g, table, 0, 7)
    with pytest.raises(ValueError, match="does not exist yet"):
        g.history(1)                                                       # one capture so far (after step 5)
    assert g.history(0).steps_ago == 2
    got += _run(g, table, 7, 40)
    _same(got, ref)
    _same(_final(g), _final(plain))
    # four ranges, deferred join, 40 back-to-back steps with no join in between
    h = _env(cfg, cm, history=(4, 5), ranges=4, deferred_join=True)
    h.reset()
    for k in range(40):
        h.step(table[k])
    h0 = h.history(0)
    assert h0.steps_ago == 0 and h0.steps == 40 and h0.obs is None
    now = h.snapshot()
    h.torch.cuda.synchronize(h.device)
    np.testing.assert_array_equal(h0.rows.view(h.torch.int32).cpu().numpy(), now.rows.view(h.torch.int32).cpu().numpy())
    np.testing.assert_array_equal(now.obs.cpu().numpy(), ref[39][0])
    h3 = h.history(3)
    assert h3.steps_ago == 15 and h3.steps == 25
    with pytest.raises(ValueError, match="outside the ring"):
        h.history(4)
    assert h.restore(h3, params=True) is None                              # ring captures carry the engine rows only
    assert h.control_steps == 25
    _same(_run(h, table, 25, 40), ref[25:])
    _same(_final(h), _final(plain))
    plain.close(); g.close(); h.close()


# ------------------------------------------------------------------------------------------------------------ 6: refusals
def test_refusals():
    import copy
    import torch
    from cosim_amd.config import GUI_RANDOM_DEFAULTS
    from cosim_amd.snapshot import Snapshot
    cfg, cm = _model("flamingo_light_v1", "flat", max_duration=0.5)
    env = _env(cfg, cm, history=(2, 1))
    n = env.num_envs
    table = _table(env, 4)
    env.reset()
    _run(env, table, 0, 2)
    snap = env.snapshot()
    before = _final(env)
    # a source index outside the snapshot: refused, named, and that env is left untouched
    for bad in (n, -1):
        src = np.arange(n, dtype=np.int32)
        src[3] = bad
        with pytest.raises(ValueError, match="env 3"):
            env.restore(snap, src=src)
    _same(_final(env), before)
    with pytest.raises(ValueError, match="row 16"):
        env.fork(snap, row=n)
    # the wrong row count without a source index
    short = Snapshot(snap.rows[:8].clone(), snap.obs[:8].clone(), snap.command[:8].clone(), snap.steps, snap.meta)
    with pytest.raises(ValueError, match="8 rows"):
        env.restore(short)
    with pytest.raises(ValueError, match="snap_rows must equal n_envs"):
        env.engine.restore(short.rows.data_ptr(), 8, None, None, False, env._stream())
    # snapshots of another robot, precision, fleet size: the message names the field
    for field, other in (("env_id", _env(*_model("flamingo_p_v3", "flat", max_duration=0.5))),
                         ("precision", _env(*_model("flamingo_light_v1", "flat", random=dict(GUI_RANDOM_DEFAULTS, precision="high"), max_duration=0.5))),
                         ("n_envs", _env(cfg, cm, 8))):
        other.reset()
        foreign = other.snapshot()
        with pytest.raises(ValueError, match=field):
            env.restore(foreign)
        other.close()
    meta = copy.deepcopy(snap.meta)
    meta["terrain"] = "rocky_hard"
    with pytest.raises(ValueError, match="terrain"):
        env.restore(Snapshot(snap.rows, snap.obs, snap.command, snap.steps, meta))
    _same(_final(env), before)
    # cosim_step under graph capture with a history set
    act = table[2].clone()
    scratch = torch.zeros(4, device=env.device)
    torch.cuda.synchronize(env.device)
    caught = []
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        scratch.add_(1.0)
        try:
            env.step(act)
        except ValueError as ex:
            caught.append(str(ex))
    assert caught and "history" in caught[0] and "captured" in caught[0]
    torch.cuda.synchronize(env.device)
    _same(_final(env), before)
    _run(env, table, 2, 4)                                                 # the engine goes on as usual
    assert env.history(0).steps_ago == 0
    env.close()


# ------------------------------------------------------------------------------------------------------------ 7: policy, runner, CLI
def test_lstm_policy_state_round_trip(tmp_path):
    import torch
    from cosim_amd.policy import build_policy, write_onnx
    rng = np.random.default_rng(1)
    I, H, A, N = 10, 6, 3, 7
    W = (0.4 * rng.standard_normal((1, 4 * H, I))).astype(np.float32)
    R = (0.4 * rng.standard_normal((1, 4 * H, H))).astype(np.float32)
    B = (0.1 * rng.standard_normal((1, 8 * H))).astype(np.float32)
    Wo = (0.5 * rng.standard_normal((A, H))).astype(np.float32)
    nodes = [{"op": "Unsqueeze", "inputs": ["obs"], "outputs": ["x3"], "attrs": {"axes": [0]}},
             {"op": "LSTM", "inputs": ["x3", "W", "R", "B", "", "h_in", "c_in"], "outputs": ["Y", "h_out", "c_out"], "attrs": {"hidden_size": H}},
             {"op": "Squeeze", "inputs": ["h_out"], "outputs": ["hs"], "attrs": {"axes": [0]}},
             {"op": "Gemm", "inputs": ["hs", "Wo", "bo"], "outputs": ["actions"], "attrs": {"transB": 1}}]
    p = str(tmp_path / "lstm.onnx")
    write_onnx(p, nodes, {"W": W, "R": R, "B": B, "Wo": Wo, "bo": np.zeros(A, dtype=np.float32)}, ["obs", "h_in", "c_in"], ["actions", "h_out", "c_out"])
    pol = build_policy({"policy": {"use_lstm": True, "h_in_dim": H, "c_in_dim": H}}, p, num_envs=N, device="cuda:0")
    xs = [torch.tensor(rng.standard_normal((N, I)).astype(np.float32), device="cuda:0") for _ in range(6)]
    for x in xs[:3]:
        pol.get_action(x)
    st = pol.state()
    h3, c3 = st["h"].clone(), st["c"].clone()
    tail = [pol.get_action(x).clone() for x in xs[3:]]
    assert not torch.equal(pol.h_in[0], h3)
    pol.load_state(st)                                                     # round trip: the same actions again
    assert torch.equal(pol.h_in[0], h3) and torch.equal(pol.c_in[0], c3)
    for x, a in zip(xs[3:], tail):
        assert torch.equal(pol.get_action(x), a)
    src = torch.tensor([6, 5, 4, 3, 2, 1, 0], device="cuda:0")
    mask = torch.tensor([1, 0, 1, 0, 1, 0, 1], dtype=torch.uint8, device="cuda:0")
    kept_h = pol.h_in[0].clone()
    pol.load_state(st, src=src, mask=mask)
    keep = mask.bool()[:, None]
    assert torch.equal(pol.h_in[0], torch.where(keep, h3[src], kept_h))
    assert torch.equal(pol.c_in[0][mask.bool()], c3[src][mask.bool()])
    pol.load_state(st, src=src)
    assert torch.equal(pol.h_in[0], h3[src]) and torch.equal(pol.c_in[0], c3[src])


def test_runner_resume_with_a_push_after_the_checkpoint():
    from cosim_amd.reporter import FleetReporter
    from cosim_amd.runner import Runner, SinusoidPolicy
    cfg, cm = _model("flamingo_light_v1", "flat", max_duration=0.5)

    def session(env):
        pol = SinusoidPolicy(env.num_envs, env.action_dim, env.device, seed=3)
        rep = FleetReporter(env, trace_env=2)
        run = Runner(env, pol, reporter=rep)
        run.update_command(0, 0.5)

        def before_step(k):                           # the session's schedule: a command change at 12, a push held over 22..23
            if k == 12:
                run.update_command(0, 0.8)
            if 22 <= k < 24:
                run.activate_push_event(np.array([0.5, 0.0, 0.0], dtype=np.float32))
            else:
                run.deactivate_push_event()
        return pol, rep, run, before_step

    a = _env(cfg, cm)
    pol, rep, run, before = session(a)
    snaps = []
    assert run.test(max_steps=30, before_step=before, on_step=lambda k, *_: snaps.append(a.snapshot(pol)) if k + 1 == 18 else None) == 30
    full = rep.trace
    assert len(full) == 30 and snaps[0].steps == 18
    b = _env(cfg, cm)
    pol2, rep2, run2, before2 = session(b)
    seen = []
    assert run2.test(max_steps=12, before_step=lambda k: (seen.append(k), before2(k))[1], resume=snaps[0]) == 12
    assert seen == list(range(18, 30)) and pol2.t == 30
    assert len(rep2.trace) == 12
    for r1, r2 in zip(full[18:], rep2.trace):
        assert r1.keys() == r2.keys()
        for k in r1:
            np.testing.assert_array_equal(np.asarray(r1[k]), np.asarray(r2[k]), err_msg=k)
    assert any(r["user_command_0"] == np.float32(0.8) for r in rep2.trace)
    a.close(); b.close()


def test_cli_checkpoint_and_resume(tmp_path, capsys):
    import yaml
    from cosim_amd import cli
    sess = tmp_path / "session.yaml"
    sess.write_text(yaml.safe_dump({"env": {"id": "flamingo_light_v1", "terrain": "flat", "max_duration": 0.8},
                                    "engine": {"num_envs": 16, "seed": 5}, "policy": {"kind": "sinusoid"},
                                    "commands": [[0, 0.5, 0, 0, 0], [20, 0.9, 0, 0.2, 0]], "pushes": [[44, 46, 0.5, 0, 0]], "trace_env": 1}))
    r1, r2, r3, ck = tmp_path / "r1.json", tmp_path / "r2.json", tmp_path / "r3.json", tmp_path / "ck.npz"
    assert cli.main(["--config", str(sess), "--steps", "60", "--checkpoint", str(ck), "--checkpoint-at", "30", "--history", "4", "10",
                     "--report", str(r1)]) == 0
    assert cli.main(["--config", str(sess), "--steps", "30", "--resume", str(ck), "--report", str(r2)]) == 0
    a, b = json.loads(r1.read_text()), json.loads(r2.read_text())
    assert a["snapshot"] == {"history": [4, 10], "checkpoint": str(ck), "checkpoint_at": 30}
    assert b["snapshot"] == {"resume": str(ck), "resume_step": 30}
    assert a["control_steps"] == 60 and b["control_steps"] == 30 and a["trace"].keys() == b["trace"].keys()
    for k in a["trace"]:
        assert a["trace"][k][30:] == b["trace"][k], k
    assert a["episodes_ended"] >= 16                                       # the 40-step time limit fell inside the overlap
    # every env from row 1 of the file: the traced env 1 is its own source, so with parameters its series is the same again
    assert cli.main(["--config", str(sess), "--steps", "5", "--resume", str(ck), "--fork-row", "1", "--report", str(r3)]) == 0
    c = json.loads(r3.read_text())
    assert c["snapshot"] == {"resume": str(ck), "resume_step": 30, "fork_row": 1}
    for k in c["trace"]:
        assert a["trace"][k][30:35] == c["trace"][k], k
    capsys.readouterr()
