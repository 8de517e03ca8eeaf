"""Spawn tables on the device (cosim_spawn_set, csrc/cosim_spawn.hip and the reset block of the shared kernel body): the placement
kernel against its float64 numpy twin (spawn.place_reference), the base pose every reset path takes from the table -- cosim_reset,
the auto-reset inside the fused, rollout, fix-up and split-pipeline kernels --, the same physics as a pose pushed in through
set_state, oracle parity from spawned poses, shard invariance and the CLI.  16 envs and 64 rows unless a test says otherwise."""
import json

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_CACHE = {}


def _model(robot, terrain="flat", random=None, **kw):
    """(config, compiled model), compiled once per distinct request."""
    from cosim_amd.compile import compile_model
    from cosim_amd.config import PARITY_RANDOM, make_config
    key = (robot, terrain, json.dumps(random, sort_keys=True), json.dumps(kw, sort_keys=True))
    if key not in _CACHE:
        cfg = make_config(robot, terrain=terrain, random=PARITY_RANDOM if random is None else random, **kw)
        if kw.get("position_command"):
            cfg["observation"]["command_dim"] = 2
        _CACHE[key] = (cfg, compile_model(cfg))
    return _CACHE[key]


def _env(cfg, cm, n, **kw):
    from cosim_amd.batched_env import BatchedEnv
    kw.setdefault("auto_reset", False)
    return BatchedEnv(cfg, num_envs=n, compiled=cm, **kw)


def _meta(env):
    t = env.torch
    buf = t.zeros((env.num_envs, 16), dtype=t.float32, device=env.device)
    env.engine.get("meta", buf.data_ptr(), env._stream())
    t.cuda.synchronize(env.device)
    return buf.view(t.int32).cpu().numpy().astype(np.int64)


def _qpos(env):
    d = env.get_data()
    env.torch.cuda.synchronize(env.device)
    return d.qpos.cpu().numpy().copy(), d.qvel.cpu().numpy().copy()


def _table(cm, rows=64, seed=0):
    """`rows` poses over the whole allowed square, yaw over (-pi, pi); row 0 sits at yaw 0 where its furthest-reaching footprint
    sphere ends half a cell inside the field's +x edge.  The seed moves on until no window bound of the table lies within 1e-9 cells
    of an integer, so the expected window does not hinge on the last bit of a double."""
    from cosim_amd import spawn as sp
    b = cm.blob
    fp = sp.footprint(cm).astype(np.float64)
    e = sp.default_extent(cm)
    for s in range(seed, seed + 20):
        rng = np.random.default_rng(s)
        t = np.column_stack([rng.uniform(-e, e, size=(rows, 2)), rng.uniform(-np.pi, np.pi, size=rows)])
        t[1:5, 0] = np.abs(t[1:5, 0]) * [1, -1, 1, -1]            # all four quadrants, whatever the draw
        t[1:5, 1] = np.abs(t[1:5, 1]) * [1, 1, -1, -1]
        if b.ground_type == 1:
            dx = 2.0 * b.hfield_size[0] / (b.hfield_ncol - 1)
            t[0] = [b.hfield_size[0] - (fp[:, 0] + fp[:, 2]).max() - 0.5 * dx, 0.25 * e, 0.0]
        t = t.astype(np.float32)
        _, _, bounds = sp.windows(cm, t)
        if bounds is None or all(np.abs(x - np.round(x)).min() > 1e-9 for x in bounds):
            return t
    raise AssertionError("no seed gave a table clear of the window boundaries")


def _assert_placed_like_reference(got, ref64):
    """x, y exact; z within 2 ulp of fp32 (the device may contract sz * hmax - free into one fused multiply-add, and adds in
    fp32); the quaternion within 1 ulp."""
    ref = ref64.astype(np.float32)
    np.testing.assert_array_equal(got[:, :2], ref[:, :2])
    dz = np.abs(got[:, 2].astype(np.float64) - ref[:, 2].astype(np.float64))
    assert np.all(dz <= 2.0 * np.spacing(np.abs(ref[:, 2])).astype(np.float64)), (dz.max(), np.spacing(ref[:, 2]).max())
    dq = np.abs(got[:, 3:].astype(np.float64) - ref[:, 3:].astype(np.float64))
    assert np.all(dq <= np.spacing(np.abs(ref[:, 3:])).astype(np.float64)), dq.max()


@pytest.mark.parametrize("robot,terrain", [("flamingo_light_v1", "stairs_up_easy"),     # 1 cm cells: thousands of vertices per geom
                                           ("w4_p_v2", "rocky_hard"),                   # 55 cm cells: windows of 2 to 5 vertices
                                           ("humanoid_p_v0", "stairs_up_hard")])        # 22 geoms
def test_placement_kernel_equals_the_numpy_rule(robot, terrain):
    from cosim_amd import spawn as sp
    cfg, cm = _model(robot, terrain)
    b = cm.blob
    table = _table(cm)
    lx, _, bounds = sp.windows(cm, table)
    r = sp.footprint(cm).astype(np.float64)[None, :, 2]
    dx = 2.0 * b.hfield_size[0] / (b.hfield_ncol - 1)
    assert 0 < b.hfield_size[0] - (np.abs(lx) + r).max() < dx                              # a footprint within a cell of the boundary
    assert {(sx > 0, sy > 0) for sx, sy in table[:, :2]} == {(True, True), (True, False), (False, True), (False, False)}
    assert table[:, 2].min() < -2.5 and table[:, 2].max() > 2.5
    width = np.ceil(bounds[1]) - np.floor(bounds[0]) + 1
    print(f"[{robot} / {terrain}] window widths {int(width.min())}..{int(width.max())} vertices, {r.shape[1]} geoms")
    env = _env(cfg, cm, 16, spawn=table)
    assert env.engine.query("spawn_rows") == 64 and env.engine.query("spawn_mode") == 0
    got = env.spawn_poses()
    assert got.shape == (64, 7) and got.dtype == np.float32
    ref = sp.place_reference(cm, table, 0.0)
    assert (ref[:, 2] - ref[:, 2].min()).max() > 0.05                                      # the rows really stand at different heights
    _assert_placed_like_reference(got, ref)
    # a clearance, per-episode mode and the same row count again: rewritten in place
    env.set_spawn(table[::-1].copy(), clearance=0.0125, per_episode=True)
    assert env.engine.query("spawn_rows") == 64 and env.engine.query("spawn_mode") == 1
    _assert_placed_like_reference(env.spawn_poses(), sp.place_reference(cm, table[::-1], 0.0125))
    env.close()


def test_bad_rows_are_refused_by_name_and_zero_rows_clear_the_table():
    from cosim_amd import spawn as sp
    cfg, cm = _model("w4_p_v2", "rocky_hard")
    table = _table(cm)
    q0 = np.array(cm.blob.init_qpos[:7], dtype=np.float32)
    env = _env(cfg, cm, 16)
    assert env.engine.query("spawn_rows") == 0 and env.spawn_poses().shape == (0, 7)
    fp = sp.footprint(cm)
    off, nan = table.copy(), table.copy()
    off[3, 0] = cm.blob.hfield_size[0] - 0.05
    nan[5, 2] = np.inf
    for bad, row in ((off, 3), (nan, 5)):
        with pytest.raises(ValueError, match=f"row {row}"):
            env.set_spawn(bad)                                           # the host-side check of spawn.resolve
        with pytest.raises(ValueError, match=f"row {row}"):
            env.engine.spawn_set(bad, fp, 0.0, False, env._stream())     # the engine's own (COSIM_EINVAL)
    with pytest.raises(ValueError):
        env.engine.spawn_set(table, fp, -1.0, False, env._stream())
    with pytest.raises(ValueError, match="yaw"):
        env.set_spawn({"poses": [[0.0, 0.0, 1.0, np.cos(0.3), 0.0, np.sin(0.3), 0.0]]})      # a pitched spawn
    assert env.engine.query("spawn_rows") == 0                           # a refused table changes nothing
    env.set_spawn(table)
    env.reset()
    assert np.array_equal(_qpos(env)[0][:, :7], env.spawn_poses()[:16])
    env.set_spawn(np.zeros((0, 3)))                                      # rows = 0 clears: resets go back to init_qpos
    assert env.engine.query("spawn_rows") == 0 and env.spawn_poses().shape == (0, 7)
    env.reset()
    assert np.array_equal(_qpos(env)[0][:, :7], np.tile(q0, (16, 1)))
    env.set_spawn(table[:10])                                            # a different row count: a new table
    env.reset()
    assert np.array_equal(_qpos(env)[0][:, :7], env.spawn_poses()[np.arange(16) % 10])
    env.set_spawn(None)
    assert env.engine.query("spawn_rows") == 0
    env.close()


def _reset_with_and_without_a_table(epw):
    """flamingo_light_v1 on the plane, init noise on, seed 5, 16 envs from global id 70: (qpos, qvel, state, poses, rows) after
    reset() of an env without a table and of one with a 64-row table; run once per kernel variant and shared."""
    key = ("reset", epw)
    if key not in _CACHE:
        from cosim_amd.config import PARITY_RANDOM
        cfg, cm = _model("flamingo_light_v1", "flat", random=dict(PARITY_RANDOM, init_noise=0.05))
        table = _table(cm, seed=3)
        out = []
        for spawn in (None, table):
            env = _env(cfg, cm, 16, seed=5, env_id0=70, spawn=spawn)
            if epw == 2:
                env.engine.set_param("envs_per_wave", np.array([2.0]))
            state, _ = env.reset()
            qp, qv = _qpos(env)
            out.append((qp, qv, state.cpu().numpy().copy(), env.spawn_poses(), env.spawn_rows()))
            env.close()
        _CACHE[key] = (cfg, cm, out)
    return _CACHE[key]


@pytest.mark.parametrize("epw", [1, 2])
def test_reset_takes_the_base_pose_from_the_table_and_nothing_else_changes(epw):
    """Plane ground, init noise on, same seed: qpos[:, :7] is row gid mod M bit for bit; the joint angles with their noise and the
    velocities are those of an env without a table.  Also through the two-envs-per-wave kernel, where the reset block must index
    by the lane of the env's group.  (The returned state vector: the next test.)"""
    _, cm, ((qp0, qv0, _, _, _), (qp1, qv1, _, poses, rows)) = _reset_with_and_without_a_table(epw)
    want = (70 + np.arange(16)) % 64
    assert np.array_equal(rows, want)
    assert np.array_equal(qp1[:, :7], poses[want])
    assert np.all(poses[:, 2] == np.float32(cm.blob.init_qpos[2]))       # plane: dz = clearance = 0
    assert np.array_equal(qp1[:, 7:], qp0[:, 7:]) and np.unique(qp0[:, 7]).size > 1     # init noise: same draws, different per env
    assert np.array_equal(qv1, qv0)
    assert not np.array_equal(qp1[:, :7], qp0[:, :7])


@pytest.mark.parametrize("epw", [1, 2])
def test_reset_state_vector_is_bit_for_bit_that_of_an_env_without_a_table(epw):
    """The whole state vector reset() returns, with a table against without one, bit for bit.  A yaw does not turn gravity in the
    body frame, and the reset block builds projected gravity from the yaw-free init quaternion; built from the yawed one its z came
    out as -0.99999994 in 7 of 16 envs (w^2 + z^2 of an fp32 unit quaternion is 1 only to an ulp)."""
    cfg, _, ((_, _, st0, _, _), (_, _, st1, _, _)) = _reset_with_and_without_a_table(epw)
    diff = st1 != st0
    cols = np.flatnonzero(diff.any(axis=0))
    print(f"[reset state epw={epw}] state_dim {st0.shape[1]}, order {cfg['observation']['stacked_obs_order']} x "
          f"{cfg['observation']['stack_size']} + {cfg['observation']['non_stacked_obs_order']}; differing columns {cols.tolist()}, "
          f"envs with a difference {int(diff.any(axis=1).sum())} of 16, max |difference| {np.abs(st1 - st0).max():.3e}, "
          f"values there: with {st1[diff][:4].tolist()} without {st0[diff][:4].tolist()}")
    assert np.array_equal(st1, st0)


@pytest.mark.parametrize("robot,terrain", [("flamingo_light_v1", "stairs_up_easy"), ("w4_p_v2", "rocky_hard")])
def test_a_spawned_env_steps_like_one_given_the_same_pose_through_set_state(robot, terrain):
    import torch
    cfg, cm = _model(robot, terrain)
    table = _table(cm, seed=1)
    a = _env(cfg, cm, 16, spawn=table)
    b = _env(cfg, cm, 16)
    a.reset(); b.reset()
    qa = _qpos(a)[0]
    assert np.array_equal(qa[:, :7], a.spawn_poses()[:16])
    b.set_state(qpos=qa)
    acts = torch.tensor(np.random.default_rng(2).uniform(-1, 1, size=(3, 16, a.action_dim)), dtype=torch.float32, device=a.device)
    for t in range(3):
        a.step(acts[t]); b.step(acts[t])
        (pa, va), (pb, vb) = _qpos(a), _qpos(b)
        assert np.array_equal(pa, pb) and np.array_equal(va, vb), t
        assert torch.equal(a.info_buf, b.info_buf), t
    assert np.isfinite(pa).all() and np.abs(pa[:, :2] - qa[:, :2]).max() < 0.5
    a.close(); b.close()


def test_one_step_from_spawned_poses_follows_the_oracle():
    """w4_p_v2 on rocky_hard, one control step from 64 spawned poses (the whole table) against the fp64 oracle started from the
    same fp32 poses: the per-state bounds test_gpu_parity.test_heightfield_terrain_replay_and_height_map applies to w4_p_v2."""
    import torch
    from oracle.oracle import Oracle
    cfg, cm = _model("w4_p_v2", "rocky_hard")
    b = cm.blob
    env = _env(cfg, cm, 64, spawn=_table(cm, seed=2))
    env.reset()
    q, _ = _qpos(env)
    acts = np.clip(0.1 * np.random.default_rng(3).normal(size=(64, b.nu)), -1, 1)
    env.step(torch.tensor(acts, dtype=torch.float32, device=env.device))
    qp, qv = _qpos(env)
    o = Oracle(cm)
    ep, ev = np.zeros(64), np.zeros(64)
    for i in range(64):
        o.reset(q[i].astype(np.float64))
        o.control_step(acts[i])
        assert not o.bad
        ep[i] = np.abs(qp[i] - o.qpos).max()
        ev[i] = np.abs(qv[i] - o.qvel).max()
    st = env.solver_stats()
    print(f"[spawn parity] |dqpos| median {np.median(ep):.2e} q90 {np.quantile(ep, 0.9):.2e} max {ep.max():.2e}; |dqvel| median "
          f"{np.median(ev):.2e} q90 {np.quantile(ev, 0.9):.2e} max {ev.max():.2e}")
    assert st["dropped_contacts"] == 0 and st["nan_resets"] == 0
    assert np.median(ep) < 2e-5 and np.quantile(ep, 0.9) < 2e-4, (np.median(ep), np.quantile(ep, 0.9), ep.max())
    assert np.median(ev) < 1e-3 and np.quantile(ev, 0.9) < 2e-2, (np.median(ev), np.quantile(ev, 0.9), ev.max())
    env.close()


def _auto_reset_run(env, table_rows, use_rollout=False):
    """8 control steps with max_sim_step == 3: episodes end at steps 2 and 5.  After each truncating launch the base pose is the row
    predicted on the host from the step counter (meta word 1) read before that launch, and spawn_rows() agrees."""
    import torch
    from cosim_amd import spawn as sp
    assert env.max_sim_step == 3 and env.auto_reset and env.engine.query("spawn_mode") == 1
    n, gids = env.num_envs, env.env_id0 + np.arange(env.num_envs)
    poses = env.spawn_poses()
    acts = torch.tensor(np.random.default_rng(6).uniform(-0.3, 0.3, size=(8, n, env.action_dim)), dtype=torch.float32, device=env.device)
    used = []
    sc = _meta(env)[:, 1]
    env.reset()
    row = sp.episode_row(env.seed, gids, sc, table_rows)
    assert np.array_equal(env.spawn_rows(), row) and np.array_equal(_qpos(env)[0][:, :7], poses[row])
    used.append(row)
    if use_rollout:
        # two launches: 3 steps (the last one truncates: the pose can be read), then 5 (truncation at its step 2, two more steps after)
        for k0, K, k_trunc in ((0, 3, 2), (3, 5, 2)):
            sc = _meta(env)[:, 1]
            _, _, trunc, _ = env.rollout(acts[k0:k0 + K])
            assert trunc.cpu().numpy()[k_trunc].all() and trunc.cpu().numpy().sum() == n
            row = sp.episode_row(env.seed, gids, sc + k_trunc, table_rows)
            assert np.array_equal(env.spawn_rows(), row), (k0, env.spawn_rows(), row)
            if k_trunc == K - 1:
                assert np.array_equal(_qpos(env)[0][:, :7], poses[row])
            used.append(row)
    else:
        for t in range(8):
            sc = _meta(env)[:, 1]
            _, _, trunc, _ = env.step(acts[t])
            assert bool(trunc.all()) == (t in (2, 5)) and bool(trunc.any()) == (t in (2, 5)), t
            if t in (2, 5):
                row = sp.episode_row(env.seed, gids, sc, table_rows)
                assert np.array_equal(env.spawn_rows(), row), (t, env.spawn_rows(), row)
                assert np.array_equal(_qpos(env)[0][:, :7], poses[row]), t
                used.append(row)
    used = np.array(used)
    assert used.shape == (3, n) and all(np.unique(used[:, e]).size >= 2 for e in range(n)), used.T
    st = env.solver_stats()
    assert st["episodes_ended"] == 2 * n and st["nan_resets"] == 0
    return st


@pytest.mark.parametrize("case", ["step_plane", "rollout_plane", "hfield_fixup_stairs", "split_humanoid_stairs"])
def test_auto_reset_inside_the_kernels_draws_a_row_per_episode(case):
    robot, terrain, n, kw = {"step_plane": ("flamingo_light_v1", "flat", 16, {}),
                             "rollout_plane": ("flamingo_light_v1", "flat", 16, {}),
                             "hfield_fixup_stairs": ("flamingo_light_v1", "stairs_up_easy", 16, {"hfield_fixup": True}),
                             "split_humanoid_stairs": ("humanoid_p_v0", "stairs_up_hard", 4, {})}[case]
    cfg, cm = _model(robot, terrain, max_duration=0.06)
    env = _env(cfg, cm, n, auto_reset=True, seed=11, env_id0=5,
               spawn={"pattern": "poses", "poses": _table(cm, seed=4), "per_episode": True, "clearance": 0.01}, **kw)
    if case == "rollout_plane":
        assert env.engine.query("rollout") == 1
    if case == "hfield_fixup_stairs":
        assert env.engine.query("fixup_contact_slots") == 650
    if case == "split_humanoid_stairs":
        assert env.engine.query("split") > 0
    _auto_reset_run(env, 64, use_rollout=case == "rollout_plane")
    env.close()


@pytest.mark.parametrize("per_episode", [False, True])
def test_shards_that_set_the_same_table_give_the_results_of_one_fleet(per_episode):
    """16 envs at env_id0 0 against two engines of 8 at env_id0 0 and 8, GUI-default randomisation (sensor noise, action delay, mass
    and init noise), 8 steps with auto-resets at steps 2 and 5: bit-identical qpos, qvel and state."""
    import torch
    from cosim_amd.config import GUI_RANDOM_DEFAULTS
    cfg, cm = _model("flamingo_light_v1", "rocky_hard", random=dict(GUI_RANDOM_DEFAULTS), max_duration=0.06)
    spawn = {"pattern": "poses", "poses": _table(cm, seed=5), "per_episode": per_episode}
    full = _env(cfg, cm, 16, auto_reset=True, seed=7, env_id0=0, spawn=spawn)
    parts = [_env(cfg, cm, 8, auto_reset=True, seed=7, env_id0=i0, spawn=spawn) for i0 in (0, 8)]
    sf, _ = full.reset()
    sp_ = torch.cat([p.reset()[0] for p in parts])
    assert torch.equal(sf, sp_)
    acts = torch.tensor(np.random.default_rng(1).uniform(-1, 1, size=(8, 16, full.action_dim)), dtype=torch.float32, device=full.device)
    rows = [full.spawn_rows()]
    for t in range(8):
        sf, _, cf, _ = full.step(acts[t])
        sp_ = torch.cat([p.step(acts[t, 8 * i:8 * i + 8])[0] for i, p in enumerate(parts)])
        assert torch.equal(sf, sp_), t
        assert bool(cf.all()) == (t in (2, 5))
        (qf, vf), qs = _qpos(full), [_qpos(p) for p in parts]
        assert np.array_equal(qf, np.concatenate([q[0] for q in qs])) and np.array_equal(vf, np.concatenate([q[1] for q in qs])), t
        rows.append(full.spawn_rows())
    assert np.array_equal(full.spawn_rows(), np.concatenate([p.spawn_rows() for p in parts]))
    rows = np.array(rows)
    if per_episode:
        assert np.any(rows[-1] != rows[0])
    else:
        assert np.all(rows == np.arange(16) % 64)
    for e in [full] + parts:
        e.close()


def test_cli_spawn_flags_reach_the_engine_and_change_the_report(tmp_path, monkeypatch):
    import yaml
    from cosim_amd import batched_env, cli
    seen = []

    class Spy(batched_env.BatchedEnv):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            seen.append((int(self.engine.query("spawn_rows")), int(self.engine.query("spawn_mode"))))
    monkeypatch.setattr(batched_env, "BatchedEnv", Spy)
    base = ["--terrain", "rocky_hard", "--env", "w4_p_v2", "--num-envs", "16", "--steps", "5", "--policy", "sinusoid"]
    r0, r1 = tmp_path / "plain.json", tmp_path / "spawn.json"
    assert cli.main(base + ["--report", str(r0)]) == 0
    assert cli.main(base + ["--spawn", "uniform", "--spawn-count", "32", "--report", str(r1)]) == 0
    sess = tmp_path / "session.yaml"
    sess.write_text(yaml.safe_dump({"env": {"id": "w4_p_v2", "terrain": "rocky_hard"}, "engine": {"num_envs": 16}, "steps": 2,
                                    "spawn": {"pattern": "grid", "count": 9, "extent": 50.0, "per_episode": True}}))
    assert cli.main(["--config", str(sess)]) == 0
    assert cli.main(["--config", str(sess), "--spawn-count", "4", "--spawn-clearance", "0.02"]) == 0
    assert seen == [(0, 0), (32, 0), (9, 1), (4, 1)], seen
    a, b = json.loads(r0.read_text()), json.loads(r1.read_text())
    assert a["metrics"].keys() == b["metrics"].keys() and a["metrics"] != b["metrics"]
