"""Fall rules on the device (cosim_fall_set; the rule is in env_body, csrc/cosim_kernels.hip) against the numpy twin
(cosim_amd/fall.py reference_fall) applied to the poses read back from the device, and the episode-end machinery a fall rides on:
flags, info row, auto-reset, episode count, ledger, scenario cycle.

Fleets are at most 66 envs, runs at most 150 control steps.  Poses are chosen away from the thresholds (each test asserts that
where it matters), so the verdicts compared are exact: no tolerance, no quota.  Each test asserts that what it is about happened."""
import json
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TILT, HEIGHT, CONTACT = 1, 2, 4
_CACHE = {}


def _model(robot, terrain="flat", max_duration=120.0):
    from cosim_amd.compile import compile_model
    from cosim_amd.config import PARITY_RANDOM, make_config
    key = (robot, terrain, max_duration)
    if key not in _CACHE:
        cfg = make_config(robot, terrain=terrain, random=PARITY_RANDOM, max_duration=max_duration)
        _CACHE[key] = (cfg, compile_model(cfg))
    return _CACHE[key]


def _env(robot, n, terrain="flat", max_duration=120.0, **kw):
    from cosim_amd.batched_env import BatchedEnv
    cfg, cm = _model(robot, terrain, max_duration)
    env = BatchedEnv(cfg, num_envs=n, compiled=cm, seed=3, **kw)
    env.receive_user_command(np.zeros(max(env.command_dim, 1), dtype=np.float32))
    return env


def _init_qpos(cm):
    from cosim_amd.model import get_field
    return np.array(get_field(cm.blob, "init_qpos")[:cm.blob.nq], dtype=np.float64)


def _meta(env):
    t = env.torch
    buf = t.zeros((env.num_envs, 16), dtype=t.float32, device=env.device)
    env.engine.get("meta", buf.data_ptr(), env._stream())
    t.cuda.synchronize(env.device)
    return buf.view(t.int32).cpu().numpy().copy()


def _qpos(env):
    d = env.get_data()
    env.torch.cuda.synchronize(env.device)
    return d.qpos.cpu().numpy().copy(), d.qvel.cpu().numpy().copy()


def _zero(env):
    return env.torch.zeros((env.num_envs, env.action_dim), device=env.device)


def _quat(axis, angle):
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    return np.concatenate([[math.cos(angle / 2)], math.sin(angle / 2) * a])


def _qmul(a, b):
    w1, x1, y1, z1 = a
    w2, x2, y2, z2 = b
    return np.array([w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2,
                     w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2])


# ------------------------------------------------------------------------------------------------------------ 1: rule against twin
TILTS = (0.0, 0.3, 0.7, 0.9, 1.5, 3.0)
AXES = ([1, 0, 0], [0, 1, 0], [0.6, -0.8, 0])
# base heights below the 0.06 m rule, as (z, tilt, axis index): an inverted robot near the ground (tilt and height), and an upright
# one pushed deep into the plane, which one control step does not lift back over the threshold (height alone)
LOW = {"flamingo_light_v1": [(0.045, 3.0, 0), (0.045, 3.0, 1), (0.045, 3.0, 2), (0.03, 3.0, 0), (0.03, 3.0, 1), (0.03, 3.0, 2),
                             (-0.02, 0.0, 0), (-0.02, 0.0, 1), (-0.02, 0.0, 2), (-0.03, 0.0, 0), (-0.03, 0.0, 1), (-0.03, 0.0, 2)],
       "flamingo_p_v3": [(-0.3, 0.0, 0), (-0.35, 0.0, 1), (0.0, 3.0, 0), (0.0, 3.0, 1)],
       "w4_p_v2": [(-0.3, 0.0, 0), (0.03, 3.0, 1)]}
FLEET = {"flamingo_light_v1": 66, "flamingo_p_v3": 16, "w4_p_v2": 8}


def fall_poses(robot, cm):
    """``[n, nq]`` start poses: the six tilts about x, y and a mixed horizontal axis, each behind a yaw of its own, in the air (one
    control step of free fall moves the base 2.5 mm and turns nothing), repeated at further heights and yaws until the fleet is
    full but for the ``LOW`` poses."""
    q0, n = _init_qpos(cm), FLEET[robot]
    poses, i = [], 0
    while len(poses) < n - len(LOW[robot]):
        t, ax = TILTS[i % 6], AXES[(i // 6) % 3]
        q = q0.copy()
        q[2] = q0[2] + 1.0 + 0.1 * (i // 18)
        q[3:7] = _qmul(_quat([0, 0, 1], 0.9 + 0.37 * i), _quat(ax, t))
        poses.append(q)
        i += 1 if n >= 18 else 5          # (a fleet under 18 envs strides through the 18 poses: every tilt, every axis)
    for z, t, ia in LOW[robot]:
        q = q0.copy()
        q[2] = z
        q[3:7] = _qmul(_quat([0, 0, 1], -0.6), _quat(AXES[ia], t))
        poses.append(q)
    return np.array(poses)


@pytest.mark.parametrize("robot", ["flamingo_light_v1", "flamingo_p_v3", "w4_p_v2"])
def test_rule_equals_twin_on_poses_on_both_sides(robot):
    from cosim_amd.fall import FallRule, Terrain, base_height, reference_fall, up_component
    rule = FallRule(tilt=0.8, height=0.06)
    n = FLEET[robot]
    env = _env(robot, n, auto_reset=False, fall=rule)
    own = robot == "flamingo_p_v3"                  # its own _is_done body list stays on
    assert env.engine.query("fall") == (TILT | HEIGHT | (CONTACT if own else 0))
    poses = fall_poses(robot, env.cm)
    assert poses.shape == (n, env.nq)
    env.reset()
    env.set_state(qpos=poses, qvel=np.zeros((n, env.nv)), qacc_warmstart=np.zeros((n, env.nv)))
    _, term, trunc, _ = env.step(_zero(env))
    term, cause = term.cpu().numpy().astype(bool), env.end_cause().cpu().numpy()
    q, qv = _qpos(env)
    assert np.isfinite(q).all() and np.isfinite(qv).all() and int(trunc.sum()) == 0 and env.solver_stats()["nan_resets"] == 0
    # a property of the chosen poses, not of the rule: none ends the step near a threshold
    up, (hgt, inside) = up_component(q), base_height(q, Terrain.of(env.cm))
    print(f"[{robot}] closest to min_up: {np.abs(up - np.float32(rule.min_up)).min():.4f}, to min_height: {np.abs(hgt - np.float32(0.06)).min():.4f} m")
    assert inside.all() and (np.abs(up - np.float32(rule.min_up)) > 0.02).all() and (np.abs(hgt - np.float32(0.06)) > 0.005).all()
    want = reference_fall(q, 1, rule, Terrain.of(env.cm))
    assert np.array_equal(cause & 3, want), np.nonzero((cause & 3) != want)[0]
    if own:
        assert np.array_equal(term, cause != 0)    # bit 4: the model's own block (the existing parity tests check it against the oracle)
    else:
        assert np.array_equal(cause, want) and np.array_equal(term, want != 0)
    # every verdict occurs: upright, tilted alone, low alone, both
    assert {0, TILT, HEIGHT, TILT | HEIGHT} <= set(want.tolist())
    tilted = np.array([TILTS[i % 6] for i in range(18)]) > 0.8
    if n >= 18:
        assert np.array_equal((want[:18] & TILT) != 0, tilted)
    env.close()


# ------------------------------------------------------------------------------------------------------------ 2: heightfield
def _terrain_start(env, xy):
    """Poses over the points ``xy`` at ONE base height for all: the highest no-penetration placement among the points (the spawn
    kernel works it out per point) plus 2 cm.  The height of the base over the ground then differs from env to env purely by the
    ground beneath it."""
    rows = np.concatenate([np.asarray(xy, dtype=np.float32), np.zeros((len(xy), 1), dtype=np.float32)], axis=1)
    env.set_spawn(rows)
    placed = env.spawn_poses()
    env.set_spawn(None)
    q0 = _init_qpos(env.cm)
    poses = np.tile(q0, (len(xy), 1))
    poses[:, 0:2] = placed[:, 0:2]
    poses[:, 2] = placed[:, 2].max() + 0.02
    return poses


def _height_threshold(hgt):
    """The middle of the widest gap between the sorted start heights: envs on either side, as far from both as the points allow."""
    s = np.sort(hgt.astype(np.float64))
    i = int(np.argmax(np.diff(s)))
    return float(0.5 * (s[i] + s[i + 1])), float(s[i + 1] - s[i])


HF_CASES = {"humanoid_stairs": ("humanoid_p_v0", "stairs_up_hard", False), "humanoid_stairs_fixup": ("humanoid_p_v0", "stairs_up_hard", True),
            "light_rocky": ("flamingo_light_v1", "rocky_easy", None)}
HF_POINTS = {"stairs_up_hard": [(-3.0, 0.4), (-2.0, -0.3), (-1.0, 0.2), (0.0, 0.0), (1.0, -0.4), (2.0, 0.3), (3.0, -0.2), (4.0, 0.1)],
             "rocky_easy": [(-3.1, 1.3), (-1.7, -2.2), (-0.4, 0.9), (0.3, -0.6), (1.2, 2.4), (2.6, -1.1), (3.3, 0.2), (0.9, 3.1)]}


@pytest.mark.parametrize("case", sorted(HF_CASES))
def test_heightfield_rule_equals_twin(case):
    from cosim_amd.fall import FallRule, Terrain, base_height, reference_fall
    robot, terrain, fixup = HF_CASES[case]
    n, steps = 8, 6
    env = _env(robot, n, terrain=terrain, auto_reset=False, **({} if fixup is None else {"hfield_fixup": fixup}))
    if robot == "humanoid_p_v0":
        assert env.engine.query("split") > 0                      # the split pipeline: the rule runs in the last substep launch
    T = Terrain.of(env.cm)
    assert T.data is not None
    poses = _terrain_start(env, HF_POINTS[terrain])
    # two envs tilted past the rule, lifted clear of the ground
    for e in (2, 5):
        poses[e, 2] += 1.0
        poses[e, 3:7] = _quat([1, 0, 0], 1.1 if e == 2 else -1.3)
    hgt0, inside0 = base_height(poses.astype(np.float32), T)
    assert inside0.all()
    level = np.delete(hgt0, (2, 5))
    thr, gap = _height_threshold(level)
    print(f"[{case}] start heights over the ground {np.round(np.sort(level), 3).tolist()}, rule {thr:.3f} m (gap {gap:.3f} m)")
    assert gap > 0.02, "the points do not spread over different terrain heights"
    rule = FallRule(tilt=0.8, height=thr)
    env.set_fall(rule)
    assert env.engine.query("fall") == (TILT | HEIGHT)
    env.reset()
    env.set_state(qpos=poses, qvel=np.zeros((n, env.nv)), qacc_warmstart=np.zeros((n, env.nv)))
    pairs = excluded = seen_low = seen_tilt = 0
    for k in range(steps):
        _, term, _, _ = env.step(_zero(env))
        term, cause = term.cpu().numpy().astype(bool), env.end_cause().cpu().numpy()
        q, _ = _qpos(env)
        assert np.isfinite(q).all()
        h, inside = base_height(q, T)
        want = reference_fall(q, k + 1, rule, T)
        ok = ~(np.abs(h - np.float32(rule.min_height)) <= 1e-5)     # the band: the kernel may contract the interpolation into FMAs
        pairs += n
        excluded += int((~ok).sum())
        assert inside.all()
        assert np.array_equal(term[ok], want[ok] != 0), (k, np.nonzero(term != (want != 0))[0])
        assert np.array_equal(cause[ok & term], want[ok & term])    # (the word keeps an env's latest end: compared where this step ended one)
        seen_low += int(((want & HEIGHT) != 0).sum())
        seen_tilt += int(((want & TILT) != 0).sum())
    print(f"[{case}] {excluded} of {pairs} (env, step) pairs within 1e-5 m of the threshold: {excluded / pairs:.4%}")
    assert excluded <= pairs / 1000
    # under the rule purely because of the ground: level envs at one base height, some under, some over; and the tilted two
    assert 0 < int((level < thr).sum()) < len(level) and seen_low >= steps and seen_tilt >= 2 * steps
    assert env.solver_stats()["nan_resets"] == 0
    env.close()


# ------------------------------------------------------------------------------------------------------------ 3: episode end
SCN3 = [{}, {"pushes": [[10, 15, 3.0, 0.0, 0.0]]}, {"pushes": [[20, 25, -3.0, 0.0, 0.0]]}]


def test_a_fall_is_an_episode_end_like_any_other():
    """66 envs, scenario mode "cycle": scenario 1 / 2 pushes its env over at episode step 10 / 20 (3 m/s held for five steps), scenario
    0 does not.  A: the rule (tilt 0.8 rad), a ledger, every step issued as two uneven range launches joined afterwards.  B: the
    same fleet without a rule, stepped alongside: until an env of A first falls the two hold the same bits, so B's post-step pose is
    the pose A fell in (A has reset it away) and B's info row is the fallen step's."""
    import torch
    from cosim_amd.fall import FallRule, reference_fall
    from cosim_amd.ledger import FELL_TILT, TERMINATED, TRUNCATED, reference_ledger, same_records
    n, steps, limit = 66, 150, 100
    rule = FallRule(tilt=0.8)
    A = _env("flamingo_light_v1", n, max_duration=2.0, auto_reset=True, ledger=4, scenarios=SCN3, scenario_mode="cycle", fall=rule)
    B = _env("flamingo_light_v1", n, max_duration=2.0, auto_reset=True, scenarios=SCN3, scenario_mode="cycle")
    assert A.max_sim_step == limit and A.engine.query("fall") == TILT and B.engine.query("fall") == 0
    shards = [(0, 41), (41, 25)]
    streams = [torch.cuda.Stream(device=A.device) for _ in shards]
    A.reset(); B.reset()
    torch.cuda.synchronize(A.device)
    reset_state = A.state.cpu().numpy().copy()
    act = _zero(A)
    gid = np.arange(n)
    sync = np.ones(n, dtype=bool)                    # A and B still hold the same bits (no fall yet)
    fall_step = np.zeros(n, dtype=np.int64)
    info, te, tr, cmd, rows, causes = [], [], [], [], [], []
    for k in range(steps):
        before = _meta(A)
        for (first, count), st in zip(shards, streams):
            st.wait_stream(torch.cuda.current_stream(A.device))
            with torch.cuda.stream(st):
                A.step_range(first, count, act)
        for st in streams:
            torch.cuda.current_stream(A.device).wait_stream(st)
        A.join()
        B.step(act)
        torch.cuda.synchronize(A.device)
        after = _meta(A)
        a_te, a_tr = A.terminated.cpu().numpy().astype(bool), A.truncated.cpu().numpy().astype(bool)
        a_info, a_state = A.info_buf.cpu().numpy().copy(), A.state.cpu().numpy().copy()
        info.append(a_info); te.append(a_te); tr.append(a_tr); causes.append(after[:, 15].copy())
        cmd.append(A.applied_command.cpu().numpy()[:, :A.command_dim].copy()); rows.append(A.scenario_rows().astype(np.int32))
        assert np.array_equal(rows[-1], (gid + before[:, 11]) % 3)             # cycle: one scenario per episode
        if sync.any() and k < limit:
            qb, _ = _qpos(B)
            want = reference_fall(qb, k + 1, rule)
            if k == limit - 1:                       # the time limit: both fleets reset, B's pose is no longer the end-of-step pose
                assert a_tr[sync].all() and not a_te[sync].any() and (after[sync, 15] == 0).all()
                sync[:] = False
                continue
            assert (before[sync, 0] == k).all()
            assert np.array_equal(a_te[sync], want[sync] != 0), k
            fell = sync & a_te
            if fell.any():
                assert not a_tr[fell].any() and (after[fell, 15] == TILT).all()
                # the info row is the fallen step's; the state vector is a reset observation, every stack row filled with it
                assert np.array_equal(a_info[fell].view(np.uint32), B.info_buf.cpu().numpy()[fell].view(np.uint32))
                assert np.array_equal(a_state[fell].view(np.uint32), reset_state[fell].view(np.uint32))
                sd, S = A._stacked_obs_dim, A.stack_size
                assert S > 1 and all(np.array_equal(a_state[fell, :sd], a_state[fell, j * sd:(j + 1) * sd]) for j in range(1, S))
                assert (after[fell, 11] == before[fell, 11] + 1).all() and (after[fell, 0] == 0).all()
                fall_step[fell] = k + 1
                sync[fell] = False
            still = sync & ~a_te
            assert (after[still, 11] == before[still, 11]).all() and (after[still, 15] == 0).all()
            assert np.array_equal(a_state[still].view(np.uint32), B.state.cpu().numpy()[still].view(np.uint32))
    # the known subset fell in its first episode, when its push came; the others ran into the time limit with cause 0
    assert (fall_step[gid % 3 == 0] == 0).all() and (fall_step[gid % 3 != 0] > 0).all()
    assert (fall_step[gid % 3 == 1] > 10).all() and (fall_step[gid % 3 == 1] < 40).all() and (fall_step[gid % 3 == 2] > 20).all()
    led = A.ledger()
    first = led.episode == 0
    assert np.array_equal(led.env[first], gid)
    pushed = gid % 3 != 0
    assert (led.flags[first][pushed] == (TERMINATED | FELL_TILT)).all() and np.array_equal(led.length[first][pushed], fall_step[pushed])
    assert (led.flags[first][~pushed] == TRUNCATED).all() and (led.length[first][~pushed] == limit).all()
    # the env that fell runs the next scenario in its next episode (asserted per step above) -- scenario 0's envs meet the push of
    # scenario 1 in their second episode and fall there
    second = (led.episode == 1) & np.isin(led.env, gid[gid % 3 == 0])
    assert second.sum() == (gid % 3 == 0).sum() and (led.flags[second] == (TERMINATED | FELL_TILT)).all() and (led.scenario[second] == 1).all()
    twin = reference_ledger(np.stack(info), np.stack(te), np.stack(tr), np.stack(cmd), None, None, 4, A.action_dim, A.command_dim,
                            scenario_rows=np.stack(rows), causes=np.stack(causes))
    diff = same_records(led, twin)
    assert diff is None, diff
    c = led.counts()
    assert c["fell"] == c["fell_tilt"] == int(np.stack(te).sum()) >= n and c["fell_height"] == c["fell_contact"] == 0 and c["lost"] == 0
    by = led.by_scenario()
    assert by[0]["fell"] == 0 and by[1]["fell_share"] == 1.0 and by[2]["fell_share"] == 1.0
    assert A.solver_stats()["episodes_ended"] == int((np.stack(te) | np.stack(tr)).sum())
    A.close(); B.close()


# ------------------------------------------------------------------------------------------------------------ 4: grace
def test_grace_holds_the_rule_off_and_no_longer():
    from cosim_amd.fall import FallRule
    n = 8
    env = _env("flamingo_light_v1", n, auto_reset=False)
    q0 = _init_qpos(env.cm)
    poses = np.tile(q0, (n, 1))
    poses[:, 2] = 3.0                                # in the air for the whole test: the tilt stays what it is
    poses[1::2, 3:7] = _quat([0.6, -0.8, 0], 1.2)    # odd envs: tilted past the rule
    for grace in (0, 3, 7):
        env.set_fall(FallRule(tilt=0.8, grace=grace))
        env.reset()
        env.set_state(qpos=poses, qvel=np.zeros((n, env.nv)), qacc_warmstart=np.zeros((n, env.nv)))
        for k in range(1, grace + 3):                # k: the episode clock of the step
            _, term, _, _ = env.step(_zero(env))
            term = term.cpu().numpy()
            assert not term[0::2].any()
            assert (term[1::2] == (1 if k > grace else 0)).all(), (grace, k)
        assert (env.end_cause().cpu().numpy()[1::2] == TILT).all()
    env.close()


# ------------------------------------------------------------------------------------------------------------ 5: every path
def _fleet5(n, **kw):
    return _env("flamingo_light_v1", n, max_duration=1.0, auto_reset=True, **kw)


def _start5(env):
    """Reset, then three envs in four roll off with 3 .. 4 m/s, forwards or backwards: they pitch over within a dozen steps (falls inside the run), the
    auto-reset stands them up again and they run into the time limit (step 50) like the rest."""
    from cosim_amd.fall import FallRule
    env.set_fall(FallRule(tilt=0.8, height=0.06))
    env.reset()
    n = env.num_envs
    q, _ = _qpos(env)
    qvel = np.zeros((n, env.nv), dtype=np.float32)
    e = np.arange(n)
    qvel[:, 0] = np.where(e % 4 == 0, 0.0, 3.0 + 0.5 * (e % 4 - 1)) * np.where(e % 8 < 4, 1.0, -1.0)
    env.set_state(qpos=q, qvel=qvel, qacc_warmstart=np.zeros((n, env.nv)))


def _table5(n, steps, nu):
    rng = np.random.default_rng(21)
    return rng.uniform(-0.2, 0.2, size=(steps, n, nu)).astype(np.float32)


def _final5(env):
    q, qv = _qpos(env)
    return {"qpos": q, "qvel": qv, "meta": _meta(env)}


def _loop5(env, steps, step=None):
    t = env.torch
    tb = t.tensor(_table5(env.num_envs, steps, env.action_dim), device=env.device)
    _start5(env)
    out = {"state": [], "terminated": [], "truncated": [], "info": []}
    for k in range(steps):
        if step is None:
            env.step(tb[k])
        else:
            step(k, tb)
        env.join()
        t.cuda.synchronize(env.device)
        out["state"].append(env.state.cpu().numpy().copy()); out["info"].append(env.info_buf.cpu().numpy().copy())
        out["terminated"].append(env.terminated.cpu().numpy().copy()); out["truncated"].append(env.truncated.cpu().numpy().copy())
    out = {k: np.stack(v) for k, v in out.items()}
    out.update(_final5(env))
    return out


def _same5(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        x, y = a[k], b[k]
        if x.dtype == np.float32:
            x, y = x.view(np.uint32), y.view(np.uint32)
        assert np.array_equal(x, y), f"{what}: {k} differs"


def _reference5():
    """The step loop on the default path: 64 envs, 120 steps.  Shared, never modified."""
    if "ref5" not in _CACHE:
        env = _fleet5(64)
        assert env.engine.query("step_kernel") == 1
        r = _loop5(env, 120)
        assert env.engine.query("fall") == (TILT | HEIGHT)
        env.close()
        te, tr = r["terminated"].astype(bool), r["truncated"].astype(bool)
        e = np.arange(64)
        # what the comparisons are about: falls inside the run, by the rule, and time limits after them
        assert te[:30, e % 4 != 0].any(axis=0).all() and not te[:, e % 4 == 0].any() and tr[49, e % 4 == 0].all() and tr[50:].any()
        assert (r["meta"][:, 4] == 0).all() and set(r["meta"][:, 15].tolist()) == {0}   # the latest end of every env: a time limit
        _CACHE["ref5"] = r
    return _CACHE["ref5"]


def test_general_kernel_and_ranges_give_the_same_bits():
    ref = _reference5()
    env = _fleet5(64)
    env.engine.set_param("step_kernel", np.array([0.0]))
    assert env.engine.query("step_kernel") == 0
    _same5(ref, _loop5(env, 120), "general kernel (step_kernel 0)")
    env.close()
    env = _fleet5(64, ranges=4)
    assert env.engine.query("ranges") == 4
    _same5(ref, _loop5(env, 120), "4 ranges")
    env.close()


def test_two_envs_per_wave_kernel_applies_the_rule_exactly():
    """The two-envs-per-wave kernel sums in another order than the default one (test_two_envs_per_wave_variant_agrees_with_the_
    default_kernel: same physics, not the same bits), so its rule is held to the twin on its OWN poses, step by step, exactly: the
    same roll-off start without auto-reset, so the pose a step ended in can be read back.  The two halves of a wave are different
    envs: env 2i stands while env 2i + 1 falls, and each half must get its own verdict."""
    from cosim_amd.fall import FallRule, reference_fall
    rule = FallRule(tilt=0.8, height=0.06)
    env = _env("flamingo_light_v1", 64, max_duration=1.0, auto_reset=False)
    env.engine.set_param("envs_per_wave", np.array([2.0]))
    t = env.torch
    tb = t.tensor(_table5(64, 30, env.action_dim), device=env.device)
    _start5(env)
    assert env.engine.query("fall") == (TILT | HEIGHT)
    seen, pairs = set(), 0
    split_waves = 0
    for k in range(30):
        _, term, _, _ = env.step(tb[k])
        term, meta = term.cpu().numpy().astype(bool), _meta(env)
        q, _ = _qpos(env)
        ok = meta[:, 4] == 0                        # (a non-finite state is the non-finite check's case: reset, cause 0)
        want = reference_fall(q, k + 1, rule)
        assert np.array_equal(term[ok], want[ok] != 0), (k, np.nonzero(term != (want != 0))[0])
        assert np.array_equal(meta[ok & term, 15], want[ok & term]), k
        pairs += int(ok.sum())
        seen |= set(want[ok].tolist())
        split_waves += int((term[0::2] != term[1::2]).sum())
    assert pairs >= 30 * 60 and {0, TILT} <= seen and (TILT | HEIGHT) in seen and split_waves > 0
    env.close()


def test_captured_graph_gives_the_same_bits():
    import torch
    ref = _reference5()
    g = _fleet5(64)
    buf = torch.empty((64, g.action_dim), device=g.device)
    graph = []

    def replay(k, tb):
        buf.copy_(tb[k])
        if k == 0:                                   # the first step eagerly on a side stream, then one step recorded (not run)
            side = torch.cuda.Stream(device=g.device)
            torch.cuda.synchronize(g.device)
            side.wait_stream(torch.cuda.current_stream(g.device))
            with torch.cuda.stream(side):
                g.step(buf)
            torch.cuda.current_stream(g.device).wait_stream(side)
            torch.cuda.synchronize(g.device)
            graph.append(torch.cuda.CUDAGraph())
            with torch.cuda.graph(graph[0]):
                g.step(buf)
        else:
            graph[0].replay()
    _same5(ref, _loop5(g, 120, replay), "captured step")
    g.close()


def test_rollout_rows_are_the_step_loop():
    ref = _reference5()
    env = _fleet5(64)
    assert env.engine.query("rollout") == 1
    t = env.torch
    tb = t.tensor(_table5(64, 120, env.action_dim), device=env.device)
    _start5(env)
    states, term, trunc, inf = env.rollout(tb)
    t.cuda.synchronize(env.device)
    out = {"state": states.cpu().numpy(), "terminated": term.cpu().numpy(), "truncated": trunc.cpu().numpy(), "info": inf.cpu().numpy()}
    out.update(_final5(env))
    # rows, flags and the physics state bit for bit; of the meta words the clocks, the episode count and the cause (a rollout launch
    # keeps its solver counters per launch)
    words = [0, 1, 2, 4, 11, 15]
    _same5({k: (v[:, words] if k == "meta" else v) for k, v in ref.items()}, {k: (v[:, words] if k == "meta" else v) for k, v in out.items()},
           "rollout")
    assert out["terminated"][:30].any() and out["truncated"][49:].any()
    env.close()


@pytest.fixture(scope="module")
def drop_poses():
    """Eight pre-step states whose control step ends with more than 14 ground contacts (the fleet kernel gives such a step up and
    the large-capacity kernel redoes it): the robot dropped in an arbitrary pose, as in test_gpu_step_kernel.py.  They lie on the
    ground in arbitrary orientations: under a height rule they fall by construction."""
    from oracle.oracle import Oracle
    cfg, cm = _model("flamingo_light_v1")
    q0 = _init_qpos(cm)
    o = Oracle(cm)
    rng = np.random.default_rng(3)
    R = dict(qpos=[], qvel=[], warm=[], act=[])
    for trial in range(200):
        q = q0.copy()
        quat = rng.normal(size=4)
        q[2] = rng.uniform(0.05, 0.25)
        q[3:7] = quat / np.linalg.norm(quat)
        q[7:] += rng.uniform(-0.3, 0.3, size=q.size - 7)
        o.reset(q)
        for t in range(2):
            a = 0.3 * np.sin(0.3 * t + np.arange(4))
            pre = (o.qpos.copy(), o.qvel.copy(), o.qacc_warmstart.copy(), a)
            o.control_step(a)
            if o.ncon > 14:
                for k, v in zip(("qpos", "qvel", "warm", "act"), pre):
                    R[k].append(v)
        if len(R["qpos"]) >= 8:
            break
    assert len(R["qpos"]) >= 8
    return {k: np.array(v[:8]) for k, v in R.items()}


def test_the_fixup_path_applies_the_rule_the_same(drop_poses):
    from cosim_amd.fall import FallRule, Terrain, reference_fall
    rule = FallRule(tilt=0.8, height=0.3)            # every one of these poses is under 0.3 m
    res = []
    for sk in (1, 0):
        env = _env("flamingo_light_v1", 8, auto_reset=False, fall=rule)
        env.engine.set_param("step_kernel", np.array([float(sk)]))
        assert env.engine.query("step_kernel") == sk and env.engine.query("contact_slots") == 14
        env.reset()
        env.set_state(drop_poses["qpos"], drop_poses["qvel"], drop_poses["warm"])
        act = env.torch.tensor(drop_poses["act"], dtype=env.torch.float32, device=env.device)
        rows = {"state": [], "terminated": [], "info": [], "cause": []}
        for t in range(2):
            env.step(act)
            env.torch.cuda.synchronize(env.device)
            rows["state"].append(env.state.cpu().numpy().copy()); rows["info"].append(env.info_buf.cpu().numpy().copy())
            rows["terminated"].append(env.terminated.cpu().numpy().copy()); rows["cause"].append(env.end_cause().cpu().numpy().copy())
            q, _ = _qpos(env)
            want = reference_fall(q, t + 1, rule, Terrain.of(env.cm))
            assert (want & HEIGHT).all() and np.array_equal(rows["cause"][-1], want) and rows["terminated"][-1].all()
        out = {k: np.stack(v) for k, v in rows.items()}
        out.update(_final5(env))
        stats = env.solver_stats()
        assert stats["fixup_steps"] > 0 and stats["dropped_contacts"] == 0 and stats["max_contacts"] > 14
        env.close()
        res.append(out)
    _same5(res[0], res[1], "fix-up path, step_kernel 1 against 0")


# ------------------------------------------------------------------------------------------------------------ 6: body rule
BODIES = ["base_link", "left_leg_link", "right_leg_link"]


def test_body_rule_on_a_robot_that_has_none():
    """flamingo_light_v1 with the body list its reference env has commented out.  Envs 0..3 stand; 4..7 lie on their front (pitched a
    quarter turn: the base rests on the ground with ~50 N), 8..11 on their back (inverted: ~9 N).  All at rest after 25 steps
    without a rule, so the verdict does not hinge on a contact switching on: the forces are 9 and 50 times the 1.0 threshold or
    exactly zero (a standing robot touches the ground with wheels and casters, which are bodies of their own)."""
    from cosim_amd.fall import FallRule
    from oracle.oracle import Oracle
    n = 12
    env = _env("flamingo_light_v1", n, auto_reset=False)
    cm = env.cm
    q0 = _init_qpos(cm)
    poses = np.tile(q0, (n, 1))
    for e in range(4, 8):
        poses[e, 2], poses[e, 3:7] = 0.3, _qmul(_quat([0, 0, 1], 0.3 * e), _quat([0, 1, 0], 1.5))
    for e in range(8, 12):
        poses[e, 2], poses[e, 3:7] = 0.3, _qmul(_quat([0, 0, 1], 0.3 * e), _quat([1, 0, 0] if e % 2 else [0, 1, 0], 3.1))
    env.reset()
    env.set_state(qpos=poses, qvel=np.zeros((n, env.nv)), qacc_warmstart=np.zeros((n, env.nv)))
    for _ in range(25):
        _, term, _, _ = env.step(_zero(env))
    assert int(term.sum()) == 0 and env.engine.query("fall") == 0          # no rule: nothing ends, however the robot lies
    q, qv = _qpos(env)
    assert np.abs(qv).max() < 0.5 and (q[4:, 2] < 0.1).all() and (q[:4, 2] > 0.12).all()
    env.set_fall(FallRule(bodies=BODIES))
    assert env.engine.query("fall") == CONTACT
    _, term, _, _ = env.step(_zero(env))
    term, cause = term.cpu().numpy(), env.end_cause().cpu().numpy()
    assert term.tolist() == [0] * 4 + [1] * 8 and cause.tolist() == [0] * 4 + [CONTACT] * 8
    # the same verdict from the oracle's cfrc_ext of those bodies after the same control step from the same state
    ids = [cm.body_names.index(b) for b in BODIES]
    o = Oracle(cm)
    peak = []
    for e in range(n):
        o.reset(q[e].astype(np.float64), qv[e].astype(np.float64))
        o.control_step(np.zeros(env.action_dim))
        peak.append(float(o.cfrc_ext[ids].max()))
    print("[body rule] largest cfrc_ext component of the listed bodies per env (oracle):", np.round(peak, 2).tolist())
    assert [p > 1.0 for p in peak] == [False] * 4 + [True] * 8
    assert all(p == 0.0 for p in peak[:4]) and all(p > 4.0 for p in peak[4:])          # nowhere near the threshold
    env.close()


# ------------------------------------------------------------------------------------------------------------ 7: off means off
def test_a_cleared_rule_leaves_no_trace():
    from cosim_amd.fall import FallRule
    n, steps = 32, 35
    rng = np.random.default_rng(8)
    actions = rng.uniform(-0.6, 0.6, size=(steps, n, 4)).astype(np.float32)
    x = _env("flamingo_light_v1", n, max_duration=0.4, auto_reset=True, fall=FallRule(tilt=0.8, height=0.06, grace=2, bodies=BODIES))
    y = _env("flamingo_light_v1", n, max_duration=0.4, auto_reset=True)
    assert x.engine.query("fall") == 7 and y.engine.query("fall") == 0 and x.max_sim_step == 20
    t = x.torch
    x.reset(); y.reset()
    for k in range(steps):
        if k == 5:
            x.set_fall(None)
            assert x.engine.query("fall") == 0 and x.fall_rule is None
        for env in (x, y):
            env.step(t.tensor(actions[k], device=env.device))
        t.cuda.synchronize(x.device)
        assert np.array_equal(x.state.cpu().numpy().view(np.uint32), y.state.cpu().numpy().view(np.uint32)), k
        assert t.equal(x.terminated, y.terminated) and t.equal(x.truncated, y.truncated)
        assert np.array_equal(x.info_buf.cpu().numpy().view(np.uint32), y.info_buf.cpu().numpy().view(np.uint32))
    # the whole record, meta word 15 included: episodes ended (the time limit, step 20) after the rule was cleared and wrote nothing
    rx, ry = x.snapshot().rows.cpu().numpy(), y.snapshot().rows.cpu().numpy()
    assert np.array_equal(rx.view(np.uint32), ry.view(np.uint32))
    assert (_meta(x)[:, 15] == 0).all() and x.solver_stats()["episodes_ended"] >= n
    x.close(); y.close()


def test_p_v3_own_termination_is_back_after_an_override_is_cleared():
    from cosim_amd.fall import FallRule
    n = 4
    env = _env("flamingo_p_v3", n, auto_reset=False)
    q0 = _init_qpos(env.cm)
    poses = np.tile(q0, (n, 1))
    poses[:, 2] = 0.25
    poses[:, 3:7] = _quat([1, 0, 0], 1.5)            # on its side: hip and shoulder links carry it (~150 N, oracle)
    env.reset()
    env.set_state(qpos=poses, qvel=np.zeros((n, env.nv)), qacc_warmstart=np.zeros((n, env.nv)))
    for _ in range(25):
        env.step(_zero(env))

    def term():
        _, te, _, _ = env.step(_zero(env))
        return te.cpu().numpy().tolist()
    assert term() == [1] * n and env.engine.query("fall") == 0            # its own _is_done
    env.set_fall(FallRule(bodies=[]))                                      # no body rule at all
    assert env.engine.query("fall") == 0 and term() == [0] * n
    env.set_fall(FallRule(tilt=3.0, bodies=[]))                            # a tilt rule that does not fire here, still no body rule
    assert env.engine.query("fall") == TILT and term() == [0] * n
    env.set_fall(FallRule(tilt=3.0))                                       # the model's own list again, its hits recorded
    assert env.engine.query("fall") == (TILT | CONTACT) and term() == [1] * n and env.end_cause().cpu().numpy().tolist() == [CONTACT] * n
    env.set_fall(None)
    assert env.engine.query("fall") == 0 and term() == [1] * n
    env.close()


# ------------------------------------------------------------------------------------------------------------ 8: refusals, CLI
def test_refusals_through_the_c_abi():
    env = _env("flamingo_light_v1", 4, auto_reset=False)
    nbody = env.engine.query("nbody")
    with pytest.raises(ValueError, match=r"body id 0 is not a body of the robot"):
        env.engine.fall_set(-1.0, 0.0, 0, [1, 0])
    with pytest.raises(ValueError, match=rf"body id {nbody} is not a body"):
        env.engine.fall_set(-1.0, 0.0, 0, [nbody])
    with pytest.raises(ValueError, match=r"body id -3 "):
        env.engine.fall_set(0.5, 0.0, 0, [-3])
    with pytest.raises(ValueError, match=r"grace_steps -1 is negative"):
        env.engine.fall_set(0.5, 0.0, -1, None)
    with pytest.raises(ValueError, match=r"min_up is not finite"):
        env.engine.fall_set(float("nan"), 0.0, 0, None)
    with pytest.raises(ValueError, match=r"the model has no body 'tail_link'"):
        env.set_fall({"bodies": ["base_link", "tail_link"]})
    assert env.engine.query("fall") == 0 and env.fall_rule is None        # nothing was set by the refused calls
    env.engine.fall_set(0.5, 0.1, 3, [nbody - 1])
    assert env.engine.query("fall") == 7
    env.engine.fall_set(-1.0, 0.0, 0, None)
    assert env.engine.query("fall") == 0
    env.reset()
    env.step(_zero(env))
    assert np.isfinite(env.state.cpu().numpy()).all()
    env.close()


@pytest.mark.parametrize("path", ["--graph", "--pipelined"])
def test_cli_fall_rule_on_the_fast_paths(tmp_path, capsys, path):
    from cosim_amd import cli
    from cosim_amd.ledger import EpisodeLedger
    report, records = tmp_path / "r.json", tmp_path / "episodes.npz"
    assert cli.main(["--env", "flamingo_light_v1", "--num-envs", "32", "--steps", "60", "--max-duration", "0.5", "--seed", "5", "--policy",
                     "random-mlp", "--fall-tilt", "0.8", "--fall-height", "0.05", "--fall-grace", "2", path, "--ledger", "4",
                     "--ledger-out", str(records), "--report", str(report)]) == 0
    r = json.loads(report.read_text())
    c = EpisodeLedger.load(str(records)).counts()
    ep = r["episodes"]
    assert ep["episodes"] == c["episodes"] >= 32
    assert (ep["fell"], ep["fell_tilt"], ep["fell_height"], ep["fell_contact"]) == (c["fell"], c["fell_tilt"], c["fell_height"], c["fell_contact"])
    assert ep["fell"] <= ep["terminated"] and "fell" in ep["by_spawn_row"]["-1"]
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line["episodes"]["fell"] == c["fell"] and line["control_steps"] == 60
