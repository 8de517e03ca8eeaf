"""Heightfield fix-up (engine scalar "hfield_fixup", opt-in): on heightfield terrain a control step -- on the split pipeline of
humanoid_p_v0 a substep -- whose ground contacts exceed the fleet kernel's slots is given up before anything is written and redone by
a kernel with 50 (mjMAXCONPAIR) slots per ground geom, the most the narrowphase can emit.  MuJoCo's arena keeps every contact
(reference flamingo_light_v1.py:154, do_simulation); with the path on nothing is left out for want of a slot, and every state is
compared against the fp64 oracle, the overflowing ones included.  With the path off (the default) the engine is unchanged: those
tests live in test_gpu_parity.py."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _meta(env):
    """Per-env engine counters [N, 16] (cosim_get "meta"): [8] dropped contacts, [10] most contacts, [12] fix-up passes,
    [13] truncated walks."""
    t = env.torch
    buf = t.zeros((env.num_envs, 16), dtype=t.float32, device=env.device)
    env.engine.get("meta", buf.data_ptr(), env._stream())
    t.cuda.synchronize(env.device)
    return buf.view(t.int32).cpu().numpy().astype(np.int64)


def _stairs_states(o, b, q0, rng, spots, steps, amp, lying=False):
    """test_gpu_parity._stairs_states, plus `lying`: the robot spawned on its back or front (pitch +-90 degrees) 12 cm above the local
    terrain, so that its first steps lay the torso and limbs across stair edges -- hundreds of prism contacts, up to ~800 -- and
    `nsub`: the most contacts of any substep of the step (the same control step replayed one mj_step at a time; `ncon` is the last
    substep's count, and a robot landing on the steps gains contacts inside the step)."""
    R = dict(qpos=[], qvel=[], warm=[], act=[], qpos1=[], qvel1=[], ncon=[], tq=[], nsub=[])
    for spot in range(spots):
        q = q0.copy()
        q[0:2] = rng.uniform(-3.5, 3.5, size=2)                          # anywhere in the pit: floor, treads, risers' edges
        yaw = rng.uniform(-np.pi, np.pi)
        q[3:7] = [np.cos(yaw / 2), 0, 0, np.sin(yaw / 2)]
        q[2] = q0[2] + (10.0 - o.ray_down(q[0], q[1], 10.0)) + 0.02
        if lying:                                                        # yaw, then pitch +-90 degrees about the body y axis
            c, s, h = np.cos(yaw / 2), np.sin(yaw / 2), np.sqrt(0.5) * rng.choice([-1.0, 1.0])
            q[3:7] = [c * np.sqrt(0.5), -s * h, c * h, s * np.sqrt(0.5)]
            q[2] = (10.0 - o.ray_down(q[0], q[1], 10.0)) + 0.12
        o.reset(q)
        for t in range(steps):
            a = np.clip(amp * rng.normal(size=b.nu), -1, 1)
            R["qpos"].append(o.qpos.copy()); R["qvel"].append(o.qvel.copy()); R["warm"].append(o.qacc_warmstart.copy()); R["act"].append(a)
            tq = o.control_step(a)
            R["qpos1"].append(o.qpos.copy()); R["qvel1"].append(o.qvel.copy()); R["ncon"].append(o.ncon); R["tq"].append(tq)
            assert not o.bad
            post = (o.qpos.copy(), o.qvel.copy(), o.qacc_warmstart.copy())
            o.reset(R["qpos"][-1], R["qvel"][-1])
            o.qacc_warmstart[:] = R["warm"][-1]
            o.ctrl[:] = tq
            nsub = 0
            for _ in range(b.frame_skip):
                o.step()
                nsub = max(nsub, o.ncon)
            R["nsub"].append(nsub)
            o.reset(post[0], post[1])
            o.qacc_warmstart[:] = post[2]
    return {k: np.array(v) for k, v in R.items()}


@pytest.fixture(scope="module")
def light_stairs():
    """flamingo_light_v1 on stairs_up_easy (1 cm cells), the states of test_heightfield_terrain_replay_and_height_map: 12 spots x 40
    steps, default_rng(11)."""
    from cosim_amd.compile import compile_model
    from cosim_amd.config import PARITY_RANDOM, make_config
    from cosim_amd.model import get_field
    from oracle.oracle import Oracle
    cfg = make_config("flamingo_light_v1", terrain="stairs_up_easy", random=PARITY_RANDOM)
    cm = compile_model(cfg)
    b = cm.blob
    half = 0.7 * b.hfield_size[0]
    rng = np.random.default_rng(11)
    o = Oracle(cm)
    q0 = np.array(get_field(b, "init_qpos")[:b.nq])
    R = dict(qpos=[], qvel=[], warm=[], act=[], qpos1=[], qvel1=[], ncon=[])
    for spot in range(12):
        q = q0.copy()
        q[0:2] = rng.uniform(-half, half, size=2)
        yaw = rng.uniform(-np.pi, np.pi)
        q[3:7] = [np.cos(yaw / 2), 0, 0, np.sin(yaw / 2)]
        q[2] = q0[2] + (10.0 - o.ray_down(q[0], q[1], 10.0)) + 0.02
        o.reset(q)
        for t in range(40):
            a = np.clip(0.1 * rng.normal(size=b.nu), -1, 1)
            R["qpos"].append(o.qpos.copy()); R["qvel"].append(o.qvel.copy()); R["warm"].append(o.qacc_warmstart.copy()); R["act"].append(a)
            o.control_step(a)
            R["qpos1"].append(o.qpos.copy()); R["qvel1"].append(o.qvel.copy()); R["ncon"].append(o.ncon)
    return dict(cfg=cfg, cm=cm, o=o, R={k: np.array(v) for k, v in R.items()})


@pytest.fixture(scope="module")
def humanoid_stairs():
    """BASELINE config 5 (humanoid_p_v0, stairs_up_hard, position command): the states of test_humanoid_on_stairs_up_hard_with_position_
    command (standing to fallen, at most ~100 contacts) and 32 lying spawns x 8 steps (about one state in five above the fleet kernel's
    256 slots)."""
    from cosim_amd.compile import compile_model
    from cosim_amd.config import PARITY_RANDOM, make_config
    from cosim_amd.model import get_field
    from oracle.oracle import Oracle
    cfg = make_config("humanoid_p_v0", terrain="stairs_up_hard", random=PARITY_RANDOM, position_command=True)
    cfg["observation"]["command_dim"] = 2
    cm = compile_model(cfg)
    b = cm.blob
    o = Oracle(cm)
    q0 = np.array(get_field(b, "init_qpos")[:b.nq])
    R1 = _stairs_states(o, b, q0, np.random.default_rng(21), spots=16, steps=40, amp=0.5)
    R2 = _stairs_states(o, b, q0, np.random.default_rng(22), spots=32, steps=8, amp=0.5, lying=True)
    R = {k: np.concatenate([R1[k], R2[k]]) for k in R1}
    return dict(cfg=cfg, cm=cm, o=o, R=R, n_standing=len(R1["qpos"]))


def _light_env(ls, n, **kw):
    from cosim_amd.batched_env import BatchedEnv
    return BatchedEnv(ls["cfg"], num_envs=n, auto_reset=False, compiled=ls["cm"], **kw)


def _replay(env, R, target=None):
    import torch
    if target is not None:
        env.receive_user_command(target)
    env.reset()
    env.set_state(R["qpos"], R["qvel"], R["warm"])
    state, _, _, _ = env.step(torch.tensor(R["act"], dtype=torch.float32, device=env.device))
    d = env.get_data()
    qp, qv = d.qpos.cpu().numpy().astype(np.float64), d.qvel.cpu().numpy().astype(np.float64)
    w = torch.empty((env.num_envs, env.nv), device=env.device)
    env.engine.get("qacc_warmstart", w.data_ptr(), env._stream())
    torch.cuda.synchronize(env.device)
    return dict(qp=qp, qv=qv, warm=w.cpu().numpy(), state=state.cpu().numpy().copy(), info=env.info_buf.cpu().numpy().copy(),
                meta=_meta(env), st=env.solver_stats())


def _dbg_contacts(dbg):
    """Every contact of a debug forward pass: (geom code, dist, pos[3] base-relative, normal[3]) from the 8-float records at 4096."""
    n = min(int(dbg[0]), 512)
    rec = np.asarray(dbg[4096:4096 + 8 * n]).reshape(n, 8)
    return [(int(r[7]), float(r[0]), r[1:4].copy(), r[4:7].copy()) for r in rec]


def test_light_v1_on_stairs_keeps_every_contact_and_follows_the_oracle_in_every_state(light_stairs):
    """flamingo_light_v1 on 1 cm stairs: 128 ground-contact slots in the fleet kernel, up to 230 contacts in the oracle.  With the
    fix-up on (650 slots = 50 x 13 ground geoms) nothing is left out, the overflowing steps are redone, every state follows the
    oracle within the bounds of test_heightfield_terrain_replay_and_height_map (no capacity mask), and the prism contact sets of the
    overflowing states -- dumped by a debug pass at the fix-up's capacity -- are the oracle's."""
    R, o = light_stairs["R"], light_stairs["o"]
    n = len(R["qpos"])
    env = _light_env(light_stairs, n, hfield_fixup=True)
    assert env.engine.query("contact_slots") == 128 and env.engine.query("fixup_contact_slots") == 650
    assert R["ncon"].max() > 128
    r = _replay(env, R)
    st = r["st"]
    ep = np.abs(r["qp"] - R["qpos1"]).max(axis=1)
    ev = np.abs(r["qv"] - R["qvel1"]).max(axis=1)
    over = R["ncon"] > 128
    print(f"[light stairs] overflow states {int(over.sum())} (> 136: {int((R['ncon'] > 136).sum())}), fixup_steps {st['fixup_steps']}, "
          f"max_contacts {st['max_contacts']} (oracle {R['ncon'].max()}); |dqpos| median {np.median(ep):.2e} q90 {np.quantile(ep, 0.9):.2e} "
          f"max {ep.max():.2e}; |dqvel| median {np.median(ev):.2e} q90 {np.quantile(ev, 0.9):.2e} max {ev.max():.2e}; "
          f"overflow states |dqvel| max {ev[over].max():.2e}")
    assert st["dropped_contacts"] - st["truncated_walks"] == 0 and st["nan_resets"] == 0
    assert int((R["ncon"] > 128 + 8).sum()) <= st["fixup_steps"] <= n
    assert st["max_contacts"] >= R["ncon"].max() - 8
    assert np.median(ep) < 2e-5 and np.quantile(ep, 0.9) < 2e-4, (np.median(ep), np.quantile(ep, 0.9), ep.max())
    assert np.median(ev) < 1e-3 and np.quantile(ev, 0.9) < 2e-2, (np.median(ev), np.quantile(ev, 0.9), ev.max())
    # --- narrowphase parity of the overflowing states (more than 128 oracle contacts in the state itself): same prisms hit, same
    # depth / position / normal
    env.set_state(R["qpos"], R["qvel"], R["warm"])
    same_set = tight = total = 0
    loose = [0, 0, 0]
    sample = []
    for w in range(n):
        o.reset(R["qpos"][w], R["qvel"][w])
        o.forward()
        if o.ncon > 128:
            sample.append(w)
    assert len(sample) >= 3, sample
    for w in sample:
        o.reset(R["qpos"][w], R["qvel"][w])
        o.forward()
        oc = o.contacts()
        dbg = env.engine.debug_forward(int(w))
        base = R["qpos"][w][:3].copy(); base[2] = 0.0
        key = lambda c: (c[0], round(float(c[2][0]), 3), round(float(c[2][1]), 3))
        gl = sorted([(gg & 255, gd, gp + base, gn) for gg, gd, gp, gn in _dbg_contacts(dbg) if (gg >> 8) == 0], key=key)
        ol = sorted([(int(c[7]), c[0], c[1:4], c[4:7]) for c in oc if c[9] < 0], key=key)
        if len(gl) != len(ol) or any(a[0] != c[0] for a, c in zip(gl, ol)):
            continue
        same_set += 1
        for a, c in zip(gl, ol):
            total += 1
            ok = (abs(a[1] - c[1]) < 2e-5, np.abs(a[3] - c[3]).max() < 2e-3, np.abs(a[2] - c[2]).max() < 2e-3)
            tight += all(ok)
            loose[0] += not ok[0]; loose[1] += not ok[1]; loose[2] += not ok[2]
    print(f"[light stairs] overflow contact sets: {same_set} of {len(sample)} equal, {tight} of {total} contacts tight "
          f"(outside: depth {loose[0]}, normal {loose[1]}, position {loose[2]})")
    # (tight: measured 85 %, the 93 % of the states that fit is not reached -- a fallen robot's 130-230 contacts are mostly on prism
    # ridges, where the fp32 portal lands on the other face)
    assert same_set >= 0.97 * len(sample) and total > 128 and tight >= 0.8 * total, (same_set, len(sample), tight, total)
    env.close()


@pytest.mark.parametrize("split", [1, 0])
def test_humanoid_on_stairs_up_hard_keeps_every_contact(humanoid_stairs, split):
    """BASELINE config 5 with the fix-up on, on the split pipeline (default: the solver substep is what is redone, 1100 = 50 x 22
    slots) and on the fused kernel ("split" 0: the control step is).  States from standing to fallen and lying across the stairs, up to
    ~800 oracle contacts against the fleet kernel's 256 slots: nothing is left out, and the most contacts seen in a substep is the oracle's
    (its per-substep maximum: a robot landing on the steps gains contacts inside the control step).  The standing-to-fallen states of
    test_humanoid_on_stairs_up_hard_with_position_command keep that test's bounds; over ALL states the medians keep them and the tail
    is wider (measured, split / fused: |dqpos| q75 9.8e-4 / 8.0e-4, q95 1.9e-2; |dqvel| q75 8.3e-2 / 8.1e-2).  Cause: the lying spawns
    drop 12 cm onto stair edges with hundreds of contacts each -- prism ridges, where fp32 / fp64 MPR portals land on either face, and
    an impact that amplifies the difference.  The overflowing states are exactly those impacts: the fp64 oracle itself, started from
    the state rounded to fp32, lands a median 9.6e-3 away from its own result there (2.9e-5 in the lying states that fit); the engine's
    median there (1.2e-2 / 1.3e-2) is held to within 3x of that sensitivity, measured again in the test."""
    import torch
    from cosim_amd.batched_env import BatchedEnv
    R = humanoid_stairs["R"]
    n = len(R["qpos"])
    over = R["nsub"] > 256
    stand = np.arange(n) < humanoid_stairs["n_standing"]
    assert over.sum() >= 20 and R["nsub"].max() > 400
    env = BatchedEnv(humanoid_stairs["cfg"], num_envs=n, auto_reset=False, compiled=humanoid_stairs["cm"], hfield_fixup=True)
    if not split:
        env.engine.set_param("split", np.array([0.0]))
    assert env.engine.query("contact_slots") == 256 and env.engine.query("fixup_contact_slots") == 1100
    assert (env.engine.query("split") > 0) == bool(split)
    target = np.random.default_rng(4).uniform(-3, 3, size=(n, 2)).astype(np.float32)
    r = _replay(env, R, target)
    st = r["st"]
    ep = np.abs(r["qp"] - R["qpos1"]).max(axis=1)
    ev = np.abs(r["qv"] - R["qvel1"]).max(axis=1)
    print(f"[humanoid stairs split={split}] overflow states {int(over.sum())}, fixup_steps {st['fixup_steps']}, max_contacts "
          f"{st['max_contacts']} (oracle {R['ncon'].max()}); |dqpos| median {np.median(ep):.2e} q75 {np.quantile(ep, 0.75):.2e} "
          f"q95 {np.quantile(ep, 0.95):.2e} max {ep.max():.2e}; |dqvel| median {np.median(ev):.2e} q75 {np.quantile(ev, 0.75):.2e} "
          f"max {ev.max():.2e}; |dqpos| median: overflow states {np.median(ep[over]):.2e}, lying states that fit "
          f"{np.median(ep[~stand & ~over]):.2e}, standing-to-fallen {np.median(ep[stand]):.2e}")
    assert st["dropped_contacts"] - st["truncated_walks"] == 0 and st["nan_resets"] == 0
    assert abs(st["max_contacts"] - R["nsub"].max()) <= 3 and R["nsub"].max() >= R["ncon"].max()
    assert st["fixup_steps"] >= int((R["nsub"] > 256 + 8).sum())
    np.testing.assert_allclose(env.info_buf[:, 4:4 + env.action_dim].cpu().numpy(), R["tq"], rtol=1e-4, atol=2e-3)
    o = humanoid_stairs["o"]
    sens = []
    for w in np.flatnonzero(over):                                       # the oracle's own sensitivity to fp32 rounding of the input
        o.reset(R["qpos"][w].astype(np.float32).astype(np.float64), R["qvel"][w].astype(np.float32).astype(np.float64))
        o.qacc_warmstart[:] = R["warm"][w].astype(np.float32)
        o.control_step(R["act"][w])
        sens.append(np.abs(o.qpos - R["qpos1"][w]).max())
    print(f"[humanoid stairs split={split}] overflow states: engine |dqpos| median {np.median(ep[over]):.2e}, oracle from fp32-rounded "
          f"input {np.median(sens):.2e}")
    assert np.median(ep[over]) < 3 * np.median(sens)
    es, vs = ep[stand], ev[stand]
    assert np.median(es) < 2e-5 and np.quantile(es, 0.75) < 5e-4 and np.quantile(es, 0.95) < 2e-2, (np.median(es), np.quantile(es, [0.75, 0.95]))
    assert np.median(vs) < 2e-3 and np.quantile(vs, 0.75) < 5e-2, (np.median(vs), np.quantile(vs, 0.75))
    assert np.median(ep) < 2e-5 and np.quantile(ep, 0.75) < 2e-3 and np.quantile(ep, 0.95) < 5e-2, (np.median(ep), np.quantile(ep, [0.75, 0.95]))
    assert np.median(ev) < 2e-3 and np.quantile(ev, 0.75) < 2e-1, (np.median(ev), np.quantile(ev, 0.75))
    env.close()


def _unchanged_where_it_fits(make_env, R, target=None):
    off = _replay(make_env(False), R, target)
    on = _replay(make_env(True), R, target)
    flagged = on["meta"][:, 12] > 0
    dropped_off = (off["meta"][:, 8] - off["meta"][:, 13]) > 0
    assert flagged.any() and np.array_equal(flagged, dropped_off), (np.flatnonzero(flagged), np.flatnonzero(dropped_off))
    assert off["st"]["fixup_steps"] == 0 and on["st"]["dropped_contacts"] == on["st"]["truncated_walks"]
    keep = ~flagged
    for k in ("qp", "qv", "warm", "state", "info"):
        assert np.array_equal(off[k][keep], on[k][keep]), k
    return int(flagged.sum())


def test_envs_that_fit_are_bit_identical_with_the_fixup_on(light_stairs, humanoid_stairs):
    """The fix-up only ever touches envs the fleet kernel flagged: every other env's qpos, qvel, qacc_warmstart, state vector and
    info are bit-identical with "hfield_fixup" 0 and 1, and the flagged envs are exactly those the off-run left contacts out for --
    on the fused kernel (flamingo_light_v1) and on the split pipeline (humanoid_p_v0), where a substep is flagged."""
    from cosim_amd.batched_env import BatchedEnv
    R = light_stairs["R"]
    nl = _unchanged_where_it_fits(lambda on: _light_env(light_stairs, len(R["qpos"]), hfield_fixup=on), R)
    H = humanoid_stairs["R"]
    n = len(H["qpos"])
    target = np.random.default_rng(4).uniform(-3, 3, size=(n, 2)).astype(np.float32)
    nh = _unchanged_where_it_fits(lambda on: BatchedEnv(humanoid_stairs["cfg"], num_envs=n, auto_reset=False, compiled=humanoid_stairs["cm"],
                                                        hfield_fixup=on), H, target)
    print(f"[unchanged] flagged envs: light {nl} of {len(R['qpos'])}, humanoid {nh} of {n}")


def test_ranges_deferred_join_and_graph_replay_equal_one_eager_launch(humanoid_stairs):
    """With the fix-up on, a humanoid stairs fleet stepped as 4 ranges with a deferred join, and replayed from a captured HIP graph,
    is bit-identical to single eager launches; overflowing envs sit in every range (the fix-up launches go on the range's stream,
    behind each solver launch of the range)."""
    import torch
    from cosim_amd.batched_env import BatchedEnv
    H = humanoid_stairs["R"]
    n = len(H["qpos"])
    perm = np.random.default_rng(0).permutation(n)
    R = {k: v[perm] for k, v in H.items()}
    K = 4
    rng = np.random.default_rng(9)
    acts = torch.tensor(np.clip(0.5 * rng.normal(size=(K, n, R["act"].shape[1])), -1, 1), dtype=torch.float32, device="cuda:0")

    def make(**kw):
        e = BatchedEnv(humanoid_stairs["cfg"], num_envs=n, auto_reset=False, compiled=humanoid_stairs["cm"], hfield_fixup=True, **kw)
        e.receive_user_command(np.zeros(2, dtype=np.float32))
        e.reset()
        e.set_state(R["qpos"], R["qvel"], R["warm"])
        return e
    a = make()
    for t in range(K):
        a.step(acts[t])
    torch.cuda.synchronize()
    c = make(ranges=4, deferred_join=True)
    c_first = [f for f, _ in c.range_list]
    buf = torch.empty_like(acts[0])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())

    def one():
        c.step(buf)
        c.join()
    buf.copy_(acts[0])
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        one()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    fix0 = c.solver_stats()["fixup_steps"]
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        one()
    for t in range(1, K):
        buf.copy_(acts[t])
        g.replay()
    torch.cuda.synchronize()
    ma, mc = _meta(a), _meta(c)
    sa, sc = a.solver_stats(), c.solver_stats()
    ranges_hit = {int(np.searchsorted(c_first, e, side="right")) - 1 for e in np.flatnonzero(mc[:, 12] > 0)}
    print(f"[ranges + graph] fixup passes {sc['fixup_steps']} ({sc['fixup_steps'] - fix0} in the replays), ranges with flagged envs {sorted(ranges_hit)}")
    assert len(ranges_hit) >= 2 and sc["fixup_steps"] > fix0 > 0
    assert sa["step_count"] == sc["step_count"] and np.array_equal(ma, mc)
    assert torch.equal(a.state, c.state) and torch.equal(a.info_buf, c.info_buf)
    assert torch.equal(a.get_data().qpos, c.get_data().qpos) and torch.equal(a.get_data().qvel, c.get_data().qvel)
    a.close(); c.close()


def test_interface_rejects_what_has_no_fixup_and_the_cli_reaches_the_engine(light_stairs, monkeypatch, tmp_path):
    """"hfield_fixup" 1 is refused on the plane (the plane's own fix-up is always on) and with two envs per wave; "fixup" 0 after it
    switches it off again (the drops come back); --hfield-fixup and the session file's key reach the engine."""
    import yaml
    from cosim_amd import batched_env, cli
    from cosim_amd.config import make_config
    plane = make_config("flamingo_light_v1", num_envs=64)
    with pytest.raises(ValueError):
        batched_env.BatchedEnv(plane, num_envs=64, auto_reset=False, hfield_fixup=True)
    e = batched_env.BatchedEnv(plane, num_envs=64, auto_reset=False)
    e.engine.set_param("envs_per_wave", np.array([2.0]))
    with pytest.raises(ValueError):
        e.engine.set_param("hfield_fixup", np.array([1.0]))
    e.close()
    R = light_stairs["R"]
    n = len(R["qpos"])
    env = _light_env(light_stairs, n)
    assert env.engine.query("fixup_contact_slots") == 0
    env.engine.set_param("hfield_fixup", np.array([1.0]))
    assert env.engine.query("fixup_contact_slots") == 650
    env.engine.set_param("fixup", np.array([0.0]))
    assert env.engine.query("fixup_contact_slots") == 0
    with pytest.raises(ValueError):
        env.engine.set_param("hfield_fixup", np.array([1.0]))
    r = _replay(env, R)
    assert r["st"]["fixup_steps"] == 0 and r["st"]["dropped_contacts"] - r["st"]["truncated_walks"] > 0
    env.close()
    seen = []

    class Spy(batched_env.BatchedEnv):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            seen.append(int(self.engine.query("fixup_contact_slots")))
    monkeypatch.setattr(batched_env, "BatchedEnv", Spy)
    base = ["--env", "flamingo_light_v1", "--terrain", "stairs_up_easy", "--num-envs", "64", "--steps", "2"]
    assert cli.main(base) == 0
    assert cli.main(base + ["--hfield-fixup"]) == 0
    sess = tmp_path / "session.yaml"
    sess.write_text(yaml.safe_dump({"env": {"id": "flamingo_light_v1", "terrain": "stairs_up_easy"}, "engine": {"num_envs": 64},
                                    "steps": 2, "hfield_fixup": True}))
    assert cli.main(["--config", str(sess)]) == 0
    assert seen == [0, 650, 650], seen
