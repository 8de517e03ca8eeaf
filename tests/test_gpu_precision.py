"""The HIP path at the reference's other precision levels (config/random_table.yaml: low 10 ms x 2, high 2.5 ms x 8, ultra
1.25 ms x 16, extreme 0.625 ms x 32 substeps; Newton iterations 50 / 75 / 75 / 100), against the fp64 oracle built from the same
compiled blob.  The medium-level tests live in test_gpu_parity.py / test_gpu_envlayer.py; this file repeats their comparisons with
the level changed and the same bounds, except where a docstring says otherwise and cites the oracle measurement the bound rests on.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LEVELS = {"low": (0.010, 2, 50), "medium": (0.005, 4, 50), "high": (0.0025, 8, 75), "ultra": (0.00125, 16, 75),
          "extreme": (0.000625, 32, 100)}
EDGE_LEVELS = ["low", "high", "extreme"]


def _setup(env_id, level, terrain="flat", **kw):
    from cosim_amd.compile import compile_model
    from cosim_amd.config import PARITY_RANDOM, make_config
    from cosim_amd.model import get_field
    cfg = make_config(env_id, terrain=terrain, random=dict(PARITY_RANDOM, precision=level), **kw)
    cm = compile_model(cfg)
    b = cm.blob
    assert (b.timestep, b.frame_skip, b.iterations) == LEVELS[level]
    return cfg, cm, b, np.array(get_field(b, "init_qpos")[:b.nq])


def _env(cfg, cm, n, **kw):
    from cosim_amd.batched_env import BatchedEnv
    env = BatchedEnv(cfg, num_envs=n, auto_reset=kw.pop("auto_reset", False), compiled=cm, **kw)
    assert env.engine.query("frame_skip") == cm.blob.frame_skip
    return env


def _tri_to_dense(tri, nv):
    M = np.zeros((nv, nv))
    e = 0
    for r in range(nv):
        for c in range(r + 1):
            M[r, c] = M[c, r] = tri[e]
            e += 1
    return M


def _sin_action(t, phase=np.array([0.0, 1.0, 2.0, 3.0])):
    return 0.25 * np.sin(2 * np.pi * 0.5 * 0.02 * t + phase)


def _record(o, steps, action, term_ids=None):
    """States along an oracle trajectory and where one control step takes each."""
    R = dict(qpos=[], qvel=[], warm=[], act=[], qpos1=[], qvel1=[], tq=[], ncon=[], term=[])
    for t in range(steps):
        a = action(t)
        R["qpos"].append(o.qpos.copy()); R["qvel"].append(o.qvel.copy()); R["warm"].append(o.qacc_warmstart.copy()); R["act"].append(a)
        tq = o.control_step(a)
        R["qpos1"].append(o.qpos.copy()); R["qvel1"].append(o.qvel.copy()); R["tq"].append(tq); R["ncon"].append(o.ncon)
        R["term"].append(bool((o.cfrc_ext[term_ids] > 1.0).any()) if term_ids is not None else False)
        assert not o.bad
    return {k: np.array(v) for k, v in R.items()}


def _replay(env, R):
    import torch
    env.reset()
    env.set_state(R["qpos"], R["qvel"], R["warm"])
    _, term, _, info = env.step(torch.tensor(R["act"], dtype=torch.float32, device=env.device))
    d = env.get_data()
    return d.qpos.cpu().numpy().astype(np.float64), d.qvel.cpu().numpy().astype(np.float64), term.cpu().numpy().astype(bool), info


# ---------------------------------------------------------------------------------------------------------------- solver caps

@pytest.mark.parametrize("level", list(LEVELS))
def test_newton_cap_is_the_models_iterations_unless_lowered(level):
    """The solver runs with the level's own Newton iteration count (50 / 50 / 75 / 75 / 100), not with an engine default below it;
    an explicit "max_newton" still caps, and is still bounded by the model.  The line search keeps its deliberate cap of 24
    evaluations against the models' ls_iterations = 50 (cosim.h).  Behaviour: with the cap lowered to 1 the step takes at most one
    Newton iteration per env and substep, and the default takes more than that on the same states.  (Which states would need
    more than 50 iterations is not known: the solver also stops on a zero step and on an improvement below tolerance, and in an
    fp64 probe at extreme no solve took more than 8.  So the default is pinned through the query, which reads the same function
    that fills the kernel's arguments; the behavioural part alone would also pass with a default cap of 50.)"""
    import torch
    cfg, cm, b, q0 = _setup("flamingo_light_v1", level)
    n = 64
    env = _env(cfg, cm, n)
    assert env.engine.query("max_newton") == b.iterations == LEVELS[level][2]
    assert env.engine.query("max_ls") == 24 and b.ls_iterations == 50
    for cap, want in ((30, 30), (500, b.iterations), (-1, b.iterations), (1, 1)):
        env.engine.set_param("max_newton", np.array([float(cap)]))
        assert env.engine.query("max_newton") == want, (cap, want)
    env.engine.set_param("max_ls", np.array([60.0]))
    assert env.engine.query("max_ls") == 50
    env.engine.set_param("max_ls", np.array([24.0]))
    # states along the all-contact-modes trajectory (within the fleet kernel's slots: no redo launch adds iterations of its own)
    from oracle.oracle import Oracle
    o = Oracle(cm)
    o.reset(q0)
    R = _record(o, n, _sin_action)
    assert R["ncon"].max() <= 14
    counts = {}
    for cap in (1, -1):
        env.engine.set_param("max_newton", np.array([float(cap)]))
        env.reset()
        before = env.solver_stats()["newton_iters"]
        env.set_state(R["qpos"], R["qvel"], R["warm"])
        env.step(torch.tensor(R["act"], dtype=torch.float32, device=env.device))
        counts[cap] = env.solver_stats()["newton_iters"] - before
    subs = n * b.frame_skip
    print(f"[newton cap {level}] Newton iterations per substep: cap 1 {counts[1] / subs:.2f}, default {counts[-1] / subs:.2f}")
    assert 0 < counts[1] <= subs and counts[-1] > counts[1], (counts, subs)
    env.close()


# ------------------------------------------------------------------------------------------------------------- forward stages

@pytest.mark.parametrize("level", EDGE_LEVELS)
def test_forward_stages_match_oracle_at_level(level):
    """test_forward_stages_match_oracle at the initial pose and at a resting pose (wheels and casters on the ground): the
    reference acceleration of every constraint row depends on h (refsafe: solref time constant >= 2h, and at `low` the default
    0.02 is exactly 2h), so qacc and qfrc_constraint see whether the device steps with the level's timestep.  The medium test
    compares only the contact-free initial pose, where the bounds are the medium ones.  At the resting pose (6 contacts, 40 rows),
    qfrc_constraint keeps the medium bound.  qacc there differs from the oracle by 2.3e-3 / 7.9e-3 / 6.0e-3 at low / medium / high
    (measured; |qacc| max 0.35), the same at medium, the headline level, and unchanged with the fp32 solver tolerance at 1e-8:
    the fp32 solve's floor on a stiff contact set, where a 4e-4 N force difference moves light dofs' accelerations.  So qacc
    is held there to 1e-2, the medium level's measured gap with margin."""
    import torch
    from oracle.oracle import Oracle
    cfg, cm, b, q0 = _setup("flamingo_light_v1", level)
    o = Oracle(cm)
    o.reset(q0)
    for _ in range(60):
        o.control_step(np.zeros(4))
    rest = (o.qpos.copy(), o.qvel.copy())
    env = _env(cfg, cm, 4)
    env.reset()
    nv, nb = 18, 14
    for qp, qv in ((q0, np.zeros(nv)), rest):
        o.reset(qp, qv)
        o.forward()
        env.set_state(np.tile(qp, (4, 1)), np.tile(qv, (4, 1)), np.zeros((4, nv)))
        D = env.engine.debug_forward(0)
        assert (int(D[0]), int(D[1]), int(D[2]), int(D[3]), int(D[4])) == (o.ncon, o.nefc, o.ne, o.nf, o.nl)
        base = np.r_[qp[:2], 0.0]                                  # (the engine works in a frame that follows the base in x, y)
        np.testing.assert_allclose(D[64 + 3:64 + nb * 3].reshape(nb - 1, 3) + base, o.xpos[1:], atol=1e-6)   # (body 0: the world)
        np.testing.assert_allclose(D[192:192 + nb * 4].reshape(nb, 4), o.xquat, atol=1e-6)
        np.testing.assert_allclose(D[1200:1200 + nv * 6].reshape(nv, 6), o.cdof, atol=1e-6)
        M = _tri_to_dense(D[512:512 + nv * (nv + 1) // 2], nv)
        assert np.abs(M - o.M).max() < 1e-5 * np.abs(o.M).max()
        np.testing.assert_allclose(D[1140:1140 + nv], o.qfrc_bias, atol=1e-4)
        np.testing.assert_allclose(D[1720:1720 + o.ncon], o.contacts()[:, 0], atol=1e-6)
        np.testing.assert_allclose(D[1000:1000 + nv], o.qacc, rtol=1e-4, atol=2e-3 if qp is q0 else 1e-2)
        np.testing.assert_allclose(D[1040:1040 + nv], o.qfrc_constraint, rtol=1e-4, atol=1e-3)
    assert o.ncon >= 4                                         # the resting pose does have ground contacts
    env.close()


# ------------------------------------------------------------------------------------------------- one-control-step replays

def _oracle_spread(cm, R, draws=6, eps=1e-6):
    """Per state: how far the fp64 oracle's own control step lands from the recorded one when its start (qpos, qvel) is moved by
    `eps` relative -- about the size of an fp32 engine's round-off over one substep.  Returns (max |dqpos|, max |dqvel|) over
    `draws` random moves.  A state where this already exceeds a bound sits on a branch point (a contact or joint limit switching
    on within the step one substep earlier or later); one-step parity is not defined there at that bound."""
    from oracle.oracle import Oracle
    o = Oracle(cm)
    rng = np.random.default_rng(0)
    n, nq, nv = len(R["qpos"]), R["qpos"].shape[1], R["qvel"].shape[1]
    dq, dv = np.zeros(n), np.zeros(n)
    for i in range(n):
        for _ in range(draws):
            o.reset(R["qpos"][i] * (1 + eps * rng.standard_normal(nq)), R["qvel"][i] * (1 + eps * rng.standard_normal(nv)) + eps * rng.standard_normal(nv))
            o.view("qacc_warmstart")[:] = R["warm"][i]
            o.control_step(R["act"][i])
            dq[i] = max(dq[i], np.abs(o.qpos - R["qpos1"][i]).max())
            dv[i] = max(dv[i], np.abs(o.qvel - R["qvel1"][i]).max())
    return dq, dv


@pytest.mark.parametrize("level", ["low", "high", pytest.param("extreme", marks=pytest.mark.xfail(strict=True, reason=(
    "open: states 302, 308, 385 land past 1.5x the oracle's 6-draw spread (385: 9.0e-4 against 1.9e-4, while 8 draws of the same "
    "probe reach 9.0e-4); the spread estimate is too coarse at 32 substeps (DESIGN.md §8)")))])
def test_one_control_step_replay_over_all_contact_modes_at_level(level):
    """test_one_control_step_replay_over_all_contact_modes with the trajectory recorded by the oracle at the level: the dense
    fleet kernel, same bounds per state, except where the oracle itself spreads wider under a 1e-6 move of the start
    (_oracle_spread): there the engine must land within 1.5x that spread.  Measured: at high states 65 and 108 and at extreme states 48, 183 and 385 the engine misses qpos by
    1.4e-3 / 2.3e-3 / 1.3e-3 / 8.9e-4 / 9.0e-4, and the oracle moved by 1e-6 lands within 1 % of exactly those misses (worst dofs 10, 16,
    17): a contact that switches on one substep earlier or later.  (At medium no state is on such a branch: the worst
    miss is 1.5e-5.)"""
    from oracle.oracle import Oracle
    cfg, cm, b, q0 = _setup("flamingo_light_v1", level)
    T = 400
    o = Oracle(cm)
    o.reset(q0)
    R = _record(o, T, _sin_action)
    assert R["ncon"].min() == 0 and R["ncon"].max() >= 6
    sq, sv = _oracle_spread(cm, R)
    allow_q, allow_v = np.maximum(1e-4, 1.5 * sq), np.maximum(5e-3, 1.5 * sv)
    env = _env(cfg, cm, T)
    qp, qv, _, info = _replay(env, R)
    np.testing.assert_allclose(info["torque"].cpu().numpy(), R["tq"], atol=2e-4)
    ep = np.abs(qp - R["qpos1"]).max(axis=1)
    ev = np.abs(qv - R["qvel1"]).max(axis=1)
    wide = np.flatnonzero((ep > 1e-4) | (ev > 5e-3))
    print(f"[replay light_v1 {level}] states past the medium bounds {wide.tolist()}: engine |dqpos| {ep[wide].round(6).tolist()}, "
          f"oracle spread {sq[wide].round(6).tolist()}; |dqvel| median {np.median(ev):.2e}")
    assert (ep <= allow_q).all(), [(i, ep[i], sq[i]) for i in np.flatnonzero(ep > allow_q)]
    assert (ev <= allow_v).all(), [(i, ev[i], sv[i]) for i in np.flatnonzero(ev > allow_v)]
    assert np.median(ev) < 5e-4 and len(wide) <= 8, (np.median(ev), wide)
    env.close()


@pytest.mark.parametrize("env_id,steps,level", [(e, s, lv) for e, s in (("flamingo_p_v3", 45), ("w4_p_v2", 100), ("humanoid_p_v0", 80))
                                                for lv in EDGE_LEVELS if (e, lv) != ("humanoid_p_v0", "extreme")] + [
    pytest.param("humanoid_p_v0", 80, "extreme", marks=pytest.mark.xfail(strict=True, reason=(
        "open: 97 % |dqpos| quantile over the states the oracle's spread calls well posed is 4.3e-4 against 2e-4 (DESIGN.md §8)")))])
def test_other_robots_one_control_step_replay_flat_at_level(env_id, steps, level):
    """test_other_robots_one_control_step_replay_flat at the level: torque, the replay quantiles and the cfrc_ext termination
    agreement (flamingo_p_v3), same bounds: the quantiles over the states where the oracle's own spread under a 1e-6 move of the
    start stays below 1e-4 in qpos (_oracle_spread), the maxima per state widened to 1.5x that spread where it is larger.  Measured for humanoid_p_v0 at extreme: states 20, 55 and 62 miss qpos by 2.8e-3 / 1.6e-3 / 1.8e-3, a contact
    switching on at substep 20 of 32 (found per substep), and the oracle moved by 1e-6 lands at 2.8e-3 / 1.2e-3 / 1.8e-3."""
    from cosim_amd.model import get_field
    from oracle.oracle import Oracle
    cfg, cm, b, q0 = _setup(env_id, level)
    o = Oracle(cm)
    o.reset(q0)
    rng = np.random.default_rng(3)
    ids = list(get_field(b, "term_body")[:b.nterm_body]) if b.term_mode == 1 else None
    R = _record(o, steps, lambda t: np.clip(0.15 * rng.normal(size=b.nu), -1, 1), ids)
    sq, sv = _oracle_spread(cm, R)
    posed = sq < 1e-4
    assert posed.mean() > 0.7, posed.mean()
    env = _env(cfg, cm, steps)
    qp, qv, term, info = _replay(env, R)
    np.testing.assert_allclose(info["torque"].cpu().numpy(), R["tq"], rtol=1e-4, atol=2e-3)
    st = env.solver_stats()
    assert st["dropped_contacts"] == 0 and st["dropped_limit_rows"] == 0
    ep_all, ev_all = np.abs(qp - R["qpos1"]).max(axis=1), np.abs(qv - R["qvel1"]).max(axis=1)
    ep, ev = ep_all[posed], ev_all[posed]
    print(f"[replay {env_id} {level}] branch-point states {np.flatnonzero(~posed).tolist()}; well posed: |dqpos| q97 {np.quantile(ep, 0.97):.2e} "
          f"max {ep.max():.2e}; |dqvel| median {np.median(ev):.2e} q97 {np.quantile(ev, 0.97):.2e} max {ev.max():.2e}")
    assert np.quantile(ep, 0.97) < 2e-4 and np.quantile(ev, 0.97) < 2e-2 and np.median(ev_all) < 2e-3, (np.quantile(ep, 0.97), np.quantile(ev, 0.97))
    assert (ep_all <= np.maximum(2e-3, 1.5 * sq)).all(), [(i, ep_all[i], sq[i]) for i in np.flatnonzero(ep_all > np.maximum(2e-3, 1.5 * sq))]
    assert (ev_all <= np.maximum(0.5, 1.5 * sv)).all(), [(i, ev_all[i], sv[i]) for i in np.flatnonzero(ev_all > np.maximum(0.5, 1.5 * sv))]
    if b.term_mode == 1:
        agree = (term == R["term"]).mean()
        print(f"[replay {env_id} {level}] termination flags agree on {agree:.3%} ({int(R['term'].sum())} terminal in the oracle)")
        assert agree > 0.9
    env.close()


@pytest.mark.parametrize("level", EDGE_LEVELS)
def test_w4_on_rocky_hard_replay_at_level(level):
    """test_heightfield_terrain_replay_and_height_map's w4_p_v2 / rocky_hard replay (prism MPR, contact-twist kernel) at the level:
    robots dropped at scattered places, one control step from every state, same quantile bounds; nothing is left out."""
    from oracle.oracle import Oracle
    cfg, cm, b, q0 = _setup("w4_p_v2", level, terrain="rocky_hard")
    half = 0.7 * b.hfield_size[0]
    rng = np.random.default_rng(11)
    o = Oracle(cm)
    parts = []
    for spot in range(8):
        q = q0.copy()
        q[0:2] = rng.uniform(-half, half, size=2)
        yaw = rng.uniform(-np.pi, np.pi)
        q[3:7] = [np.cos(yaw / 2), 0, 0, np.sin(yaw / 2)]
        q[2] = q0[2] + (10.0 - o.ray_down(q[0], q[1], 10.0)) + 0.02
        o.reset(q)
        parts.append(_record(o, 30, lambda t: np.clip(0.1 * rng.normal(size=b.nu), -1, 1)))
    R = {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}
    assert R["ncon"].max() >= 4
    env = _env(cfg, cm, len(R["qpos"]))
    qp, qv, _, _ = _replay(env, R)
    st = env.solver_stats()
    ep = np.abs(qp - R["qpos1"]).max(axis=1)
    ev = np.abs(qv - R["qvel1"]).max(axis=1)
    print(f"[rocky w4 {level}] contacts max {R['ncon'].max()} (device {st['max_contacts']}), dropped {st['dropped_contacts']}; "
          f"|dqpos| median {np.median(ep):.2e} q90 {np.quantile(ep, 0.9):.2e}; |dqvel| median {np.median(ev):.2e} q90 {np.quantile(ev, 0.9):.2e}")
    assert env.engine.query("contact_slots") == 48
    assert st["dropped_contacts"] == 0 and st["max_contacts"] >= R["ncon"].max() - 2
    assert np.median(ep) < 2e-5 and np.quantile(ep, 0.9) < 2e-4, (np.median(ep), np.quantile(ep, 0.9), ep.max())
    assert np.median(ev) < 1e-3 and np.quantile(ev, 0.9) < 2e-2, (np.median(ev), np.quantile(ev, 0.9), ev.max())
    env.close()


@pytest.mark.parametrize("level", ["low", "high", pytest.param("extreme", marks=pytest.mark.xfail(strict=True, reason=(
    "open: 75 % |dqvel| quantile 0.2 against 5e-2 at 64 launches per control step, not yet probed for well-posedness (DESIGN.md §8)")))])
def test_humanoid_on_stairs_replay_at_level(level):
    """test_humanoid_on_stairs_up_hard_with_position_command's replay at the level: the split pipeline (prism walk and solver in
    launches of their own, one pair per substep: 4 / 16 / 64 launches per control step at low / high / extreme), same quantile
    bounds, the same `fits` mask and dropped-contact accounting.  The drop count per level is printed.  Extreme is a strict xfail:
    its 75 % quantile of |dqvel| is 0.2 against the 5e-2 bound, unexplained."""
    from oracle.oracle import Oracle
    cfg, cm, b, q0 = _setup("humanoid_p_v0", level, terrain="stairs_up_hard")
    o = Oracle(cm)
    rng = np.random.default_rng(21)
    parts = []
    for spot in range(8):
        q = q0.copy()
        q[0:2] = rng.uniform(-3.5, 3.5, size=2)
        yaw = rng.uniform(-np.pi, np.pi)
        q[3:7] = [np.cos(yaw / 2), 0, 0, np.sin(yaw / 2)]
        q[2] = q0[2] + (10.0 - o.ray_down(q[0], q[1], 10.0)) + 0.02
        o.reset(q)
        parts.append(_record(o, 25, lambda t: np.clip(0.5 * rng.normal(size=b.nu), -1, 1)))
    R = {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}
    n = len(R["qpos"])
    slots = 256
    fits = R["ncon"] <= slots
    assert R["ncon"].max() >= 100 and np.quantile(R["ncon"], 0.75) >= 40 and fits.mean() > 0.95   # contact-rich samples (50 at q75)
    env = _env(cfg, cm, n)
    assert env.engine.query("contact_slots") == slots and env.engine.query("split") > 0
    qp, qv, _, info = _replay(env, R)
    np.testing.assert_allclose(info["torque"].cpu().numpy(), R["tq"], rtol=1e-4, atol=2e-3)
    st = env.solver_stats()
    print(f"[stairs humanoid {level}] oracle contacts max {R['ncon'].max()}, states over {slots}: {int((~fits).sum())} of {n}; "
          f"device dropped_contacts {st['dropped_contacts']}, max_contacts {st['max_contacts']}")
    assert st["dropped_contacts"] == int(np.maximum(R["ncon"] - slots, 0).sum()) or st["dropped_contacts"] <= 4 * int((~fits).sum()) + 8
    if fits.all():
        assert st["dropped_contacts"] == 0
    assert abs(st["max_contacts"] - R["ncon"].max()) <= 3
    ep = np.abs(qp - R["qpos1"])[fits].max(axis=1)
    ev = np.abs(qv - R["qvel1"])[fits].max(axis=1)
    assert np.median(ep) < 2e-5 and np.quantile(ep, 0.75) < 5e-4 and np.quantile(ep, 0.95) < 2e-2, (np.median(ep), np.quantile(ep, [0.75, 0.95]))
    assert np.median(ev) < 2e-3 and np.quantile(ev, 0.75) < 5e-2, (np.median(ev), np.quantile(ev, [0.75, 0.9]))
    env.close()


# ---------------------------------------------------------------------------------------------------------- multi-step runs

def _self_divergence(cm, b, q0, T):
    """Worst RMS joint-angle divergence of the fp64 oracle from itself, started with the joint angles moved by 1e-7, over T zero-
    action control steps; also returns the unperturbed trajectory's final state."""
    from oracle.oracle import Oracle
    o1, o2 = Oracle(cm), Oracle(cm)
    o1.reset(q0)
    q = q0.copy()
    q[7:] += 1e-7
    o2.reset(q)
    worst, traj = 0.0, np.empty((T, b.nq))
    for t in range(T):
        o1.control_step(np.zeros(b.nu)); o2.control_step(np.zeros(b.nu))
        traj[t] = o1.qpos
        worst = max(worst, float(np.sqrt(np.mean((o1.qpos[7:] - o2.qpos[7:]) ** 2))))
    return worst, traj


@pytest.mark.parametrize("level", ["low", "high", "ultra", "extreme"])
@pytest.mark.parametrize("env_id", ["flamingo_light_v1", "w4_p_v2"])
def test_zero_action_trajectory_1000_steps_at_level(env_id, level):
    """The north-star bound (1e-3 rad RMS joint angle, base pose 1e-3) over 1000 zero-action control steps at every level but
    medium (test_gpu_parity.py has it).  Only where the oracle is well posed: its own divergence from a start perturbed by 1e-7 rad
    is checked here to stay below 5e-4 (measured: light_v1 3.2e-4 / 7.7e-5 / 3.2e-5 / 9.7e-6, w4 3.0e-4 / 1.9e-4 / 2.0e-5 / 7.2e-5 at
    low / high / ultra / extreme; flamingo_p_v3 is not well posed in the same probe, 7e-3 ... 3e-2, and is left out)."""
    import torch
    T = 1000
    cfg, cm, b, q0 = _setup(env_id, level)
    probe, traj = _self_divergence(cm, b, q0, T)
    assert probe < 5e-4, probe
    env = _env(cfg, cm, 4)
    env.reset()
    act = torch.zeros((4, b.nu), device=env.device)
    worst = 0.0
    for t in range(T):
        env.step(act)
        if t % 25 == 24:
            q = env.get_data().qpos.cpu().numpy().astype(np.float64)
            worst = max(worst, float(np.sqrt(np.mean((q[:, 7:] - traj[t][None, 7:]) ** 2))))
            assert np.abs(q - q[0:1]).max() == 0.0
    print(f"[zero action {env_id} {level}] engine {worst:.2e} rad RMS, oracle self-divergence {probe:.2e}")
    assert worst < 1e-3, (worst, probe)
    q = env.get_data().qpos.cpu().numpy().astype(np.float64)
    assert np.abs(q[0, :7] - traj[-1][:7]).max() < 1e-3
    assert env.solver_stats()["dropped_contacts"] == 0
    env.close()


@pytest.mark.parametrize("level", EDGE_LEVELS)
@pytest.mark.parametrize("env_id", ["flamingo_light_v1", "w4_p_v2"])
def test_driven_k_step_replays_at_level(env_id, level):
    """Driven trajectories are chaotic (a 1e-7 start perturbation reaches O(0.1 ... 1) rad within 100 ... 300 control steps), so
    they are tested as K-step replays: 200 states along a driven oracle trajectory, each advanced K = 10 control steps by the
    engine with the recorded actions (at extreme, 320 substeps per env) and compared with where the oracle went.  The ceiling of
    any fp32 engine is the oracle itself started from the fp32-rounded state: per state, that run is computed here, and the states
    where it already parts from the fp64 trajectory by more than 1e-4 rad RMS are ill posed over K steps and left out (measured
    for this drive, well-posed share at low / high / extreme: flamingo_light_v1 99 / 100 / 98.5 %, w4_p_v2 96 / 91 / 73 % -- its
    free-rolling wheels; the median of that fp32-start divergence is 1e-7 rad everywhere).  On the rest, the north-star bound
    (1e-3 rad RMS joint angle) for 90 % of the states and one tenth of it at the median; the base pose likewise for 90 %."""
    import torch
    from oracle.oracle import Oracle
    K, N = 10, 200
    cfg, cm, b, q0 = _setup(env_id, level)
    o = Oracle(cm)
    o.reset(q0)
    for _ in range(50):
        o.control_step(np.zeros(b.nu))
    rng = np.random.default_rng(7)
    phi = rng.uniform(0, 6.28, b.nu)
    Q, V, W, A = [], [], [], []
    for t in range(N + K):
        a = np.clip(0.5 * np.sin(2 * np.pi * 0.5 * 0.02 * t + phi) + 0.1 * rng.normal(size=b.nu), -1, 1)
        Q.append(o.qpos.copy()); V.append(o.qvel.copy()); W.append(o.qacc_warmstart.copy()); A.append(a)
        o.control_step(a)
    Q.append(o.qpos.copy())
    Q, V, W, A = map(np.array, (Q, V, W, A))
    f32 = lambda x: x.astype(np.float32).astype(np.float64)
    ceil = np.empty(N)
    o2 = Oracle(cm)
    for i in range(N):
        o2.reset(f32(Q[i]), f32(V[i]))
        o2.view("qacc_warmstart")[:] = f32(W[i])
        for k in range(K):
            o2.control_step(A[i + k])
        ceil[i] = np.sqrt(np.mean((o2.qpos[7:] - Q[i + K][7:]) ** 2))
    posed = ceil < 1e-4
    assert posed.mean() > 0.6, posed.mean()
    env = _env(cfg, cm, N)
    env.reset()
    env.set_state(Q[:N], V[:N], W[:N])
    acts = torch.tensor(np.stack([A[k:k + N] for k in range(K)]), dtype=torch.float32, device=env.device)   # [K, N, nu]
    for k in range(K):
        env.step(acts[k])
    q = env.get_data().qpos.cpu().numpy().astype(np.float64)
    err = np.sqrt(np.mean((q[:, 7:] - Q[K:K + N, 7:]) ** 2, axis=1))
    base = np.abs(q[:, :7] - Q[K:K + N, :7]).max(axis=1)
    print(f"[K-step {env_id} {level}] well posed {posed.mean():.1%}; engine RMS joint angle median {np.median(err[posed]):.2e} "
          f"q90 {np.quantile(err[posed], 0.9):.2e} max {err[posed].max():.2e}; base q90 {np.quantile(base[posed], 0.9):.2e}")
    assert np.quantile(err[posed], 0.9) < 1e-3 and np.median(err[posed]) < 1e-4, (np.median(err[posed]), np.quantile(err[posed], 0.9))
    assert np.quantile(base[posed], 0.9) < 1e-3
    st = env.solver_stats()
    assert st["dropped_contacts"] == 0 and st["nan_resets"] == 0
    env.close()


@pytest.mark.parametrize("level", [pytest.param("high", marks=pytest.mark.xfail(strict=True, reason=(
    "open: env 1 is ill posed (its twin parts from itself by 4.9e-3 under a 1e-7 start move) but another env misses by 3.1e-2 "
    "where its twin is well posed (DESIGN.md §8)"))), "extreme"])
def test_randomised_light_v1_envs_follow_their_cpu_twins_at_level(level):
    """test_randomised_light_v1_envs_follow_their_cpu_twins_for_1000_steps at the level (oracle/fleet.py twins: per-env masses,
    load, gains and init noise), same bounds, eight envs.  High is a strict xfail: env 1 misses by 4.8e-3, and its twin is
    ill posed (4.9e-3 from itself under a 1e-7 rad start move; the other twins stay below 2e-5).  But one more env misses by 3.1e-2,
    and that one is unexplained."""
    import torch
    from cosim_amd.batched_env import BatchedEnv
    from cosim_amd.compile import compile_model
    from cosim_amd.config import PARITY_RANDOM, make_config
    from oracle.fleet import FleetEnvTwin
    rnd = dict(PARITY_RANDOM, mass_noise=0.05, load=1.0, init_noise=0.05, precision=level)
    cfg = make_config("flamingo_light_v1", random=rnd, seed=77)
    cm = compile_model(cfg)
    n, T, id0 = 8, 1000, 500
    env = BatchedEnv(cfg, num_envs=n, seed=77, auto_reset=False, env_id0=id0, gain_noise=0.1, compiled=cm)
    env.reset()
    twins = [FleetEnvTwin(cfg, cm, 77, id0 + k, gain_noise=0.1, auto_reset=False) for k in range(n)]
    for tw in twins:
        tw.reset()
    q = env.get_data().qpos.cpu().numpy().astype(np.float64)
    np.testing.assert_allclose(q, np.array([tw.qpos for tw in twins]), atol=1e-6)
    act = torch.zeros((n, 4), device=env.device)
    worst = np.zeros(n)
    for t0 in range(0, T, 25):
        for _ in range(25):
            env.step(act)
        for tw in twins:
            tw.rollout(np.zeros((25, 4)))
        q = env.get_data().qpos.cpu().numpy().astype(np.float64)
        ref = np.array([tw.qpos for tw in twins])
        worst = np.maximum(worst, np.sqrt(np.mean((q[:, 7:] - ref[:, 7:]) ** 2, axis=1)))
    print(f"[twins {level}] worst RMS joint angle {worst.max():.2e}")
    assert worst.max() < 1e-3, worst
    assert np.abs(q[:, :7] - ref[:, :7]).max() < 1e-3
    assert np.abs(ref[:, 2] - ref[0, 2]).max() > 20 * np.abs(q[:, 2] - ref[:, 2]).max()
    assert env.solver_stats()["dropped_contacts"] == 0
    env.close()


# ------------------------------------------------------------------------------------------------------- observation pipeline

@pytest.mark.parametrize("level", ["low", "extreme"])
def test_observation_pipeline_matches_wrapper_restatement_at_level(level):
    """test_observation_pipeline_matches_wrapper_restatement at the level: the IMU readings lag one substep (10 ms at low, 0.625 ms
    at extreme), the oracle's sensors carry the same lag at the same h; same bounds."""
    import torch
    from cosim_amd.batched_env import BatchedEnv
    from cosim_amd.robots import obs_to_dim
    from oracle.envlayer import WrapperOracle, projected_gravity
    from oracle.oracle import Oracle
    settle, T = 150, 30
    cfg, cm, b, q0 = _setup("flamingo_light_v1", level, max_duration=(settle + T) / 50.0)
    cfg["observation"]["dof_vel"]["freq"] = 10
    cfg["observation"]["ang_vel"]["freq"] = 25
    from cosim_amd.compile import compile_model
    cm = compile_model(cfg)
    env = BatchedEnv(cfg, num_envs=2, auto_reset=False, compiled=cm)
    w = WrapperOracle(cfg, obs_to_dim("flamingo_light_v1", cfg))
    o = Oracle(cm)
    o.reset(q0)
    o.forward()

    def raw_obs(action):
        return {"dof_pos": o.qpos[[7, 10]], "dof_vel": o.qvel[[6, 9, 8, 11]], "ang_vel": o.sensor_gyro.copy(),
                "lin_vel": o.sensor_vel.copy(), "projected_gravity": projected_gravity(o.sensor_quat), "last_action": action}

    cmd = np.array([0.5, 0.0, 0.1, 0.2])
    env.receive_user_command(cmd.astype(np.float32))
    w.receive_user_command(cmd)
    s, _ = env.reset()
    np.testing.assert_allclose(s[0].cpu().numpy(), w.reset(raw_obs(np.zeros(4))), atol=1e-6)
    worst = 0.0
    for t in range(settle + T):
        a = np.zeros(4) if t < settle else _sin_action(t) * 0.1
        cmd = np.array([0.5 + 0.01 * t, 0.0, 0.1, 0.2])
        env.receive_user_command(cmd.astype(np.float32))
        w.receive_user_command(cmd)
        s, term, trunc, info = env.step(torch.tensor(np.tile(a, (2, 1)), dtype=torch.float32, device=env.device))
        o.control_step(a)
        ref, rterm, rtrunc = w.step(raw_obs(a))
        got = s[0].cpu().numpy()
        if t >= settle:
            worst = max(worst, float(np.abs(got - ref).max()))
        np.testing.assert_allclose(got, ref, atol=2e-4 if t >= settle else 5e-2, err_msg=f"step {t}")
        np.testing.assert_allclose(got[48:52], ref[48:52], atol=1e-6)
        np.testing.assert_allclose(got[12:16], a, atol=1e-7)
        assert bool(trunc[0]) == rtrunc and bool(term[0]) is False
        if t > 0:
            np.testing.assert_array_equal(got[16:32], prev[0:16])
        prev = got
    print(f"[observations {level}] worst |state - restatement| after settling {worst:.2e}")
    assert bool(trunc[0]) is True
    env.close()


def test_time_limit_ends_the_episode_at_the_same_control_step_at_every_level():
    """max_duration 0.3 s is 15 control steps at every level (control_freq 50): truncated exactly at the 15th, with auto-reset."""
    import torch
    for level in LEVELS:
        cfg, cm, b, q0 = _setup("flamingo_light_v1", level, max_duration=0.3)
        env = _env(cfg, cm, 3, auto_reset=True)
        assert env.max_sim_step == 15
        env.reset()
        a = torch.zeros((3, 4), device=env.device)
        ends = []
        for t in range(32):
            _, term, trunc, _ = env.step(a)
            if bool(trunc.any()):
                assert bool(trunc.all()) and not bool(term.any())
                ends.append(t)
        assert ends == [14, 29], (level, ends)
        env.close()


# ------------------------------------------------------------------------------------------------ device paths against each other

@pytest.mark.parametrize("level", ["high", "extreme"])
def test_rollout_rows_equal_the_step_loop_at_level(level):
    """test_rollout_rows_equal_the_step_loop (flamingo_light_v1, one range) at the level: bit for bit for every env that stayed in
    the fleet kernel, the same rule for the few the fleet kernel abandons."""
    import torch
    from cosim_amd.batched_env import BatchedEnv
    from cosim_amd.compile import compile_model
    from cosim_amd.config import make_config
    n, K = 192, 120
    cfg = make_config("flamingo_light_v1", num_envs=n, seed=21, max_duration=1.6, random={"precision": level})
    cm = compile_model(cfg)
    assert cm.blob.frame_skip == LEVELS[level][1]
    cmd = np.array([0.6, 0.0, 0.2, 0.0], dtype=np.float32)
    a = BatchedEnv(cfg, num_envs=n, seed=21, auto_reset=True, gain_noise=0.1, compiled=cm)
    acts = (0.4 * torch.randn((K, n, 4), device="cuda:0", generator=torch.Generator(device="cuda:0").manual_seed(5))).clamp_(-1, 1).contiguous()
    b = BatchedEnv(cfg, num_envs=n, seed=21, auto_reset=True, gain_noise=0.1, compiled=cm)
    assert b.engine.query("rollout") == 1
    for e in (a, b):
        e.receive_user_command(cmd)
        e.reset()
    rows = []
    for k in range(K):
        s, te, tr, info = a.step(acts[k])
        rows.append((s.clone(), te.clone(), tr.clone(), a.info_buf.clone()))
    fix_a = a.solver_stats()["fixup_steps"]
    S, TE, TR, INF = b.rollout(acts)
    torch.cuda.synchronize()
    sb = b.solver_stats()
    assert sb["step_count"] == a.solver_stats()["step_count"] == n * (1 + K)
    ref_s = torch.stack([r[0] for r in rows]); ref_te = torch.stack([r[1] for r in rows]); ref_tr = torch.stack([r[2] for r in rows])
    ref_inf = torch.stack([r[3] for r in rows])
    assert (ref_tr | ref_te).sum().item() >= n
    same = ((S == ref_s).all(dim=2) & (INF == ref_inf).all(dim=2) & (TE == ref_te) & (TR == ref_tr)).all(dim=0)
    odd = (~same).nonzero().flatten().tolist()
    if fix_a == 0 and sb["fixup_steps"] == 0:
        assert not odd
    assert len(odd) <= max(2, n // 16), (len(odd), fix_a, sb["fixup_steps"])
    for i in odd:
        first = int((~((S[:, i] == ref_s[:, i]).all(dim=1))).nonzero()[0])
        assert torch.equal(S[:first, i], ref_s[:first, i])
        np.testing.assert_allclose(S[first, i].cpu().numpy(), ref_s[first, i].cpu().numpy(), rtol=0, atol=5e-3)
    assert torch.equal(b.state, S[-1]) and torch.equal(b.terminated, TE[-1])
    a.close(); b.close()


@pytest.mark.parametrize("level", ["high", "extreme"])
def test_step_ranges_and_graph_capture_equal_the_single_eager_launch_at_level(level):
    """test_step_range_shards_on_streams_equal_the_single_launch and test_range_launches_inside_a_captured_graph_equal_the_eager_loop
    at the level: the GUI-default randomised workload with auto-reset as one launch, as four ranges on caller streams, and as four
    engine-owned ranges captured in a graph and replayed -- the same bits."""
    import torch
    from cosim_amd.batched_env import BatchedEnv
    from cosim_amd.compile import compile_model
    from cosim_amd.config import make_config
    n, S, K, R = 256, 4, 3, 5
    cfg = make_config("flamingo_light_v1", max_duration=0.2, num_envs=n, seed=3, random={"precision": level})
    cm = compile_model(cfg)
    acts = (0.5 * torch.randn((K * R, n, 4), device="cuda:0", generator=torch.Generator(device="cuda:0").manual_seed(2))).contiguous()
    a = BatchedEnv(cfg, num_envs=n, auto_reset=True, seed=3, compiled=cm, gain_noise=0.1)
    b = BatchedEnv(cfg, num_envs=n, auto_reset=True, seed=3, compiled=cm, gain_noise=0.1)
    c = BatchedEnv(cfg, num_envs=n, auto_reset=True, seed=3, compiled=cm, gain_noise=0.1, ranges=4, deferred_join=True)
    a.reset(); b.reset(); c.reset()
    streams = [torch.cuda.Stream(device=a.device) for _ in range(S)]
    torch.cuda.synchronize()
    ns = n // S
    for t in range(K * R):
        a.step(acts[t])
        for i, st in enumerate(streams):
            with torch.cuda.stream(st):
                b.step_range(i * ns, ns, acts[t])
    torch.cuda.synchronize()
    assert torch.equal(a.state, b.state) and torch.equal(a.info_buf, b.info_buf) and torch.equal(a.truncated, b.truncated)
    assert torch.equal(a.get_data().qpos, b.get_data().qpos)
    # graph: the first chunk eager (warm-up), then R - 1 replays of a captured chunk; the chunk reads a fixed action buffer
    buf = torch.empty((K, n, 4), device=c.device)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())

    def chunk():
        for k in range(K):
            c.step(buf[k])
        c.join()
    buf.copy_(acts[0:K])
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        chunk()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        chunk()
    for r in range(1, R):
        buf.copy_(acts[r * K:(r + 1) * K])
        g.replay()
    torch.cuda.synchronize()
    assert c.solver_stats()["step_count"] == a.solver_stats()["step_count"] == n * (1 + K * R)
    assert torch.equal(a.state, c.state) and torch.equal(a.get_data().qpos, c.get_data().qpos)
    assert a.solver_stats()["episodes_ended"] >= n                  # the 10-step time limit fired inside the run
    a.close(); b.close(); c.close()


@pytest.mark.parametrize("level", ["high", "extreme"])
def test_two_envs_per_wave_variant_agrees_with_the_default_kernel_at_level(level):
    """test_two_envs_per_wave_variant_agrees_with_the_default_kernel at the level, same bounds (different summation orders)."""
    import torch
    cfg, cm, b_, q0 = _setup("flamingo_light_v1", level)
    a, b = _env(cfg, cm, 256), _env(cfg, cm, 256)
    b.engine.set_param("envs_per_wave", np.array([2.0]))
    a.reset(); b.reset()
    rng = np.random.default_rng(5)
    for t in range(40):
        a.step(torch.tensor(0.5 * rng.normal(size=(256, 4)), dtype=torch.float32, device=a.device))
    d = a.get_data()
    w = torch.empty((256, 18), device=a.device)
    a.engine.get("qacc_warmstart", w.data_ptr(), None)
    torch.cuda.synchronize()
    b.set_state(d.qpos.cpu().numpy(), d.qvel.cpu().numpy(), w.cpu().numpy())
    act = torch.tensor(0.5 * rng.normal(size=(256, 4)), dtype=torch.float32, device=a.device)
    a.step(act); b.step(act)
    ev = (a.get_data().qvel - b.get_data().qvel).abs().max(dim=1).values
    assert float(ev.median()) < 5e-5 and float(ev.quantile(0.95)) < 1e-3, (float(ev.median()), float(ev.max()))
    a.close(); b.close()


@pytest.mark.parametrize("level", ["high", "extreme"])
def test_more_contacts_than_the_fleet_kernel_holds_are_redone_at_level(level):
    """test_more_contacts_than_the_fleet_kernel_holds_are_redone_not_dropped at the level: the drop poses, a control step whose
    contacts overflow the fleet kernel's 14 slots in any of its 8 / 32 substeps is redone whole by the 40-slot kernel; nothing is
    left out and the results follow the oracle with the medium bounds."""
    import torch
    from oracle.oracle import Oracle
    cfg, cm, b, q0 = _setup("flamingo_light_v1", level)
    o = Oracle(cm)
    rng = np.random.default_rng(3)
    R = dict(qpos=[], qvel=[], warm=[], act=[], qpos1=[], qvel1=[], ncon=[])
    for trial in range(200):
        q = q0.copy()
        quat = rng.normal(size=4)
        q[2] = rng.uniform(0.05, 0.25)
        q[3:7] = quat / np.linalg.norm(quat)
        q[7:] += rng.uniform(-0.3, 0.3, size=q.size - 7)
        o.reset(q)
        for t in range(2):
            a = 0.3 * np.sin(0.3 * t + np.arange(4))
            R["qpos"].append(o.qpos.copy()); R["qvel"].append(o.qvel.copy()); R["warm"].append(o.qacc_warmstart.copy()); R["act"].append(a)
            o.control_step(a)
            R["qpos1"].append(o.qpos.copy()); R["qvel1"].append(o.qvel.copy()); R["ncon"].append(o.ncon)
    R = {k: np.array(v) for k, v in R.items()}
    big = R["ncon"] > 14
    assert big.sum() >= 40 and R["ncon"].max() >= 30, (big.sum(), R["ncon"].max())
    n = len(R["ncon"])
    env = _env(cfg, cm, n)
    assert env.engine.query("contact_slots") == 14 and env.engine.query("fixup_contact_slots") == 40
    qp, qv, _, _ = _replay(env, R)
    st = env.solver_stats()
    ev = np.abs(qv - R["qvel1"]).max(axis=1)
    print(f"[fix-up {level}] redone {st['fixup_steps']} of {n} (last-substep overflow in the oracle: {int(big.sum())}); "
          f"|dqpos| max {np.abs(qp - R['qpos1']).max():.2e}; |dqvel| max {ev.max():.2e} median {np.median(ev):.2e}")
    assert st["dropped_contacts"] == 0 and st["nan_resets"] == 0 and 30 <= st["max_contacts"] <= 40
    assert big.sum() <= st["fixup_steps"] <= n
    assert np.abs(qp - R["qpos1"]).max() < 2e-5
    assert ev.max() < 2e-3 and np.median(ev) < 2e-4, (ev.max(), np.median(ev))
    env.close()
