"""Failure traces on the host (no GPU): the numpy twin of the trace kernels (cosim_amd/ftrace.py reference_traces) against
hand-written rows; the .npz round trip, select, summary and the join against the ledger twin; validation messages; the kernels'
per-env bodies (csrc/cosim_ftrace.h) compiled as plain C++ and driven lane by lane against the twin, a second time under
AddressSanitizer / UBSan; and the kernel-resource tables recorded before and after the change.  Every comparison is bit for bit:
the feature only copies."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
K, N, NQ, NV, NU, CD, NI = 11, 3, 3, 2, 2, 1, 5                       # the hand-written case: F = 20 words
FRAMES, KEEP = 3, 2


def _hand_case():
    """11 steps of three envs; every float names its step, env and word, so a frame can be read off: qpos[k, n, j] = 100 k + 10 n + j
    is the state step k of env n started from.
      env 0: terminated in steps 1, 6 and 8 -- three triggering ends (lengths 2, 5, 2): one lost, the two newest kept; the 5-step
             episode wraps the ring of 3 (oldest position 2), the last one is shorter than the window; open with length 2 at the end
      env 1: truncated in step 3 (no trigger under the default selection: the window is emptied), terminated in step 9 (length 6)
      env 2: cut by the host before step 4 (a masked begin with flag 8), terminated in step 7 (length 4, flags 1 | 8), open with
             length 3: a full ring, so two whole frames"""
    f32 = np.float32
    k, n = np.arange(K + 1)[:, None, None], np.arange(N)[None, :, None]
    c = dict(qpos=(100 * k + 10 * n + np.arange(NQ)).astype(f32), qvel=(0.5 + 100 * k + 10 * n + np.arange(NV)).astype(f32))
    k = k[:K]
    c["actions"] = (1000 + 100 * k + 10 * n + np.arange(NU)).astype(f32)
    c["commands"] = (2000 + 100 * k + 10 * n + np.arange(CD)).astype(f32)
    c["info"] = (3000 + 100 * k + 10 * n + np.arange(NI)).astype(f32)
    c["actions"][5, 0, 1] = np.nan                                         # NaN stays NaN
    te, tr = np.zeros((K, N), dtype=np.uint8), np.zeros((K, N), dtype=np.uint8)
    te[[1, 6, 8], 0] = 1
    tr[3, 1] = 1
    te[9, 1] = 1
    te[7, 2] = 1
    c["term"], c["trunc"] = te, tr
    c["meta4"] = np.zeros((K + 1, N), dtype=np.int32)
    c["meta14"] = (np.arange(K + 1)[:, None] + 7 * np.arange(N)[None, :]).astype(np.int32)   # "spawn rows": distinct per step and env
    c["meta15"] = None
    c["begins"] = [(4, np.array([0, 0, 1], dtype=np.uint8), 8)]
    return c


def _twin(c, frames=FRAMES, keep=KEEP, on=None, **kw):
    from cosim_amd.ftrace import reference_traces
    return reference_traces(c["qpos"], c["qvel"], c["actions"], c["commands"], c["info"], c["term"], c["trunc"], c["meta4"], c["meta14"],
                            c["meta15"], frames, keep, on, begins=c.get("begins", ()), scenario_rows=c.get("scn"),
                            open_scenario_rows=c.get("open_scn"), **kw)


# ------------------------------------------------------------------------------------------------------------ 1: the twin, by hand
def test_twin_against_hand_written_rows():
    c = _hand_case()
    tr = _twin(c)
    assert len(tr) == 4 and tr.env.tolist() == [0, 0, 1, 2] and tr.episode.tolist() == [1, 2, 1, 0]
    assert tr.lost.tolist() == [1, 0, 0] and tr.counts.tolist() == [[0, 3, 1], [1, 1, 0], [1, 1, 0]]
    assert tr.length.tolist() == [5, 2, 6, 4] and tr.frames.tolist() == [3, 2, 3, 3] and tr.flags.tolist() == [1, 1, 1, 1 | 8]
    assert tr.oldest.tolist() == [2, 0, 0, 1], "the 5-step episode wrapped: its oldest frame is not at ring position 0"
    assert tr.steps_seen.tolist() == [7, 9, 10, 8] and (tr.scenario == -1).all() and (tr.headers[:, 8:] == 0).all()
    # spawn row: meta word 14 as it stood when the episode began (after the step that ended the one before; at the cut for env 2)
    assert tr.spawn_row.tolist() == [2, 7, 7 + 4, 14 + 4]
    # env 0, episode 1 = steps 2 .. 6, the window keeps 4, 5, 6; time order, the state each step started from
    assert tr.t[0].tolist() == [3, 4, 5] and tr.terminated[0].tolist() == [0, 0, 1] and tr.truncated[0].tolist() == [0, 0, 0]
    assert tr.qpos[0, :, 0].tolist() == [400.0, 500.0, 600.0] and tr.qvel[0, :, 1].tolist() == [401.5, 501.5, 601.5]
    assert tr.action[0, :, 0].tolist() == [1400.0, 1500.0, 1600.0] and np.isnan(tr.action[0, 1, 1]) and tr.action[0, 2, 1] == 1601.0
    assert tr.command[0, :, 0].tolist() == [2400.0, 2500.0, 2600.0] and tr.info[0, :, 4].tolist() == [3404.0, 3504.0, 3604.0]
    # the NaN travelled as its bits
    assert tr.words[0, 1, 4 + NQ + NV + 1] == c["actions"][5, 0, 1].view(np.int32)
    # env 0, episode 2 = steps 7, 8: shorter than the window -- left-aligned, padded with -1 / NaN
    assert tr.t[1].tolist() == [1, 2, -1] and tr.terminated[1].tolist() == [0, 1, -1] and tr.truncated[1].tolist() == [0, 0, -1]
    assert tr.qpos[1, :2, 0].tolist() == [700.0, 800.0] and np.isnan(tr.qpos[1, 2]).all() and np.isnan(tr.info[1, 2]).all()
    assert (tr.words[1, 2] == 0).all()
    # env 1: the truncated 4-step episode left nothing; episode 1 = steps 4 .. 9 keeps 7, 8, 9
    assert tr.t[2].tolist() == [4, 5, 6] and tr.qpos[2, :, 0].tolist() == [710.0, 810.0, 910.0]
    # env 2: the cut before step 4 emptied the window; steps 4 .. 7 keep 5, 6, 7
    assert tr.t[3].tolist() == [2, 3, 4] and tr.qpos[3, :, 1].tolist() == [521.0, 621.0, 721.0]
    # padding words of a frame stay zero
    F = tr.words.shape[2]
    assert F == 20 and (tr.words[:, :, 4 + NQ + NV + NU + CD + NI:] == 0).all()

    opn = _twin(c, include_open=True)
    o = (opn.flags & 16) != 0
    assert len(opn) == 7 and opn.env[o].tolist() == [0, 1, 2] and opn.episode[o].tolist() == [3, 2, 1]
    assert opn.length[o].tolist() == [2, 1, 3] and opn.flags[o].tolist() == [16, 16, 16]
    # an open window's cursor frame already holds the next step's state: a full ring has frames - 1 whole frames
    assert opn.frames[o].tolist() == [2, 1, 2] and opn.oldest[o].tolist() == [0, 0, 1]
    assert opn.t[o][2].tolist() == [2, 3, -1] and opn.qpos[o][2][:2, 0].tolist() == [920.0, 1020.0]
    assert opn.t[o][0].tolist() == [1, 2, -1] and opn.qpos[o][0][:2, 0].tolist() == [900.0, 1000.0]
    np.testing.assert_array_equal(opn.headers[~o], tr.headers)

    # a selection that includes the time limit keeps env 1's truncated episode too; "truncated" alone keeps only that one
    both = _twin(c, on=("terminated", "truncated"))
    assert both.env.tolist() == [0, 0, 1, 1, 2] and both.length[2:4].tolist() == [4, 6] and both.flags[2] == 2
    assert both.t[2].tolist() == [2, 3, 4] and both.truncated[2].tolist() == [0, 0, 1]
    only = _twin(c, on="truncated")
    assert only.env.tolist() == [1] and only.episode.tolist() == [0] and only.meta["on_mask"] == 2
    assert _twin(c, on=("tilt",)).env.tolist() == []                       # no fall rule: no cause bits, nothing is kept
    # set on a stepped fleet: every env's first episode carries flag 8
    first = _twin(c, keep=4, initial_flags=8)
    assert first.flags[first.episode == 0].tolist() == [1 | 8, 1 | 8] and first.lost.tolist() == [0, 0, 0]


def test_twin_fall_causes_and_nonfinite():
    c = _hand_case()
    c["meta15"] = np.zeros((K, N), dtype=np.int32)
    c["meta15"][1, 0], c["meta15"][6, 0], c["meta15"][8, 0], c["meta15"][9, 1], c["meta15"][7, 2] = 1, 2, 4, 1, 9   # (9 & 7 = 1)
    c["meta4"][6:, 1] = 1                                                  # a non-finite reset during env 1's second episode
    tr = _twin(c, keep=4)
    assert tr.flags.tolist() == [1 | 32, 1 | 64, 1 | 128, 1 | 4 | 32, 1 | 8 | 32]
    assert _twin(c, keep=4, on=("height",)).episode.tolist() == [1] and _twin(c, keep=4, on=("nonfinite",)).env.tolist() == [1]
    assert _twin(c, keep=4, on=("tilt", "contact")).flags.tolist() == [1 | 32, 1 | 128, 1 | 4 | 32, 1 | 8 | 32]


# ------------------------------------------------------------------------------------------------------------ 2: container
def test_npz_select_summary_and_join(tmp_path):
    from cosim_amd.ftrace import FailureTraces, same_traces
    from cosim_amd.ledger import reference_ledger
    c = _hand_case()
    c["scn"] = (np.arange(K)[:, None] + np.arange(N)[None, :]).astype(np.int32) % 4
    c["open_scn"] = np.array([1, 2, 3], dtype=np.int32)
    tr = _twin(c, include_open=True)
    path = str(tmp_path / "traces.npz")
    tr.save(path)
    with np.load(path, allow_pickle=False) as z:                           # plain arrays: loads with pickle refused
        assert sorted(z.files) == ["env", "headers", "lost", "meta", "words"]
    back = FailureTraces.load(path)
    assert same_traces(back, tr) is None and back.meta == tr.meta and back.meta["window"] == 3 and back.meta["keep"] == 2
    np.testing.assert_array_equal(back.qpos.view(np.int32), tr.qpos.view(np.int32))
    np.testing.assert_array_equal(back.t, tr.t)
    assert tr.summary() == {"traces": 4, "terminated": 4, "truncated": 0, "nonfinite": 0, "tilt": 0, "height": 0, "contact": 0,
                            "no_reset_start": 1, "open": 3, "lost": 1}
    sel = tr.select(flags=("terminated",))
    assert len(sel) == 4 and sel.ended().all() and tr.select(flags=("truncated",)).env.tolist() == []
    assert tr.select(env=2).env.tolist() == [2, 2] and tr.select(flags=1, env=[0, 2]).episode.tolist() == [1, 2, 0]
    # the scenario row of a trace is the row of the step that ended it
    assert tr.scenario[tr.ended()].tolist() == [c["scn"][6, 0], c["scn"][8, 0], c["scn"][9, 1], c["scn"][7, 2]]
    assert tr.scenario[~tr.ended()].tolist() == [1, 2, 3]
    # join against the ledger twin on the same rows: every trace finds one record with equal flags and length
    info = np.zeros((K, N, 4 + 2 * NU), dtype=np.float32)
    led = reference_ledger(info, c["term"], c["trunc"], np.zeros((N, 3), dtype=np.float32), c["meta4"], c["meta14"], 8, NU, 3,
                           begins=c["begins"], scenario_rows=c["scn"], include_open=True, open_scenario_rows=c["open_scn"])
    at = tr.join(led)
    assert (at >= 0).all() and len(set(at.tolist())) == len(tr)
    np.testing.assert_array_equal(led.flags[at], tr.flags)
    np.testing.assert_array_equal(led.length[at], tr.length)
    np.testing.assert_array_equal(led.env[at], tr.env)
    np.testing.assert_array_equal(led.spawn_row[at], tr.spawn_row)
    np.testing.assert_array_equal(led.scenario[at], tr.scenario)
    np.testing.assert_array_equal(led.steps_seen[at], tr.steps_seen)
    assert len(led) == len(tr) + 2                                         # the truncated episode and the lost trace are in the ledger only
    short = reference_ledger(info, c["term"], c["trunc"], np.zeros((N, 3), dtype=np.float32), None, None, 1, NU, 3, begins=c["begins"])
    assert tr.select(env=0).join(short).tolist() == [-1, 0, -1]            # a ledger ring of one slot has lost episode 1


# ------------------------------------------------------------------------------------------------------------ 3: validation
@pytest.mark.parametrize("spec, on, message", [
    ((0, 2), None, r"frames 0 outside 1\.\.1024"),
    ((1025, 2), None, r"frames 1025 outside 1\.\.1024"),
    ((8, 0), None, r"keep 0 outside 1\.\.64"),
    ({"frames": 8, "keep": 65}, None, r"keep 65 outside 1\.\.64"),
    ((8.5, 2), None, r"frames 8\.5 is not an integer"),
    ((8,), None, r"expected \(frames, keep\)"),
    ({"frames": 8, "keep": 2, "slots": 1}, None, r"unknown key 'slots'"),
    ({"frames": 8}, None, r"needs 'frames' and 'keep'"),
    ((8, 2), (), r"'on' is empty"),
    ({"frames": 8, "keep": 2, "on": []}, None, r"'on' is empty"),
    ((8, 2), ("terminated", "fell"), r"unknown 'on' name 'fell'"),
    ((8, 2), 0, r"on mask 0 must be a non-empty subset"),
    ((8, 2), 8, r"on mask 8 must be a non-empty subset"),
])
def test_validation_names_the_value(spec, on, message):
    from cosim_amd.ftrace import resolve
    with pytest.raises(ValueError, match=message):
        resolve(spec, on)


def test_resolve_and_masks():
    from cosim_amd.ftrace import DEFAULT_ON, frame_words, on_mask, on_names, resolve
    assert resolve((50, 2)) == (50, 2, 1 | 4) and on_names(1 | 4) == list(DEFAULT_ON)
    assert resolve({"frames": 1, "keep": 64, "on": ["tilt", "height", "contact"]}) == (1, 64, 32 | 64 | 128)
    assert resolve([1024, 1], "truncated") == (1024, 1, 2) and on_mask(np.int32(3)) == 3
    assert frame_words(9, 8, 2, 4, 45) == 72 and frame_words(0, 0, 0, 0, 0) == 4 and frame_words(1, 0, 0, 0, 0) == 8


# ------------------------------------------------------------------------------------------------------------ 4: the kernel bodies, as host C++
def _build(tmp, *flags):
    exe = str(tmp / ("ftrace_lanes" + ("_san" if flags else "")))
    cxx = os.environ.get("CXX", "c++")
    p = subprocess.run([cxx, "-std=c++17", "-O1", "-g", *flags, "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "cosim_amd", "csrc"), "-o", exe,
                        os.path.join(ROOT, "tests", "ftrace_lanes.cpp")], capture_output=True, text=True)
    return exe if p.returncode == 0 else None


@pytest.fixture(scope="module")
def lanes_exes(tmp_path_factory):
    """tests/ftrace_lanes.cpp + csrc/cosim_ftrace.h as a plain C++ program (no HIP, no GPU), and once more with
    -fsanitize=address,undefined (None where the host compiler has no sanitizer runtime)."""
    tmp = tmp_path_factory.mktemp("ftrace")
    plain = _build(tmp)
    assert plain is not None, "tests/ftrace_lanes.cpp does not compile"
    return plain, _build(tmp, "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined")


def _run_lanes(exe, c, frames, keep, on, lanes, reverse, split, initial_flags=0, scn_rows=0, scn_mode=0, scn_off=0, meta11=None):
    """The case as the driver's operations: the state before step 0 and the begin of cosim_ftrace_set, then per step the host cuts
    ahead of it, the step's rows and the state it left."""
    from cosim_amd.ftrace import on_mask
    u = lambda a: np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).reshape(-1).tolist()   # noqa: E731
    Kc, Nc = c["actions"].shape[:2]
    m15 = np.zeros((Kc, Nc), dtype=np.int32) if c["meta15"] is None else c["meta15"]
    m11 = np.zeros((Kc + 1, Nc), dtype=np.int32) if meta11 is None else meta11

    def state(k, cause):
        w = [3]
        for n in range(Nc):
            w += u(c["qpos"][k, n]) + u(c["qvel"][k, n]) + [int(c["meta4"][k, n]), int(c["meta14"][k, n]), int(cause[n]), int(m11[k, n])]
        return w
    words = [Nc, c["qpos"].shape[2], c["qvel"].shape[2], c["actions"].shape[2], c["commands"].shape[2], c["info"].shape[2], frames, keep,
             on_mask(on), 1, int(c["meta15"] is not None), scn_rows, lanes, int(reverse), split]
    words += state(0, np.zeros(Nc, dtype=np.int32)) + [2, initial_flags] + [1] * Nc
    scn = c.get("scn")
    for k in range(Kc + 1):
        for kb, mask, flag in c.get("begins", ()):
            if kb == k:
                words += [2, int(flag)] + (np.ones(Nc, dtype=int) if mask is None else np.asarray(mask).astype(int)).tolist()
        if k == Kc:
            break
        words += state(k + 1, m15[k])                                      # the kernel runs behind the step: it finds the state the step left
        words += [1] + u(c["actions"][k]) + u(c["commands"][k]) + u(c["info"][k]) + c["term"][k].astype(int).tolist()
        words += c["trunc"][k].astype(int).tolist() + (np.zeros(Nc, dtype=int) if scn is None else scn[k]).tolist()
    words += [0] + (np.zeros(Nc, dtype=int) if c.get("open_scn") is None else c["open_scn"]).tolist() + [scn_mode, scn_off]
    p = subprocess.run([exe], input=" ".join(str(int(w)) for w in words), capture_output=True, text=True)
    assert p.returncode == 0, (p.returncode, p.stderr[-2000:])
    out = np.array(p.stdout.split(), dtype=np.int64).astype(np.int32)
    F = (4 + sum(c[k].shape[2] for k in ("qpos", "qvel", "actions", "commands", "info")) + 3) & ~3
    nb = Nc * (keep + 1) * (16 + frames * F)
    assert len(out) == nb + 3 * Nc + 16 * Nc
    return out[:nb].reshape(Nc, keep + 1, -1), out[nb:nb + 3 * Nc].reshape(Nc, 3), out[nb + 3 * Nc:].reshape(Nc, 16)


def _assert_lanes_equal_twin(exe, c, frames, keep, on, configs=((64, False), (64, True), (5, True), (1, False)), **kw):
    tw = _twin(c, frames, keep, on, include_open=True, initial_flags=kw.get("initial_flags", 0))
    for lanes, reverse in configs:
        buf, cnt, opn = _run_lanes(exe, c, frames, keep, on, lanes, reverse, **kw)
        np.testing.assert_array_equal(buf, tw.buffers)
        np.testing.assert_array_equal(cnt, tw.counts)
        np.testing.assert_array_equal(opn, tw.open_headers)
    return tw


def _random_case(seed=7, Kr=40, Nr=11):
    """11 envs, 40 steps, a frame of 100 words (more than one pass of a 64-lane wave); ends of every kind at random, non-finite
    resets, fall causes, scenario rows in mode "cycle", NaN and Inf payloads, two host cuts."""
    rng = np.random.default_rng(seed)
    nq, nv, nu, cd, ni = 19, 18, 12, 3, 43
    c = {}
    for name, shape in (("qpos", (Kr + 1, Nr, nq)), ("qvel", (Kr + 1, Nr, nv)), ("actions", (Kr, Nr, nu)), ("commands", (Kr, Nr, cd)),
                        ("info", (Kr, Nr, ni))):
        x = rng.normal(size=shape).astype(np.float32)
        x[rng.random(shape) < 0.01] = np.nan
        x[rng.random(shape) < 0.01] = np.inf
        c[name] = x
    c["term"] = (rng.random((Kr, Nr)) < 0.12).astype(np.uint8)
    c["trunc"] = (rng.random((Kr, Nr)) < 0.08).astype(np.uint8)
    c["trunc"][:, 3] = 0
    c["term"][:, 3] = 0                                                     # env 3 never ends: its ring wraps many times
    c["term"][:, 5] = 1                                                     # env 5 ends every step
    c["meta4"] = np.cumsum(rng.random((Kr + 1, Nr)) < 0.05, axis=0).astype(np.int32)
    c["meta14"] = rng.integers(0, 9, size=(Kr + 1, Nr)).astype(np.int32)
    c["meta15"] = rng.integers(0, 16, size=(Kr, Nr)).astype(np.int32)
    done = (c["term"] | c["trunc"]).astype(np.int64)
    S, off = 7, 4
    ended = np.concatenate([np.zeros((1, Nr), dtype=np.int64), np.cumsum(done, axis=0)])   # meta word 11 before step k / after the last
    rows = (off + np.arange(Nr)[None, :]) % S
    rows = (rows + ended % S) % S
    c["scn"], c["open_scn"] = rows[:Kr].astype(np.int32), rows[Kr].astype(np.int32)
    c["begins"] = [(13, (rng.random(Nr) < 0.5).astype(np.uint8), 0), (29, (rng.random(Nr) < 0.5).astype(np.uint8), 8), (Kr, None, 8)]
    return c, dict(scn_rows=S, scn_mode=1, scn_off=off, meta11=ended.astype(np.int32))


def test_kernel_bodies_as_host_cpp_equal_the_twin(lanes_exes):
    """The functions the kernels call, lane by lane (64 lanes, 5, 1) and with the two ranges in either order: buffers, counters and
    open headers equal the twin's, on the hand-written rows under three selections and on a random case with a frame wider than a
    wave."""
    plain, _ = lanes_exes
    c = _hand_case()
    for on in (None, ("truncated",), ("terminated", "truncated", "nonfinite")):
        tw = _assert_lanes_equal_twin(plain, c, FRAMES, KEEP, on, split=1)
    assert len(tw) == 5 + 3
    _assert_lanes_equal_twin(plain, c, FRAMES, KEEP, None, split=2, initial_flags=8)
    _assert_lanes_equal_twin(plain, c, 1, 1, None, split=0)                 # a ring of one frame, one kept trace
    r, kw = _random_case()
    for frames, keep, on in ((5, 2, None), (4, 1, ("truncated", "tilt")), (64, 3, ("terminated", "truncated"))):
        tw = _assert_lanes_equal_twin(plain, r, frames, keep, on, split=4, **kw)
        assert tw.words.shape[2] == 100
    assert (tw.lost > 0).any() and (tw.frames[tw.ended()] < 64).all() and tw.scenario.min() >= 0
    tw = _twin(r, 5, 2, None)
    assert (tw.frames < 5).any() and ((tw.length > 5) & (tw.oldest != 0)).any() and (tw.lost > 0).any() and ((tw.flags & 4) != 0).any()


def test_kernel_bodies_under_sanitizers(lanes_exes):
    """The same program built with -fsanitize=address,undefined and run as the stand-alone program it is: an access outside a
    buffer, a counter or a row ends it with a report and a non-zero status."""
    _, san = lanes_exes
    if san is None:
        pytest.skip("the host compiler has no sanitizer runtime")
    _assert_lanes_equal_twin(san, _hand_case(), FRAMES, KEEP, None, split=1)
    _assert_lanes_equal_twin(san, _hand_case(), 1, 1, ("terminated", "truncated"), split=3)
    r, kw = _random_case(seed=8)
    _assert_lanes_equal_twin(san, r, 5, 2, None, split=4, **kw)
    _assert_lanes_equal_twin(san, r, 200, 3, ("terminated", "truncated", "nonfinite", "tilt", "height", "contact"), configs=((64, True),),
                             split=11, **kw)


# ------------------------------------------------------------------------------------------------------------ 5: kernel resources
def _kres(name):
    with open(os.path.join(ROOT, "profiles", name)) as f:
        lines = [ln.rstrip() for ln in f if ln.strip()]
    return lines[0], lines[1:]


def test_kernel_resources_of_existing_kernels_are_unchanged():
    """tools/kres.py before (profiles/ftrace_kres_parent.txt) and after (ftrace_kres_this.txt): every existing kernel's line is
    identical, in the same order; the only added lines are the three trace kernels', which use no LDS, no scratch and spill nothing."""
    head_a, a = _kres("ftrace_kres_parent.txt")
    head_b, b = _kres("ftrace_kres_this.txt")
    assert head_a == head_b and len(a) >= 40
    assert [ln for ln in b if ln in a] == a, "an existing kernel's resources changed"
    added = {ln.split("(")[0]: [int(x) for x in re.split(r"\s+", ln.strip())[-7:]] for ln in b if ln not in a}
    assert sorted(added) == ["ftrace_begin_kernel", "ftrace_open_kernel", "ftrace_step_kernel"], sorted(added)
    for name, (vgpr, agpr, sspill, vspill, scratch, occ, lds) in added.items():
        assert (agpr, sspill, vspill, scratch, lds) == (0, 0, 0, 0, 0) and vgpr <= 64 and occ == 8, (name, vgpr, occ)
