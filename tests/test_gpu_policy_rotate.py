"""Rotating policy tables on the device (``PolicyTable(rotate_every=)`` / ``RecurrentPolicyTable(rotate_every=)``,
``cosim_*_table_forward_rotating``, poltab_regroup_kernel in csrc/cosim_mlp.hip).  The lists the kernel rebuilds are compared word for
word with a numpy restatement of ``build_policy_tiles`` on the current assignment; every env's action has the bits of
``MLPPolicy(current file, fused=True)`` (recurrent: of the composed single-policy entry points); the three runner loops agree bit for
bit with a host loop over single policies; ledger and verdict records are attributed to the policy that drove the episode; a snapshot
continues the rotation; the CLI reports both files."""
import ctypes
import json

import numpy as np
import pytest

from cosim_amd.policy import MLPPolicy, PolicyTable, RecurrentPolicyTable, write_onnx, write_random_mlp
from test_gpu_policy_table import _bits, _inputs, _single_rows, family  # noqa: F401  (family: the fixture with the files of both widths)
from test_gpu_recurrent_table import _Composed, _layers, _lstm

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CALLS = 6


# ------------------------------------------------------------------------------------------ the numpy restatement of the host's rules
def _rule(base, e, every, K):
    return (np.asarray(base) + np.asarray(e) // every) % K


def _capacity(count, K):
    return count // 32 + min(K, count)


def _lists(now, K, first, count):
    """build_policy_tiles for one range of the assignment ``now``: (rows [count], tiles [capacity, 4] padded with zeros, tiles in use)."""
    rows, tiles = [], []
    for k in range(K):
        mine = first + np.nonzero(now[first:first + count] == k)[0]
        for j in range(0, len(mine), 32):
            tiles.append((k, first + len(rows) + j, min(32, len(mine) - j), 0))
        rows.extend(mine.tolist())
    out = np.zeros((_capacity(count, K), 4), np.int32)
    out[:len(tiles)] = np.asarray(tiles, np.int32).reshape(-1, 4)
    return np.asarray(rows, np.int32), out, len(tiles)


def _read_lists(tab, i, fn="cosim_policy_table_lists"):
    first, count = tab.ranges[i]
    rows, tiles, used = np.full(count, -7, np.int32), np.full((_capacity(count, len(tab.paths)), 4), -7, np.int32), ctypes.c_int(-7)
    assert getattr(tab._lib, fn)(tab._handle, i, rows.ctypes.data, tiles.ctypes.data, ctypes.byref(used)) == 0, tab._lib.cosim_last_error()
    return rows, tiles, used.value


def _base(n, K, seed):
    """32 rows of policy 0 and 33 of policy 1 among the first 65 (shuffled), the rest on the last policy: with K = 3 and n = 65 policy 2
    owns no row at the first call."""
    rng = np.random.default_rng(seed)
    if K == 1:
        return np.zeros(n, np.int64)
    if K == 64:
        return rng.permutation(n) % K                                   # n <= 64: a single row per policy, the capacity is met
    a = np.full(n, K - 1)
    head = rng.permutation(np.array([0] * 32 + [1] * 33))
    a[:min(n, 65)] = head[:min(n, 65)]
    return a


def _script(n, seed):
    """Per call (terminated, truncated) uint8: none at the first call, then about 40 % of the envs, some by both flags."""
    rng = np.random.default_rng(seed)
    out = [(np.zeros(n, np.uint8), np.zeros(n, np.uint8))]
    for _ in range(CALLS - 1):
        out.append(((rng.random(n) < 0.3).astype(np.uint8), (rng.random(n) < 0.2).astype(np.uint8)))
    return out


def _range_sets(n):
    return [[(0, n)]] + ([[(0, 33), (33, 1), (34, n - 34)]] if n > 34 else [])


@pytest.fixture(scope="module")
def tiny64(tmp_path_factory):
    """64 one-layer policies 12 -> 4 and their fused single evaluations."""
    d = tmp_path_factory.mktemp("rot64")
    files = []
    for k in range(64):
        files.append(str(d / f"q{k}.onnx"))
        write_random_mlp(files[-1], 12, 4, hidden=(), seed=500 + k)
    return files, [MLPPolicy(f, device=DEV, fused=True) for f in files]


# ------------------------------------------------------------------------------------------------------------- 4 + 5: lists and bits
@pytest.mark.parametrize("every", [1, 2])
@pytest.mark.parametrize("K", [1, 3, 64])
@pytest.mark.parametrize("n", [1, 31, 33, 65, 97])
def test_lists_counters_and_bits_call_by_call(family, tiny64, n, K, every):  # noqa: F811
    import torch
    files, singles = (tiny64 if K == 64 else (family[12][0][:K], family[12][2][:K]))
    base = _base(n, K, seed=n + K)
    owned = set()
    for ranges in _range_sets(n):
        tab = PolicyTable(files, num_envs=n, device=DEV, assign=base, ranges=ranges, rotate_every=every)
        assert tab._handle is not None and tab.graph_safe
        for i, (first, count) in enumerate(ranges):                      # armed: the static lists, padded to the capacity
            rows, tiles, used = _read_lists(tab, i)
            w_rows, w_tiles, w_used = _lists(base, K, first, count)
            assert (rows == w_rows).all() and (tiles == w_tiles).all() and used == w_used, (n, K, ranges, i)
        e = np.zeros(n, np.int64)
        for call, (term, trunc) in enumerate(_script(n, seed=31 * n + K)):
            xd = torch.tensor(_inputs(n, 12, seed=call + n), device=DEV)
            done = (torch.tensor(term, device=DEV), torch.tensor(trunc, device=DEV))
            out = torch.full((n, 4), 7.0, device=DEV)
            for i, (first, count) in enumerate(ranges):
                inside = np.zeros(n, bool)
                inside[first:first + count] = True
                sel = torch.tensor(inside, device=DEV)
                before = (out.clone(), tab.episode.clone(), tab.policy_now.clone())
                tab.get_action_range(i, xd, out, done=done)
                e[inside] += (term | trunc)[inside]
                now = _rule(base, e, every, K)
                rows, tiles, used = _read_lists(tab, i)
                w_rows, w_tiles, w_used = _lists(now, K, first, count)
                assert (rows == w_rows).all(), (n, K, every, ranges, call, i)
                assert (tiles == w_tiles).all() and used == w_used and (tiles[used:] == 0).all(), (n, K, every, ranges, call, i)
                assert (tab.episode.cpu().numpy()[inside] == e[inside]).all() and (tab.policy_now.cpu().numpy()[inside] == now[inside]).all()
                # a range call writes its own rows and advances its own counters only
                assert torch.equal(_bits(out[~sel]), _bits(before[0][~sel])) and torch.equal(tab.episode[~sel], before[1][~sel])
                assert torch.equal(tab.policy_now[~sel], before[2][~sel])
                if len(ranges) == 1:
                    owned.update(np.bincount(now, minlength=K).tolist())
            now = _rule(base, e, every, K)
            want = _single_rows(singles, xd, now)
            assert torch.equal(_bits(out), _bits(want)), (n, K, every, ranges, call)
            # the whole-fleet call without done flags: the same actions, no counter moves
            got = tab.get_action(xd)
            assert torch.equal(_bits(got), _bits(want)) and (tab.episode.cpu().numpy() == e).all(), (n, K, every, ranges, call)
        assert n < 31 or e.max() >= 2
        tab.close()
    if K == 3 and n == 65:
        assert {0, 32, 33} <= owned, owned                              # a policy without a row, with a full tile, with a full tile and one row
    if K == 3 and n == 97:
        assert {32, 33} <= owned, owned


@pytest.mark.parametrize("every", [1, 2])
def test_odd_input_width_and_differing_depths(family, every):  # noqa: F811
    """The in_dim 7 family (1, 2 and 3 layers, no width a multiple of 4) under rotation, one whole range and three uneven ones."""
    import torch
    files, _, singles = family[7]
    n, K = 97, 3
    base = _base(n, K, seed=5)
    for ranges in _range_sets(n):
        tab = PolicyTable(files, num_envs=n, device=DEV, assign=base, ranges=ranges, rotate_every=every)
        e = np.zeros(n, np.int64)
        for call, (term, trunc) in enumerate(_script(n, seed=77)):
            xd = torch.tensor(_inputs(n, 7, seed=call), device=DEV)
            done = (torch.tensor(term, device=DEV), torch.tensor(trunc, device=DEV))
            out = torch.full((n, 4), 7.0, device=DEV)
            for i in range(len(ranges)):
                tab.get_action_range(i, xd, out, done=done)
            e += term | trunc
            assert torch.equal(_bits(out), _bits(_single_rows(singles, xd, _rule(base, e, every, K)))), (ranges, call)
            assert (tab.episode.cpu().numpy() == e).all()
        tab.close()


def test_non_finite_row_follows_the_single_kernel_and_touches_no_other_env(family):  # noqa: F811
    import torch
    files, _, singles = family[12]
    n, K = 65, 3
    base = np.arange(n) % K
    tab = PolicyTable(files, num_envs=n, device=DEV, assign=base, rotate_every=1)
    ended = np.zeros(n, np.uint8)
    ended[::2] = 1
    done = (torch.tensor(ended, device=DEV), torch.zeros(n, dtype=torch.uint8, device=DEV))
    x = _inputs(n, 12, seed=21)
    clean = torch.full((n, 4), 7.0, device=DEV)
    tab.get_action_range(0, torch.tensor(x, device=DEV), clean, done=done)
    now = _rule(base, ended, 1, K)
    x[3] = np.nan
    x[8, 5] = np.inf
    xd = torch.tensor(x, device=DEV)
    got = tab.get_action(xd).clone()
    want = _single_rows(singles, xd, now)
    bad = torch.zeros(n, dtype=torch.bool, device=DEV)
    bad[[3, 8]] = True
    assert torch.equal(_bits(got[~bad]), _bits(clean[~bad]))
    g, w = got[bad], want[bad]
    assert torch.equal(torch.isnan(g), torch.isnan(w)) and torch.equal(_bits(torch.nan_to_num(g, nan=5.0)), _bits(torch.nan_to_num(w, nan=5.0)))
    assert bool(torch.isnan(got[3]).all())
    tab.close()


def test_entry_point_refusals(family):  # noqa: F811
    import torch
    files = family[12][0]
    n = 8
    L = PolicyTable(files, num_envs=n, device=DEV)._lib
    stream = torch.cuda.current_stream().cuda_stream
    x, out = torch.zeros((n, 12), device=DEV), torch.zeros((n, 4), device=DEV)
    ep = torch.zeros(n, dtype=torch.int32, device=DEV)

    def err():
        return L.cosim_last_error().decode()
    static = PolicyTable(files, num_envs=n, device=DEV)
    assert L.cosim_policy_table_forward_rotating(static._handle, x.data_ptr(), out.data_ptr(), ep.data_ptr(), None, None, None, 0, 1.0, stream) == -1
    assert "cosim_policy_table_forward_rotating: the table does not rotate" in err()
    for every in (0, -3):
        assert L.cosim_policy_table_rotate(static._handle, every) == -1 and f"cosim_policy_table_rotate: every {every} is below 1" in err()
    assert L.cosim_policy_table_rotate(static._handle, 2) == 0
    assert L.cosim_policy_table_rotate(static._handle, 3) == -1 and "already rotates (every 2)" in err()
    armed = static
    assert L.cosim_policy_table_forward(armed._handle, x.data_ptr(), out.data_ptr(), 0, 1.0, stream) == -1
    assert "cosim_policy_table_forward: the table rotates (every 2)" in err()
    for args, want in (((None, out.data_ptr(), ep.data_ptr()), "null argument"), ((x.data_ptr(), None, ep.data_ptr()), "null argument"),
                       ((x.data_ptr(), out.data_ptr(), None), "null argument")):
        assert L.cosim_policy_table_forward_rotating(armed._handle, *args, None, None, None, 0, 1.0, stream) == -1 and want in err()
    for r in (1, -2):
        assert L.cosim_policy_table_forward_rotating(armed._handle, x.data_ptr(), out.data_ptr(), ep.data_ptr(), None, None, None, r, 1.0, stream) == -1
        assert f"range {r} outside -1..0" in err()
    used = ctypes.c_int()
    rows, tiles = np.zeros(n, np.int32), np.zeros((_capacity(n, 3), 4), np.int32)
    assert L.cosim_policy_table_lists(armed._handle, 1, rows.ctypes.data, tiles.ctypes.data, ctypes.byref(used)) == -1 and "range 1 outside 0..0" in err()
    # either done pointer may be null, and policy_now is optional
    term = torch.ones(n, dtype=torch.uint8, device=DEV)
    assert L.cosim_policy_table_forward_rotating(armed._handle, x.data_ptr(), out.data_ptr(), ep.data_ptr(), None, None, term.data_ptr(), -1, 1.0, stream) == 0
    assert L.cosim_policy_table_forward_rotating(armed._handle, x.data_ptr(), out.data_ptr(), ep.data_ptr(), None, term.data_ptr(), None, -1, 1.0, stream) == 0
    torch.cuda.synchronize()
    assert (ep.cpu().numpy() == 2).all()
    armed.close()


# ------------------------------------------------------------------------------------------------------------------ 6: recurrent
REC = [([], _lstm(11, 8, 61, True), _layers((8, 4), [None], 62, last_scale=0.5)),                       # hidden 8
       (_layers((11, 16), ["Elu"], 63), _lstm(16, 20, 64, False), _layers((20, 4), [None], 65, last_scale=0.5)),   # hidden 20, an encoder
       ([], _lstm(11, 12, 66, True), _layers((12, 6, 4), ["Tanh", None], 67, last_scale=0.5))]           # hidden 12, two head layers


@pytest.mark.parametrize("every", [1, 2])
def test_recurrent_bits_and_stale_columns(tmp_path, every):
    import torch
    from cosim_amd.policy import write_recurrent_actor
    files = []
    for k, (enc, lstm, head) in enumerate(REC):
        files.append(str(tmp_path / f"r{k}.onnx"))
        write_recurrent_actor(files[-1], enc, lstm, head)
    n, K, Hs = 70, 3, [8, 20, 12]
    ranges = [(0, 33), (33, 1), (34, 36)]
    base = np.random.default_rng(2).integers(0, K, n)
    tab = RecurrentPolicyTable(files, num_envs=n, device=DEV, assign=base, ranges=ranges, rotate_every=every)
    comp = [_Composed(p, n) for p in REC]
    e = np.zeros(n, np.int64)
    rng = np.random.default_rng(12)
    for call, (term, trunc) in enumerate(_script(n, seed=99)):
        xd = torch.tensor(rng.standard_normal((n, 11)).astype(np.float32), device=DEV)
        done = (torch.tensor(term, device=DEV), torch.tensor(trunc, device=DEV))
        e += term | trunc
        now = _rule(base, e, every, K)
        fresh = torch.tensor((term | trunc) != 0, device=DEV)
        h0, c0 = tab.h.clone(), tab.c.clone()
        want, want_h, want_c = torch.zeros((n, 4), device=DEV), h0.clone(), c0.clone()
        for k in range(K):                                               # the chain of policy k on every row, kept where k drives the row now
            H = Hs[k]
            comp[k].h = h0[:, :H].masked_fill(fresh[:, None], 0.0).contiguous()
            comp[k].c = c0[:, :H].masked_fill(fresh[:, None], 0.0).contiguous()
            a = comp[k].step(xd)
            mine = torch.tensor(now == k, device=DEV)
            want = torch.where(mine[:, None], a, want)
            want_h[:, :H] = torch.where(mine[:, None], comp[k].h, want_h[:, :H])
            want_c[:, :H] = torch.where(mine[:, None], comp[k].c, want_c[:, :H])
        # the columns beyond the current policy's hidden size: NaN before the launch, never read by it
        width = torch.tensor(np.asarray(Hs)[now], device=DEV)
        stale = torch.arange(tab.h.shape[1], device=DEV)[None, :] >= width[:, None]
        tab.h.masked_fill_(stale, float("nan"))
        tab.c.masked_fill_(stale, float("nan"))
        out = torch.full((n, 4), 7.0, device=DEV)
        for i in (1, 2, 0):
            tab.get_action_range(i, xd, out, done=done)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(out).all()) and torch.equal(_bits(out), _bits(want)), call
        assert (tab.episode.cpu().numpy() == e).all() and (tab.policy_now.cpu().numpy() == now).all(), call
        assert torch.equal(_bits(tab.h[~stale]), _bits(want_h[~stale])) and torch.equal(_bits(tab.c[~stale]), _bits(want_c[~stale])), call
        assert bool(torch.isnan(tab.h[stale]).all())                     # and never written
        tab.h.masked_fill_(stale, 0.0)
        tab.c.masked_fill_(stale, 0.0)
        for i, (first, count) in enumerate(ranges):
            rows, tiles, used = _read_lists(tab, i, "cosim_recurrent_table_lists")
            w_rows, w_tiles, w_used = _lists(now, K, first, count)
            assert (rows == w_rows).all() and (tiles == w_tiles).all() and used == w_used, (call, i)
    assert e.max() >= 2
    tab.close()


def test_recurrent_entry_point_refusals(tmp_path):
    """``test_entry_point_refusals`` for the ``cosim_recurrent_table_*`` family: every refusal by its whole message, which begins with the
    recurrent entry point's own name."""
    import torch
    from cosim_amd.policy import write_recurrent_actor
    files = []
    for k, (enc, lstm, head) in enumerate(REC[:2]):
        files.append(str(tmp_path / f"r{k}.onnx"))
        write_recurrent_actor(files[-1], enc, lstm, head)
    n = 8
    tab = RecurrentPolicyTable(files, num_envs=n, device=DEV)
    L, p = tab._lib, tab._handle
    stream = torch.cuda.current_stream().cuda_stream
    x, out = torch.zeros((n, 11), device=DEV), torch.zeros((n, 4), device=DEV)
    h, c = torch.zeros((n, 20), device=DEV), torch.zeros((n, 20), device=DEV)
    ep = torch.zeros(n, dtype=torch.int32, device=DEV)
    ptr = {"x": x.data_ptr(), "h": h.data_ptr(), "c": c.data_ptr(), "out": out.data_ptr(), "episode": ep.data_ptr()}

    def rotating(r=0, da=None, db=None, **other):
        a = {**ptr, **other}
        return L.cosim_recurrent_table_forward_rotating(p, a["x"], a["h"], a["c"], a["out"], a["episode"], None, da, db, r, 1.0, stream)

    def err():
        return L.cosim_last_error().decode()
    assert rotating() == -1
    assert err() == "cosim_recurrent_table_forward_rotating: the table does not rotate (cosim_*_table_rotate arms it)"
    for every in (0, -3):
        assert L.cosim_recurrent_table_rotate(p, every) == -1 and err() == f"cosim_recurrent_table_rotate: every {every} is below 1"
    assert L.cosim_recurrent_table_rotate(p, 2) == 0
    assert L.cosim_recurrent_table_rotate(p, 3) == -1 and err() == "cosim_recurrent_table_rotate: the table already rotates (every 2)"
    assert L.cosim_recurrent_table_forward(p, ptr["x"], ptr["h"], ptr["c"], ptr["out"], None, None, 0, 1.0, stream) == -1
    assert err() == ("cosim_recurrent_table_forward: the table rotates (every 2): its lists change per step, use "
                     "cosim_recurrent_table_forward_rotating")
    for name in ptr:
        assert rotating(**{name: None}) == -1 and err() == "cosim_recurrent_table_forward_rotating: null argument", name
    for r in (1, -2):
        assert rotating(r) == -1 and err() == f"cosim_recurrent_table_forward_rotating: range {r} outside -1..0"
    used = ctypes.c_int()
    rows, tiles = np.zeros(n, np.int32), np.zeros((_capacity(n, 2), 4), np.int32)
    assert L.cosim_recurrent_table_lists(p, 1, rows.ctypes.data, tiles.ctypes.data, ctypes.byref(used)) == -1
    assert err() == "cosim_recurrent_table_lists: range 1 outside 0..0"
    # either done pointer may be null, and policy_now is optional
    term = torch.ones(n, dtype=torch.uint8, device=DEV)
    assert rotating(-1, None, term.data_ptr()) == 0
    assert rotating(-1, term.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert (ep.cpu().numpy() == 2).all() and bool(torch.isfinite(out).all())
    tab.close()


# ---------------------------------------------------------------------------------------------------------------------- 7 - 9: loops
NE, STEPS = 64, 40
CHECKS = [[0, 5, "up", 0, "always", ">", -2.0, "upright"]]


class _RotHostLoop:
    """The K single policies on the whole fleet, merged by the rule from a counter of its own that ``reset(mask)`` advances."""
    graph_safe = False

    def __init__(self, files, base, every, device):
        import torch
        self.torch, self.every, self.K = torch, every, len(files)
        self.pols = [MLPPolicy(f, device=device, fused=True) for f in files]
        self.base = torch.as_tensor(np.asarray(base), device=device).long()
        self.e = torch.zeros_like(self.base)

    def get_action(self, state):
        now = (self.base + self.e // self.every) % self.K
        out = None
        for k, p in enumerate(self.pols):
            a = p.get_action(state)
            out = a.clone() if out is None else self.torch.where((now == k)[:, None], a, out)
        return out

    def reset(self, mask=None):
        if mask is not None:
            self.e += (mask != 0).long()


def _env(**kw):
    from cosim_amd.batched_env import BatchedEnv
    from cosim_amd.config import make_config
    cfg = make_config("flamingo_light_v1", num_envs=NE, seed=7, max_duration=0.2)          # 10-step episodes: 4 rotations in 40 steps
    return BatchedEnv(cfg, num_envs=NE, seed=7, auto_reset=True, ledger=8, scenarios=[{"checks": CHECKS}, {"checks": CHECKS}], scenario_mode="env",
                      check_slots=8, **kw)


def _end(env, tab):
    import torch
    torch.cuda.synchronize()
    led = env.ledger()
    return {"state": env.state.clone(), "qpos": env.get_data().qpos.clone(), "episode": None if tab is None else tab.episode.clone(),
            "words": led.words.copy(), "env": led.env.copy()}


def _equal(a, b):
    import torch
    return (torch.equal(a["state"], b["state"]) and torch.equal(a["qpos"], b["qpos"]) and torch.equal(a["episode"], b["episode"])
            and np.array_equal(a["words"], b["words"]) and np.array_equal(a["env"], b["env"]))


@pytest.fixture(scope="module")
def rot_loop(tmp_path_factory):
    """Runner.test with the rotating table: the end state, and per step the policy that drove every env and the done flags."""
    import torch
    from cosim_amd.runner import Runner
    env = _env()
    d = tmp_path_factory.mktemp("rotloop")
    files = [str(d / f"actor{k}.onnx") for k in range(3)]
    for k, f in enumerate(files):
        write_random_mlp(f, env.state_dim, env.action_dim, hidden=(64, 64), seed=20 + k)
    base = np.random.default_rng(9).integers(0, 3, NE)
    tab = PolicyTable(files, num_envs=NE, device=env.device, assign=base, rotate_every=1)
    drove, ended, snap = [], [], {}

    def on_step(k, state, terminated, truncated, info):
        drove.append(tab.policy_now.cpu().numpy().copy())
        ended.append((terminated | truncated).cpu().numpy().astype(bool))
        if k + 1 == 15:
            snap["snap"] = env.snapshot(tab)
    run = Runner(env, tab)
    run.update_command(0, 0.5)
    assert run.test(max_steps=STEPS, on_step=on_step) == STEPS
    out = _end(env, tab)
    out.update({"files": files, "base": base, "drove": np.stack(drove), "ended": np.stack(ended), "snap": snap["snap"], "table": tab,
                "ledger": env.ledger(), "verdicts": env.verdicts()})
    assert int(out["episode"].min()) >= 3                                                  # at least 3 rotations per env
    env.close()
    return out


def test_eager_loop_equals_the_host_loop_over_single_policies(rot_loop):
    from cosim_amd.runner import Runner
    env = _env()
    host = _RotHostLoop(rot_loop["files"], rot_loop["base"], 1, env.device)
    run = Runner(env, host)
    run.update_command(0, 0.5)
    assert run.test(max_steps=STEPS) == STEPS
    got = _end(env, None)
    got["episode"] = host.e.int()
    assert _equal(got, rot_loop)
    env.close()


def test_graphed_loop_equals_the_eager_loop(rot_loop):
    from cosim_amd.runner import Runner
    env = _env()
    tab = PolicyTable(rot_loop["files"], num_envs=NE, device=env.device, assign=rot_loop["base"], rotate_every=1)
    run = Runner(env, tab)
    run.update_command(0, 0.5)
    assert run.test_graphed(STEPS) == STEPS
    assert _equal(_end(env, tab), rot_loop)
    env.close()


def test_pipelined_loop_equals_the_eager_loop(rot_loop):
    from cosim_amd.runner import Runner
    env = _env(ranges=4, deferred_join=True)
    tab = PolicyTable(rot_loop["files"], num_envs=NE, device=env.device, assign=rot_loop["base"], ranges=env.range_list, rotate_every=1)
    run = Runner(env, tab)
    run.update_command(0, 0.5)
    assert run.test_pipelined(STEPS) == STEPS
    # the pipelined loop counts an env's ended episode in the forward that FOLLOWS its last step; the eager loop right behind the step
    tab.reset(env.terminated | env.truncated)
    assert _equal(_end(env, tab), rot_loop)
    env.close()


def test_records_are_attributed_to_the_policy_that_drove_the_episode(rot_loop):
    tab, drove, ended = rot_loop["table"], rot_loop["drove"], rot_loop["ended"]
    # (env, ordinal) -> the policies seen while that episode ran: one, and the rule's
    ordinal = np.zeros(NE, np.int64)
    seen = {}
    for k in range(STEPS):
        for i in range(NE):
            seen.setdefault((i, int(ordinal[i])), set()).add(int(drove[k, i]))
        ordinal += ended[k]
    assert all(len(v) == 1 for v in seen.values())
    for rec in (rot_loop["ledger"], rot_loop["verdicts"]):
        m = rec.ended()
        assert m.sum() >= 3 * NE
        got = tab.policy_of(rec.env[m], rec.episode[m])
        want = np.array([next(iter(seen[(int(g), int(o))])) for g, o in zip(rec.env[m], rec.episode[m])])
        assert (got == want).all()
        by = rec.by_policy(tab)
        assert set(by) == {"actor0", "actor1", "actor2"} and sum(v["episodes"] for v in by.values()) == rec.counts()["episodes"] == int(m.sum())
        cells = rec.by_policy(tab, scenario=True)
        assert set(cells) == {(f"actor{k}", s) for k in range(3) for s in range(2)}          # every robot met every checkpoint
    with pytest.raises(ValueError, match="pass episodes="):
        tab.policy_of(rot_loop["ledger"].env)


def test_snapshot_continues_the_rotation(rot_loop):
    import torch
    from cosim_amd.runner import Runner
    snap = rot_loop["snap"]
    assert snap.policy_state is not None and set(snap.policy_state) == {"episode"} and int(snap.policy_state["episode"].max()) >= 1
    env = _env()
    tab = PolicyTable(rot_loop["files"], num_envs=NE, device=env.device, assign=rot_loop["base"], rotate_every=1)
    run = Runner(env, tab)
    assert run.test(max_steps=STEPS - 15, resume=snap) == STEPS - 15
    torch.cuda.synchronize()
    assert torch.equal(env.state, rot_loop["state"]) and torch.equal(env.get_data().qpos, rot_loop["qpos"])
    assert torch.equal(tab.episode, rot_loop["episode"])
    env.close()


# ------------------------------------------------------------------------------------------------------------------------- 10: CLI
@pytest.mark.parametrize("mode", ["", "--graph", "--pipelined"])
def test_cli_rotates_two_policies(tmp_path, capsys, rot_loop, mode):
    from cosim_amd import cli
    rep = tmp_path / "report.json"
    argv = ["--env", "flamingo_light_v1", "--num-envs", "32", "--steps", "60", "--max-duration", "0.3", "--seed", "5", "--policy", *rot_loop["files"][:2],
            "--policy-names", "a", "b", "--policy-rotate", "1", "--ledger", "4", "--report", str(rep)] + ([mode] if mode else [])
    assert cli.main(argv) == 0
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    by = json.loads(rep.read_text())["episodes"]["by_policy"]
    assert "rotate=1" in line["policy_table"]
    assert set(by) == {"a", "b"} == set(line["by_policy"])
    # 15-step episodes, 60 steps: every env ends 3 or 4, and alternates between the files
    assert by["a"]["episodes"] >= 32 and by["b"]["episodes"] >= 32 and abs(by["a"]["episodes"] - by["b"]["episodes"]) <= 32
