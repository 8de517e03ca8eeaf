"""The recurrent policy table on the device: ``RecurrentPolicyTable`` / ``cosim_recurrent_table_forward`` (lstm_actor_grouped_kernel,
csrc/cosim_mlp.hip) bit for bit against the composition of the single-policy entry points -- ``cosim_mlp_forward`` (encoder, clip 0)
-> ``cosim_lstm_cell`` -> ``cosim_mlp_forward`` (head, clip 1) on each policy's gathered rows -- and against fp64 numpy; ranges; the
reset folded into the forward; non-finite rows; graph capture; the runner's three loops; snapshots; the CLI.  Bad tables are refused
on the host before any launch (tests/test_recurrent_table_host.py)."""
import ctypes
import json

import numpy as np
import pytest

from cosim_amd.policy import _ACT, RecurrentPolicyTable, write_random_lstm, write_recurrent_actor

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ATOL_STATE, ATOL_ACTION = 2e-5, 3e-5          # the tolerances of tests/test_gpu_policy_kernels.py
N, IN, OUT = 70, 11, 4


# ------------------------------------------------------------------------------------------------ the three policies of the bit test
def _layers(dims, acts, seed, last_scale=1.0, nobias=()):
    """(w, b, op, alpha) per layer: weights N(0, 1 / fan_in) (the last layer times ``last_scale``), biases 0.5 N(0, 1)."""
    rng = np.random.default_rng(seed)
    out = []
    for l in range(len(dims) - 1):
        w = rng.standard_normal((dims[l + 1], dims[l])) / np.sqrt(dims[l]) * (last_scale if l == len(dims) - 2 else 1.0)
        out.append((w.astype(np.float32), None if l in nobias else (0.5 * rng.standard_normal(dims[l + 1])).astype(np.float32), acts[l],
                    float(np.float32(0.3))))
    return out


def _lstm(I, H, seed, bias):
    rng = np.random.default_rng(seed)
    W = (rng.standard_normal((4 * H, I)) / np.sqrt(I)).astype(np.float32)
    R = (rng.standard_normal((4 * H, H)) / np.sqrt(H)).astype(np.float32)
    B = None
    if bias:
        # the two halves (Wb, Rb) clearly different, and different per gate: a kernel that indexed them wrongly could not pass
        B = (0.2 * rng.standard_normal(8 * H) + np.repeat([0.5, -1.0, 1.5, -0.5, -2.0, 0.75, -0.25, 1.0], H)).astype(np.float32)
    return W, R, B


POLICIES = [  # enc, lstm, head
    ([], _lstm(11, 6, 11, True), _layers((6, 4), [None], 12, last_scale=0.5)),                          # A: I + H = 17, odd
    (_layers((11, 16), ["Elu"], 21), _lstm(16, 70, 22, False),                                          # B: 2.2 hidden tiles, no B, float4 path
     _layers((70, 8, 4), ["Tanh", None], 23, last_scale=0.5, nobias=(1,))),
    (_layers((11, 9), ["LeakyRelu"], 31), _lstm(9, 160, 32, True), _layers((160, 4), [None], 33, last_scale=0.3)),   # C: a wave takes two hidden tiles
]
ASSIGN = np.random.default_rng(1).permutation(np.array([0] * 33 + [1] * 36 + [2]))                      # tiles 32 + 1, 32 + 4, 1


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("rectab")
    out = []
    for k, (enc, lstm, head) in enumerate(POLICIES):
        out.append(str(d / f"p{k}.onnx"))
        write_recurrent_actor(out[-1], enc, lstm, head, read="Y" if k == 1 else "Y_h")
    return out


def _bits(t):
    import torch
    return t.contiguous().view(torch.int32)


def _same(a, b):
    import torch
    return torch.equal(_bits(a), _bits(b))


# ------------------------------------------------------------------------------------- the composed entry points (the bit reference)
class _Composed:
    """One policy through the single-policy entry points on its own rows, state carried: cosim_mlp_forward (encoder, clip 0) ->
    cosim_lstm_cell -> cosim_mlp_forward (head on h', clip 1)."""

    def __init__(self, policy, n):
        import torch
        from cosim_amd.engine import load_library
        self.t, self.L = torch, load_library()
        self.L.cosim_mlp_forward.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                             ctypes.c_void_p, ctypes.c_void_p, ctypes.c_float, ctypes.c_void_p, ctypes.c_void_p]
        self.L.cosim_lstm_cell.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_int] * 3 + [ctypes.c_void_p] * 6
        enc, (W, R, B), head = policy
        dev = lambda a: None if a is None else torch.tensor(a, device=DEV)   # noqa: E731
        self.enc, self.head = [self._chain(c, dev) for c in (enc, head)]
        self.W, self.R, self.B = dev(W), dev(R), dev(B)
        self.H = R.shape[1]
        self.h = torch.zeros((n, self.H), device=DEV)
        self.c = torch.zeros((n, self.H), device=DEV)

    @staticmethod
    def _chain(layers, dev):
        if not layers:
            return None
        nl = len(layers)
        ws, bs = [dev(w) for w, *_ in layers], [dev(b) for _, b, *_ in layers]
        return {"nl": nl, "keep": (ws, bs), "dims": (ctypes.c_int * (nl + 1))(layers[0][0].shape[1], *[w.shape[0] for w, *_ in layers]),
                "w": (ctypes.c_void_p * nl)(*[w.data_ptr() for w in ws]), "b": (ctypes.c_void_p * nl)(*[None if b is None else b.data_ptr() for b in bs]),
                "act": (ctypes.c_int * nl)(*[0 if op is None else _ACT[op] for _, _, op, _ in layers]),
                "alpha": (ctypes.c_float * nl)(*[al for *_, al in layers]), "out": layers[-1][0].shape[0]}

    def _mlp(self, f, x, clip):
        t = self.t
        out = t.empty((x.shape[0], f["out"]), device=DEV)
        assert self.L.cosim_mlp_forward(x.data_ptr(), x.shape[0], f["nl"], f["dims"], f["w"], f["b"], f["act"], f["alpha"], clip, out.data_ptr(),
                                        t.cuda.current_stream().cuda_stream) == 0
        return out

    def step(self, x):
        t = self.t
        x = x.contiguous()
        xe = x if self.enc is None else self._mlp(self.enc, x, 0.0)
        hn, cn = t.empty_like(self.h), t.empty_like(self.c)
        assert self.L.cosim_lstm_cell(xe.data_ptr(), self.h.data_ptr(), self.c.data_ptr(), x.shape[0], xe.shape[1], self.H, self.W.data_ptr(),
                                      self.R.data_ptr(), None if self.B is None else self.B.data_ptr(), hn.data_ptr(), cn.data_ptr(),
                                      t.cuda.current_stream().cuda_stream) == 0
        self.h, self.c = hn, cn
        return self._mlp(self.head, hn, 1.0)


# --------------------------------------------------------------------------------------------------------------- the fp64 reference
def _act64(v, op, alpha):
    with np.errstate(all="ignore"):
        return {None: lambda: v, "Tanh": lambda: np.tanh(v), "Elu": lambda: np.where(v > 0, v, alpha * (np.exp(np.minimum(v, 0.0)) - 1.0)),
                "LeakyRelu": lambda: np.where(v > 0, v, alpha * v)}[op]()


def _chain64(x, layers):
    for w, b, op, alpha in layers:
        x = x @ w.astype(np.float64).T + (0.0 if b is None else b.astype(np.float64))
        x = _act64(x, op, alpha)
    return x


def _step64(policy, x, h, c):
    enc, (W, R, B), head = policy
    H = R.shape[1]
    sig = lambda v: 1.0 / (1.0 + np.exp(-v))   # noqa: E731
    g = _chain64(x, enc) @ W.astype(np.float64).T + h @ R.astype(np.float64).T
    if B is not None:
        g = g + B[:4 * H].astype(np.float64) + B[4 * H:].astype(np.float64)
    i, o, f, cc = g[:, :H], g[:, H:2 * H], g[:, 2 * H:3 * H], g[:, 3 * H:]
    c = sig(f) * c + sig(i) * np.tanh(cc)
    h = sig(o) * np.tanh(c)
    return _chain64(h, head), h, c


def _obs(seed, n=N):
    x = np.random.default_rng(seed).standard_normal((n, IN)).astype(np.float32)
    x[n // 2] *= 5.0
    return x


# ------------------------------------------------------------------------------------------------------------------ 1: bit equality
def test_every_env_gets_the_bits_of_the_composed_entry_points(files):
    import torch
    tab = RecurrentPolicyTable(files, num_envs=N, device=DEV, assign=ASSIGN)
    assert tab._handle is not None and tab.graph_safe and tab.recurrent and tab.hidden == [6, 70, 160] and tab.h.shape == (N, 160)
    idx = [np.nonzero(ASSIGN == k)[0] for k in range(3)]
    assert [len(i) for i in idx] == [33, 36, 1]
    tidx = [torch.as_tensor(i, device=DEV) for i in idx]
    comp = [_Composed(p, len(i)) for p, i in zip(POLICIES, idx)]
    h64 = [np.zeros((len(i), p[1][1].shape[1])) for p, i in zip(POLICIES, idx)]
    c64 = [z.copy() for z in h64]
    for step in range(3):
        x = _obs(100 + step)
        xd = torch.tensor(x, device=DEV)
        got = tab.get_action(xd)
        assert got.shape == (N, OUT) and got.data_ptr() == tab._out.data_ptr()
        for k, (cp, i, ti) in enumerate(zip(comp, idx, tidx)):
            H = cp.H
            want = cp.step(xd[ti])
            a64, h64[k], c64[k] = _step64(POLICIES[k], x[i].astype(np.float64), h64[k], c64[k])
            inside = float(np.mean(np.abs(a64) < 1.0))
            eh = np.abs(tab.h[ti, :H].cpu().numpy() - h64[k]).max()
            ec = np.abs(tab.c[ti, :H].cpu().numpy() - c64[k]).max()
            ea = np.abs(got[ti].cpu().numpy() - np.clip(a64, -1.0, 1.0)).max()
            print(f"step {step} policy {k}: inside={inside:.2f} h-fp64={eh:.2e} c-fp64={ec:.2e} action-fp64={ea:.2e} "
                  f"bits h/c/a={_same(tab.h[ti, :H], cp.h)}/{_same(tab.c[ti, :H], cp.c)}/{_same(got[ti], want)}")
            assert inside >= 0.5, (step, k, inside)                                            # saturated outputs would hide errors
            assert _same(tab.h[ti, :H], cp.h) and _same(tab.c[ti, :H], cp.c) and _same(got[ti], want), (step, k)
            assert eh <= ATOL_STATE and ec <= ATOL_STATE and ea <= ATOL_ACTION, (step, k, eh, ec, ea)
            assert bool((tab.h[ti, H:] == 0).all()) and bool((tab.c[ti, H:] == 0).all()), (step, k)   # columns H_k .. Hmax stay zero
        assert float(tab.h.abs().max()) > 0.05
    tab.close()


# ------------------------------------------------------------------------------------------------------------------------ 2: ranges
@pytest.fixture(scope="module")
def warm(files):
    """A state two steps into a run, and the observation of the step that follows."""
    import torch
    tab = RecurrentPolicyTable(files, num_envs=N, device=DEV, assign=ASSIGN)
    for s in range(2):
        tab.get_action(torch.tensor(_obs(200 + s), device=DEV))
    out = {"state": tab.state(), "x": torch.tensor(_obs(210), device=DEV)}
    tab.close()
    return out


def test_a_range_writes_its_own_rows_only(files, warm):
    import torch
    ranges = [(0, 20), (20, 50)]
    whole = RecurrentPolicyTable(files, num_envs=N, device=DEV, assign=ASSIGN, ranges=ranges)
    whole.load_state(warm["state"])
    act_whole = whole.get_action(warm["x"]).clone()
    tab = RecurrentPolicyTable(files, num_envs=N, device=DEV, assign=ASSIGN, ranges=ranges)
    tab.load_state(warm["state"])
    act = torch.full((N, OUT), 7.0, device=DEV)
    tab.get_action_range(1, warm["x"], act)
    assert bool((act[:20] == 7.0).all()) and _same(tab.h[:20], warm["state"]["h"][:20]) and _same(tab.c[:20], warm["state"]["c"][:20])
    assert _same(act[20:], act_whole[20:]) and _same(tab.h[20:], whole.h[20:]) and _same(tab.c[20:], whole.c[20:])
    assert not _same(tab.h[20:], warm["state"]["h"][20:])
    tab.get_action_range(0, warm["x"], act)
    assert _same(act, act_whole) and _same(tab.h, whole.h) and _same(tab.c, whole.c)
    # the entry point refuses what it cannot launch
    L, stream = tab._lib, torch.cuda.current_stream().cuda_stream
    args = [warm["x"].data_ptr(), tab.h.data_ptr(), tab.c.data_ptr(), act.data_ptr()]
    for rng_i in (2, -2):
        assert L.cosim_recurrent_table_forward(tab._handle, *args, None, None, rng_i, 1.0, stream) == -1
        assert f"range {rng_i} outside -1..1" in L.cosim_last_error().decode()
    for missing in range(4):
        a = list(args)
        a[missing] = None
        assert L.cosim_recurrent_table_forward(tab._handle, *a, None, None, 0, 1.0, stream) == -1
        assert "null argument" in L.cosim_last_error().decode()
    torch.cuda.synchronize()
    assert _same(tab.h, whole.h) and _same(act, act_whole)                                     # a refused call launched nothing
    with pytest.raises(ValueError, match="contiguous fp32"):
        tab.get_action_range(0, warm["x"], torch.zeros((N, 8), device=DEV)[:, ::2])
    whole.close()
    tab.close()


# -------------------------------------------------------------------------------------------------------------------- 3: reset fold
def test_done_rows_start_from_a_zero_state_in_the_same_launch(files, warm):
    import torch
    rng = np.random.default_rng(3)
    term = torch.tensor((rng.random(N) < 0.3).astype(np.uint8), device=DEV)
    trunc = torch.tensor((rng.random(N) < 0.2).astype(np.uint8), device=DEV)
    done = (term | trunc) != 0
    assert 10 < int(done.sum()) < N - 10
    # NaN and 1e30, alternating, in the state of the flagged rows, inside their policy's columns
    hid = torch.as_tensor(np.asarray([6, 70, 160])[ASSIGN], device=DEV)
    col = torch.arange(160, device=DEV)[None, :]
    plant = done[:, None] & (col < hid[:, None])
    poison = torch.where(col % 2 == 0, torch.tensor(float("nan"), device=DEV), torch.tensor(1e30, device=DEV)).expand(N, 160)
    bad = {"h": torch.where(plant, poison, warm["state"]["h"]), "c": torch.where(plant, poison.roll(1, dims=1), warm["state"]["c"])}
    assert bool(torch.isnan(bad["h"][done]).any()) and bool((bad["c"][done] == 1e30).any())
    folded = RecurrentPolicyTable(files, num_envs=N, device=DEV, assign=ASSIGN)
    folded.load_state(bad)
    act = torch.zeros((N, OUT), device=DEV)
    folded.get_action_range(0, warm["x"], act, done=(term, trunc))
    # the same as reset(mask) followed by a forward without done
    ref = RecurrentPolicyTable(files, num_envs=N, device=DEV, assign=ASSIGN)
    ref.load_state(bad)
    ref.reset(term | trunc)
    act_ref = ref.get_action(warm["x"])
    assert _same(act, act_ref) and _same(folded.h, ref.h) and _same(folded.c, ref.c)
    # flagged rows: the bits a fresh zero state gives, and finite state afterwards; unflagged rows: the run goes on
    fresh = RecurrentPolicyTable(files, num_envs=N, device=DEV, assign=ASSIGN)
    act_fresh = fresh.get_action(warm["x"])
    cont = RecurrentPolicyTable(files, num_envs=N, device=DEV, assign=ASSIGN)
    cont.load_state(warm["state"])
    act_cont = cont.get_action(warm["x"])
    assert _same(act[done], act_fresh[done]) and _same(folded.h[done], fresh.h[done]) and _same(folded.c[done], fresh.c[done])
    assert bool(torch.isfinite(folded.h).all()) and bool(torch.isfinite(folded.c).all()) and bool(torch.isfinite(act).all())
    assert _same(act[~done], act_cont[~done]) and _same(folded.h[~done], cont.h[~done]) and _same(folded.c[~done], cont.c[~done])
    assert not _same(folded.h[~done], fresh.h[~done])
    # either flag alone is enough
    for flags in ((term, None), (None, trunc)):
        one = RecurrentPolicyTable(files, num_envs=N, device=DEV, assign=ASSIGN)
        one.load_state(warm["state"])
        zero = torch.zeros_like(term)
        f = (flags[0] if flags[0] is not None else zero, flags[1] if flags[1] is not None else zero)
        one.get_action_range(0, warm["x"], act, done=f)
        m = (f[0] | f[1]) != 0
        assert _same(one.h[m], fresh.h[m]) and _same(one.h[~m], cont.h[~m])
        one.close()
    for t_ in (folded, ref, fresh, cont):
        t_.close()


# -------------------------------------------------------------------------------------------------------------------- 4: isolation
def test_a_non_finite_observation_touches_no_other_env(files, warm):
    import torch
    clean = RecurrentPolicyTable(files, num_envs=N, device=DEV, assign=ASSIGN)
    clean.load_state(warm["state"])
    act_clean = clean.get_action(warm["x"]).clone()
    x = warm["x"].clone()
    rows = [int(np.nonzero(ASSIGN == 0)[0][3]), int(np.nonzero(ASSIGN == 1)[0][5]), int(np.nonzero(ASSIGN == 1)[0][33])]   # full tiles and the 4-row tile
    x[rows[0]] = float("nan")
    x[rows[1], 4] = float("inf")
    x[rows[2], 0] = float("-inf")
    dirty = RecurrentPolicyTable(files, num_envs=N, device=DEV, assign=ASSIGN)
    dirty.load_state(warm["state"])
    act = dirty.get_action(x)
    bad = torch.zeros(N, dtype=torch.bool, device=DEV)
    bad[rows] = True
    assert _same(act[~bad], act_clean[~bad]) and _same(dirty.h[~bad], clean.h[~bad]) and _same(dirty.c[~bad], clean.c[~bad])
    assert bool(torch.isnan(act[rows[0]]).all()) and bool(torch.isnan(dirty.h[rows[0], :6]).all())     # NaN in, NaN out
    assert not _same(dirty.h[bad], clean.h[bad])
    clean.close()
    dirty.close()


# ---------------------------------------------------------------------------------------------------------------------- 5: capture
def test_captured_forward_replays_like_eager_calls(files, warm):
    import torch
    xs = [torch.tensor(_obs(300 + s), device=DEV) for s in range(3)]
    eager = RecurrentPolicyTable(files, num_envs=N, device=DEV, assign=ASSIGN)
    eager.load_state(warm["state"])
    want = [eager.get_action(x).clone() for x in xs]
    tab = RecurrentPolicyTable(files, num_envs=N, device=DEV, assign=ASSIGN)
    x_in = xs[0].clone()
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        tab.get_action(x_in)                                                               # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = tab.get_action(x_in)
    tab.load_state(warm["state"])
    for x, w in zip(xs, want):
        x_in.copy_(x)
        graph.replay()
        assert _same(out, w)
    torch.cuda.synchronize()
    assert _same(tab.h, eager.h) and _same(tab.c, eager.c)
    eager.close()
    tab.close()


# ------------------------------------------------------------------------------------------------------------------ 6: closed loop
NE, STEPS = 64, 70


def _env(**kw):
    from cosim_amd.batched_env import BatchedEnv
    from cosim_amd.config import make_config
    cfg = make_config("flamingo_light_v1", num_envs=NE, seed=7, max_duration=1.0)          # 50-step episodes: auto-reset inside the run
    return BatchedEnv(cfg, num_envs=NE, seed=7, auto_reset=True, ledger=4, **kw)


def _end(env, tab):
    import torch
    torch.cuda.synchronize()
    led = env.ledger()
    return {"state": env.state.clone(), "qpos": env.get_data().qpos.clone(), "h": tab.h.clone(), "c": tab.c.clone(), "words": led.words.copy(),
            "env": led.env.copy(), "episodes": env.solver_stats()["episodes_ended"]}


def _equal(a, b, rows=None):
    import torch
    sel = slice(None) if rows is None else torch.as_tensor(rows, device=DEV)
    ok = all(torch.equal(a[k][sel], b[k][sel]) for k in ("state", "qpos"))
    w = min(a["h"].shape[1], b["h"].shape[1])                                              # a K = 1 table is as wide as its own policy
    ok = ok and all(_same(a[k][sel][:, :w], b[k][sel][:, :w]) for k in ("h", "c"))
    if rows is None:
        return ok and np.array_equal(a["words"], b["words"]) and np.array_equal(a["env"], b["env"]) and a["episodes"] == b["episodes"]
    keep_a, keep_b = np.isin(a["env"], rows), np.isin(b["env"], rows)
    return ok and np.array_equal(a["words"][keep_a], b["words"][keep_b]) and np.array_equal(a["env"][keep_a], b["env"][keep_b])


@pytest.fixture(scope="module")
def loop_files(tmp_path_factory):
    env = _env()
    d = tmp_path_factory.mktemp("recloop")
    out = [str(d / "a.onnx"), str(d / "b.onnx")]
    write_random_lstm(out[0], env.state_dim, env.action_dim, hidden=48, head=(16,), seed=40, bias_scale=0.1)
    write_random_lstm(out[1], env.state_dim, env.action_dim, hidden=24, encoder=(32,), head=(), seed=41, bias_scale=0.1)
    env.close()
    return out


@pytest.fixture(scope="module")
def eager_loop(loop_files):
    from cosim_amd.runner import Runner
    env = _env()
    tab = RecurrentPolicyTable(loop_files, num_envs=NE, device=env.device, assign="interleave")
    run = Runner(env, tab)
    run.update_command(0, 0.5)
    assert run.test(max_steps=STEPS) == STEPS
    out = _end(env, tab)
    assert out["episodes"] >= NE and float(out["h"].abs().max()) > 0                       # the time limit fired inside the run
    env.close()
    return out


def test_graphed_loop_equals_the_eager_loop(loop_files, eager_loop):
    from cosim_amd.runner import Runner
    env = _env()
    tab = RecurrentPolicyTable(loop_files, num_envs=NE, device=env.device, assign="interleave")
    run = Runner(env, tab)
    run.update_command(0, 0.5)
    assert run.test_graphed(STEPS) == STEPS
    assert _equal(_end(env, tab), eager_loop)
    env.close()


def test_pipelined_loop_equals_the_eager_loop(loop_files, eager_loop):
    from cosim_amd.runner import Runner
    env = _env(ranges=4, deferred_join=True)
    tab = RecurrentPolicyTable(loop_files, num_envs=NE, device=env.device, assign="interleave", ranges=env.range_list)
    run = Runner(env, tab)
    run.update_command(0, 0.5)
    assert run.test_pipelined(STEPS) == STEPS
    # the pipelined loop resets an env's state in the forward that FOLLOWS its last step; the eager loop right behind the step
    tab.reset(env.terminated | env.truncated)
    assert _equal(_end(env, tab), eager_loop)
    with pytest.raises(ValueError, match="ranges"):                                        # a table built for other ranges is refused
        Runner(env, RecurrentPolicyTable(loop_files, num_envs=NE, device=env.device, assign="interleave")).test_pipelined(1)
    env.close()


@pytest.mark.parametrize("k", [0, 1])
def test_each_env_runs_as_under_a_table_of_its_own_policy(loop_files, eager_loop, k):
    from cosim_amd.runner import Runner
    env = _env()
    tab = RecurrentPolicyTable([loop_files[k]], num_envs=NE, device=env.device)
    run = Runner(env, tab)
    run.update_command(0, 0.5)
    assert run.test(max_steps=STEPS) == STEPS
    assert _equal(_end(env, tab), eager_loop, rows=np.arange(k, NE, 2))
    env.close()


# --------------------------------------------------------------------------------------------------------------------- 7: snapshot
def test_snapshot_carries_the_recurrent_state(loop_files):
    import torch
    env = _env()
    tab = RecurrentPolicyTable(loop_files, num_envs=NE, device=env.device, assign="interleave")
    env.receive_user_command(np.array([0.5, 0.0, 0.0, 0.0], dtype=np.float32)[:max(env.command_dim, 0)])

    def steps(state, n):
        for _ in range(n):
            state, terminated, truncated, _ = env.step(tab.get_action(state))
            tab.reset(terminated | truncated)
        return state
    state, _ = env.reset()
    state = steps(state, 30)
    snap = env.snapshot(tab)
    assert snap.policy_state is not None and _same(snap.policy_state["h"], tab.h) and float(tab.h.abs().max()) > 0
    steps(state, 20)
    first = {"state": env.state.clone(), "h": tab.h.clone(), "c": tab.c.clone(), "out": tab._out.clone()}
    state = env.restore(snap, params=True)
    assert not _same(tab.h, snap.policy_state["h"])
    tab.load_state(snap.policy_state)
    steps(state, 20)
    torch.cuda.synchronize()
    assert torch.equal(env.state, first["state"]) and _same(tab.h, first["h"]) and _same(tab.c, first["c"]) and _same(tab._out, first["out"])
    env.close()


# --------------------------------------------------------------------------------------------------------------------------- 8: CLI
@pytest.mark.parametrize("mode", ["", "--graph", "--pipelined"])
def test_cli_with_two_recurrent_policies(tmp_path, capsys, loop_files, mode):
    from cosim_amd import cli
    rep = tmp_path / "report.json"
    argv = ["--env", "flamingo_light_v1", "--num-envs", "64", "--steps", "40", "--max-duration", "0.3", "--seed", "5", "--policy", *loop_files,
            "--ledger", "4", "--report", str(rep)] + ([mode] if mode else [])
    assert cli.main(argv) == 0
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    by = json.loads(rep.read_text())["episodes"]["by_policy"]
    assert set(by) == {"a", "b"} == set(line["by_policy"])
    assert by["a"]["episodes"] >= 64 and by["b"]["episodes"] >= 64                          # 32 envs each, at least two time limits
