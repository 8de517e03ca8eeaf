"""The policy table on the device: ``PolicyTable`` / ``cosim_policy_table_forward`` (mlp_grouped_kernel, csrc/cosim_mlp.hip) against the
single-policy kernel bit for bit and against plain fp64 numpy chains at the project's 2e-5; ranges; non-finite rows; the runner's
three loops against a host loop over the single policies; the assignment as the engine sees it; the CLI.  Bad tables are refused on
the host before any launch (tests/test_policy_table_host.py)."""
import json

import numpy as np
import pytest

from cosim_amd.policy import MLPPolicy, PolicyTable, write_onnx, write_random_mlp

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ATOL = 2e-5


# ---------------------------------------------------------------------------------------------- fp64 reference of a Gemm / activation chain
def _act64(v, op, alpha):
    if op is None:
        return v
    if op == "Tanh":
        return np.tanh(v)
    if op == "Sigmoid":
        return 1.0 / (1.0 + np.exp(-v))
    if op == "Elu":
        return np.where(v > 0, v, alpha * (np.exp(np.minimum(v, 0.0)) - 1.0))
    if op == "LeakyRelu":
        return np.where(v > 0, v, alpha * v)
    raise AssertionError(op)


def _ref_chain(x, layers):
    h = np.asarray(x, dtype=np.float64)
    with np.errstate(all="ignore"):
        for w, b, op, alpha in layers:
            h = h @ w.astype(np.float64).T
            if b is not None:
                h = h + b.astype(np.float64)
            h = _act64(h, op, alpha)
    return h


def _make_layers(dims, acts, seed, last_scale, nobias=()):
    """Weights N(0, 1 / fan_in) (the last layer times ``last_scale``), biases 0.5 N(0, 1); ``acts``: per layer None or ("Op", alpha)."""
    rng = np.random.default_rng(seed)
    layers = []
    for li in range(len(dims) - 1):
        w = rng.standard_normal((dims[li + 1], dims[li])) / np.sqrt(dims[li])
        if li == len(dims) - 2:
            w = w * last_scale
        b = None if li in nobias else (0.5 * rng.standard_normal(dims[li + 1])).astype(np.float32)
        op, alpha = acts[li] if acts[li] is not None else (None, 1.0)
        layers.append((w.astype(np.float32), b, op, float(np.float32(alpha))))
    return layers


def _write_chain(path, layers):
    nodes, init, x = [], {}, "obs"
    for li, (w, b, op, alpha) in enumerate(layers):
        init[f"w{li}"] = w
        ins = [x, f"w{li}"]
        if b is not None:
            init[f"b{li}"] = b
            ins.append(f"b{li}")
        last = li == len(layers) - 1
        lin = "actions" if last and op is None else f"lin{li}"
        nodes.append({"op": "Gemm", "inputs": ins, "outputs": [lin], "attrs": {"transB": 1}})
        x = lin
        if op is not None:
            x = "actions" if last else f"h{li}"
            nodes.append({"op": op, "inputs": [lin], "outputs": [x], "attrs": {"alpha": alpha} if op in ("Elu", "LeakyRelu") else {}})
    write_onnx(path, nodes, init, ["obs"], ["actions"])


# two families of three chains with one input and output width each: (dims, acts, last-layer scale, layers without bias).  The first
# layer of the in_dim 12 family takes the kernel's float4 path, that of the in_dim 7 family the odd-width path; the hidden widths mix
# both.  The scales keep at least half of the fp64 outputs strictly inside (-1, 1) (asserted per case).
FAMILIES = {
    12: [((12, 40, 36, 4), [("LeakyRelu", 0.2), ("Elu", 0.3), None], 0.1, ()),
         ((12, 33, 4), [("Sigmoid", 1.0), None], 0.5, (0,)),
         ((12, 4), [None], 0.1, ())],
    7: [((7, 33, 4), [("Sigmoid", 1.0), None], 0.5, (0,)),
        ((7, 9, 10, 4), [("Tanh", 1.0), ("Elu", 0.3), None], 0.3, ()),
        ((7, 4), [None], 0.1, ())],
}


@pytest.fixture(scope="module")
def family(tmp_path_factory):
    """in_dim -> (files, layers per file, fused single policies), made once."""
    import torch  # noqa: F401
    d = tmp_path_factory.mktemp("poltab")
    out = {}
    for in_dim, chains in FAMILIES.items():
        files, layers = [], []
        for k, (dims, acts, scale, nobias) in enumerate(chains):
            layers.append(_make_layers(dims, acts, seed=100 * in_dim + k, last_scale=scale, nobias=nobias))
            files.append(str(d / f"in{in_dim}_p{k}.onnx"))
            _write_chain(files[-1], layers[-1])
        singles = [MLPPolicy(f, device=DEV, fused=True) for f in files]
        assert all(s._fused is not None for s in singles)
        out[in_dim] = (files, layers, singles)
    return out


def _inputs(n, d, seed):
    x = np.random.default_rng(seed).standard_normal((n, d)).astype(np.float32)
    x[n // 2] *= 10.0
    return x


def _assignments(n, K, seed):
    rng = np.random.default_rng(seed)
    out = {"interleave": np.arange(n) % K, "random": rng.integers(0, K, n), "policy_1_empty": np.where(rng.integers(0, 2, n) == 0, 0, K - 1)}
    if n >= 65:
        a = np.full(n, K - 1)
        a[:65] = rng.permutation(np.array([0] * 32 + [1] * 33))
        out["32_and_33"] = a
    return out


def _bits(t):
    import torch
    return t.contiguous().view(torch.int32)


def _single_rows(singles, xd, assign):
    """What each env's own policy gives it when that policy is run alone on the whole batch (cosim_mlp_forward)."""
    import torch
    a = torch.as_tensor(np.asarray(assign), device=DEV)
    want = torch.zeros((xd.shape[0], 4), dtype=torch.float32, device=DEV)
    for k, s in enumerate(singles):
        want = torch.where((a == k)[:, None], s.get_action(xd).clone(), want)
    return want


# ------------------------------------------------------------------------------------------------------------------ 1: bit equality
@pytest.mark.parametrize("n", [1, 31, 33, 65, 97])
@pytest.mark.parametrize("in_dim", [12, 7])
def test_every_env_gets_the_bits_of_its_own_policy(family, in_dim, n):
    import torch
    files, layers, singles = family[in_dim]
    x = _inputs(n, in_dim, seed=n)
    xd = torch.tensor(x, device=DEV)
    refs = [_ref_chain(x, L) for L in layers]
    for name, assign in _assignments(n, 3, seed=n).items():
        ref = np.stack(refs)[np.asarray(assign), np.arange(n)]
        inside = np.mean(np.abs(ref) < 1.0)
        assert inside >= 0.5, (in_dim, n, name, inside)                 # saturated outputs would hide errors
        tab = PolicyTable(files, num_envs=n, device=DEV, assign=np.asarray(assign))
        assert tab._handle is not None and tab.graph_safe
        got = tab.get_action(xd)
        want = _single_rows(singles, xd, assign)
        err = np.abs(got.cpu().numpy() - np.clip(ref, -1.0, 1.0)).max()
        print(f"in_dim={in_dim} n={n} {name}: inside={inside:.2f} table-fp64={err:.2e} bit-equal={torch.equal(_bits(got), _bits(want))}")
        assert got.shape == (n, 4) and got.data_ptr() == tab.get_action(xd).data_ptr()
        assert torch.equal(_bits(got), _bits(want)), (in_dim, n, name)
        np.testing.assert_allclose(got.cpu().numpy(), np.clip(ref, -1.0, 1.0), rtol=0, atol=ATOL, err_msg=f"in_dim={in_dim} n={n} {name}")
        tab.close()


# ------------------------------------------------------------------------------------------------------------------------ 2: ranges
@pytest.mark.parametrize("in_dim", [12, 7])
def test_a_range_writes_its_own_rows_only(family, in_dim):
    import torch
    files, _, singles = family[in_dim]
    n, ranges = 97, [(0, 33), (33, 1), (34, 63)]
    assign = _assignments(n, 3, seed=3)["random"]
    tab = PolicyTable(files, num_envs=n, device=DEV, assign=assign, ranges=ranges)
    xd = torch.tensor(_inputs(n, in_dim, seed=8), device=DEV)
    whole = tab.get_action(xd).clone()
    assert torch.equal(_bits(whole), _bits(_single_rows(singles, xd, assign)))
    parts = torch.full((n, 4), 7.0, device=DEV)
    for i, (first, count) in enumerate(ranges):
        one = torch.full((n, 4), 7.0, device=DEV)
        tab.get_action_range(i, xd, one)
        inside = torch.zeros(n, dtype=torch.bool, device=DEV)
        inside[first:first + count] = True
        assert torch.equal(_bits(one[inside]), _bits(whole[inside])) and bool((one[~inside] == 7.0).all()), i
        tab.get_action_range(i, xd, parts)
    assert torch.equal(_bits(parts), _bits(whole))
    # the entry point refuses what it cannot launch: a range that is not there, a null pointer
    L = tab._lib
    stream = torch.cuda.current_stream().cuda_stream
    for rng_i in (3, -2):
        assert L.cosim_policy_table_forward(tab._handle, xd.data_ptr(), parts.data_ptr(), rng_i, 1.0, stream) == -1
        assert f"range {rng_i} outside -1..2" in L.cosim_last_error().decode()
    assert L.cosim_policy_table_forward(tab._handle, None, parts.data_ptr(), 0, 1.0, stream) == -1
    assert "null argument" in L.cosim_last_error().decode()
    with pytest.raises(ValueError, match="contiguous fp32"):
        tab.get_action_range(0, xd, torch.zeros((n, 8), device=DEV)[:, ::2])
    with pytest.raises(ValueError, match="expected"):
        tab.get_action_range(0, xd[:50], parts)


# ------------------------------------------------------------------------------------------------------------ 3: non-finite input
def test_non_finite_rows_follow_the_single_kernel_and_touch_no_other_env(family):
    import torch
    files, _, singles = family[12]
    n = 65
    assign = np.arange(n) % 3                      # tiles of 22 / 22 / 21 envs: envs 3 and 7 share their tiles with 20 others each
    tab = PolicyTable(files, num_envs=n, device=DEV, assign=assign)
    x = _inputs(n, 12, seed=21)
    clean = tab.get_action(torch.tensor(x, device=DEV)).clone()
    x[3] = np.nan
    x[7, 5] = np.inf
    xd = torch.tensor(x, device=DEV)
    got = tab.get_action(xd).clone()
    want = _single_rows(singles, xd, assign)
    bad = torch.zeros(n, dtype=torch.bool, device=DEV)
    bad[[3, 7]] = True
    assert torch.equal(_bits(got[~bad]), _bits(clean[~bad]))                              # every other env keeps its bits
    g, w = got[bad], want[bad]
    assert torch.equal(torch.isnan(g), torch.isnan(w)) and torch.equal(_bits(torch.nan_to_num(g, nan=5.0)), _bits(torch.nan_to_num(w, nan=5.0)))
    assert bool(torch.isnan(got[3]).all())                                                # NaN in, NaN out: the clamp keeps it
    assert bool(((got[7].abs() <= 1.0) | torch.isnan(got[7])).all())                      # inf is clipped to +-1 (or became NaN on the way)


# ------------------------------------------------------------------------------------------------------------------------- 4: loops
class _HostLoop:
    """The K single policies evaluated one after the other on the whole fleet and merged by the assignment."""
    graph_safe = False

    def __init__(self, files, policy_of_env, device):
        import torch
        self.torch = torch
        self.pols = [MLPPolicy(f, device=device, fused=True) for f in files]
        self.of = torch.as_tensor(np.asarray(policy_of_env), device=device)

    def get_action(self, state):
        out = None
        for k, p in enumerate(self.pols):
            a = p.get_action(state)
            out = a.clone() if out is None else self.torch.where((self.of == k)[:, None], a, out)
        return out


def _actor_files(d, state_dim, action_dim):
    files = [str(d / f"actor{k}.onnx") for k in range(3)]
    for k, f in enumerate(files):
        write_random_mlp(f, state_dim, action_dim, hidden=(64, 64), seed=20 + k)
    return files


@pytest.fixture(scope="module")
def eager64(tmp_path_factory):
    """Runner.test with the table, 64 envs, 40 control steps: (files, assignment, state, qpos)."""
    import torch
    from cosim_amd.batched_env import BatchedEnv
    from cosim_amd.config import make_config
    from cosim_amd.runner import Runner
    n = 64
    cfg = make_config("flamingo_light_v1", num_envs=n, seed=7)
    env = BatchedEnv(cfg, num_envs=n, seed=7, auto_reset=True)
    files = _actor_files(tmp_path_factory.mktemp("actors"), env.state_dim, env.action_dim)
    assign = np.random.default_rng(9).integers(0, 3, n)
    tab = PolicyTable(files, num_envs=n, device=env.device, assign=assign)
    run = Runner(env, tab)
    run.update_command(0, 0.5)
    assert run.test(max_steps=40) == 40
    torch.cuda.synchronize()
    out = {"cfg": cfg, "files": files, "assign": assign, "state": env.state.clone(), "qpos": env.get_data().qpos.clone()}
    env.close()
    return out


def test_eager_loop_equals_the_host_loop_over_single_policies(eager64):
    import torch
    from cosim_amd.batched_env import BatchedEnv
    from cosim_amd.runner import Runner
    env = BatchedEnv(eager64["cfg"], num_envs=64, seed=7, auto_reset=True)
    run = Runner(env, _HostLoop(eager64["files"], eager64["assign"], env.device))
    run.update_command(0, 0.5)
    assert run.test(max_steps=40) == 40
    torch.cuda.synchronize()
    assert torch.equal(env.state, eager64["state"]) and torch.equal(env.get_data().qpos, eager64["qpos"])
    env.close()


def test_graphed_loop_equals_the_eager_loop(eager64):
    import torch
    from cosim_amd.batched_env import BatchedEnv
    from cosim_amd.runner import Runner
    env = BatchedEnv(eager64["cfg"], num_envs=64, seed=7, auto_reset=True)
    run = Runner(env, PolicyTable(eager64["files"], num_envs=64, device=env.device, assign=eager64["assign"]))
    run.update_command(0, 0.5)
    assert run.test_graphed(40) == 40
    torch.cuda.synchronize()
    assert torch.equal(env.state, eager64["state"]) and torch.equal(env.get_data().qpos, eager64["qpos"])
    env.close()


def test_pipelined_loop_equals_the_eager_loop(tmp_path):
    import torch
    from cosim_amd.batched_env import BatchedEnv
    from cosim_amd.config import make_config
    from cosim_amd.runner import Runner
    n = 256
    cfg = make_config("flamingo_light_v1", num_envs=n, seed=7, max_duration=1.0)       # 50-step episodes: auto-reset inside the run
    assign = np.random.default_rng(10).integers(0, 3, n)
    outs, files = [], None
    for pipelined in (False, True):
        env = BatchedEnv(cfg, num_envs=n, seed=7, auto_reset=True, **({"ranges": 4, "deferred_join": True} if pipelined else {}))
        files = files or _actor_files(tmp_path, env.state_dim, env.action_dim)
        tab = PolicyTable(files, num_envs=n, device=env.device, assign=assign, ranges=env.range_list)
        run = Runner(env, tab)
        run.update_command(0, 0.5)
        assert (run.test_pipelined(70) if pipelined else run.test(max_steps=70)) == 70
        torch.cuda.synchronize()
        outs.append((env.state.clone(), env.get_data().qpos.clone(), env.solver_stats()["episodes_ended"]))
        if pipelined:                                                                  # a table built for other ranges is refused
            with pytest.raises(ValueError, match="ranges"):
                Runner(env, PolicyTable(files, num_envs=n, device=env.device, assign=assign)).test_pipelined(1)
        env.close()
    assert outs[0][2] == outs[1][2] >= n                                               # the time limit fired inside the run
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


# ------------------------------------------------------------------------------------------------ 5: the assignment reaches the engine
def test_cross_assignment_reaches_the_engine(tmp_path):
    import torch
    from cosim_amd.batched_env import BatchedEnv
    from cosim_amd.config import make_config
    from cosim_amd.runner import Runner
    n = 32
    cfg = make_config("flamingo_light_v1", num_envs=n, seed=3, max_duration=0.4)       # 20-step episodes
    from cosim_amd.reporter import FleetReporter
    checks = [[0, 10, "up", 0, "always", ">", -2.0, "upright"]]
    env = BatchedEnv(cfg, num_envs=n, seed=3, auto_reset=True, env_id0=1000, ledger=8, scenarios=[{"checks": checks}, {"checks": checks}],
                     scenario_mode="env", check_slots=8, failure_traces={"frames": 6, "keep": 2, "on": ("truncated",)})
    files, const = [], (0.25, -0.25)
    for k, c in enumerate(const):                                                      # zero weights, a constant bias: a constant action
        files.append(str(tmp_path / f"const{k}.onnx"))
        write_onnx(files[-1], [{"op": "Gemm", "inputs": ["obs", "w", "b"], "outputs": ["actions"], "attrs": {"transB": 1}}],
                   {"w": np.zeros((env.action_dim, env.state_dim), np.float32), "b": np.full(env.action_dim, c, np.float32)}, ["obs"], ["actions"])
    tab = PolicyTable(files, num_envs=n, device=env.device, assign="cross", env_id0=env.env_id0, scenarios=2, names=["plus", "minus"])
    g = np.arange(1000, 1000 + n)
    assert (tab.policy_of_env == (g // 2) % 2).all()
    rep = FleetReporter(env)
    assert Runner(env, tab, reporter=rep).test(max_steps=65) == 65
    torch.cuda.synchronize()
    # the report: per policy the ledger's columns with the scenario matrix nested, and the verdicts' summary
    out = json.loads(json.dumps(rep.summary()))
    by, cby = out["episodes"]["by_policy"], out["episodes"]["checks"]["by_policy"]
    assert set(by) == set(cby) == {"plus", "minus"} and set(by["plus"]["by_scenario"]) == {"0", "1"}
    assert by["plus"]["episodes"] + by["minus"]["episodes"] == out["episodes"]["episodes"]
    assert by["plus"]["by_scenario"]["0"]["episodes"] + by["plus"]["by_scenario"]["1"]["episodes"] == by["plus"]["episodes"]
    assert cby["plus"]["episodes"] + cby["minus"]["episodes"] == out["episodes"]["checks"]["episodes"] == out["episodes"]["episodes"]
    assert cby["plus"]["episodes_passed"] == cby["plus"]["episodes"] and "upright" in cby["minus"]["checks"]
    tr = env.failure_traces()
    assert len(tr) >= n and tr.valid.any()
    want = np.asarray(const, np.float32)[tab.policy_of(tr.env)]                         # per trace
    act = tr.action                                                                    # [M, T, nu], NaN beyond the valid frames
    assert (act[tr.valid] == np.broadcast_to(want[:, None, None], act.shape)[tr.valid]).all()
    cells = env.ledger().by_policy(tab, scenario=True)
    assert set(cells) == {("plus", 0), ("plus", 1), ("minus", 0), ("minus", 1)}
    counts = {k: v["episodes"] for k, v in cells.items()}
    assert len(set(counts.values())) == 1 and sum(counts.values()) == env.ledger().counts()["episodes"] >= 3 * n, counts
    env.close()


# --------------------------------------------------------------------------------------------------------------------------- 6: CLI
@pytest.fixture(scope="module")
def cli_files(tmp_path_factory):
    from cosim_amd.batched_env import BatchedEnv
    from cosim_amd.config import make_config
    env = BatchedEnv(make_config("flamingo_light_v1", num_envs=4, seed=5), num_envs=4, seed=5, auto_reset=True)
    d = tmp_path_factory.mktemp("cli")
    files = [str(d / "a.onnx"), str(d / "b.onnx")]
    for k, f in enumerate(files):
        write_random_mlp(f, env.state_dim, env.action_dim, hidden=(64, 64), seed=30 + k)
    env.close()
    return files


@pytest.mark.parametrize("mode", ["", "--graph", "--pipelined"])
def test_cli_with_two_policies(tmp_path, capsys, cli_files, mode):
    from cosim_amd import cli
    rep = tmp_path / "report.json"
    argv = ["--env", "flamingo_light_v1", "--num-envs", "32", "--steps", "60", "--max-duration", "0.5", "--seed", "5", "--policy", *cli_files,
            "--policy-assign", "interleave", "--ledger", "4", "--report", str(rep)] + ([mode] if mode else [])
    assert cli.main(argv) == 0
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    out = json.loads(rep.read_text())
    by = out["episodes"]["by_policy"]
    assert set(by) == {"a", "b"} == set(line["by_policy"])
    assert by["a"]["episodes"] + by["b"]["episodes"] == out["episodes"]["episodes"] >= 64
    assert by["a"]["episodes"] >= 32 and by["b"]["episodes"] >= 32                      # 16 envs each, at least two time limits
    assert line["by_policy"]["a"]["episodes"] == by["a"]["episodes"] and "terminated_share" in line["by_policy"]["a"]
