"""The policy table without a GPU.  The host code of cosim_policy_table_create (csrc/cosim_poltab.h) through tests/poltab_host.cpp,
built plain and with AddressSanitizer / UBSan as a stand-alone child process: the tile list's guarantees, every refusal of the
validator word for word, and the weight image.  Then ``PolicyTable`` on the CPU (layouts against their formulas, actions against
``MLPPolicy`` per policy, the refusals that name a file) and ``by_policy`` of the ledger and the verdicts on hand-built records."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
i32 = np.int32
ML = 6


@pytest.fixture(scope="module", params=["plain", "asan-ubsan"])
def exe(request, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("poltab") / ("poltab_host_" + request.param.replace("-", "_")))
    extra = [] if request.param == "plain" else ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
    subprocess.check_call([os.environ.get("CXX", "c++"), "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unknown-pragmas", *extra, "-I",
                           os.path.join(ROOT, "cosim_amd", "csrc"), "-o", out, os.path.join(ROOT, "tests", "poltab_host.cpp")])
    return out


def _ints(a):
    if a is None:
        return ["-1"]
    a = np.asarray(a, dtype=np.int64).ravel()
    return [str(a.size)] + [str(int(x)) for x in a]


def table(policies, assign, ranges=None):
    """policies: per policy (dims, acts, has_bias per layer).  The arrays cosim_policy_table_create takes, as a dict."""
    K, n = len(policies), len(assign)
    nl = np.array([len(p[0]) - 1 for p in policies], i32)
    dims, act, hb = np.zeros((K, ML + 1), i32), np.zeros((K, ML), i32), np.zeros((K, ML), i32)
    for k, (d, a, b) in enumerate(policies):
        dims[k, :len(d)] = d
        act[k, :len(a)] = a
        hb[k, :len(b)] = b
    return {"K": K, "nl": nl, "dims": dims, "act": act, "has_bias": hb, "n": n, "por": np.asarray(assign, i32),
            "ranges": np.asarray([(0, n)] if ranges is None else ranges, i32).reshape(-1, 2)}


def run(exe, t, **over):
    t = {**t, **over}
    n_ranges = t.get("n_ranges", None if t["ranges"] is None else len(t["ranges"]))
    tok = [str(t["K"])] + _ints(t["nl"]) + _ints(t["dims"]) + _ints(t["act"]) + _ints(t["has_bias"]) + [str(t["n"])] + _ints(t["por"]) + \
        [str(n_ranges)] + _ints(t["ranges"])
    p = subprocess.run([exe], input=" ".join(tok), capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = p.stdout.splitlines()
    if lines[0].startswith("ERR "):
        return "ERR", lines[0][4:]
    assert lines[0] == "OK"
    out = {"tiles": [], "spans": [], "desc": []}
    for ln in lines[1:]:
        f = ln.split()
        v = [int(x) for x in f[1:]]
        if f[0] in ("rows", "image"):
            assert v[0] == len(v) - 1
            out[f[0]] = np.array(v[1:], dtype=np.int64)
        elif f[0] == "maxd":
            out["maxd"] = v[0]
        elif f[0] == "tile":
            out["tiles"].append(tuple(v))
        elif f[0] == "span":
            out["spans"].append(tuple(v))
        else:
            out["desc"].append({"nl": v[0], "dims": v[1:8], "act": v[8:14], "woff": v[14:20], "boff": v[20:26]})
    return "OK", out


SMALL = ((5, 3), (0,), (1,))


# ------------------------------------------------------------------------------------------------------------------ 1: the tile list
def _assignments(n, K, rng):
    out = {"interleave": np.arange(n) % K, "random": rng.integers(0, K, n)}
    if K >= 2:
        out["one_policy_empty"] = rng.integers(0, K - 1, n)                     # policy K - 1 drives no env
        assert not (out["one_policy_empty"] == K - 1).any()
    if K >= 2 and n >= 65:                                                      # 32 envs of policy 0 and 33 of policy 1, the rest of the last
        a = np.full(n, K - 1)
        a[:65] = rng.permutation(np.array([0] * 32 + [1] * 33))
        out["32_and_33"] = a
        assert (a[:65] == 0).sum() == 32 and (a[:65] == 1).sum() == 33
    return out


def _range_sets(n):
    """One range; three uneven ones (the middle one a single row), the 65 rows that hold the 32 / 33 policies first and whole."""
    sets = [[(0, n)]]
    if n >= 3:
        a = 33 if n == 97 else n // 2
        sets.append([(0, a), (a, 1), (a + 1, n - a - 1)])                       # n = 97: (0, 33), (33, 1), (34, 63)
    if n == 97:
        sets.append([(0, 65), (65, 1), (66, 31)])
    return sets


def _check_tiles(got, assign, K, ranges, n):
    rows, tiles, spans = got["rows"], got["tiles"], got["spans"]
    assert sorted(rows.tolist()) == list(range(n))                              # every row is there exactly once ...
    nxt = 0
    for pol, start, count in tiles:                                             # ... and the tiles cut rows[] into pieces end to end
        assert start == nxt and 1 <= count <= 32 and 0 <= pol < K
        nxt = start + count
        assert (assign[rows[start:start + count]] == pol).all()                 # one policy per tile
    assert nxt == n
    assert len(spans) == len(ranges)
    tnext = 0
    for (first, count), (tf, tc) in zip(ranges, spans):                         # a range's tiles are contiguous and hold its rows only
        assert tf == tnext and tc >= 1
        tnext = tf + tc
        held = np.concatenate([rows[s:s + c] for _, s, c in tiles[tf:tf + tc]])
        assert sorted(held.tolist()) == list(range(first, first + count))
        for k in range(K):                                                      # no more tiles than the policy's rows of the range need
            nk = int((assign[first:first + count] == k).sum())
            assert sum(1 for p, _, _ in tiles[tf:tf + tc] if p == k) == (nk + 31) // 32
    assert tnext == len(tiles)


def test_tile_list_guarantees(exe):
    rng = np.random.default_rng(11)
    cases = 0
    for n in (1, 31, 32, 33, 65, 97):
        for K in (1, 3, 5):
            for name, assign in _assignments(n, K, rng).items():
                for ranges in _range_sets(n):
                    status, got = run(exe, table([SMALL] * K, assign, ranges))
                    assert status == "OK", (n, K, name, ranges, got)
                    _check_tiles(got, np.asarray(assign), K, ranges, n)
                    cases += 1
    assert cases > 100
    # the 32 / 33 case by hand: one range of 65 -> one full tile of policy 0, a full one and a single row of policy 1
    a = np.array([0] * 32 + [1] * 33)
    got = run(exe, table([SMALL] * 3, a))[1]
    assert got["tiles"] == [(0, 0, 32), (1, 32, 32), (1, 64, 1)] and got["spans"] == [(0, 3)]
    # and cut by ranges (0, 33), (33, 1), (34, 31): no tile crosses a range
    got = run(exe, table([SMALL] * 3, a, [(0, 33), (33, 1), (34, 31)]))[1]
    assert got["tiles"] == [(0, 0, 32), (1, 32, 1), (1, 33, 1), (1, 34, 31)] and got["spans"] == [(0, 2), (2, 1), (3, 1)]


# ------------------------------------------------------------------------------------------------------------------ 2: the refusals
def test_every_refusal_of_the_validator(exe):
    fn = "cosim_policy_table_create"
    good = table([((12, 40, 4), (5, 0), (1, 1)), ((12, 33, 4), (4, 0), (0, 1))], [0, 1, 1, 0, 1])
    assert run(exe, good)[0] == "OK"

    def refused(want, **over):
        assert run(exe, good, **over) == ("ERR", fn + ": " + want)
    for K in (0, 65, -1):
        refused("%d policies, outside 1..64" % K, K=K)
    for n in (0, -4):
        refused("n %d is not positive" % n, n=n)
    for nl in (0, 7):
        refused("policy 1: %d layers, outside 1..6" % nl, nl=np.array([2, nl], i32))
    for width, layer in ((0, 1), (513, 1), (-2, 0), (513, 2)):
        d = good["dims"].copy()
        d[0, layer] = width
        refused("policy 0: width %d of layer %d outside 1..512" % (width, layer), dims=d)
    d = good["dims"].copy()
    d[1, 0] = 16
    refused("policy 1: input width 16 differs from policy 0's 12", dims=d)
    d = good["dims"].copy()
    d[1, 2] = 3
    refused("policy 1: output width 3 differs from policy 0's 4", dims=d)
    for code in (6, -1):
        a = good["act"].copy()
        a[1, 0] = code
        refused("policy 1, layer 0: unknown activation %d (0 none .. 5 leaky relu)" % code, act=a)
    for row, k in ((3, 2), (0, -1)):
        por = good["por"].copy()
        por[row] = k
        refused("row %d is assigned to policy %d, outside [0, 2)" % (row, k), por=por)
    refused("range 1 (2, 3) overlaps the one before it", ranges=np.array([(0, 3), (2, 3)], i32))
    refused("range 1 (4, 1) leaves rows from 3 uncovered", ranges=np.array([(0, 3), (4, 1)], i32))
    refused("the ranges leave rows from 4 uncovered", ranges=np.array([(0, 3), (3, 1)], i32))
    refused("range 0 (1, 4) leaves rows from 0 uncovered", ranges=np.array([(1, 4)], i32))
    refused("range 1 (3, 3) ends past n 5", ranges=np.array([(0, 3), (3, 3)], i32))
    refused("range 1 (3, 0) is empty", ranges=np.array([(0, 3), (3, 0), (3, 2)], i32))
    refused("0 ranges, outside 1..n", ranges=np.zeros((0, 2), i32))
    refused("null argument", por=None)
    refused("null argument", ranges=None, n_ranges=1)
    # the order: the policy count and n ahead of the arrays, a policy's layers ahead of its widths, policies ahead of rows and ranges
    refused("0 policies, outside 1..64", K=0, n=0, nl=None)
    refused("n 0 is not positive", n=0, nl=None)
    d = good["dims"].copy()
    d[1, 0] = 16
    refused("policy 1: input width 16 differs from policy 0's 12", dims=d, por=np.array([0, 1, 9, 0, 1], i32), ranges=np.array([(1, 4)], i32))


# ------------------------------------------------------------------------------------------------------------------- 3: the image
def test_image_offsets_alignment_and_biases(exe):
    pols = [((12, 40, 36, 4), (5, 3, 0), (1, 1, 1)),            # all widths multiples of 4
            ((12, 33, 4), (4, 0), (0, 1)),                      # no first bias; 12 * 33 and 33 words push the next array off the grid
            ((12, 4), (0,), (0,)),
            ((12, 7, 5, 3, 9, 1, 4), (1, 2, 3, 4, 5, 0), (1, 0, 1, 0, 1, 1))]
    status, got = run(exe, table(pols, [0, 1, 2, 3, 3]))
    assert status == "OK" and got["maxd"] == 40
    img, spans = got["image"], []
    for k, ((dims, acts, hb), d) in enumerate(zip(pols, got["desc"])):
        nl = len(dims) - 1
        assert d["nl"] == nl and d["dims"][:nl + 1] == list(dims) and d["act"][:nl] == list(acts)
        assert d["woff"][nl:] == [-1] * (ML - nl) and d["boff"][nl:] == [-1] * (ML - nl)
        for l in range(nl):
            nw, nb = dims[l] * dims[l + 1], dims[l + 1]
            assert d["woff"][l] >= 0 and d["woff"][l] % 4 == 0, (k, l)                   # the float4 path stays 16-byte aligned
            assert (img[d["woff"][l]:d["woff"][l] + nw] == 64 * k + 8 * l + 1).all()
            spans.append((d["woff"][l], nw))
            assert (d["boff"][l] == -1) == (not hb[l]), (k, l)                           # -1 exactly where there is no bias
            if hb[l]:
                assert (img[d["boff"][l]:d["boff"][l] + nb] == 64 * k + 8 * l + 2).all()
                spans.append((d["boff"][l], nb))
    spans.sort()
    for (o0, n0), (o1, _) in zip(spans, spans[1:]):
        assert o0 + n0 <= o1 < o0 + n0 + 4                                               # no overlap, at most 3 words of padding
    assert spans[-1][0] + spans[-1][1] == len(img)
    used = np.zeros(len(img), bool)
    for o, n in spans:
        used[o:o + n] = True
    assert (img[~used] == 0).all() and (~used).sum() > 0                                # the padding is there and is zero


# --------------------------------------------------------------------------------------------------------- 4: PolicyTable on the CPU
def _write_chain(path, dims, acts, seed, nobias=()):
    from cosim_amd.policy import write_onnx
    rng = np.random.default_rng(seed)
    nodes, init, x = [], {}, "obs"
    for li in range(len(dims) - 1):
        init[f"w{li}"] = (rng.standard_normal((dims[li + 1], dims[li])) / np.sqrt(dims[li])).astype(np.float32)
        ins = [x, f"w{li}"]
        if li not in nobias:
            init[f"b{li}"] = (0.5 * rng.standard_normal(dims[li + 1])).astype(np.float32)
            ins.append(f"b{li}")
        last = li == len(dims) - 2
        lin = "actions" if last and acts[li] is None else f"lin{li}"
        nodes.append({"op": "Gemm", "inputs": ins, "outputs": [lin], "attrs": {"transB": 1}})
        x = lin
        if acts[li] is not None:
            x = "actions" if last else f"h{li}"
            nodes.append({"op": acts[li], "inputs": [lin], "outputs": [x]})
    write_onnx(path, nodes, init, ["obs"], ["actions"])
    return path


@pytest.fixture()
def files(tmp_path):
    return [_write_chain(str(tmp_path / "a.onnx"), (12, 40, 36, 4), ["LeakyRelu", "Elu", None], 1),
            _write_chain(str(tmp_path / "b.onnx"), (12, 33, 4), ["Sigmoid", None], 2, nobias=(0,)),
            _write_chain(str(tmp_path / "c.onnx"), (12, 4), [None], 3)]


def test_layouts_follow_their_formulas(files):
    from cosim_amd.policy import PolicyTable, build_policy
    N, g0, S = 37, 1000, 4
    g = np.arange(g0, g0 + N)
    tab = PolicyTable(files, num_envs=N, device="cpu", assign="interleave", env_id0=g0)
    assert tab.policy_of_env.dtype == np.int32 and (tab.policy_of_env == g % 3).all() and tab.names == ["a", "b", "c"]
    assert (tab.policy_of([1000, 1001, 5000]) == [1000 % 3, 1001 % 3, 5000 % 3]).all() and tab.graph_safe
    tab = PolicyTable(files, num_envs=N, device="cpu", assign="cross", env_id0=g0, scenarios=S, names=["x", "y", "z"])
    assert (tab.policy_of_env == (g // S) % 3).all() and tab.names == ["x", "y", "z"]
    # under scenario mode env (scenario = g mod S) every (scenario, policy) pair of 3 * S consecutive envs is met exactly once
    gg = np.arange(g0 - g0 % (3 * S) + 3 * S, g0 - g0 % (3 * S) + 6 * S)
    assert len({(int(x % S), int(p)) for x, p in zip(gg, tab.policy_of(gg))}) == 3 * S
    a = np.random.default_rng(0).integers(0, 3, N)
    tab = PolicyTable(files, num_envs=N, device="cpu", assign=a, env_id0=g0)
    assert (tab.policy_of_env == a).all() and (tab.policy_of(g[5:9]) == a[5:9]).all()
    with pytest.raises(ValueError, match="cross.*scenarios"):
        PolicyTable(files, num_envs=N, device="cpu", assign="cross")
    with pytest.raises(ValueError, match="one integer per local env"):
        PolicyTable(files, num_envs=N, device="cpu", assign=a[:-1])
    with pytest.raises(ValueError, match=r"outside \[0, 3\)"):
        PolicyTable(files, num_envs=N, device="cpu", assign=np.where(a == 2, 3, a))
    with pytest.raises(ValueError, match="do not tile"):
        PolicyTable(files, num_envs=N, device="cpu", ranges=[(0, 10), (11, 26)])
    # build_policy: a list of files makes a table, one file what it made before
    tab = build_policy({"policy": {"use_lstm": False, "onnx_files": files[:2], "assign": "cross"}}, num_envs=N, device="cpu", env_id0=g0, scenarios=S)
    assert isinstance(tab, PolicyTable) and (tab.policy_of_env == (g // S) % 2).all()
    assert type(build_policy({"policy": {"use_lstm": False}}, files[0], num_envs=N, device="cpu")).__name__ == "MLPPolicy"


def test_cpu_actions_equal_each_policy_on_its_rows(files):
    import torch
    from cosim_amd.policy import MLPPolicy, PolicyTable
    N = 41
    ranges = [(0, 17), (17, 1), (18, 23)]
    a = np.random.default_rng(4).integers(0, 3, N)
    tab = PolicyTable(files, num_envs=N, device="cpu", assign=a, ranges=ranges)
    x = torch.tensor(np.random.default_rng(5).standard_normal((N, 12)).astype(np.float32) * 2.0)
    got = tab.get_action(x)
    assert got.shape == (N, 4) and got.data_ptr() == tab.get_action(x).data_ptr()          # the persistent output tensor
    singles = [MLPPolicy(f, device="cpu") for f in files]
    for k, pol in enumerate(singles):
        idx = torch.as_tensor(np.nonzero(a == k)[0])
        assert len(idx) and torch.equal(got[idx], pol.get_action(x[idx]))
    assert float(got.abs().max()) <= 1.0 and float((got.abs() < 1.0).float().mean()) > 0.5
    whole = got.clone()
    parts = torch.full((N, 4), 7.0)
    for i, (first, count) in enumerate(ranges):
        one = torch.full((N, 4), 7.0)
        tab.get_action_range(i, x, one)
        inside = torch.zeros(N, dtype=torch.bool)
        inside[first:first + count] = True
        # the library GEMM of the CPU twin picks its kernel by batch size, so a range's rows match the whole fleet's to rounding only
        # (the grouped kernel's rows are bit-equal: tests/test_gpu_policy_table.py); which rows are written is exact
        assert torch.allclose(one[inside], whole[inside], rtol=0, atol=1e-6) and bool((one[~inside] == 7.0).all())
        tab.get_action_range(i, x, parts)
    assert torch.allclose(parts, whole, rtol=0, atol=1e-6) and not bool((parts == 7.0).any())
    with pytest.raises(ValueError, match="range 3 outside 0..2"):
        tab.get_action_range(3, x, parts)


def test_refusals_name_the_file(files, tmp_path):
    from cosim_amd.policy import PolicyTable, write_onnx
    wide = _write_chain(str(tmp_path / "wide_in.onnx"), (16, 8, 4), ["Tanh", None], 7)
    with pytest.raises(ValueError, match=r"wide_in\.onnx: input width 16 differs from 12 of .*a\.onnx"):
        PolicyTable(files + [wide], num_envs=8, device="cpu")
    out5 = _write_chain(str(tmp_path / "five_out.onnx"), (12, 8, 5), ["Tanh", None], 8)
    with pytest.raises(ValueError, match=r"five_out\.onnx: output width 5 differs from 4 of .*a\.onnx"):
        PolicyTable(files + [out5], num_envs=8, device="cpu")
    soft = _write_chain(str(tmp_path / "softplus.onnx"), (12, 8, 4), ["Softplus", None], 9)
    with pytest.raises(ValueError, match=r"softplus\.onnx: the graph is not a plain Gemm / activation chain"):
        PolicyTable(files + [soft], num_envs=8, device="cpu")
    rng = np.random.default_rng(1)
    I, H, A = 12, 6, 4
    nodes = [{"op": "Unsqueeze", "inputs": ["obs"], "outputs": ["x3"], "attrs": {"axes": [0]}},
             {"op": "LSTM", "inputs": ["x3", "W", "R", "B", "", "h_in", "c_in"], "outputs": ["Y", "h_out", "c_out"], "attrs": {"hidden_size": H}},
             {"op": "Squeeze", "inputs": ["h_out"], "outputs": ["hs"], "attrs": {"axes": [0]}},
             {"op": "Gemm", "inputs": ["hs", "Wo", "bo"], "outputs": ["actions"], "attrs": {"transB": 1}}]
    init = {"W": rng.standard_normal((1, 4 * H, I)).astype(np.float32), "R": rng.standard_normal((1, 4 * H, H)).astype(np.float32),
            "B": np.zeros((1, 8 * H), np.float32), "Wo": rng.standard_normal((A, H)).astype(np.float32), "bo": np.zeros(A, np.float32)}
    lstm = str(tmp_path / "recurrent.onnx")
    write_onnx(lstm, nodes, init, ["obs", "h_in", "c_in"], ["actions", "h_out", "c_out"])
    with pytest.raises(ValueError, match=r"recurrent\.onnx: an LSTM policy"):
        PolicyTable([files[0], lstm], num_envs=8, device="cpu")
    with pytest.raises(ValueError, match="MLP actors only"):
        from cosim_amd.policy import build_policy
        build_policy({"policy": {"use_lstm": True, "onnx_files": files}}, num_envs=8, device="cpu")


def test_cli_refuses_what_a_table_cannot_take(capsys):
    """ap.error, before any device is touched: sinusoid / random-mlp among several values, --lstm, names that do not match."""
    from cosim_amd import cli
    for argv, want in ((["--policy", "a.onnx", "sinusoid"], "ONNX files only"), (["--policy", "a.onnx", "random-mlp"], "ONNX files only"),
                       (["--policy", "a.onnx", "b.onnx", "--lstm"], "MLP actors only"),
                       (["--policy", "a.onnx", "b.onnx", "--policy-names", "x"], "one name per --policy file"),
                       (["--policy", "a.onnx", "--policy-assign", "cross"], "need several --policy files")):
        with pytest.raises(SystemExit) as e:
            cli.main(argv)
        assert e.value.code == 2 and want in capsys.readouterr().err, argv


# ---------------------------------------------------------------------------------------------------------------------- 5: by_policy
class _Tab:
    """What by_policy needs of a table: names and the policy of a global env id (here: interleaved over two)."""
    names = ["old", "new"]

    @staticmethod
    def policy_of(g):
        return (np.asarray(g) % 2).astype(np.int32)


def test_ledger_by_policy_counts():
    from cosim_amd.ledger import FELL_TILT, OPEN, TERMINATED, TRUNCATED, WORDS, EpisodeLedger
    g0 = 100
    #        env  episode length flags                    scenario
    recs = [(100, 0, 10, TERMINATED, 0), (100, 1, 50, TRUNCATED, 0), (100, 2, 3, OPEN, 0),
            (101, 0, 20, TERMINATED | FELL_TILT, 1), (101, 1, 30, TERMINATED, 1),
            (102, 0, 50, TRUNCATED, 0),
            (103, 0, 50, TRUNCATED, 1), (103, 1, 40, TERMINATED, 1), (103, 2, 50, TRUNCATED, 1),
            (104, 0, 7, OPEN, 0)]
    w = np.zeros((len(recs), WORDS), np.int32)
    for r, (_, ep, ln, fl, sc) in enumerate(recs):
        w[r, 0], w[r, 1], w[r, 2], w[r, 13] = ep, ln, fl, sc + 1
        w[r, 5:13] = np.full(8, float(ln), np.float32).view(np.int32)
    led = EpisodeLedger(w, [r[0] for r in recs], np.zeros(5, np.int64), slots=4, env_id0=g0)
    by = led.by_policy(_Tab)
    # policy "old" drives envs 100, 102, 104 (all scenario 0), "new" 101 and 103 (scenario 1)
    assert set(by) == {"old", "new"}
    assert (by["old"]["episodes"], by["old"]["terminated"]) == (3, 1) and (by["new"]["episodes"], by["new"]["terminated"]) == (5, 3)
    assert by["old"]["terminated_share"] == 1 / 3 and by["new"]["fell"] == 1 and by["old"]["fell"] == 0
    assert by["old"]["length"] == {"mean": 110 / 3, "min": 10, "p50": 50.0, "max": 50} and by["new"]["length"]["mean"] == 190 / 5
    assert by["new"]["means"]["mean_abs_torque"] == 190 / 5
    assert set(by["old"]) == set(led.by_scenario()[0])                                     # the columns of by_scenario()
    assert sum(v["episodes"] for v in by.values()) == led.counts()["episodes"] == 8
    assert sum(v["terminated"] for v in by.values()) == led.counts()["terminated"] and sum(v["fell"] for v in by.values()) == led.counts()["fell"]
    cells = led.by_policy(_Tab, scenario=True)
    assert set(cells) == {("old", 0), ("new", 1)} and cells[("old", 0)] == by["old"] and cells[("new", 1)] == by["new"]
    # an int array, one entry per local env: both policies meet both scenarios
    arr = np.array([0, 0, 1, 1, 0])
    cells = led.by_policy(arr, scenario=True, fell=False)
    assert {k: v["episodes"] for k, v in cells.items()} == {("0", 0): 2, ("0", 1): 2, ("1", 0): 1, ("1", 1): 3}
    assert "fell" not in cells[("0", 0)] and sum(v["episodes"] for v in cells.values()) == led.counts()["episodes"]
    assert cells[("1", 1)]["terminated"] == 1 and cells[("0", 1)]["terminated"] == 2
    with pytest.raises(ValueError, match="local envs"):
        led.by_policy(arr[:3])


def test_verdicts_by_policy_counts():
    from cosim_amd.checks import HDR, Verdicts
    g0, I = 100, 2
    item_mode = np.array([[0, -1], [0, 2]], np.int32)                                      # scenario 0: one item, scenario 1: two
    item_t = np.zeros((2, I, 2), np.int32)
    item_t[:, :, 1] = 10
    #        env  episode flags scenario failed-bits incomplete-bits
    recs = [(100, 0, 1, 0, 0b0, 0b0), (100, 1, 2, 0, 0b1, 0b0), (101, 0, 2, 1, 0b10, 0b0), (101, 1, 2, 1, 0b0, 0b1),
            (102, 0, 2, 0, 0b0, 0b1), (103, 0, 1, 1, 0b0, 0b0), (103, 1, 16, 1, 0b1, 0b0)]
    w = np.zeros((len(recs), HDR + 2 * I), np.int32)
    for r, (_, ep, fl, sc, fb, ib) in enumerate(recs):
        w[r, 0], w[r, 1], w[r, 2], w[r, 3], w[r, 4], w[r, 6] = ep, 10, fl, sc + 1, fb, ib
    v = Verdicts(w, [r[0] for r in recs], np.zeros(4, np.int64), [["upright"], ["upright", "speed"]], item_mode, item_t, slots=4, env_id0=g0)
    by = v.by_policy(_Tab)
    old, new = by["old"], by["new"]
    assert (old["episodes"], old["episodes_passed"], old["episodes_failed"], old["episodes_incomplete"], old["items"]) == (3, 1, 1, 1, 3)
    assert (new["episodes"], new["episodes_passed"], new["episodes_failed"], new["episodes_incomplete"], new["items"]) == (3, 1, 1, 1, 6)
    assert new["items_failed"] == 1 and new["items_incomplete"] == 1 and new["items_passed"] == 4 and new["episodes_failed_share"] == 1 / 3
    assert new["checks"]["speed"]["failed"] == 1 and new["checks"]["upright"]["incomplete"] == 1 and set(old["checks"]) == {"upright"}
    total = v.counts()
    for key in ("episodes", "episodes_passed", "episodes_failed", "episodes_incomplete", "items", "items_passed", "items_failed", "items_incomplete"):
        assert old[key] + new[key] == total[key], key
    assert set(old) == set(v.by_scenario()[0])                                             # summary() per policy
    cells = v.by_policy(np.array([0, 1, 1, 0]), scenario=True)
    assert {k: c["episodes"] for k, c in cells.items()} == {("0", 0): 2, ("0", 1): 1, ("1", 1): 2, ("1", 0): 1}
    assert cells[("1", 1)]["episodes_failed"] == 1 and cells[("1", 0)]["episodes_incomplete"] == 1
    assert sum(c["episodes"] for c in cells.values()) == total["episodes"]
