"""The recurrent policy table without a GPU.  The host code of cosim_recurrent_table_create (csrc/cosim_rectab.h) through
tests/rectab_host.cpp, built plain and with AddressSanitizer / UBSan as a stand-alone child process: every refusal of the validator word
for word, the reused tile builder, the weight image and the LDS byte rule.  Then the graph recogniser, ``RecurrentPolicyTable`` on the
CPU against ``LSTMPolicy`` per policy, the factory, ``build_policy`` and the CLI's argument parsing."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
i32 = np.int32
ME, MH = 3, 3


@pytest.fixture(scope="module", params=["plain", "asan-ubsan"])
def exe(request, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("rectab") / ("rectab_host_" + request.param.replace("-", "_")))
    extra = [] if request.param == "plain" else ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
    subprocess.check_call([os.environ.get("CXX", "c++"), "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unknown-pragmas", *extra, "-I",
                           os.path.join(ROOT, "cosim_amd", "csrc"), "-o", out, os.path.join(ROOT, "tests", "rectab_host.cpp")])
    return out


def _ints(a):
    if a is None:
        return ["-1"]
    a = np.asarray(a, dtype=np.int64).ravel()
    return [str(a.size)] + [str(int(x)) for x in a]


def table(policies, assign, ranges=None, lds_limit=0):
    """policies: per policy a dict enc=(dims, acts, has_bias), I, H, B, head=(dims, acts, has_bias).  The arrays
    cosim_recurrent_table_create takes, as a dict."""
    K, n = len(policies), len(assign)
    t = {"K": K, "ne": np.zeros(K, i32), "edims": np.zeros((K, ME + 1), i32), "eact": np.zeros((K, ME), i32), "ehb": np.zeros((K, ME), i32),
         "lstm_in": np.zeros(K, i32), "hidden": np.zeros(K, i32), "has_B": np.zeros(K, i32),
         "nh": np.zeros(K, i32), "hdims": np.zeros((K, MH + 1), i32), "hact": np.zeros((K, MH), i32), "hhb": np.zeros((K, MH), i32),
         "n": n, "por": np.asarray(assign, i32), "ranges": np.asarray([(0, n)] if ranges is None else ranges, i32).reshape(-1, 2), "lds_limit": lds_limit}
    for k, p in enumerate(policies):
        for key, (d, a, b) in (("e", p["enc"]), ("h", p["head"])):
            t["ne" if key == "e" else "nh"][k] = len(d) - 1
            t[key + "dims"][k, :len(d)] = d
            t[key + "act"][k, :len(a)] = a
            t[key + "hb"][k, :len(b)] = b
        t["lstm_in"][k], t["hidden"][k], t["has_B"][k] = p["I"], p["H"], p["B"]
    return t


def run(exe, t, **over):
    t = {**t, **over}
    n_ranges = t.get("n_ranges", None if t["ranges"] is None else len(t["ranges"]))
    tok = [str(t["K"])]
    for key in ("ne", "edims", "eact", "ehb", "lstm_in", "hidden", "has_B", "nh", "hdims", "hact", "hhb"):
        tok += _ints(t[key])
    tok += [str(t["n"])] + _ints(t["por"]) + [str(n_ranges)] + _ints(t["ranges"]) + [str(t["lds_limit"])]
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
        elif f[0] == "shape":
            out["ld_m"], out["ld_x"], out["hmax"], out["lds"] = v
        elif f[0] == "tile":
            out["tiles"].append(tuple(v))
        elif f[0] == "span":
            out["spans"].append(tuple(v))
        else:
            assert len(v) == 40                                                            # RecDesc is 40 words
            out["desc"].append({"ne": v[0], "edims": v[1:5], "eact": v[5:8], "ewoff": v[11:14], "eboff": v[14:17], "I": v[17], "H": v[18],
                                "woff": v[19], "roff": v[20], "boff": v[21], "nh": v[22], "hdims": v[23:27], "hact": v[27:30], "hwoff": v[33:36],
                                "hboff": v[36:39], "vec": v[39]})
    return "OK", out


def pol(obs=12, enc=(), eact=(), ehb=(), H=8, B=1, head=(4,), hact=(0,), hhb=(1,)):
    ed = (obs, *enc)
    return {"enc": (ed, eact, ehb), "I": ed[-1], "H": H, "B": B, "head": ((H, *head), hact, hhb)}


GOOD = [pol(enc=(40,), eact=(3,), ehb=(1,), H=8), pol(H=6, B=0, head=(10, 4), hact=(2, 0), hhb=(1, 0))]


# ------------------------------------------------------------------------------------------------------------------ 1: the tile list
def test_every_row_is_in_exactly_one_tile(exe):
    rng = np.random.default_rng(5)
    for n, K, ranges in ((1, 1, None), (33, 2, None), (70, 3, [(0, 20), (20, 50)]), (97, 3, [(0, 33), (33, 1), (34, 63)])):
        for assign in (np.arange(n) % K, rng.integers(0, K, n), np.zeros(n, int)):
            status, got = run(exe, table([GOOD[k % 2] for k in range(K)], assign, ranges))
            assert status == "OK", got
            rows, nxt = got["rows"], 0
            assert sorted(rows.tolist()) == list(range(n))
            for p, start, count in got["tiles"]:
                assert start == nxt and 1 <= count <= 32 and (np.asarray(assign)[rows[start:start + count]] == p).all()
                nxt = start + count
            assert nxt == n and len(got["spans"]) == (1 if ranges is None else len(ranges))
            for (first, count), (tf, tc) in zip(ranges or [(0, n)], got["spans"]):       # a range's tiles hold its rows only
                held = np.concatenate([rows[s:s + c] for _, s, c in got["tiles"][tf:tf + tc]])
                assert sorted(held.tolist()) == list(range(first, first + count))
    # the bit test's layout by hand: 33 / 36 / 1 rows -> tiles 32 + 1, 32 + 4, 1
    a = np.array([0] * 33 + [1] * 36 + [2])
    got = run(exe, table([GOOD[0], GOOD[1], GOOD[0]], a))[1]
    assert got["tiles"] == [(0, 0, 32), (0, 32, 1), (1, 33, 32), (1, 65, 4), (2, 69, 1)] and got["spans"] == [(0, 5)]


# ------------------------------------------------------------------------------------------------------------------ 2: the refusals
def test_every_refusal_of_the_validator(exe):
    fn = "cosim_recurrent_table_create"
    good = table(GOOD, [0, 1, 1, 0, 1])
    assert run(exe, good)[0] == "OK"

    def refused(want, **over):
        assert run(exe, good, **over) == ("ERR", fn + ": " + want)

    def changed(key, idx, value):
        a = good[key].copy()
        a[idx] = value
        return {key: a}
    for K in (0, 65, -1):
        refused("%d policies, outside 1..64" % K, K=K)
    for n in (0, -4):
        refused("n %d is not positive" % n, n=n)
    for key in ("ne", "edims", "eact", "lstm_in", "hidden", "nh", "hdims", "hact", "por"):
        refused("null argument", **{key: None})
    refused("null argument", ranges=None, n_ranges=1)
    for ne in (4, -1):
        refused("policy 1: %d encoder layers, outside 0..3" % ne, **changed("ne", 1, ne))
    for nh in (0, 4):
        refused("policy 1: %d head layers, outside 1..3" % nh, **changed("nh", 1, nh))
    refused("policy 0: LSTM input width + hidden size 700 + 600 exceeds 1200", **changed("lstm_in", 0, 700), **changed("hidden", 0, 600))
    for width, layer in ((0, 0), (513, 1)):
        refused("policy 0: encoder width %d of layer %d outside 1..512" % (width, layer), **changed("edims", (0, layer), width))
    for H in (0, 513):
        refused("policy 1: hidden size %d outside 1..512" % H, **changed("hidden", 1, H))
    for width, layer in ((-3, 0), (600, 2)):
        refused("policy 1: head width %d of layer %d outside 1..512" % (width, layer), **changed("hdims", (1, layer), width))
    refused("policy 1: input width 16 differs from policy 0's 12", **changed("edims", (1, 0), 16))
    refused("policy 1: output width 3 differs from policy 0's 4", **changed("hdims", (1, 2), 3))
    refused("policy 0: the LSTM's input width 41 differs from the encoder's output width 40", **changed("lstm_in", 0, 41))
    refused("policy 1: the LSTM's input width 13 differs from the encoder's output width 12", **changed("lstm_in", 1, 13))   # no encoder: the observation
    refused("policy 0: the head's input width 9 differs from the hidden size 8", **changed("hdims", (0, 0), 9))
    for code in (6, -1):
        refused("policy 0, encoder layer 0: unknown activation %d (0 none .. 5 leaky relu)" % code, **changed("eact", (0, 0), code))
        refused("policy 1, head layer 1: unknown activation %d (0 none .. 5 leaky relu)" % code, **changed("hact", (1, 1), code))
    for row, k in ((3, 2), (0, -1)):
        refused("row %d is assigned to policy %d, outside [0, 2)" % (row, k), **changed("por", row, k))
    refused("range 1 (2, 3) overlaps the one before it", ranges=np.array([(0, 3), (2, 3)], i32))
    refused("range 1 (4, 1) leaves rows from 3 uncovered", ranges=np.array([(0, 3), (4, 1)], i32))
    refused("the ranges leave rows from 4 uncovered", ranges=np.array([(0, 3), (3, 1)], i32))
    refused("range 1 (3, 3) ends past n 5", ranges=np.array([(0, 3), (3, 3)], i32))
    refused("range 1 (3, 0) is empty", ranges=np.array([(0, 3), (3, 0), (3, 2)], i32))
    refused("0 ranges, outside 1..n", ranges=np.zeros((0, 2), i32))
    # the order: counts ahead of arrays, a policy's shape ahead of rows and ranges
    refused("0 policies, outside 1..64", K=0, n=0, ne=None)
    refused("policy 1: input width 16 differs from policy 0's 12", **changed("edims", (1, 0), 16), por=np.array([0, 1, 9, 0, 1], i32))


# ------------------------------------------------------------------------------------------------- 3: the image, Hmax and the LDS rule
def test_image_alignment_offsets_hmax_and_lds_rule(exe):
    pols = [pol(obs=11, H=6, B=1, head=(4,), hact=(0,), hhb=(1,)),                                        # no encoder, I + H = 17
            pol(obs=11, enc=(16,), eact=(3,), ehb=(1,), H=70, B=0, head=(8, 4), hact=(2, 0), hhb=(1, 0)),  # no B, last layer without bias
            pol(obs=11, enc=(9, 7, 5), eact=(1, 2, 0), ehb=(0, 1, 0), H=160, B=1, head=(33, 32, 4), hact=(4, 5, 0), hhb=(1, 1, 1))]
    status, got = run(exe, table(pols, [0, 1, 2, 2]))
    assert status == "OK"
    # ld_m: the widest of any encoder / head width or H, | 1; ld_x: the largest I + H, | 1; Hmax
    assert (got["ld_m"], got["ld_x"], got["hmax"]) == (160 | 1, (5 + 160) | 1, 160)
    assert got["lds"] == 4 * 32 * (2 * 161 + 165) + 256 == 62592
    img, spans = got["image"], []
    for k, (p, d) in enumerate(zip(pols, got["desc"])):
        (ed, ea, eb), (hd, ha, hb) = p["enc"], p["head"]
        ne, nh, I, H = len(ed) - 1, len(hd) - 1, p["I"], p["H"]
        assert (d["ne"], d["nh"], d["I"], d["H"]) == (ne, nh, I, H) and d["edims"][:ne + 1] == list(ed) and d["hdims"][:nh + 1] == list(hd)
        assert d["eact"][:ne] == list(ea) and d["hact"][:nh] == list(ha) and d["vec"] == int(I % 4 == 0 and H % 4 == 0)
        assert d["ewoff"][ne:] == [-1] * (ME - ne) and d["eboff"][ne:] == [-1] * (ME - ne) and d["hwoff"][nh:] == [-1] * (MH - nh)
        arrays = [(d["ewoff"][l], ed[l] * ed[l + 1], 10 * l + 1, True) for l in range(ne)] + \
                 [(d["eboff"][l], ed[l + 1], 10 * l + 2, False) for l in range(ne) if eb[l]] + \
                 [(d["woff"], 4 * H * I, 51, True), (d["roff"], 4 * H * H, 52, True)] + ([(d["boff"], 8 * H, 53, False)] if p["B"] else []) + \
                 [(d["hwoff"][l], hd[l] * hd[l + 1], 60 + 10 * l + 1, True) for l in range(nh)] + \
                 [(d["hboff"][l], hd[l + 1], 60 + 10 * l + 2, False) for l in range(nh) if hb[l]]
        for off, size, code, matrix in arrays:
            assert off >= 0 and (not matrix or off % 4 == 0), (k, code, off)                  # every matrix on a 4-word boundary
            assert (img[off:off + size] == 1000 * k + code).all(), (k, code)
            spans.append((off, size))
        assert (d["boff"] == -1) == (not p["B"])                                              # -1 exactly where there is no bias
        assert [o == -1 for o in d["eboff"][:ne]] == [not b for b in eb] and [o == -1 for o in d["hboff"][:nh]] == [not b for b in hb]
    spans.sort()
    for (o0, n0), (o1, _) in zip(spans, spans[1:]):
        assert o0 + n0 <= o1 < o0 + n0 + 4                                                    # no overlap, at most 3 words of padding
    used = np.zeros(len(img), bool)
    for o, n in spans:
        used[o:o + n] = True
    assert spans[-1][0] + spans[-1][1] == len(img) and (img[~used] == 0).all() and (~used).sum() > 0
    # the rule against a device limit: the table above fits 62592 bytes exactly, not one less; the refusal names the policy and both counts
    assert run(exe, table(pols, [0, 1, 2, 2], lds_limit=62592))[0] == "OK"
    assert run(exe, table(pols, [0, 1, 2, 2], lds_limit=62591)) == \
        ("ERR", "cosim_recurrent_table_create: policy 2 needs 62592 bytes of LDS (two tiles of 32 x 161 words, one of 32 x 165, 256 static), "
                "the device allows 62591")
    # the widest tiles of two policies that each fit: ld_m 513 of policy 0 (4 * 32 * (2 * 513 + 21) + 256 = 134272) and ld_x 1025 of policy 1
    # (4 * 32 * (2 * 513 + 1025) + 256 = 262784 alone already); a 64 KiB device takes neither, 160 KiB takes policy 0 only
    wide = [pol(obs=12, H=8, head=(512, 4), hact=(1, 0), hhb=(1, 1)), pol(obs=12, enc=(512,), eact=(1,), ehb=(1,), H=512)]
    assert run(exe, table(wide[:1], [0, 0], lds_limit=163840))[1]["lds"] == 134272
    assert run(exe, table(wide, [0, 1], lds_limit=163840)) == \
        ("ERR", "cosim_recurrent_table_create: policy 1 needs 262784 bytes of LDS (two tiles of 32 x 513 words, one of 32 x 1025, 256 static), "
                "the device allows 163840")
    both = [pol(obs=12, H=8, head=(300, 4), hact=(1, 0), hhb=(1, 1)), pol(obs=12, enc=(200,), eact=(1,), ehb=(1,), H=200)]
    one = [run(exe, table([p], [0]))[1]["lds"] for p in both]
    assert one == [4 * 32 * (2 * 301 + 21) + 256, 4 * 32 * (2 * 201 + 401) + 256] and max(one) < 110000
    assert run(exe, table(both, [0, 1], lds_limit=110000)) == \
        ("ERR", "cosim_recurrent_table_create: the table needs %d bytes of LDS (two tiles of 32 x 301 words, one of 32 x 401, 256 static), "
                "the device allows 110000" % (4 * 32 * (2 * 301 + 401) + 256))


# ---------------------------------------------------------------------------------------------------------------- 4: the recogniser
def _layers(dims, acts, seed, nobias=()):
    rng = np.random.default_rng(seed)
    return [((rng.standard_normal((dims[l + 1], dims[l])) / np.sqrt(dims[l])).astype(np.float32),
             None if l in nobias else (0.5 * rng.standard_normal(dims[l + 1])).astype(np.float32), acts[l], 0.3) for l in range(len(dims) - 1)]


def _lstm(I, H, seed, bias=True):
    rng = np.random.default_rng(seed)
    return ((rng.standard_normal((4 * H, I)) / np.sqrt(I)).astype(np.float32), (rng.standard_normal((4 * H, H)) / np.sqrt(H)).astype(np.float32),
            (0.5 * rng.standard_normal(8 * H)).astype(np.float32) if bias else None)


@pytest.fixture()
def files(tmp_path):
    """Three recurrent actors over 12 observations and 4 actions with hidden sizes 6, 10 and 7."""
    from cosim_amd.policy import write_recurrent_actor
    out = [str(tmp_path / f"{n}.onnx") for n in "abc"]
    write_recurrent_actor(out[0], [], _lstm(12, 6, 1), _layers((6, 4), [None], 2))
    write_recurrent_actor(out[1], _layers((12, 16), ["Elu"], 3), _lstm(16, 10, 4, bias=False), _layers((10, 8, 4), ["Tanh", None], 5, nobias=(1,)), read="Y")
    write_recurrent_actor(out[2], _layers((12, 9, 5), ["Relu", None], 6), _lstm(5, 7, 7), _layers((7, 4), ["Tanh"], 8))
    return out


def test_recogniser_accepts_the_actor_shapes(files):
    from cosim_amd.policy import _recurrent_actor, read_onnx
    want = [(0, 1, 12, 6, True), (1, 2, 16, 10, False), (2, 1, 5, 7, True)]               # encoder / head layers, I, H, B
    for f, (ne, nh, I, H, has_b) in zip(files, want):
        part, why = _recurrent_actor(read_onnx(f))
        assert why is None, (f, why)
        assert (len(part["enc"]), len(part["head"]), part["I"], part["H"], part["B"] is not None) == (ne, nh, I, H, has_b)
        assert part["W"].shape == (4 * H, I) and part["R"].shape == (4 * H, H) and (part["in_dim"], part["out_dim"]) == (12, 4)
    m = read_onnx(files[1])                                                                # the file that reads Y: its head's first Gemm follows Y
    assert any(n["op"] == "Squeeze" and n["inputs"] == ["Y"] for n in m["nodes"])
    assert _recurrent_actor(read_onnx(files[2]))[0]["head"][0][2] == 2                     # an activation on the last layer (Tanh)


def test_recogniser_refuses_and_names_the_reason(files, tmp_path):
    from cosim_amd.policy import RecurrentPolicyTable, _recurrent_actor, read_onnx, write_onnx

    def rewritten(name, change):
        m = read_onnx(files[0])
        nodes, init, inputs, outputs = [dict(n, inputs=list(n["inputs"]), outputs=list(n["outputs"]), attrs=dict(n["attrs"])) for n in m["nodes"]], \
            dict(m["init"]), list(m["inputs"]), list(m["outputs"])
        change(nodes, init, inputs, outputs)
        path = str(tmp_path / name)
        write_onnx(path, nodes, init, inputs, outputs)
        return path

    def lstm_of(nodes):
        return next(n for n in nodes if n["op"] == "LSTM")

    def bidirectional(nodes, init, inputs, outputs):
        lstm_of(nodes)["attrs"]["direction"] = "bidirectional"

    def second_lstm(nodes, init, inputs, outputs):
        i = nodes.index(lstm_of(nodes))
        nodes.insert(i + 1, {"op": "LSTM", "inputs": ["Y2", "R", "R", "", "", "h_out", "c_out"], "outputs": ["Y3", "h3", "c3"], "attrs": {"hidden_size": 6}})

    def head_not_a_chain(nodes, init, inputs, outputs):
        nodes[-1]["outputs"] = ["pre"]
        nodes.append({"op": "Softplus", "inputs": ["pre"], "outputs": ["actions"], "attrs": {}})

    def initial_h_unwired(nodes, init, inputs, outputs):
        lstm_of(nodes)["inputs"][5] = ""

    def mlp_inputs(nodes, init, inputs, outputs):
        del inputs[1:]
    for change, want in ((bidirectional, r"LSTM direction 'bidirectional' \(forward only\)"), (second_lstm, "a second LSTM node"),
                         (head_not_a_chain, r"the head is not a Gemm / activation chain.*node 'Softplus'"),
                         (initial_h_unwired, "initial_h is not wired to h_in"), (mlp_inputs, r"the inputs are \['obs'\], not \(obs, 'h_in', 'c_in'\)")):
        path = rewritten(change.__name__ + ".onnx", change)
        part, why = _recurrent_actor(read_onnx(path))
        assert part is None and why, change.__name__
        with pytest.raises(ValueError, match=change.__name__ + r"\.onnx: not a recurrent actor: " + want):
            RecurrentPolicyTable([files[0], path], num_envs=4, device="cpu")


# ------------------------------------------------------------------------------------------------- 5: the torch twin against LSTMPolicy
def test_cpu_twin_equals_each_lstm_policy_on_its_rows(files):
    import torch
    from cosim_amd.policy import LSTMPolicy, RecurrentPolicyTable
    N, hidden = 23, [6, 10, 7]
    a = np.random.default_rng(4).integers(0, 3, N)
    tab = RecurrentPolicyTable(files, num_envs=N, device="cpu", assign=a, ranges=[(0, 9), (9, 14)])
    assert tab.recurrent and tab.graph_safe and tab.hidden == hidden and tab.h.shape == tab.c.shape == (N, 10) and tab.names == ["a", "b", "c"]
    idx = [torch.as_tensor(np.nonzero(a == k)[0]) for k in range(3)]
    singles = [LSTMPolicy({"policy": {"h_in_dim": H, "c_in_dim": H}}, f, num_envs=len(i), device="cpu") for f, H, i in zip(files, hidden, idx)]
    rng = np.random.default_rng(5)
    mask = torch.tensor(rng.integers(0, 2, N).astype(np.uint8))

    def same_state():
        for k, (s, i, H) in enumerate(zip(singles, idx, hidden)):
            assert torch.equal(tab.h[i, :H], s.h_in[0]) and torch.equal(tab.c[i, :H], s.c_in[0]), k
            assert bool((tab.h[i, H:] == 0).all()) and bool((tab.c[i, H:] == 0).all())   # the columns past H_k stay zero
    saved = None
    for step in range(4):
        x = torch.tensor(rng.standard_normal((N, 12)).astype(np.float32))
        got = tab.get_action(x)
        assert got.shape == (N, 4) and got.data_ptr() == tab._out.data_ptr()
        for s, i in zip(singles, idx):
            assert len(i) and torch.equal(got[i], s.get_action(x[i]))
        same_state()
        assert float(tab.h.abs().max()) > 0
        if step == 1:                                                                       # a masked reset in between
            tab.reset(mask)
            for s, i in zip(singles, idx):
                s.reset(mask[i])
            same_state()
            assert bool((tab.h[mask != 0] == 0).all()) and float(tab.h[mask == 0].abs().max()) > 0
            saved = tab.state()
    # state() / load_state(src, mask): masked rows take the saved row of another env of their own policy, the others keep theirs
    before = tab.state()
    src = np.arange(N)
    for i in idx:
        src[i.numpy()] = np.roll(i.numpy(), 1)
    tab.load_state(saved, src=torch.as_tensor(src), mask=mask)
    m = mask != 0
    assert torch.equal(tab.h[m], saved["h"][torch.as_tensor(src)][m]) and torch.equal(tab.c[~m], before["c"][~m])
    tab.load_state(before)
    assert torch.equal(tab.h, before["h"]) and torch.equal(tab.c, before["c"]) and tab.h.data_ptr() != before["h"].data_ptr()
    with pytest.raises(ValueError, match="load_state: h has shape"):
        tab.load_state({"h": before["h"][:, :6], "c": before["c"]})
    # a range steps its own rows only, and done = (terminated, truncated) gives flagged rows a fresh state in the same call
    x = torch.tensor(rng.standard_normal((N, 12)).astype(np.float32))
    ref = RecurrentPolicyTable(files, num_envs=N, device="cpu", assign=a, ranges=[(0, 9), (9, 14)])
    ref.load_state(before)
    ref.reset(mask)
    act_ref = torch.full((N, 4), 7.0)
    ref.get_action_range(1, x, act_ref)
    act = torch.full((N, 4), 7.0)
    tab.get_action_range(1, x, act, done=(mask, torch.zeros_like(mask)))
    assert torch.equal(act, act_ref) and bool((act[:9] == 7.0).all()) and not bool((act[9:] == 7.0).any())
    assert torch.equal(tab.h[9:], ref.h[9:]) and torch.equal(tab.c[9:], ref.c[9:]) and torch.equal(tab.h[:9], before["h"][:9])
    with pytest.raises(ValueError, match="range 2 outside 0..1"):
        tab.get_action_range(2, x, act)
    with pytest.raises(ValueError, match=r"done is \(terminated, truncated\)"):
        tab.get_action_range(0, x, act, done=(mask[:5], mask[:5]))


def test_refusals_name_the_file(files, tmp_path):
    from cosim_amd.policy import RecurrentPolicyTable, write_recurrent_actor
    wide = str(tmp_path / "wide_in.onnx")
    write_recurrent_actor(wide, [], _lstm(16, 6, 1), _layers((6, 4), [None], 2))
    with pytest.raises(ValueError, match=r"wide_in\.onnx: input width 16 differs from 12 of .*a\.onnx"):
        RecurrentPolicyTable(files + [wide], num_envs=8, device="cpu")
    out5 = str(tmp_path / "five_out.onnx")
    write_recurrent_actor(out5, [], _lstm(12, 6, 1), _layers((6, 5), [None], 2))
    with pytest.raises(ValueError, match=r"five_out\.onnx: output width 5 differs from 4 of .*a\.onnx"):
        RecurrentPolicyTable(files + [out5], num_envs=8, device="cpu")
    with pytest.raises(ValueError, match="do not tile"):
        RecurrentPolicyTable(files, num_envs=8, device="cpu", ranges=[(0, 3), (4, 4)])
    with pytest.raises(ValueError, match=r"RecurrentPolicyTable: assign holds 0\.\.3, outside \[0, 3\)"):
        RecurrentPolicyTable(files, num_envs=4, device="cpu", assign=np.arange(4))


# -------------------------------------------------------------------------------------------------- 6: factory, build_policy, CLI
def test_factory_build_policy_and_cli(files, tmp_path, capsys):
    from cosim_amd.policy import PolicyTable, RecurrentPolicyTable, build_policy, open_policy_table, write_random_lstm, write_random_mlp
    mlps = [str(tmp_path / f"mlp{k}.onnx") for k in range(2)]
    for k, f in enumerate(mlps):
        write_random_mlp(f, 12, 4, hidden=(8,), seed=k)
    assert type(open_policy_table(mlps, num_envs=6, device="cpu")) is PolicyTable
    tab = open_policy_table(files, num_envs=6, device="cpu", assign="cross", scenarios=2, env_id0=10, names=["x", "y", "z"])
    assert type(tab) is RecurrentPolicyTable and (tab.policy_of_env == (np.arange(10, 16) // 2) % 3).all() and tab.names == ["x", "y", "z"]
    with pytest.raises(ValueError, match=r"mlp0\.onnx: an MLP actor among recurrent ones .*a table is all one kind"):
        open_policy_table(files[:2] + mlps, num_envs=6, device="cpu")
    with pytest.raises(ValueError, match=r"c\.onnx: a recurrent actor among MLP ones .*a table is all one kind"):
        open_policy_table(mlps + files[2:], num_envs=6, device="cpu")
    tab = build_policy({"policy": {"use_lstm": False, "onnx_files": files, "assign": "interleave"}}, num_envs=7, device="cpu", env_id0=3)
    assert type(tab) is RecurrentPolicyTable and (tab.policy_of_env == np.arange(3, 10) % 3).all()
    assert type(build_policy({"policy": {"onnx_files": mlps}}, num_envs=7, device="cpu")) is PolicyTable
    with pytest.raises(ValueError, match="MLP actors only"):                               # use_lstm belongs to a single file
        build_policy({"policy": {"use_lstm": True, "onnx_files": files}}, num_envs=8, device="cpu")
    # the random writer gives a file of the kind, with the shapes asked for
    f = str(tmp_path / "rand.onnx")
    write_random_lstm(f, 12, 4, hidden=20, encoder=(16,), head=(8,), seed=3, bias_scale=0.1)
    one = RecurrentPolicyTable([f], num_envs=3, device="cpu")
    assert one.hidden == [20] and (one.in_dim, one.out_dim) == (12, 4)
    # the CLI, argument parsing only: what it refuses before any device is touched stays as it was, and --help states the rule
    from cosim_amd import cli
    for argv, want in ((files[:2] + ["--lstm"], "MLP actors only"), (files[:2] + ["--policy-names", "x"], "one name per --policy file"),
                       (files[:1] + ["--policy-assign", "cross"], "need several --policy files")):
        with pytest.raises(SystemExit) as e:
            cli.main(["--policy", *argv])
        assert e.value.code == 2 and want in capsys.readouterr().err, argv
    with pytest.raises(SystemExit) as e:
        cli.main(["--help"])
    assert e.value.code == 0 and "the kind is detected from the files" in " ".join(capsys.readouterr().out.split())
