"""Batched policy module: ONNX reader + interpreter against numpy evaluations of the same graphs.
PARITY UNPINNED against onnxruntime (absent here; no policy file ships with the reference)."""
import numpy as np
import pytest

from cosim_amd.policy import LSTMPolicy, MLPPolicy, build_policy, read_onnx, write_onnx, write_random_mlp


def test_mlp_policy_matches_numpy_and_clips(tmp_path):
    p = str(tmp_path / "actor.onnx")
    write_random_mlp(p, state_dim=52, action_dim=4, hidden=(64, 32), seed=3, activation="Elu")
    m = read_onnx(p)
    assert m["inputs"] == ["obs"] and m["outputs"] == ["actions"] and [n["op"] for n in m["nodes"]] == ["Gemm", "Elu", "Gemm", "Elu", "Gemm"]
    assert m["nodes"][0]["attrs"]["transB"] == 1 and m["init"]["w0"].shape == (64, 52)
    pol = MLPPolicy(p, device="cpu")
    x = (3.0 * np.random.default_rng(0).standard_normal((7, 52))).astype(np.float32)
    h = x
    for li in range(3):
        h = h @ m["init"][f"w{li}"].T + m["init"][f"b{li}"]
        if li < 2:
            h = np.where(h > 0, h, np.exp(np.minimum(h, 0)) - 1)
    got = pol.get_action(x).numpy()
    np.testing.assert_allclose(got, np.clip(h, -1, 1), atol=2e-5)
    assert np.abs(h).max() > 1.0 and np.abs(got).max() <= 1.0          # the clip of core/policy.py:20 is exercised
    single = pol.get_action(x[2])                                        # single-state call keeps the reference's shape
    assert single.shape == (4,) and np.allclose(single.numpy(), got[2], atol=1e-6)


def test_lstm_policy_carries_state_per_env(tmp_path):
    rng = np.random.default_rng(1)
    I, H, A = 10, 6, 3
    W = (0.4 * rng.standard_normal((1, 4 * H, I))).astype(np.float32)
    R = (0.4 * rng.standard_normal((1, 4 * H, H))).astype(np.float32)
    B = (0.1 * rng.standard_normal((1, 8 * H))).astype(np.float32)
    Wo = (0.5 * rng.standard_normal((A, H))).astype(np.float32)
    bo = np.zeros(A, dtype=np.float32)
    nodes = [{"op": "Unsqueeze", "inputs": ["obs"], "outputs": ["x3"], "attrs": {"axes": [0]}},
             {"op": "LSTM", "inputs": ["x3", "W", "R", "B", "", "h_in", "c_in"], "outputs": ["Y", "h_out", "c_out"], "attrs": {"hidden_size": H}},
             {"op": "Squeeze", "inputs": ["h_out"], "outputs": ["hs"], "attrs": {"axes": [0]}},
             {"op": "Gemm", "inputs": ["hs", "Wo", "bo"], "outputs": ["actions"], "attrs": {"transB": 1}}]
    p = str(tmp_path / "lstm.onnx")
    write_onnx(p, nodes, {"W": W, "R": R, "B": B, "Wo": Wo, "bo": bo}, ["obs", "h_in", "c_in"], ["actions", "h_out", "c_out"])
    cfg = {"policy": {"use_lstm": True, "h_in_dim": H, "c_in_dim": H}}
    pol = build_policy(cfg, p, num_envs=5, device="cpu")
    assert isinstance(pol, LSTMPolicy)
    sig = lambda v: 1 / (1 + np.exp(-v))
    h = np.zeros((5, H)); c = np.zeros((5, H))
    for t in range(4):
        x = rng.standard_normal((5, I)).astype(np.float32)
        g = x @ W[0].T + h @ R[0].T + B[0, :4 * H] + B[0, 4 * H:]
        i, o, f, cc = g[:, :H], g[:, H:2 * H], g[:, 2 * H:3 * H], g[:, 3 * H:]
        c = sig(f) * c + sig(i) * np.tanh(cc)
        h = sig(o) * np.tanh(c)
        np.testing.assert_allclose(pol.get_action(x).numpy(), np.clip(h @ Wo.T + bo, -1, 1), atol=2e-5)
    pol.reset(mask=np.array([1, 0, 0, 0, 1]))
    assert float(pol.h_in[0, 0].abs().max()) == 0.0 and float(pol.h_in[0, 1].abs().max()) > 0.0
    with pytest.raises(AssertionError, match="h_in"):                     # core/policy.py:28-29
        write_onnx(p, nodes, {"W": W, "R": R, "B": B, "Wo": Wo, "bo": bo}, ["obs", "hidden", "cell"], ["actions", "h_out", "c_out"])
        LSTMPolicy(cfg, p, num_envs=1, device="cpu")


def test_unknown_operator_fails_loudly(tmp_path):
    p = str(tmp_path / "bad.onnx")
    write_onnx(p, [{"op": "Einsum", "inputs": ["obs"], "outputs": ["actions"]}], {}, ["obs"], ["actions"])
    with pytest.raises(NotImplementedError, match="Einsum"):
        MLPPolicy(p, device="cpu").get_action(np.zeros((1, 3), dtype=np.float32))


# ---------------------------------------------------------------------------------------------- the rest of the operator subset
def _run(tmp_path, nodes, init, x, inputs=("obs",), outputs=("y",)):
    """One small graph through the interpreter on the CPU (no clip: OnnxGraph.run, not get_action)."""
    import torch
    from cosim_amd.policy import OnnxGraph
    p = str(tmp_path / "g.onnx")
    write_onnx(p, nodes, init, list(inputs), list(outputs))
    g = OnnxGraph(read_onnx(p), torch.device("cpu"))
    return [o.numpy() for o in g.run({"obs": torch.as_tensor(x)})]


def _x(d=6, seed=0):
    return (1.5 * np.random.default_rng(seed).standard_normal((3, d))).astype(np.float32)


@pytest.mark.parametrize("op,attrs,ref", [
    ("Relu", {}, lambda v: np.maximum(v, 0)),
    ("Tanh", {}, np.tanh),
    ("Sigmoid", {}, lambda v: 1 / (1 + np.exp(-v))),
    ("LeakyRelu", {}, lambda v: np.where(v > 0, v, 0.01 * v)),
    ("LeakyRelu", {"alpha": 0.2}, lambda v: np.where(v > 0, v, float(np.float32(0.2)) * v)),
    ("Elu", {"alpha": 0.3}, lambda v: np.where(v > 0, v, float(np.float32(0.3)) * (np.exp(np.minimum(v, 0)) - 1))),
    ("Softplus", {}, lambda v: np.logaddexp(0, v)),
    ("Identity", {}, lambda v: v),
    ("Clip", {"min": -0.5, "max": 0.75}, lambda v: np.clip(v, -0.5, 0.75)),
    ("Clip", {"max": 0.25}, lambda v: np.minimum(v, 0.25)),
])
def test_unary_operators_match_numpy(tmp_path, op, attrs, ref):
    x = _x()
    y, = _run(tmp_path, [{"op": op, "inputs": ["obs"], "outputs": ["y"], "attrs": attrs}], {}, x)
    assert y.dtype == np.float32 and y.shape == x.shape
    np.testing.assert_allclose(y, ref(x.astype(np.float64)), rtol=0, atol=1e-6)
    assert (x < 0).any() and (x > 1).any()                               # both branches of every activation / clip are hit


@pytest.mark.parametrize("op,ref", [("Add", np.add), ("Sub", np.subtract), ("Mul", np.multiply), ("Div", np.divide)])
def test_binary_operators_broadcast_like_numpy(tmp_path, op, ref):
    x = _x()
    k = np.array([0.5, -2.0, 3.0, 1.5, -0.25, 4.0], dtype=np.float32)    # [d] against [3, d]; not symmetric, so operand order shows
    y, = _run(tmp_path, [{"op": op, "inputs": ["obs", "k"], "outputs": ["y"]}], {"k": k}, x)
    np.testing.assert_allclose(y, ref(x.astype(np.float64), k.astype(np.float64)), rtol=1e-6, atol=1e-6)
    z, = _run(tmp_path, [{"op": op, "inputs": ["k", "obs"], "outputs": ["y"]}], {"k": k}, x)
    np.testing.assert_allclose(z, ref(k.astype(np.float64), x.astype(np.float64)), rtol=1e-6, atol=1e-6)


def test_clip_with_min_max_inputs(tmp_path):
    """Opset 11+: min / max are inputs (0-d initialisers), either may be left out."""
    x = _x()
    init = {"lo": np.array(-0.5, dtype=np.float32), "hi": np.array(0.75, dtype=np.float32)}
    y, = _run(tmp_path, [{"op": "Clip", "inputs": ["obs", "lo", "hi"], "outputs": ["y"]}], init, x)
    np.testing.assert_array_equal(y, np.clip(x, np.float32(-0.5), np.float32(0.75)))
    y, = _run(tmp_path, [{"op": "Clip", "inputs": ["obs", "", "hi"], "outputs": ["y"]}], init, x)
    np.testing.assert_array_equal(y, np.minimum(x, np.float32(0.75)))
    y, = _run(tmp_path, [{"op": "Clip", "inputs": ["obs", "lo"], "outputs": ["y"]}], init, x)
    np.testing.assert_array_equal(y, np.maximum(x, np.float32(-0.5)))


def test_shape_operators_match_numpy(tmp_path):
    """Reshape with a 0 entry, Flatten, Transpose (with and without perm), Concat, Squeeze / Unsqueeze with axes as an input."""
    x = _x(d=8)
    i64 = lambda *v: np.array(v, dtype=np.int64)
    nodes = [{"op": "Reshape", "inputs": ["obs", "shape"], "outputs": ["r"]},                        # [3, 8] -> [3, 2, 4]: 0 keeps the batch
             {"op": "Transpose", "inputs": ["r"], "outputs": ["t"], "attrs": {"perm": [0, 2, 1]}},   # [3, 4, 2]
             {"op": "Flatten", "inputs": ["t"], "outputs": ["f"], "attrs": {"axis": 1}},             # [3, 8], other element order
             {"op": "Concat", "inputs": ["f", "obs"], "outputs": ["c"], "attrs": {"axis": 1}},       # [3, 16]
             {"op": "Unsqueeze", "inputs": ["c", "ax02"], "outputs": ["u"]},                         # [1, 3, 1, 16]
             {"op": "Squeeze", "inputs": ["u", "ax2"], "outputs": ["s"]},                            # [1, 3, 16]
             {"op": "Transpose", "inputs": ["s"], "outputs": ["y"]}]                                 # default: reversed -> [16, 3, 1]
    outs = _run(tmp_path, nodes, {"shape": i64(0, 2, -1), "ax02": i64(0, 2), "ax2": i64(2)}, x, outputs=("r", "t", "f", "c", "u", "s", "y"))
    r = x.reshape(3, 2, 4)
    t = r.transpose(0, 2, 1)
    f = t.reshape(3, 8)
    c = np.concatenate([f, x], axis=1)
    s = c[None]
    for got, want in zip(outs, (r, t, f, c, c[None, :, None, :], s, s.transpose(2, 1, 0))):
        assert got.shape == want.shape
        np.testing.assert_array_equal(got, want)
    assert not np.array_equal(f, x)                                      # the transpose really moved elements
    y, = _run(tmp_path, [{"op": "Flatten", "inputs": ["obs"], "outputs": ["y"], "attrs": {"axis": 0}}], {}, x)
    assert y.shape == (1, 24) and np.array_equal(y[0], x.reshape(-1))
    y, = _run(tmp_path, [{"op": "Unsqueeze", "inputs": ["obs", "ax"], "outputs": ["u"]}, {"op": "Squeeze", "inputs": ["u"], "outputs": ["y"]}],
              {"ax": i64(0)}, x[:1])                                     # Squeeze without axes drops every 1
    assert y.shape == (8,)


def test_gemm_with_transA_alpha_beta(tmp_path):
    x = _x(d=5)                                                          # [3, 5], used as A^T: A' = x.T is [5, 3]
    rng = np.random.default_rng(4)
    B, C = rng.standard_normal((3, 4)).astype(np.float32), rng.standard_normal(4).astype(np.float32)
    y, = _run(tmp_path, [{"op": "Gemm", "inputs": ["obs", "B", "C"], "outputs": ["y"], "attrs": {"transA": 1, "alpha": 0.5, "beta": 2.0}}],
              {"B": B, "C": C}, x)
    np.testing.assert_allclose(y, 0.5 * (x.T.astype(np.float64) @ B) + 2.0 * C, rtol=0, atol=2e-6)
    y, = _run(tmp_path, [{"op": "Gemm", "inputs": ["obs", "Bt"], "outputs": ["y"], "attrs": {"transA": 1, "transB": 1, "alpha": -1.5}}],
              {"Bt": np.ascontiguousarray(B.T)}, x)                      # no C at all
    np.testing.assert_allclose(y, -1.5 * (x.T.astype(np.float64) @ B), rtol=0, atol=2e-6)


def test_matmul_add_tanh_actor_equals_its_gemm_twin(tmp_path):
    """The other common export form: MatMul with a pre-transposed weight + Add, ending in Tanh."""
    rng = np.random.default_rng(5)
    d, hdim, adim = 7, 12, 3
    w0, b0 = (rng.standard_normal((hdim, d)) / np.sqrt(d)).astype(np.float32), (0.5 * rng.standard_normal(hdim)).astype(np.float32)
    w1, b1 = (rng.standard_normal((adim, hdim)) / np.sqrt(hdim)).astype(np.float32), (0.5 * rng.standard_normal(adim)).astype(np.float32)
    gemm = [{"op": "Gemm", "inputs": ["obs", "w0", "b0"], "outputs": ["l0"], "attrs": {"transB": 1}},
            {"op": "Tanh", "inputs": ["l0"], "outputs": ["h0"]},
            {"op": "Gemm", "inputs": ["h0", "w1", "b1"], "outputs": ["l1"], "attrs": {"transB": 1}},
            {"op": "Tanh", "inputs": ["l1"], "outputs": ["actions"]}]
    mm = [{"op": "MatMul", "inputs": ["obs", "w0t"], "outputs": ["m0"]}, {"op": "Add", "inputs": ["m0", "b0"], "outputs": ["l0"]},
          {"op": "Tanh", "inputs": ["l0"], "outputs": ["h0"]},
          {"op": "MatMul", "inputs": ["h0", "w1t"], "outputs": ["m1"]}, {"op": "Add", "inputs": ["b1", "m1"], "outputs": ["l1"]},
          {"op": "Tanh", "inputs": ["l1"], "outputs": ["actions"]}]
    pa, pb = str(tmp_path / "gemm.onnx"), str(tmp_path / "matmul.onnx")
    write_onnx(pa, gemm, {"w0": w0, "b0": b0, "w1": w1, "b1": b1}, ["obs"], ["actions"])
    write_onnx(pb, mm, {"w0t": np.ascontiguousarray(w0.T), "b0": b0, "w1t": np.ascontiguousarray(w1.T), "b1": b1}, ["obs"], ["actions"])
    x = _x(d=d)
    a, b = MLPPolicy(pa, device="cpu").get_action(x).numpy(), MLPPolicy(pb, device="cpu").get_action(x).numpy()
    ref = np.tanh(np.tanh(x.astype(np.float64) @ w0.T + b0) @ w1.T + b1)
    np.testing.assert_allclose(a, ref, rtol=0, atol=2e-6)
    np.testing.assert_allclose(b, ref, rtol=0, atol=2e-6)
    np.testing.assert_allclose(a, b, rtol=0, atol=1e-6)


def test_chain_matcher_accepts_and_refuses_what_it_says(tmp_path):
    """_mlp_chain decides which graphs take the fused kernel: pin both lists (the GPU tests run them)."""
    from cosim_amd.policy import _mlp_chain
    w0, b0, w1 = np.ones((4, 3), np.float32), np.ones(4, np.float32), np.ones((2, 4), np.float32)

    def chain(act="Elu", act_attrs=None, g0=None, bias=True, final=None):
        nodes = [{"op": "Gemm", "inputs": ["obs", "w0"] + (["b0"] if bias else []), "outputs": ["l0"], "attrs": {"transB": 1, **(g0 or {})}},
                 {"op": act, "inputs": ["l0"], "outputs": ["h0"], "attrs": act_attrs or {}},
                 {"op": "Gemm", "inputs": ["h0", "w1"], "outputs": ["l1" if final else "actions"], "attrs": {"transB": 1}}]
        if final:
            nodes.append({"op": final, "inputs": ["l1"], "outputs": ["actions"]})
        p = str(tmp_path / "c.onnx")
        write_onnx(p, nodes, {"w0": w0, "b0": b0, "w1": w1}, ["obs"], ["actions"])
        return _mlp_chain(read_onnx(p))

    ok = chain(g0={"alpha": 1.0, "beta": 1.0})
    assert ok is not None and [(a, al) for *_, a, al in ok] == [(3, 1.0), (0, 1.0)]
    assert [(a, round(al, 6)) for *_, a, al in chain(act_attrs={"alpha": 0.3})] == [(3, 0.3), (0, 1.0)]
    assert [(a, round(al, 6)) for *_, a, al in chain(act="LeakyRelu")] == [(5, 0.01), (0, 1.0)]
    nb = chain(bias=False)
    assert nb is not None and nb[0][1] is None and nb[1][1] is None
    assert [a for *_, a, _ in chain(final="Tanh")] == [3, 2]
    assert chain(g0={"alpha": 0.5}) is None and chain(g0={"beta": 0.5}) is None and chain(act="Softplus") is None
    assert chain(g0={"transA": 1}) is None


# ---------------------------------------------------------------------------------------------- reader: the other tensor encodings
def _raw_model(nodes: bytes, tensors, inputs, outputs):
    """A ModelProto assembled by hand from pre-encoded NodeProto / TensorProto bytes (write_onnx only emits raw fp32 / int64)."""
    from cosim_amd.policy import _enc
    g = nodes + b"".join(_enc(5, 2, t) for t in tensors)
    g += b"".join(_enc(11, 2, _enc(1, 2, n.encode())) for n in inputs) + b"".join(_enc(12, 2, _enc(1, 2, n.encode())) for n in outputs)
    return _enc(1, 0, 8) + _enc(7, 2, g)


def _raw_tensor(name, dims, dtype_code, payload: bytes):
    from cosim_amd.policy import _enc
    return b"".join(_enc(1, 0, int(d)) for d in dims) + _enc(2, 0, dtype_code) + _enc(8, 2, name.encode()) + payload


def _raw_node(op, inputs, outputs, attrs=b""):
    from cosim_amd.policy import _enc
    nb = b"".join(_enc(1, 2, i.encode()) for i in inputs) + b"".join(_enc(2, 2, o.encode()) for o in outputs) + _enc(4, 2, op.encode()) + attrs
    return _enc(1, 2, nb)


def test_reader_takes_float_data_int64_data_and_wide_or_narrow_raw_data(tmp_path):
    import struct
    from cosim_amd.policy import _enc, _enc_varint
    a = np.array([[1.5, -2.25, 3.0], [0.1, 1e-8, -7e3]], dtype=np.float32)
    i = np.array([0, -1, 2, 1 << 40, -(1 << 40)], dtype=np.int64)
    tensors = [
        _raw_tensor("packed", a.shape, 1, _enc(4, 2, a.tobytes())),                                         # float_data, packed
        _raw_tensor("unpacked", a.shape, 1, b"".join(_enc(4, 5, struct.pack("<f", v)) for v in a.ravel())),  # one fixed32 per element
        _raw_tensor("ipacked", i.shape, 7, _enc(7, 2, b"".join(_enc_varint(int(v)) for v in i))),           # int64_data, packed varints
        _raw_tensor("iunpacked", i.shape, 7, b"".join(_enc(7, 0, int(v)) for v in i)),
        _raw_tensor("f64", a.shape, 11, _enc(9, 2, a.astype("<f8").tobytes())),
        _raw_tensor("f16", a.shape, 10, _enc(9, 2, a.astype("<f2").tobytes())),
        _raw_tensor("scalar", (), 1, _enc(4, 5, struct.pack("<f", 0.75))),
    ]
    p = str(tmp_path / "t.onnx")
    open(p, "wb").write(_raw_model(_raw_node("Identity", ["obs"], ["y"]), tensors, ["obs", "packed"], ["y"]))
    m = read_onnx(p)
    assert m["inputs"] == ["obs"]                                          # an initialiser listed as a graph input is not an input
    for k in ("packed", "unpacked"):
        assert m["init"][k].dtype == np.float32 and np.array_equal(m["init"][k], a), k
    for k in ("ipacked", "iunpacked"):
        assert m["init"][k].dtype == np.int64 and np.array_equal(m["init"][k], i), k
    assert m["init"]["f64"].dtype == np.float64 and np.array_equal(m["init"]["f64"], a.astype(np.float64))
    assert m["init"]["f16"].dtype == np.float16 and np.array_equal(m["init"]["f16"], a.astype(np.float16))
    assert m["init"]["scalar"].shape == () and float(m["init"]["scalar"]) == 0.75


def test_constant_node_with_a_tensor_attribute(tmp_path):
    import torch
    from cosim_amd.policy import OnnxGraph, _enc
    k = np.array([0.5, -2.0, 3.0], dtype=np.float32)
    value = _enc(1, 2, b"value") + _enc(5, 2, _raw_tensor("", k.shape, 1, _enc(9, 2, k.tobytes()))) + _enc(20, 0, 4)
    nodes = _raw_node("Constant", [], ["k"], _enc(5, 2, value)) + _raw_node("Mul", ["obs", "k"], ["y"])
    p = str(tmp_path / "c.onnx")
    open(p, "wb").write(_raw_model(nodes, [], ["obs"], ["y"]))
    x = _x(d=3)
    y, = OnnxGraph(read_onnx(p), torch.device("cpu")).run({"obs": torch.as_tensor(x)})
    np.testing.assert_array_equal(y.numpy(), x * k)


@pytest.mark.parametrize("code,dtype", [(11, np.float64), (10, np.float16)])
def test_fp64_and_fp16_initialisers_are_cast_to_fp32_on_load(tmp_path, code, dtype):
    """A policy exported from a double- or half-precision checkpoint evaluates (it used to die on a torch dtype error inside run):
    the weights are cast to fp32 when the graph is loaded, the values are those of the stored numbers."""
    from cosim_amd.policy import _enc, _mlp_chain
    rng = np.random.default_rng(6)
    w = (rng.standard_normal((4, 6)) / np.sqrt(6)).astype(dtype)
    b = (0.5 * rng.standard_normal(4)).astype(dtype)
    le = np.dtype(dtype).newbyteorder("<")
    tensors = [_raw_tensor("w", w.shape, code, _enc(9, 2, w.astype(le).tobytes())), _raw_tensor("b", b.shape, code, _enc(9, 2, b.astype(le).tobytes()))]
    node = _raw_node("Gemm", ["obs", "w", "b"], ["actions"], _enc(5, 2, _enc(1, 2, b"transB") + _enc(3, 0, 1) + _enc(20, 0, 2)))
    p = str(tmp_path / "w.onnx")
    open(p, "wb").write(_raw_model(node, tensors, ["obs"], ["actions"]))
    m = read_onnx(p)
    assert m["init"]["w"].dtype == dtype and m["nodes"][0]["attrs"] == {"transB": 1}
    assert _mlp_chain(m) is None                                         # the fused kernel takes fp32 files only
    pol = MLPPolicy(p, device="cpu")
    assert pol.graph.const["w"].dtype == pol.torch.float32 and pol.graph.const["b"].dtype == pol.torch.float32
    x = (0.5 * _x(d=6)).astype(np.float32)
    ref = x.astype(np.float64) @ w.astype(np.float64).T + b.astype(np.float64)
    assert np.mean(np.abs(ref) < 1) >= 0.5
    np.testing.assert_allclose(pol.get_action(x).numpy(), np.clip(ref, -1, 1), rtol=0, atol=2e-6)


def test_write_random_mlp_default_is_unchanged_and_bias_scale_fills_the_biases(tmp_path):
    """bias_scale = 0 (the default) writes what write_random_mlp always wrote: zero biases and, for seed 3, these weights and this
    file.  bias_scale > 0 leaves the weights alone and draws different biases per layer."""
    import hashlib
    p, q = str(tmp_path / "a.onnx"), str(tmp_path / "b.onnx")
    write_random_mlp(p, state_dim=52, action_dim=4, hidden=(64, 32), seed=3, activation="Elu")
    m = read_onnx(p)
    assert all(np.abs(m["init"][f"b{li}"]).max() == 0.0 for li in range(3))
    pinned = {"w0": (0.28302454948425293, -0.09586327522993088), "w1": (0.07093870639801025, -0.08436153829097748),
              "w2": (-0.038529444485902786, -0.05240444093942642)}
    for k, (first, last) in pinned.items():
        assert float(m["init"][k][0, 0]) == first and float(m["init"][k][-1, -1]) == last, k
    data = open(p, "rb").read()
    assert len(data) == 22719 and hashlib.sha256(data).hexdigest() == "bfc02695d8bb4712967f3906f5b37a2da49662d3720b0b1772c588d9041f58e4"
    write_random_mlp(q, state_dim=52, action_dim=4, hidden=(64, 32), seed=3, activation="Elu", bias_scale=0.5)
    mb = read_onnx(q)
    for li, width in enumerate((64, 32, 4)):
        assert np.array_equal(mb["init"][f"w{li}"], m["init"][f"w{li}"])
        b = mb["init"][f"b{li}"]
        assert b.shape == (width,) and b.dtype == np.float32 and np.abs(b).min() > 0.0 and 0.1 < b.std() < 1.0
    assert not np.array_equal(mb["init"]["b1"][:4], mb["init"]["b2"])
    x = _x(d=52)
    h = x.astype(np.float64)
    for li in range(3):
        h = h @ mb["init"][f"w{li}"].T.astype(np.float64) + mb["init"][f"b{li}"]
        if li < 2:
            h = np.where(h > 0, h, np.exp(np.minimum(h, 0)) - 1)
    np.testing.assert_allclose(MLPPolicy(q, device="cpu").get_action(x).numpy(), np.clip(h, -1, 1), rtol=0, atol=2e-5)
