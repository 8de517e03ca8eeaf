"""The fused actor grammar without a GPU: what ``_actor_graph`` (cosim_amd/policy.py) accepts and how it describes it, what it refuses
and why, that it describes every plain chain exactly as ``_mlp_chain`` does, the interpreter's new operators against fp64 numpy on the
CPU device, the writer's new keywords, and the ABI rows of include/cosim_actor.h."""
import ctypes
import os
import re

import numpy as np
import pytest

import actor_ext_graphs as G
from cosim_amd.policy import MLPPolicy, OnnxGraph, PolicyTable, _actor_graph, _mlp_chain, read_onnx, write_onnx, write_random_mlp

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
f32 = np.float32


def _spec(dims=(5, 8, 3), acts=("Elu", None), **over):
    spec = {"input": [], "ln0": None, "output": [], "layers": G.make_layers(dims, list(acts), seed=3, last_scale=0.5)}
    spec.update(over)
    return spec


def _describe(tmp_path, spec, **how):
    p = str(tmp_path / "a.onnx")
    G.write_actor(p, spec, **how)
    return _actor_graph(read_onnx(p))


def _ln(width, bias=True):
    rng = np.random.default_rng(width)
    return f32(1.0 + 0.3 * rng.standard_normal(width)), f32(0.2 * rng.standard_normal(width)) if bias else None, 1e-5


# ------------------------------------------------------------------------------------------------------------------ 1: what is accepted
def test_matcher_accepts_every_production_and_describes_it(tmp_path):
    mean, std = f32(np.arange(5) * 0.1), f32(1.0 + np.arange(5) * 0.2)
    # Sub / Div
    d, why = _describe(tmp_path, _spec(input=[("Sub", mean), ("Div", std)]))
    assert why is None and [c for c, *_ in d["input"]] == [2, 4] and np.array_equal(d["input"][0][1], mean) and np.array_equal(d["input"][1][1], std)
    assert d["output"] == [] and d["ln"] == {} and len(d["layers"]) == 2
    # Sub / Div / Clip, bounds as inputs; one bound absent
    d, why = _describe(tmp_path, _spec(input=[("Sub", mean), ("Div", std), ("Clip", (-5.0, 5.0))]))
    assert why is None and d["input"][2] == (5, None, -5.0, 5.0)
    d, why = _describe(tmp_path, _spec(input=[("Clip", (None, 2.0))]))
    assert why is None and d["input"] == [(5, None, -np.inf, 2.0)]
    d, why = _describe(tmp_path, _spec(input=[("Clip", (-1.5, None))]))
    assert why is None and d["input"] == [(5, None, -1.5, np.inf)]
    # Clip with its bounds as attributes
    spec = _spec()
    p = str(tmp_path / "attr.onnx")
    L = spec["layers"]
    write_onnx(p, [{"op": "Clip", "inputs": ["obs"], "outputs": ["k"], "attrs": {"min": -3.0, "max": 4.0}},
                   {"op": "Gemm", "inputs": ["k", "w0"], "outputs": ["actions"], "attrs": {"transB": 1}}], {"w0": L[0]["w"]}, ["obs"], ["actions"])
    d, why = _actor_graph(read_onnx(p))
    assert why is None and d["input"] == [(5, None, -3.0, 4.0)]
    # scalar, [1] and [1, W] constants are broadcast to [W] on the host
    for c in (f32(0.5), f32([0.5]), f32(np.full((1, 5), 0.5))):
        d, why = _describe(tmp_path, _spec(input=[("Mul", c)]))
        assert why is None and d["input"][0][0] == 3 and d["input"][0][1].shape == (5,) and (d["input"][0][1] == 0.5).all()
        assert d["input"][0][1].dtype == np.float32 and d["input"][0][1].flags["C_CONTIGUOUS"]
    # Constant-node operands; Add / Mul with the constant on the left
    d, why = _describe(tmp_path, _spec(input=[("Sub", mean), ("Clip", (-5.0, 5.0))], output=[("Mul", f32([1, 2, 3]))]), constant_nodes=True)
    assert why is None and [c for c, *_ in d["input"]] == [2, 5] and np.array_equal(d["output"][0][1], f32([1, 2, 3]))
    d, why = _describe(tmp_path, _spec(input=[("Add", mean), ("Mul", std)]), add_left=True)
    assert why is None and [c for c, *_ in d["input"]] == [1, 3] and np.array_equal(d["input"][1][1], std)
    # MatMul with and without Add (either operand order): the weight is transposed back to [O, I]
    for left in (False, True):
        spec = _spec()
        for L in spec["layers"]:
            L["matmul"] = True
        spec["layers"][1]["b"] = None
        d, why = _describe(tmp_path, spec, add_left=left)
        assert why is None and d["input"] == [] and d["output"] == []
        for got, L in zip(d["layers"], spec["layers"]):
            assert np.array_equal(got[0], L["w"]) and got[0].flags["C_CONTIGUOUS"] and (got[1] is None) == (L["b"] is None)
        assert np.array_equal(d["layers"][0][1], spec["layers"][0]["b"]) and [a for *_, a, _ in d["layers"]] == [3, 0]
    # LN before and after the activation, with and without bias; LN on the observation
    spec = _spec(dims=(5, 8, 6, 3), acts=("Elu", "Tanh", None))
    spec["layers"][0]["ln"] = ("before", *_ln(8))
    spec["layers"][1]["ln"] = ("after", *_ln(6, bias=False))
    spec["ln0"] = _ln(5)
    d, why = _describe(tmp_path, spec)
    assert why is None and set(d["ln"]) == {0, 1, 2} and [d["ln"][s][0] for s in (0, 1, 2)] == [1, 1, 2]
    assert np.array_equal(d["ln"][1][1], _ln(8)[0]) and np.array_equal(d["ln"][1][2], _ln(8)[1]) and d["ln"][2][2] is None
    assert d["ln"][1][3] == float(f32(1e-5)) and [a for *_, a, _ in d["layers"]] == [3, 2, 0]
    # the output stage: Tanh, Mul, Add, Clip
    d, why = _describe(tmp_path, _spec(acts=("Elu", "Tanh"), output=[("Mul", f32([1, 2, 3])), ("Add", f32(0.1)), ("Sub", f32([0, 1, 0])), ("Clip", (-0.8, 0.9))]))
    assert why is None and [c for c, *_ in d["output"]] == [3, 1, 2, 5] and d["output"][3][2:] == (float(f32(-0.8)), float(f32(0.9)))
    assert (d["output"][1][1] == f32(0.1)).all() and d["output"][1][1].shape == (3,)


# ------------------------------------------------------------------------------------------------------------------- 2: what is refused
def test_matcher_refuses_with_a_reason_that_names_the_node(tmp_path):
    mean = f32(np.arange(5) * 0.1)
    w0, w1 = np.ones((8, 5), f32), np.ones((3, 8), f32)

    def graph(nodes, init, inputs=("obs",)):
        p = str(tmp_path / "r.onnx")
        write_onnx(p, nodes, {"w0": w0, "w1": w1, **init}, list(inputs), ["actions"])
        return _actor_graph(read_onnx(p))
    tail = [{"op": "Gemm", "inputs": ["x", "w0"], "outputs": ["l0"], "attrs": {"transB": 1}}, {"op": "Tanh", "inputs": ["l0"], "outputs": ["h0"]},
            {"op": "Gemm", "inputs": ["h0", "w1"], "outputs": ["actions"], "attrs": {"transB": 1}}]
    for op, words in (("Sub", "c - x"), ("Div", "c / x")):
        d, why = graph([{"op": op, "inputs": ["m", "obs"], "outputs": ["x"]}] + tail, {"m": mean})
        assert d is None and words in why and f"'{op}'" in why and "'x'" in why
    five = [{"op": "Add", "inputs": ["obs" if k == 0 else f"t{k - 1}", "m"], "outputs": [f"t{k}" if k < 4 else "x"]} for k in range(5)]
    d, why = graph(five + tail, {"m": mean})
    assert d is None and "fifth item in the input stage" in why and "'Add'" in why
    g8, g3 = np.ones(8, f32), np.ones(3, f32)
    nodes = [dict(n) for n in tail]
    nodes[0] = {**nodes[0], "inputs": ["obs", "w0"]}
    last_ln = nodes[:2] + [{"op": "Gemm", "inputs": ["h0", "w1"], "outputs": ["l1"], "attrs": {"transB": 1}},
                           {"op": "LayerNormalization", "inputs": ["l1", "g3"], "outputs": ["actions"]}]
    d, why = graph(last_ln, {"g3": g3})
    assert d is None and "LayerNormalization on the last layer" in why
    mid = [nodes[0], {"op": "LayerNormalization", "inputs": ["l0", "g8"], "outputs": ["n0"], "attrs": {"axis": 0}}, {"op": "Tanh", "inputs": ["n0"], "outputs": ["h0"]}, nodes[2]]
    d, why = graph(mid, {"g8": g8})
    assert d is None and "axis 0" in why and "'LayerNormalization'" in why
    mid[1] = {"op": "LayerNormalization", "inputs": ["l0"], "outputs": ["n0"]}
    d, why = graph(mid, {})
    assert d is None and "LayerNormalization without scale" in why
    mid[1] = {"op": "LayerNormalization", "inputs": ["l0", "g8"], "outputs": ["n0"]}
    assert graph(mid, {"g8": g8})[1] is None       # and with a scale over the last axis it is accepted
    d, why = graph([{"op": "MatMul", "inputs": ["obs", "other"], "outputs": ["actions"]}], {}, inputs=("obs", "other"))
    assert d is None and "2 graph inputs" in why
    d, why = graph([{"op": "MatMul", "inputs": ["obs", "computed"], "outputs": ["actions"]}], {})
    assert d is None and "MatMul with a non-initialiser weight" in why
    d, why = graph([{"op": "MatMul", "inputs": ["w0", "obs"], "outputs": ["actions"]}], {})
    assert d is None and "MatMul with a non-initialiser weight" in why and "'MatMul'" in why
    # fp16 constants: written by hand (write_onnx emits fp32 only)
    from cosim_amd.policy import _enc
    h = np.arange(5).astype("<f2")
    t16 = b"".join(_enc(1, 0, int(k)) for k in h.shape) + _enc(2, 0, 10) + _enc(8, 2, b"m") + _enc(9, 2, h.tobytes())
    t32 = b"".join(_enc(1, 0, int(k)) for k in w0.shape) + _enc(2, 0, 1) + _enc(8, 2, b"w0") + _enc(9, 2, w0.tobytes())

    def node(op, ins, outs, attrs=b""):
        return _enc(1, 2, b"".join(_enc(1, 2, i.encode()) for i in ins) + b"".join(_enc(2, 2, o.encode()) for o in outs) + _enc(4, 2, op.encode()) + attrs)
    gb = node("Sub", ["obs", "m"], ["x"]) + node("Gemm", ["x", "w0"], ["actions"], _enc(5, 2, _enc(1, 2, b"transB") + _enc(3, 0, 1) + _enc(20, 0, 2)))
    gb += _enc(5, 2, t16) + _enc(5, 2, t32) + _enc(11, 2, _enc(1, 2, b"obs")) + _enc(12, 2, _enc(1, 2, b"actions"))
    p = str(tmp_path / "h.onnx")
    open(p, "wb").write(_enc(1, 0, 8) + _enc(7, 2, gb))
    d, why = _actor_graph(read_onnx(p))
    assert d is None and "float16, not fp32" in why and "'Sub'" in why
    # and an fp16 bound of a Clip: one element of the same fp16 tensor type, as the upper bound
    h1 = np.array(5.0).astype("<f2")
    b16 = _enc(2, 0, 10) + _enc(8, 2, b"hi") + _enc(9, 2, h1.tobytes())
    gb = node("Clip", ["obs", "", "hi"], ["x"]) + node("Gemm", ["x", "w0"], ["actions"], _enc(5, 2, _enc(1, 2, b"transB") + _enc(3, 0, 1) + _enc(20, 0, 2)))
    gb += _enc(5, 2, b16) + _enc(5, 2, t32) + _enc(11, 2, _enc(1, 2, b"obs")) + _enc(12, 2, _enc(1, 2, b"actions"))
    open(p, "wb").write(_enc(1, 0, 8) + _enc(7, 2, gb))
    d, why = _actor_graph(read_onnx(p))
    assert d is None and "bound 'hi' is float16, not fp32" in why and "'Clip'" in why


def _old_chain(tmp_path, layers, inputs=("obs",)):
    """A graph written the way tests/test_gpu_policy_kernels.py writes its chains (Gemm attributes included)."""
    nodes, init, x = [], {}, "obs"
    for li, L in enumerate(layers):
        init[f"w{li}"] = L["w"]
        ins = [x, f"w{li}"]
        if L["b"] is not None:
            init[f"b{li}"] = L["b"]
            ins.append(f"b{li}")
        last = li == len(layers) - 1
        attrs = {"transB": L.get("transB", 1)}
        for k, name in (("galpha", "alpha"), ("gbeta", "beta")):
            if k in L:
                attrs[name] = float(L[k])
        lin = "actions" if last and L["act"] is None else f"lin{li}"
        nodes.append({"op": "Gemm", "inputs": ins, "outputs": [lin], "attrs": attrs})
        x = lin
        if L["act"] is not None:
            y = "actions" if last else f"h{li}"
            nodes.append({"op": L["act"], "inputs": [lin], "outputs": [y], "attrs": {} if L.get("alpha_attr") is None else {"alpha": float(L["alpha_attr"])}})
            x = y
    p = str(tmp_path / "old.onnx")
    write_onnx(p, nodes, init, list(inputs), ["actions"])
    return read_onnx(p)


def _unfusable(kind):
    """The graphs tests/test_gpu_policy_kernels.py pins as outside the fused subset, and the words of the reason."""
    inputs, words = ("obs",), "Gemm(transB=1, alpha=beta=1, transA=0)"
    if kind == "seven_layers":
        layers, words = G.make_layers((6, 9, 8, 7, 9, 8, 7, 3), ["Tanh"] * 6 + [None], seed=40, last_scale=0.5), "seventh layer"
    elif kind == "wide_513":
        layers, words = G.make_layers((10, 513, 3), ["Tanh", None], seed=41, last_scale=0.5), "width 513"
    elif kind == "softplus":
        layers, words = G.make_layers((7, 12, 3), ["Softplus", None], seed=42, last_scale=0.3), "'Softplus'"
    else:
        layers = G.make_layers((7, 12, 3), ["Elu", None], seed=43, last_scale=0.5)
        if kind == "alpha_half":
            layers[0]["galpha"] = 0.5
        elif kind == "beta_half":
            layers[1]["gbeta"] = 0.5
        elif kind == "transB_0":
            layers[0]["w"] = np.ascontiguousarray(layers[0]["w"].T)
            layers[0]["transB"] = 0
        elif kind == "two_inputs":
            inputs, words = ("obs", "unused"), "2 graph inputs"
    return layers, inputs, words


@pytest.mark.parametrize("kind", ["alpha_half", "beta_half", "transB_0", "softplus", "seven_layers", "wide_513", "two_inputs"])
def test_matcher_refuses_what_the_chain_matcher_refuses(tmp_path, kind):
    layers, inputs, words = _unfusable(kind)
    m = _old_chain(tmp_path, layers, inputs)
    assert _mlp_chain(m) is None
    d, why = _actor_graph(m)
    assert d is None and words in why, why


# ----------------------------------------------------------------------------------------------------------- 3: plain chains, unchanged
PLAIN = {
    "one_layer": ((5, 3), [None], ()),
    "sigmoid_nobias0": ((7, 33, 3), ["Sigmoid", None], (0,)),
    "leaky_elu_float4": ((12, 40, 36, 4), ["LeakyRelu", "Elu", None], ()),
    "six_layers": ((9, 34, 31, 33, 30, 35, 2), ["Relu", None, "Tanh", "Sigmoid", "Elu", "Tanh"], ()),
    "widest": ((512, 512, 1), ["Tanh", None], ()),
}


@pytest.mark.parametrize("name", list(PLAIN) + ["explicit_alpha_beta", "alpha_attr", "random_mlp"])
def test_plain_chains_are_described_as_the_chain_matcher_describes_them(tmp_path, name):
    if name == "random_mlp":
        p = str(tmp_path / "r.onnx")
        write_random_mlp(p, state_dim=52, action_dim=4, hidden=(64, 32), seed=3, bias_scale=0.5)
        m = read_onnx(p)
    else:
        dims, acts, nobias = PLAIN.get(name, ((6, 10, 3), ["Elu", None], ()))
        layers = G.make_layers(dims, acts, seed=sum(map(ord, name)), nobias=nobias)
        if name == "explicit_alpha_beta":
            for L in layers:
                L["galpha"], L["gbeta"] = 1.0, 1.0
        if name == "alpha_attr":
            layers[0]["alpha_attr"] = 0.3
        m = _old_chain(tmp_path, layers)
    want = _mlp_chain(m)
    d, why = _actor_graph(m)
    assert want is not None and why is None
    assert d["input"] == [] and d["output"] == [] and d["ln"] == {} and set(d) == {"layers", "input", "output", "ln"}
    assert len(d["layers"]) == len(want)
    for (w, b, a, al), (w2, b2, a2, al2) in zip(d["layers"], want):
        assert w is w2 and b is b2 and (a, al) == (a2, al2)


# -------------------------------------------------------------------------------------------------------- 4: the interpreter's operators
def test_interpreter_layer_normalization_and_its_decomposed_spelling_match_fp64(tmp_path):
    import torch
    rng = np.random.default_rng(2)
    x = (2.0 * rng.standard_normal((9, 13)) + 0.5).astype(f32)
    g, b = f32(1.0 + 0.3 * rng.standard_normal(13)), f32(0.2 * rng.standard_normal(13))
    for bias, eps in ((b, 1e-5), (None, 1e-3)):
        p = str(tmp_path / "ln.onnx")
        write_onnx(p, [{"op": "LayerNormalization", "inputs": ["obs", "g"] + (["b"] if bias is not None else []), "outputs": ["y"], "attrs": {"axis": -1, "epsilon": eps}}],
                   {"g": g, **({"b": b} if bias is not None else {})}, ["obs"], ["y"])
        y, = OnnxGraph(read_onnx(p), torch.device("cpu")).run({"obs": torch.as_tensor(x)})
        np.testing.assert_allclose(y.numpy(), G.ln64(x.astype(np.float64), g, bias, eps), rtol=0, atol=2e-6)
    # default epsilon 1e-5, default axis -1
    write_onnx(p, [{"op": "LayerNormalization", "inputs": ["obs", "g", "b"], "outputs": ["y"]}], {"g": g, "b": b}, ["obs"], ["y"])
    y, = OnnxGraph(read_onnx(p), torch.device("cpu")).run({"obs": torch.as_tensor(x)})
    np.testing.assert_allclose(y.numpy(), G.ln64(x.astype(np.float64), g, b, 1e-5), rtol=0, atol=2e-6)
    # the decomposed spelling inside an actor: ReduceMean / Sub / Pow / Sqrt / Div / Mul / Add
    dims, spec = G.decomposed_layernorm_actor(p)
    xs = (0.7 * rng.standard_normal((11, dims[0]))).astype(f32)
    pol = MLPPolicy(p, device="cpu")
    ref = G.ref_actor(xs, spec)
    assert np.mean(np.abs(ref) < 1.0) >= 0.5
    np.testing.assert_allclose(pol.get_action(xs).numpy(), np.clip(ref, -1.0, 1.0), rtol=0, atol=2e-6)
    # ReduceMean with axes as an input and keepdims 0; Pow; Sqrt
    write_onnx(p, [{"op": "Pow", "inputs": ["obs", "two"], "outputs": ["sq"]}, {"op": "ReduceMean", "inputs": ["sq", "ax"], "outputs": ["m"], "attrs": {"keepdims": 0}},
                   {"op": "Sqrt", "inputs": ["m"], "outputs": ["y"]}], {"two": f32(2.0), "ax": np.array([1], np.int64)}, ["obs"], ["y"])
    y, = OnnxGraph(read_onnx(p), torch.device("cpu")).run({"obs": torch.as_tensor(x)})
    assert y.shape == (9,)
    np.testing.assert_allclose(y.numpy(), np.sqrt((x.astype(np.float64) ** 2).mean(axis=1)), rtol=0, atol=2e-6)


def test_cpu_policies_and_tables_run_extended_actors_through_the_interpreter(tmp_path):
    """On the CPU device MLPPolicy and the table's twin evaluate an extended actor with the interpreter: fp64 values, no fused path."""
    import torch
    files, specs = [], []
    for name in ("normaliser_clip_float4", "layernorm_before_and_after", "output_affine"):
        dims, spec = G.make_case(name)
        p = str(tmp_path / f"{name}.onnx")
        G.write_actor(p, spec)
        pol = MLPPolicy(p, device="cpu")
        assert pol._fused is None
        x = G.inputs(33, dims[0], seed=50)
        np.testing.assert_allclose(pol.get_action(x).numpy(), np.clip(G.ref_actor(x, spec), -1.0, 1.0), rtol=0, atol=2e-6)
        with pytest.raises(ValueError, match="fused=True"):
            MLPPolicy(p, device="cpu", fused=True)
    # a table of two extended files and a plain one of the same widths, on the CPU
    for k, (acts, extra) in enumerate(((["Elu", None], {}), (["Tanh", None], {"input": [("Sub", f32(np.arange(12) * 0.1)), ("Clip", (-2.0, 2.0))]}),
                                       (["Elu", "Tanh"], {"output": [("Mul", f32([0.5, 1.0, 1.5, 0.7]))]}))):
        spec = {"input": [], "ln0": None, "output": [], "layers": G.make_layers((12, 20, 4), acts, seed=60 + k, last_scale=0.5), **extra}
        if k == 2:
            spec["layers"][0]["ln"] = ("before", *_ln(20))
        files.append(str(tmp_path / f"t{k}.onnx"))
        G.write_actor(files[-1], spec)
        specs.append(spec)
    tab = PolicyTable(files, num_envs=10, device="cpu")
    x = G.inputs(10, 12, seed=61)
    got = tab.get_action(torch.as_tensor(x)).numpy()
    for k, spec in enumerate(specs):
        rows = np.nonzero(tab.policy_of_env == k)[0]
        np.testing.assert_allclose(got[rows], np.clip(G.ref_actor(x[rows], spec), -1.0, 1.0), rtol=0, atol=2e-6)
    # a file outside the grammar is refused with the file and the node
    G.decomposed_layernorm_actor(str(tmp_path / "decomposed.onnx"))
    with pytest.raises(ValueError, match=r"decomposed\.onnx: .*'ReduceMean'"):
        PolicyTable(files[:1] + [str(tmp_path / "decomposed.onnx")], num_envs=4, device="cpu")


# ------------------------------------------------------------------------------------------------------------------------- 5: the writer
def _write_random_mlp_before(path, state_dim, action_dim, hidden, seed, activation, bias_scale):
    """write_random_mlp as it was before the keywords: the untouched code path is write_onnx on the same nodes and initialisers."""
    rng, brng = np.random.default_rng(seed), np.random.default_rng([seed, 1])
    dims = [state_dim, *hidden, action_dim]
    nodes, init, x = [], {}, "obs"
    for li in range(len(dims) - 1):
        w = (rng.standard_normal((dims[li + 1], dims[li])) / np.sqrt(dims[li])).astype(f32)
        b = (bias_scale * brng.standard_normal(dims[li + 1])).astype(f32) if bias_scale else np.zeros(dims[li + 1], dtype=f32)
        init[f"w{li}"], init[f"b{li}"] = w, b
        y = f"h{li}" if li < len(dims) - 2 else "actions"
        nodes.append({"op": "Gemm", "inputs": [x, f"w{li}", f"b{li}"], "outputs": [y + "_lin" if li < len(dims) - 2 else y], "attrs": {"transB": 1}})
        if li < len(dims) - 2:
            nodes.append({"op": activation, "inputs": [y + "_lin"], "outputs": [y]})
        x = y
    write_onnx(path, nodes, init, ["obs"], ["actions"])


def test_writer_defaults_write_the_same_bytes_and_the_keywords_the_extras(tmp_path):
    for k, (hidden, seed, act, bs) in enumerate((((64, 32), 3, "Elu", 0.0), ((256, 128), 0, "Tanh", 0.5), ((), 7, "Relu", 0.0))):
        p, q = str(tmp_path / f"new{k}.onnx"), str(tmp_path / f"old{k}.onnx")
        write_random_mlp(p, state_dim=52, action_dim=4, hidden=hidden, seed=seed, activation=act, bias_scale=bs)
        _write_random_mlp_before(q, 52, 4, hidden, seed, act, bs)
        assert open(p, "rb").read() == open(q, "rb").read()
        write_random_mlp(p, state_dim=52, action_dim=4, hidden=hidden, seed=seed, activation=act, bias_scale=bs, normaliser=False, layer_norm=False, output_scale=None)
        assert open(p, "rb").read() == open(q, "rb").read()
    p, q = str(tmp_path / "ext.onnx"), str(tmp_path / "plain.onnx")
    write_random_mlp(p, 52, 4, hidden=(64, 32), seed=3, normaliser=True, layer_norm=True, output_scale=[0.5, 1.0, 1.5, 2.0])
    write_random_mlp(q, 52, 4, hidden=(64, 32), seed=3)
    d, why = _actor_graph(read_onnx(p))
    plain = _mlp_chain(read_onnx(q))
    assert why is None and [c for c, *_ in d["input"]] == [2, 4, 5] and d["input"][2][2:] == (-5.0, 5.0)
    assert set(d["ln"]) == {1, 2} and all(d["ln"][s][0] == 1 for s in (1, 2)) and [a for *_, a, _ in d["layers"]] == [3, 3, 2]
    assert [c for c, *_ in d["output"]] == [3] and np.array_equal(d["output"][0][1], f32([0.5, 1.0, 1.5, 2.0]))
    assert 0.5 <= d["input"][1][1].min() and d["input"][1][1].max() <= 2.0
    for (w, b, *_), (w2, b2, *_) in zip(d["layers"], plain):                    # the weights are the seed's, with or without the extras
        assert np.array_equal(w, w2) and np.array_equal(b, b2)


# ---------------------------------------------------------------------------------------------------------------------------- 6: the ABI
def test_actor_abi_rows_match_their_header():
    from cosim_amd.engine import ABI, ABI_ACTOR
    from cosim_amd.policy import _Extras
    hdr = open(os.path.join(ROOT, "include", "cosim_actor.h")).read()
    hdr = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    protos = {name: args.count(",") + 1 for name, args in re.findall(r"\b(cosim_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", hdr)}
    assert set(protos) == set(ABI_ACTOR) == {"cosim_mlp_forward_ex", "cosim_policy_table_create_ex"} and not set(ABI_ACTOR) & set(ABI)
    for name, n in protos.items():
        assert len(ABI_ACTOR[name][1]) == n and ABI_ACTOR[name][0] is ctypes.c_int, name
    assert len(ABI_ACTOR["cosim_mlp_forward_ex"][1]) == len(ABI["cosim_mlp_forward"][1]) + 1
    assert len(ABI_ACTOR["cosim_policy_table_create_ex"][1]) == len(ABI["cosim_policy_table_create"][1]) + 1
    # the struct: 10 ints, 8 pointers, 16 floats, 7 ints, 7 floats, 14 pointers, naturally aligned
    assert ctypes.sizeof(_Extras) == 40 + 64 + 64 + 28 + 28 + 112 and _Extras.in_vec.offset == 40 and _Extras.ln_gamma.offset == 224
