"""Extended actors for the tests of the fused actor grammar (``cosim_amd.policy._actor_graph``): a spec of one actor, the ONNX file
of it, its plain fp64 numpy evaluation, and the cases the GPU tests run.  No test lives here.

A spec is a dict: ``input`` / ``output`` -- stage items ``(op, constant)`` with op Add / Sub / Mul / Div, or ``("Clip", (lo, hi))`` (a bound
may be None); ``ln0`` -- LayerNorm on the observation ``(scale, bias or None, eps)`` or None; ``layers`` -- dicts ``w [O, I]``, ``b`` or
None, ``act``, ``alpha``, ``alpha_attr``, ``ln`` (None or ``(where, scale, bias or None, eps)`` with where "before" / "after" the activation),
``matmul`` (spell the layer as MatMul [+ Add])."""
import numpy as np

from cosim_amd.policy import write_onnx

ATOL = 2e-5
BATCHES = (1, 31, 32, 33, 65)


def act64(v, op, alpha):
    if op is None:
        return v
    if op == "Relu":
        return np.where(np.isnan(v), v, np.maximum(v, 0.0))
    if op == "Tanh":
        return np.tanh(v)
    if op == "Sigmoid":
        return 1.0 / (1.0 + np.exp(-v))
    if op == "Elu":
        return np.where(v > 0, v, alpha * (np.exp(np.minimum(v, 0.0)) - 1.0))
    if op == "LeakyRelu":
        return np.where(v > 0, v, alpha * v)
    raise AssertionError(op)


def ln64(h, g, b, eps):
    """LayerNormalization over the last axis in fp64: biased variance, eps as the fp32 attribute the file holds."""
    mean = h.mean(axis=-1, keepdims=True)
    var = ((h - mean) ** 2).mean(axis=-1, keepdims=True)
    y = (h - mean) / np.sqrt(var + float(np.float32(eps))) * g.astype(np.float64)
    return y if b is None else y + b.astype(np.float64)


def stage64(h, items):
    for op, c in items:
        if op == "Clip":
            lo, hi = c
            # np.clip propagates NaN, as the interpreter's clamp does
            h = np.clip(h, -np.inf if lo is None else float(np.float32(lo)), np.inf if hi is None else float(np.float32(hi)))
        else:
            c = np.asarray(c, np.float32).astype(np.float64)
            h = {"Add": h + c, "Sub": h - c, "Mul": h * c, "Div": h / c}[op]
    return h


def ref_actor(x, spec):
    """Unclipped fp64 output of the spec on ``x``."""
    h = np.asarray(x, dtype=np.float64)
    with np.errstate(all="ignore"):
        h = stage64(h, spec.get("input", ()))
        if spec.get("ln0") is not None:
            h = ln64(h, *spec["ln0"])
        for L in spec["layers"]:
            h = h @ L["w"].astype(np.float64).T
            if L["b"] is not None:
                h = h + L["b"].astype(np.float64)
            ln = L.get("ln")
            if ln is not None and ln[0] == "before":
                h = ln64(h, *ln[1:])
            h = act64(h, L["act"], L["alpha"])
            if ln is not None and ln[0] == "after":
                h = ln64(h, *ln[1:])
        h = stage64(h, spec.get("output", ()))
    return h


def make_layers(dims, acts, seed, last_scale=1.0, nobias=()):
    """The recipe of tests/test_gpu_policy_kernels.py: weights N(0, 1 / fan_in) (the last layer times ``last_scale``), biases 0.5 N(0, 1)."""
    rng = np.random.default_rng(seed)
    layers = []
    for li in range(len(dims) - 1):
        w = rng.standard_normal((dims[li + 1], dims[li])) / np.sqrt(dims[li])
        if li == len(dims) - 2:
            w = w * last_scale
        b = None if li in nobias else (0.5 * rng.standard_normal(dims[li + 1])).astype(np.float32)
        op = acts[li]
        layers.append({"w": w.astype(np.float32), "b": b, "act": op, "alpha": {"Elu": 1.0, "LeakyRelu": 0.01}.get(op, 1.0), "alpha_attr": None,
                       "ln": None, "matmul": False})
    return layers


def inputs(n, d, seed):
    """randn with row ``n // 2`` scaled by 10."""
    x = np.random.default_rng(seed).standard_normal((n, d)).astype(np.float32)
    x[n // 2] *= 10.0
    return x


def write_actor(path, spec, constant_nodes=False, add_left=False):
    """The spec as an ONNX file.  ``constant_nodes``: the stage constants come from Constant nodes, not initialisers (written by hand:
    write_onnx has no tensor attributes).  ``add_left``: Add / Mul items and MatMul biases take their constant as the FIRST operand."""
    nodes, init, x = [], {}, "obs"
    count = [0]

    def fresh(stem):
        count[0] += 1
        return f"{stem}{count[0]}"

    def stage(items, x):
        for op, c in items:
            y = fresh("s")
            if op == "Clip":
                ins = [x]
                for v, nm in ((c[0], "lo"), (c[1], "hi")):
                    if v is None:
                        ins.append("")
                    else:
                        k = fresh(nm)
                        init[k] = np.array(v, np.float32)
                        ins.append(k)
                while ins[-1] == "":
                    ins.pop()
                nodes.append({"op": "Clip", "inputs": ins, "outputs": [y]})
            else:
                k = fresh("c")
                init[k] = np.asarray(c, np.float32)
                nodes.append({"op": op, "inputs": [k, x] if add_left and op in ("Add", "Mul") else [x, k], "outputs": [y]})
            x = y
        return x

    def norm(x, g, b, eps):
        y, gk = fresh("n"), fresh("g")
        init[gk] = np.asarray(g, np.float32)
        ins = [x, gk]
        if b is not None:
            bk = fresh("beta")
            init[bk] = np.asarray(b, np.float32)
            ins.append(bk)
        nodes.append({"op": "LayerNormalization", "inputs": ins, "outputs": [y], "attrs": {"axis": -1, "epsilon": float(eps)}})
        return y

    x = stage(spec.get("input", ()), x)
    if spec.get("ln0") is not None:
        x = norm(x, *spec["ln0"])
    for li, L in enumerate(spec["layers"]):
        if L.get("matmul"):
            init[f"wt{li}"] = np.ascontiguousarray(L["w"].T)
            y = fresh("m")
            nodes.append({"op": "MatMul", "inputs": [x, f"wt{li}"], "outputs": [y]})
            x = y
            if L["b"] is not None:
                init[f"b{li}"] = L["b"]
                y = fresh("l")
                nodes.append({"op": "Add", "inputs": [f"b{li}", x] if add_left else [x, f"b{li}"], "outputs": [y]})
                x = y
        else:
            init[f"w{li}"] = L["w"]
            ins = [x, f"w{li}"]
            if L["b"] is not None:
                init[f"b{li}"] = L["b"]
                ins.append(f"b{li}")
            y = fresh("l")
            nodes.append({"op": "Gemm", "inputs": ins, "outputs": [y], "attrs": {"transB": 1}})
            x = y
        ln = L.get("ln")
        if ln is not None and ln[0] == "before":
            x = norm(x, *ln[1:])
        if L["act"] is not None:
            y = fresh("h")
            nodes.append({"op": L["act"], "inputs": [x], "outputs": [y], "attrs": {} if L["alpha_attr"] is None else {"alpha": float(L["alpha_attr"])}})
            x = y
        if ln is not None and ln[0] == "after":
            x = norm(x, *ln[1:])
    x = stage(spec.get("output", ()), x)
    # the last node writes the graph output
    last = nodes[-1]["outputs"][0]
    nodes[-1]["outputs"][0] = "actions"
    assert all(last not in n["inputs"] for n in nodes)
    if constant_nodes:
        return _write_with_constant_nodes(path, nodes, init)
    write_onnx(path, nodes, init, ["obs"], ["actions"])


def _write_with_constant_nodes(path, nodes, init):
    """As write_onnx, with every stage constant (names c*, lo*, hi*) as a Constant node ahead of the others."""
    import os
    import struct
    from cosim_amd.policy import _enc

    def tensor(name, a):
        a = np.ascontiguousarray(a, np.float32)
        return b"".join(_enc(1, 0, int(d)) for d in a.shape) + _enc(2, 0, 1) + _enc(8, 2, name.encode()) + _enc(9, 2, a.tobytes())

    def node(n, extra=b""):
        nb = b"".join(_enc(1, 2, i.encode()) for i in n["inputs"]) + b"".join(_enc(2, 2, o.encode()) for o in n["outputs"]) + _enc(4, 2, n["op"].encode())
        for k, v in n.get("attrs", {}).items():
            ab = _enc(1, 2, k.encode())
            ab += (_enc(2, 5, struct.pack("<f", v)) + _enc(20, 0, 1)) if isinstance(v, float) else (_enc(3, 0, v) + _enc(20, 0, 2))
            nb += _enc(5, 2, ab)
        return _enc(1, 2, nb + extra)

    consts = {k: v for k, v in init.items() if k[0] == "c" or k[:2] in ("lo", "hi")}
    g = b""
    for k, v in consts.items():
        value = _enc(1, 2, b"value") + _enc(5, 2, tensor("", v)) + _enc(20, 0, 4)
        g += node({"op": "Constant", "inputs": [], "outputs": [k]}, _enc(5, 2, value))
    g += b"".join(node(n) for n in nodes)
    g += b"".join(_enc(5, 2, tensor(k, v)) for k, v in init.items() if k not in consts)
    g += _enc(11, 2, _enc(1, 2, b"obs")) + _enc(12, 2, _enc(1, 2, b"actions"))
    with open(os.fspath(path), "wb") as f:
        f.write(_enc(1, 0, 8) + _enc(7, 2, g))


# ---------------------------------------------------------------------------------------------- the cases of the GPU tests
# name -> (dims, acts, last-layer scale).  The scale keeps at least half of the fp64 outputs strictly inside (-1, 1) at every batch
# size (asserted by the tests): 0.5, but at n = 1 the only row is the one scaled by 10, and ``normaliser`` and ``matmul_add`` need less.
CASES = {
    "normaliser": ((7, 33, 3), ["Elu", None], 0.2),
    "normaliser_clip_float4": ((12, 40, 36, 4), ["Elu", "Tanh", None], 0.5),
    "layernorm_before_and_after": ((9, 34, 31, 2), ["Elu", "Tanh", None], 0.5),
    "layernorm_on_obs": ((6, 40, 3), ["Relu", None], 0.5),
    "matmul_add": ((5, 33, 3), ["Elu", None], 0.05),
    "output_affine": ((7, 12, 3), ["Elu", "Tanh"], 0.5),
    "all_widest": ((512, 512, 33, 1), ["Elu", "Tanh", None], 0.5),
}


def make_case(name):
    """(dims, spec) of one case; the extras come from a generator of their own, so the weights are the recipe's."""
    dims, acts, last_scale = CASES[name]
    seed = sum(map(ord, name))
    spec = {"input": [], "ln0": None, "output": [], "layers": make_layers(dims, acts, seed, last_scale, nobias=(1,) if name == "matmul_add" else ())}
    rng = np.random.default_rng([seed, 7])
    N, U = rng.standard_normal, rng.uniform

    def f32(a):
        return np.asarray(a, np.float32)

    def normaliser(clip):
        spec["input"] = [("Sub", f32(0.5 * N(dims[0]))), ("Div", f32(U(0.5, 2.0, dims[0])))] + ([("Clip", (-5.0, 5.0))] if clip else [])

    def ln(width):
        return f32(1.0 + 0.3 * N(width)), f32(0.2 * N(width)), 1e-5

    if name == "normaliser":
        normaliser(False)
    elif name == "normaliser_clip_float4":
        normaliser(True)
    elif name == "layernorm_before_and_after":
        spec["layers"][0]["ln"] = ("before", *ln(dims[1]))
        spec["layers"][1]["ln"] = ("after", *ln(dims[2]))
    elif name == "layernorm_on_obs":
        spec["ln0"] = ln(dims[0])
    elif name == "matmul_add":
        for L in spec["layers"]:
            L["matmul"] = True
    elif name == "output_affine":
        spec["output"] = [("Mul", f32(U(0.5, 1.5, dims[-1]))), ("Add", f32(0.2 * N(dims[-1]))), ("Clip", (-0.8, 0.9))]
    elif name == "all_widest":
        normaliser(True)
        spec["layers"][0]["ln"] = ("before", *ln(dims[1]))
        spec["layers"][1]["ln"] = ("before", *ln(dims[2]))
        spec["output"] = [("Mul", f32(U(0.5, 1.5, dims[-1]))), ("Add", f32(0.2 * N(dims[-1])))]
    else:
        raise AssertionError(name)
    return dims, spec


def decomposed_layernorm_actor(path, seed=5):
    """Gemm -> LayerNorm spelled ReduceMean / Sub / Pow / ReduceMean / Add / Sqrt / Div / Mul / Add -> Tanh -> Gemm: outside the fused
    grammar.  Returns the equivalent spec (for ref_actor)."""
    dims = (7, 12, 3)
    layers = make_layers(dims, ["Tanh", None], seed, last_scale=0.5)
    rng = np.random.default_rng([seed, 7])
    g, b = (1.0 + 0.3 * rng.standard_normal(12)).astype(np.float32), (0.2 * rng.standard_normal(12)).astype(np.float32)
    layers[0]["ln"] = ("before", g, b, 1e-5)
    init = {"w0": layers[0]["w"], "b0": layers[0]["b"], "w1": layers[1]["w"], "b1": layers[1]["b"], "g": g, "beta": b,
            "two": np.array(2.0, np.float32), "eps": np.array(1e-5, np.float32)}
    nodes = [{"op": "Gemm", "inputs": ["obs", "w0", "b0"], "outputs": ["l0"], "attrs": {"transB": 1}},
             {"op": "ReduceMean", "inputs": ["l0"], "outputs": ["mu"], "attrs": {"axes": [-1], "keepdims": 1}},
             {"op": "Sub", "inputs": ["l0", "mu"], "outputs": ["d"]},
             {"op": "Pow", "inputs": ["d", "two"], "outputs": ["d2"]},
             {"op": "ReduceMean", "inputs": ["d2"], "outputs": ["var"], "attrs": {"axes": [-1], "keepdims": 1}},
             {"op": "Add", "inputs": ["var", "eps"], "outputs": ["ve"]},
             {"op": "Sqrt", "inputs": ["ve"], "outputs": ["sd"]},
             {"op": "Div", "inputs": ["d", "sd"], "outputs": ["nrm"]},
             {"op": "Mul", "inputs": ["nrm", "g"], "outputs": ["sc"]},
             {"op": "Add", "inputs": ["sc", "beta"], "outputs": ["ln"]},
             {"op": "Tanh", "inputs": ["ln"], "outputs": ["h0"]},
             {"op": "Gemm", "inputs": ["h0", "w1", "b1"], "outputs": ["actions"], "attrs": {"transB": 1}}]
    write_onnx(path, nodes, init, ["obs"], ["actions"])
    return dims, {"layers": layers}
