"""ONNX files without the ``onnx`` package or onnxruntime (neither is available in this build): a small protobuf wire-format decoder
(``read_onnx``), a tiny interpreter over the operator subset RL policy exports use (``OnnxGraph``: Gemm / MatMul / elementwise / activations /
LayerNormalization and its ReduceMean / Pow / Sqrt spelling / LSTM / shape glue, on torch tensors) and the writer the tests and the synthetic policies use (``write_onnx``, ``write_random_mlp``,
``write_random_lstm``, ``write_recurrent_actor``).  ``policy.py`` builds the policies and the tables on top of it and re-exports
every name of this module that was imported from there.
"""
from __future__ import annotations

import struct
from typing import Dict, List

import numpy as np

# ---------------------------------------------------------------------------------------------- protobuf wire format
_DT = {1: np.float32, 6: np.int32, 7: np.int64, 10: np.float16, 11: np.float64}


def _varint(b: bytes, i: int):
    r, s = 0, 0
    while True:
        c = b[i]
        i += 1
        r |= (c & 0x7F) << s
        if c < 0x80:
            return r, i
        s += 7


def _fields(b: bytes):
    """(field number, wire type, value) over one message; length-delimited values come back as bytes."""
    i, n = 0, len(b)
    while i < n:
        key, i = _varint(b, i)
        f, w = key >> 3, key & 7
        if w == 0:
            v, i = _varint(b, i)
        elif w == 1:
            v, i = b[i:i + 8], i + 8
        elif w == 2:
            ln, i = _varint(b, i)
            v, i = b[i:i + ln], i + ln
        elif w == 5:
            v, i = b[i:i + 4], i + 4
        else:
            raise ValueError(f"unsupported protobuf wire type {w}")
        yield f, w, v


def _packed_varints(v) -> List[int]:
    if isinstance(v, int):
        return [v]
    out, i = [], 0
    while i < len(v):
        x, i = _varint(v, i)
        out.append(x)
    return out


def _signed(x: int) -> int:
    return x - (1 << 64) if x >= (1 << 63) else x


def _tensor(b: bytes):
    dims, dt, name, raw, fdata, idata = [], 1, "", None, [], []
    for f, w, v in _fields(b):
        if f == 1:
            dims += [_signed(x) for x in _packed_varints(v)]
        elif f == 2:
            dt = v
        elif f == 8:
            name = v.decode()
        elif f == 9:
            raw = v
        elif f == 4:
            fdata.append(np.frombuffer(v, dtype="<f4") if w == 2 else np.frombuffer(v, dtype="<f4", count=1))
        elif f == 7:
            idata += [_signed(x) for x in _packed_varints(v)]
    if dt not in _DT:
        raise NotImplementedError(f"ONNX tensor data type {dt} ({name})")
    if raw is not None:
        a = np.frombuffer(raw, dtype=np.dtype(_DT[dt]).newbyteorder("<"))
    elif fdata:
        a = np.concatenate(fdata)
    else:
        a = np.asarray(idata, dtype=_DT[dt])
    return name, a.astype(_DT[dt]).reshape(dims)


def _attribute(b: bytes):
    name, val, ints, floats = "", None, [], []
    for f, w, v in _fields(b):
        if f == 1:
            name = v.decode()
        elif f == 2:
            val = struct.unpack("<f", v)[0]
        elif f == 3:
            val = _signed(v)
        elif f == 4:
            val = v.decode(errors="replace")
        elif f == 5:
            val = _tensor(v)[1]
        elif f == 7:
            floats += list(np.frombuffer(v, dtype="<f4")) if w == 2 else [struct.unpack("<f", v)[0]]
        elif f == 8:
            ints += [_signed(x) for x in _packed_varints(v)]
    if ints:
        val = ints
    elif floats:
        val = floats
    return name, val


def read_onnx(path: str) -> dict:
    """ModelProto -> {"nodes": [{op, inputs, outputs, attrs}], "init": {name: ndarray}, "inputs": [...], "outputs": [...]}."""
    data = open(path, "rb").read()
    graph = None
    for f, w, v in _fields(data):
        if f == 7:
            graph = v
    if graph is None:
        raise ValueError(f"{path}: no graph in the ONNX model")
    nodes, init, inputs, outputs = [], {}, [], []
    for f, w, v in _fields(graph):
        if f == 1:
            n = {"op": "", "inputs": [], "outputs": [], "attrs": {}}
            for g, _, x in _fields(v):
                if g == 1:
                    n["inputs"].append(x.decode())
                elif g == 2:
                    n["outputs"].append(x.decode())
                elif g == 4:
                    n["op"] = x.decode()
                elif g == 5:
                    k, a = _attribute(x)
                    n["attrs"][k] = a
            nodes.append(n)
        elif f == 5:
            k, a = _tensor(v)
            init[k] = a
        elif f in (11, 12):
            name = next((x.decode() for g, _, x in _fields(v) if g == 1), "")
            (inputs if f == 11 else outputs).append(name)
    return {"nodes": nodes, "init": init, "inputs": [i for i in inputs if i not in init], "outputs": outputs}


# ---------------------------------------------------------------------------------------------- graph interpreter
class OnnxGraph:
    """Runs the operator subset of RL policy exports on torch tensors (weights resident on ``device``)."""

    def __init__(self, model: dict, device):
        import torch
        self.torch, self.device = torch, device
        self.nodes, self.inputs, self.outputs = model["nodes"], model["inputs"], model["outputs"]
        # fp16 / fp64 initialisers (exports of half- or double-precision checkpoints) are cast to fp32 on load: every op below runs in fp32
        self.const = {k: torch.as_tensor(np.ascontiguousarray(v.astype(np.float32) if v.dtype in (np.float16, np.float64) else v), device=device)
                      for k, v in model["init"].items()}

    def run(self, feeds: Dict[str, "object"]) -> List["object"]:
        t = self.torch
        env = dict(self.const)
        env.update(feeds)
        for n in self.nodes:
            x = [env[i] if i else None for i in n["inputs"]]
            a, op = n["attrs"], n["op"]
            if op == "Gemm":
                A = x[0].transpose(-1, -2) if a.get("transA", 0) else x[0]
                B = x[1].transpose(-1, -2) if a.get("transB", 0) else x[1]
                al, be = a.get("alpha", 1.0), a.get("beta", 1.0)
                if len(x) > 2 and x[2] is not None and A.dim() == 2 and x[2].dim() <= 2:
                    y = t.addmm(x[2], A, B, beta=be, alpha=al)      # one library GEMM with the bias folded in
                else:
                    y = al * (A @ B)
                    if len(x) > 2 and x[2] is not None:
                        y = y + be * x[2]
            elif op == "MatMul":
                y = x[0] @ x[1]
            elif op in ("Add", "Sub", "Mul", "Div"):
                y = {"Add": t.add, "Sub": t.sub, "Mul": t.mul, "Div": t.div}[op](x[0], x[1])
            elif op == "Relu":
                y = t.relu(x[0])
            elif op == "Tanh":
                y = t.tanh(x[0])
            elif op == "Sigmoid":
                y = t.sigmoid(x[0])
            elif op == "Elu":
                y = t.nn.functional.elu(x[0], alpha=a.get("alpha", 1.0))
            elif op == "LeakyRelu":
                y = t.nn.functional.leaky_relu(x[0], negative_slope=a.get("alpha", 0.01))
            elif op == "Softplus":
                y = t.nn.functional.softplus(x[0])
            elif op == "Identity":
                y = x[0]
            elif op == "Clip":
                lo = x[1] if len(x) > 1 and x[1] is not None else a.get("min")
                hi = x[2] if len(x) > 2 and x[2] is not None else a.get("max")
                y = t.clamp(x[0], min=None if lo is None else float(lo), max=None if hi is None else float(hi))
            elif op == "LayerNormalization":
                ax = a.get("axis", -1) % x[0].dim()
                y = t.nn.functional.layer_norm(x[0], tuple(x[0].shape[ax:]), x[1], x[2] if len(x) > 2 else None, float(a.get("epsilon", 1e-5)))
            elif op == "ReduceMean":
                axes = a.get("axes")
                if axes is None and len(x) > 1 and x[1] is not None:
                    axes = [int(v) for v in x[1].tolist()]
                keep = bool(a.get("keepdims", 1))
                y = x[0].mean(dim=tuple(axes) if axes else tuple(range(x[0].dim())), keepdim=keep)
            elif op == "Pow":
                y = t.pow(x[0], x[1])
            elif op == "Sqrt":
                y = t.sqrt(x[0])
            elif op == "Flatten":
                ax = a.get("axis", 1)
                y = x[0].reshape(int(np.prod(x[0].shape[:ax])) if ax else 1, -1)
            elif op == "Concat":
                y = t.cat(x, dim=a.get("axis", 0))
            elif op in ("Squeeze", "Unsqueeze"):
                axes = a.get("axes")
                if axes is None:
                    axes = [int(v) for v in x[1].tolist()] if len(x) > 1 and x[1] is not None else None
                y = x[0]
                if op == "Squeeze":
                    for ax in sorted([ax % y.dim() for ax in axes], reverse=True) if axes is not None else []:
                        y = y.squeeze(ax)
                    if axes is None:
                        y = y.squeeze()
                else:
                    for ax in sorted(axes):
                        y = y.unsqueeze(ax)
            elif op == "Reshape":
                shape = [int(v) for v in x[1].tolist()]
                shape = [x[0].shape[i] if s == 0 else s for i, s in enumerate(shape)]
                y = x[0].reshape(shape)
            elif op == "Transpose":
                y = x[0].permute(a["perm"]) if "perm" in a else x[0].permute(*reversed(range(x[0].dim())))
            elif op == "Constant":
                y = t.as_tensor(np.ascontiguousarray(a["value"]), device=self.device)
            elif op == "LSTM":
                outs = self._lstm(x, a)
                for name, val in zip(n["outputs"], outs):
                    if name:
                        env[name] = val
                continue
            else:
                raise NotImplementedError(f"ONNX operator '{op}' is not in the policy subset of cosim_amd.policy")
            env[n["outputs"][0]] = y
        return [env[o] for o in self.outputs]

    def _lstm(self, x, a):
        """ONNX LSTM, one direction, default activations: X [T,B,I], W [1,4H,I] (i o f c), R [1,4H,H], B [1,8H]."""
        t = self.torch
        if a.get("direction", "forward") != "forward" or a.get("layout", 0):
            raise NotImplementedError("LSTM: only direction=forward, layout=0")
        X, W, R = x[0], x[1][0], x[2][0]
        H = R.shape[1]
        Bv = x[3][0] if len(x) > 3 and x[3] is not None else t.zeros(8 * H, device=X.device)
        h = x[5][0] if len(x) > 5 and x[5] is not None else t.zeros((X.shape[1], H), device=X.device)
        c = x[6][0] if len(x) > 6 and x[6] is not None else t.zeros((X.shape[1], H), device=X.device)
        if X.is_cuda and X.shape[0] == 1 and X.dtype == t.float32:
            # one step for all envs: the engine's fused cell (gates on the matrix pipe + activations, one launch)
            out = self._lstm_cell_hip(X[0], h, c, W, R, Bv)
            if out is not None:
                hn, cn = out
                return hn.unsqueeze(0).unsqueeze(1), hn.unsqueeze(0), cn.unsqueeze(0)
        bias = Bv[:4 * H] + Bv[4 * H:]
        ys = []
        for s in range(X.shape[0]):
            g = X[s] @ W.T + h @ R.T + bias
            i, o, f, cc = g[:, :H], g[:, H:2 * H], g[:, 2 * H:3 * H], g[:, 3 * H:]
            c = t.sigmoid(f) * c + t.sigmoid(i) * t.tanh(cc)
            h = t.sigmoid(o) * t.tanh(c)
            ys.append(h)
        return t.stack(ys).unsqueeze(1), h.unsqueeze(0), c.unsqueeze(0)

    _lstm_lib = None      # None: not asked for yet; False: the library is not available; else the library

    def _lstm_cell_hip(self, x, h, c, W, R, Bv):
        """``cosim_lstm_cell`` (csrc/cosim_mlp.hip): None when the library is not available (the interpreter's own ops then run)."""
        t = self.torch
        if self._lstm_lib is None:
            try:
                from .engine import load_library
                self._lstm_lib = load_library()
            except Exception:  # noqa: BLE001
                self._lstm_lib = False
        if not self._lstm_lib:
            return None
        x, h, c, W, R, Bv = (a.contiguous() for a in (x, h, c, W, R, Bv))
        hn, cn = t.empty_like(h), t.empty_like(c)
        rc = self._lstm_lib.cosim_lstm_cell(x.data_ptr(), h.data_ptr(), c.data_ptr(), x.shape[0], x.shape[1], h.shape[1], W.data_ptr(), R.data_ptr(),
                                            Bv.data_ptr(), hn.data_ptr(), cn.data_ptr(), t.cuda.current_stream(x.device).cuda_stream)
        if rc == -1:      # COSIM_EINVAL: a shape the fused cell does not take (in_dim + hidden > 1200): the interpreter's own ops run
            return None
        if rc != 0:
            raise RuntimeError(self._lstm_lib.cosim_last_error().decode())
        return hn, cn


# ---------------------------------------------------------------------------------------------- writer (tests / synthetic policies)
def _enc_varint(x: int) -> bytes:
    x &= (1 << 64) - 1
    out = bytearray()
    while True:
        c = x & 0x7F
        x >>= 7
        out.append(c | (0x80 if x else 0))
        if not x:
            return bytes(out)


def _enc(field: int, wire: int, payload) -> bytes:
    key = _enc_varint((field << 3) | wire)
    if wire == 0:
        return key + _enc_varint(payload)
    if wire == 2:
        return key + _enc_varint(len(payload)) + payload
    return key + payload


def write_onnx(path: str, nodes: List[dict], init: Dict[str, np.ndarray], inputs: List[str], outputs: List[str]):
    """Minimal ONNX writer for the same subset (no policy ships with the reference: synthetic policies and the tests use it)."""
    def tensor(name, a):
        a = np.ascontiguousarray(a)
        dt = {np.dtype(np.float32): 1, np.dtype(np.int64): 7}[a.dtype]
        return b"".join(_enc(1, 0, int(d)) for d in a.shape) + _enc(2, 0, dt) + _enc(8, 2, name.encode()) + _enc(9, 2, a.tobytes())

    def attr(k, v):
        b = _enc(1, 2, k.encode())
        if isinstance(v, float):
            return b + _enc(2, 5, struct.pack("<f", v)) + _enc(20, 0, 1)
        if isinstance(v, int):
            return b + _enc(3, 0, v) + _enc(20, 0, 2)
        if isinstance(v, str):
            return b + _enc(4, 2, v.encode()) + _enc(20, 0, 3)
        return b + b"".join(_enc(8, 0, int(x)) for x in v) + _enc(20, 0, 7)

    g = b""
    for n in nodes:
        nb = b"".join(_enc(1, 2, i.encode()) for i in n["inputs"]) + b"".join(_enc(2, 2, o.encode()) for o in n["outputs"])
        nb += _enc(4, 2, n["op"].encode()) + b"".join(_enc(5, 2, attr(k, v)) for k, v in n.get("attrs", {}).items())
        g += _enc(1, 2, nb)
    g += _enc(2, 2, b"cosim_amd_policy")
    for k, a in init.items():
        g += _enc(5, 2, tensor(k, a))
    for name in inputs:
        g += _enc(11, 2, _enc(1, 2, name.encode()))
    for name in outputs:
        g += _enc(12, 2, _enc(1, 2, name.encode()))
    model = _enc(1, 0, 8) + _enc(7, 2, g) + _enc(8, 2, _enc(2, 0, 17))
    with open(path, "wb") as f:
        f.write(model)


def write_recurrent_actor(path: str, enc, lstm, head, read: str = "Y_h"):
    """A recurrent actor of the shape ``_recurrent_actor`` recognises and ``LSTMPolicy`` runs.  ``enc`` / ``head``: layers
    ``(w [O, I], b [O] or None, op or None, alpha)``; ``lstm``: ``(W [4H, I], R [4H, H], B [8H] or None)``; ``read``: the LSTM output
    the head takes, ``"Y_h"`` or ``"Y"``."""
    nodes, init = [], {}

    def chain(layers, x, tag, last_name=None):
        for li, (w, b, op, alpha) in enumerate(layers):
            init[f"{tag}w{li}"] = np.asarray(w, np.float32)
            ins = [x, f"{tag}w{li}"]
            if b is not None:
                init[f"{tag}b{li}"] = np.asarray(b, np.float32)
                ins.append(f"{tag}b{li}")
            last = last_name is not None and li == len(layers) - 1
            lin = last_name if last and op is None else f"{tag}lin{li}"
            nodes.append({"op": "Gemm", "inputs": ins, "outputs": [lin], "attrs": {"transB": 1}})
            x = lin
            if op is not None:
                x = last_name if last else f"{tag}a{li}"
                nodes.append({"op": op, "inputs": [lin], "outputs": [x], "attrs": {"alpha": float(alpha)} if op in ("Elu", "LeakyRelu") else {}})
        return x
    x = chain(enc, "obs", "e")
    W, R, B = lstm
    H = R.shape[1]
    init["W"], init["R"] = np.asarray(W, np.float32)[None], np.asarray(R, np.float32)[None]
    if B is not None:
        init["B"] = np.asarray(B, np.float32)[None]
    nodes.append({"op": "Unsqueeze", "inputs": [x], "outputs": ["x3"], "attrs": {"axes": [0]}})
    nodes.append({"op": "LSTM", "inputs": ["x3", "W", "R", "B" if B is not None else "", "", "h_in", "c_in"], "outputs": ["Y", "h_out", "c_out"],
                  "attrs": {"hidden_size": int(H)}})
    nodes.append({"op": "Squeeze", "inputs": ["Y" if read == "Y" else "h_out"], "outputs": ["hs"], "attrs": {"axes": [0, 1] if read == "Y" else [0]}})
    chain(head, "hs", "h", last_name="actions")
    write_onnx(path, nodes, init, ["obs", "h_in", "c_in"], ["actions", "h_out", "c_out"])


def write_random_lstm(path: str, state_dim: int, action_dim: int, hidden: int = 256, encoder=(), head=(128,), seed: int = 0,
                      activation: str = "Elu", bias_scale: float = 0.0):
    """A random-weight recurrent actor (``encoder`` widths -> LSTM(``hidden``) -> ``head`` widths -> action): the recurrent
    counterpart of ``write_random_mlp``.  Weights N(0, 1 / fan_in); biases ``bias_scale * standard_normal`` (0: none but zeros)."""
    rng = np.random.default_rng([seed, 2])

    def layers(dims, act_last):
        out = []
        for li in range(len(dims) - 1):
            w = (rng.standard_normal((dims[li + 1], dims[li])) / np.sqrt(dims[li])).astype(np.float32)
            b = (bias_scale * rng.standard_normal(dims[li + 1])).astype(np.float32)
            out.append((w, b, activation if (act_last or li < len(dims) - 2) else None, 1.0))
        return out
    enc = layers([state_dim, *encoder], True)
    I = encoder[-1] if encoder else state_dim
    W = (rng.standard_normal((4 * hidden, I)) / np.sqrt(I)).astype(np.float32)
    R = (rng.standard_normal((4 * hidden, hidden)) / np.sqrt(hidden)).astype(np.float32)
    B = (bias_scale * rng.standard_normal(8 * hidden)).astype(np.float32)
    write_recurrent_actor(path, enc, (W, R, B), layers([hidden, *head, action_dim], False))


def write_random_mlp(path: str, state_dim: int, action_dim: int, hidden=(256, 128), seed: int = 0, activation: str = "Elu",
                     bias_scale: float = 0.0, normaliser: bool = False, layer_norm: bool = False, output_scale=None):
    """A random-weight actor with the usual export shape (Gemm + activation ... Gemm): stands in for the missing policy files.
    Biases are ``bias_scale * standard_normal`` from a generator of their own: the default 0 writes all-zero biases and exactly the
    weights (and bytes) earlier versions wrote for the same seed.

    What trained actors carry besides (``_actor_graph``), each from a generator of its own, so the weights stay those of the seed and
    the defaults write the bytes they always did: ``normaliser`` -- ``Clip((obs - mean) / std, -5, 5)`` ahead of the first layer (mean
    N(0, 1), std uniform in [0.5, 2]); ``layer_norm`` -- ``LayerNormalization`` between every hidden Gemm and its activation (scale 1 +
    0.3 N, bias 0.2 N); ``output_scale`` (a number or one per action) -- ``Tanh`` then ``Mul`` behind the last Gemm."""
    rng = np.random.default_rng(seed)
    brng = np.random.default_rng([seed, 1])
    dims = [state_dim, *hidden, action_dim]
    nodes, init, x = [], {}, "obs"
    if normaliser:
        nrng = np.random.default_rng([seed, 3])
        init["obs_mean"] = nrng.standard_normal(state_dim).astype(np.float32)
        init["obs_std"] = nrng.uniform(0.5, 2.0, state_dim).astype(np.float32)
        init["obs_lo"], init["obs_hi"] = np.array(-5.0, np.float32), np.array(5.0, np.float32)
        nodes += [{"op": "Sub", "inputs": ["obs", "obs_mean"], "outputs": ["obs_c"]}, {"op": "Div", "inputs": ["obs_c", "obs_std"], "outputs": ["obs_n"]},
                  {"op": "Clip", "inputs": ["obs_n", "obs_lo", "obs_hi"], "outputs": ["obs_k"]}]
        x = "obs_k"
    lrng = np.random.default_rng([seed, 4])
    for li in range(len(dims) - 1):
        w = (rng.standard_normal((dims[li + 1], dims[li])) / np.sqrt(dims[li])).astype(np.float32)
        b = (bias_scale * brng.standard_normal(dims[li + 1])).astype(np.float32) if bias_scale else np.zeros(dims[li + 1], dtype=np.float32)
        init[f"w{li}"], init[f"b{li}"] = w, b
        hidden_layer = li < len(dims) - 2
        y = f"h{li}" if hidden_layer else "actions"
        lin = y + "_lin" if hidden_layer or output_scale is not None else y
        nodes.append({"op": "Gemm", "inputs": [x, f"w{li}", f"b{li}"], "outputs": [lin], "attrs": {"transB": 1}})
        if hidden_layer:
            if layer_norm:
                init[f"g{li}"] = (1.0 + 0.3 * lrng.standard_normal(dims[li + 1])).astype(np.float32)
                init[f"beta{li}"] = (0.2 * lrng.standard_normal(dims[li + 1])).astype(np.float32)
                nodes.append({"op": "LayerNormalization", "inputs": [lin, f"g{li}", f"beta{li}"], "outputs": [y + "_ln"], "attrs": {"axis": -1, "epsilon": 1e-5}})
                lin = y + "_ln"
            nodes.append({"op": activation, "inputs": [lin], "outputs": [y]})
        elif output_scale is not None:
            init["action_scale"] = np.broadcast_to(np.asarray(output_scale, np.float32), (action_dim,)).copy()
            nodes += [{"op": "Tanh", "inputs": [lin], "outputs": ["actions_t"]}, {"op": "Mul", "inputs": ["actions_t", "action_scale"], "outputs": [y]}]
        x = y
    write_onnx(path, nodes, init, ["obs"], ["actions"])
