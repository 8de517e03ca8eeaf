"""Batched on-device policies: the counterpart of the reference's ``core/policy.py:5-54`` for N environments.

The reference runs an ONNX file through onnxruntime on the CPU, one state at a time (``MLPPolicy.get_action`` :11-21,
``LSTMPolicy.get_action`` :34-47, ``build_policy`` :49-53).  Here the same contract — ``get_action(state) -> action``
clipped to [-1, 1], LSTM ``h``/``c`` carried between calls — is kept over ``[N, state_dim]`` device tensors, so the
rollout loop never leaves the GPU.  onnxruntime and the ``onnx`` package are not available in this
build, so the file is read with a small protobuf wire-format decoder (``read_onnx``) and the graph is run by a tiny
interpreter over the operator subset RL policy exports use (Gemm / MatMul / Add / activations / LSTM / shape glue).
The GEMMs go through torch (rocBLAS / hipBLASLt): plain library matrix products, not part of the §8 hot path.

Two rules the tests pin.  Non-finite values: a NaN that reaches the output stays NaN on both paths (the interpreter's ``clamp``, like
the reference's ``np.clip``, propagates it; the fused kernel's Relu and final clip do the same), +-inf is clipped to +-1, and a bad
row never touches another row.  Initialisers stored as fp16 or fp64 are cast to fp32 when the graph is loaded (such a graph runs
through the interpreter; the fused kernel takes fp32 files only).

PARITY UNPINNED against onnxruntime (no policy file ships with the reference; onnxruntime is absent): the
tests compare with a numpy evaluation of the same graph.
"""
from __future__ import annotations

import os
import struct
from typing import Dict, List, Optional

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


def _lstm_cell_hip(self, x, h, c, W, R, Bv):
    """``cosim_lstm_cell`` (csrc/cosim_mlp.hip): None when the library is not available (the interpreter's own ops then run)."""
    import ctypes
    t = self.torch
    if getattr(self, "_lstm_lib", None) is None:
        try:
            from .engine import load_library
            L = load_library()
            L.cosim_lstm_cell.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_int] * 3 + [ctypes.c_void_p] * 6
            L.cosim_lstm_cell.restype = ctypes.c_int
            L.cosim_last_error.restype = ctypes.c_char_p
            self._lstm_lib = L
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


OnnxGraph._lstm_cell_hip = _lstm_cell_hip


# ---------------------------------------------------------------------------------------------- the reference's classes, batched
_ACT = {"Relu": 1, "Tanh": 2, "Elu": 3, "Sigmoid": 4, "LeakyRelu": 5}


def _gemm_layers(nodes, i: int, cur: str, init: dict, src=lambda name: name):
    """The Gemm(transB=1, alpha=beta=1) [+ activation] layers that follow one another from ``nodes[i]`` on, the first fed by ``cur``:
    ``(layers, cur, i)`` with ``i`` the first node that is not of that shape.  ``src(name)``: the tensor a name stands for."""
    layers = []
    while i < len(nodes):
        n = nodes[i]
        a = n["attrs"]
        if n["op"] != "Gemm" or src(n["inputs"][0]) != cur or a.get("transB", 0) != 1 or a.get("transA", 0) or \
                a.get("alpha", 1.0) != 1.0 or a.get("beta", 1.0) != 1.0 or n["inputs"][1] not in init:
            break
        w = init[n["inputs"][1]]
        b = init.get(n["inputs"][2]) if len(n["inputs"]) > 2 and n["inputs"][2] else None
        if w.ndim != 2 or w.dtype != np.float32 or (b is not None and (b.shape != (w.shape[0],) or b.dtype != np.float32)):
            break
        cur, act, alpha = n["outputs"][0], 0, 1.0
        i += 1
        if i < len(nodes) and nodes[i]["op"] in _ACT and [src(x) for x in nodes[i]["inputs"]] == [cur]:
            act = _ACT[nodes[i]["op"]]
            alpha = float(nodes[i]["attrs"].get("alpha", 1.0 if act == 3 else 0.01))
            cur = nodes[i]["outputs"][0]
            i += 1
        layers.append((w, b, act, alpha))
    return layers, cur, i


def _mlp_chain(model: dict):
    """The graph as a plain actor MLP -- Gemm(transB=1, alpha=beta=1) [+ activation] ... -- or None if it is anything else."""
    nodes = model["nodes"]
    if len(model["inputs"]) != 1 or len(model["outputs"]) != 1:
        return None
    layers, cur, i = _gemm_layers(nodes, 0, model["inputs"][0], model["init"])
    if i != len(nodes) or cur != model["outputs"][0] or not 1 <= len(layers) <= 6 or any(max(w.shape) > 512 for w, *_ in layers):
        return None
    return layers


_SHAPE_ONLY = ("Unsqueeze", "Squeeze", "Reshape", "Identity")


def _recurrent_actor(model: dict):
    """The graph as a recurrent actor: inputs (obs, "h_in", "c_in"), outputs (action, h_out, c_out); 0..3 Gemm / activation layers on
    ``obs``, ONE LSTM node (forward, layout 0, default activations, one step per call, ``initial_h`` / ``initial_c`` wired to ``h_in`` /
    ``c_in``), 1..3 Gemm / activation layers from ``Y`` or ``Y_h`` to the action; ``Unsqueeze`` / ``Squeeze`` / ``Reshape`` / ``Identity``
    nodes that only move unit axes may sit between them.  Returns ``(parts, None)`` -- ``parts``: ``enc`` and ``head`` (layers as
    ``_mlp_chain`` gives them), ``W [4H, I]``, ``R [4H, H]``, ``B [8H]`` or None, ``I``, ``H`` -- or ``(None, reason)``."""
    init = model["init"]
    if len(model["inputs"]) != 3 or model["inputs"][1:] != ["h_in", "c_in"]:
        return None, f"the inputs are {model['inputs']}, not (obs, 'h_in', 'c_in')"
    if len(model["outputs"]) != 3:
        return None, f"{len(model['outputs'])} outputs, not (action, h_out, c_out)"
    stands_for, body = {}, []
    for n in model["nodes"]:
        if n["op"] in _SHAPE_ONLY:
            if n["op"] == "Reshape" and (n["inputs"][1] not in init or int((np.asarray(init[n["inputs"][1]]).ravel() != 1).sum()) > 2):
                return None, "a Reshape that does more than move unit axes"
            stands_for[n["outputs"][0]] = n["inputs"][0]
        else:
            body.append(n)

    def src(name):
        while name in stands_for:
            name = stands_for[name]
        return name
    n_lstm = sum(1 for n in body if n["op"] == "LSTM")
    if n_lstm == 0:
        return None, "no LSTM node"
    if n_lstm > 1:
        return None, "a second LSTM node (stacked cells are out of scope)"
    enc, cur, i = _gemm_layers(body, 0, model["inputs"][0], init, src)
    if body[i]["op"] != "LSTM" or src(body[i]["inputs"][0]) != cur:
        return None, f"node '{body[i]['op']}' between the observation and the LSTM node is not part of a Gemm / activation chain"
    n = body[i]
    a, ins, outs = n["attrs"], n["inputs"] + [""] * 8, n["outputs"] + [""] * 3
    if a.get("direction", "forward") != "forward":
        return None, f"LSTM direction '{a.get('direction')}' (forward only)"
    if a.get("layout", 0):
        return None, "LSTM layout 1 (layout 0 only)"
    if a.get("activations") or a.get("clip") is not None or a.get("input_forget", 0) or ins[4] or ins[7]:
        return None, "LSTM with non-default activations, clip, input_forget, sequence_lens or peepholes"
    if src(ins[5]) != "h_in":
        return None, "initial_h is not wired to h_in"
    if src(ins[6]) != "c_in":
        return None, "initial_c is not wired to c_in"
    if ins[1] not in init or ins[2] not in init or (ins[3] and ins[3] not in init):
        return None, "LSTM weights that are not initialisers"
    W, R, B = init[ins[1]], init[ins[2]], init[ins[3]] if ins[3] else None
    if W.dtype != np.float32 or R.dtype != np.float32 or (B is not None and B.dtype != np.float32):
        return None, "LSTM weights that are not fp32"
    if W.ndim != 3 or W.shape[0] != 1 or R.ndim != 3 or R.shape[0] != 1 or W.shape[1] % 4:
        return None, f"LSTM weights of shape {W.shape} / {R.shape}, not [1, 4H, I] / [1, 4H, H]"
    H, I = W.shape[1] // 4, W.shape[2]
    if R.shape != (1, 4 * H, H) or (B is not None and B.shape != (1, 8 * H)) or a.get("hidden_size", H) != H:
        return None, f"LSTM shapes W {W.shape}, R {R.shape}, B {None if B is None else B.shape}, hidden_size {a.get('hidden_size')} do not agree"
    if enc and enc[-1][0].shape[0] != I:
        return None, f"the LSTM's input width {I} differs from the encoder's output width {enc[-1][0].shape[0]}"
    if src(model["outputs"][1]) != outs[1] or not outs[1] or src(model["outputs"][2]) != outs[2] or not outs[2]:
        return None, "the second and third output are not the LSTM's Y_h and Y_c"
    first = body[i + 1]["inputs"][0] if i + 1 < len(body) and body[i + 1]["inputs"] else ""
    if not first or src(first) not in (outs[0], outs[1]):
        return None, "the head does not read the LSTM's Y or Y_h"
    head, cur, j = _gemm_layers(body, i + 1, src(first), init, src)
    if j != len(body) or src(model["outputs"][0]) != cur:
        return None, "the head is not a Gemm / activation chain from the LSTM's output to the action" + \
            (f" (node '{body[j]['op']}')" if j < len(body) else "")
    if len(enc) > 3 or not 1 <= len(head) <= 3:
        return None, f"{len(enc)} encoder and {len(head)} head layers (0..3 and 1..3)"
    if head[0][0].shape[1] != H:
        return None, f"the head's input width {head[0][0].shape[1]} differs from the hidden size {H}"
    return {"enc": enc, "head": head, "W": W[0], "R": R[0], "B": None if B is None else B[0], "I": int(I), "H": int(H),
            "in_dim": int(enc[0][0].shape[1] if enc else I), "out_dim": int(head[-1][0].shape[0])}, None


class MLPPolicy:
    """``core/policy.py:5-21``: ``get_action(state[N, state_dim]) -> action[N, action_dim]`` in [-1, 1].

    A graph that is a plain Gemm / activation chain runs as ONE launch of the engine's fused MFMA kernel
    (``cosim_mlp_forward``, csrc/cosim_mlp.hip) when the policy lives on a GPU; anything else goes through the interpreter."""

    def __init__(self, policy_path: str, device=None, fused: Optional[bool] = None):
        import ctypes
        import torch
        self.torch = torch
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        model = read_onnx(policy_path)
        self.graph = OnnxGraph(model, self.device)
        self.input_name = self.graph.inputs[0]
        chain = _mlp_chain(model) if (fused is not False and self.device.type == "cuda") else None
        if fused and chain is None:
            raise ValueError("fused=True needs a Gemm/activation chain on a GPU device")
        self._fused = None
        if chain is not None:
            from .engine import load_library
            L = load_library()
            L.cosim_mlp_forward.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                            ctypes.c_void_p, ctypes.c_void_p, ctypes.c_float, ctypes.c_void_p, ctypes.c_void_p]
            L.cosim_last_error.restype = ctypes.c_char_p
            ws = [torch.as_tensor(np.ascontiguousarray(w), device=self.device) for w, *_ in chain]
            bs = [None if b is None else torch.as_tensor(np.ascontiguousarray(b), device=self.device) for _, b, *_ in chain]
            nl = len(chain)
            self._fused = dict(
                L=L, nl=nl, keep=(ws, bs),
                dims=(ctypes.c_int * (nl + 1))(chain[0][0].shape[1], *[w.shape[0] for w, *_ in chain]),
                w=(ctypes.c_void_p * nl)(*[w.data_ptr() for w in ws]),
                b=(ctypes.c_void_p * nl)(*[None if b is None else b.data_ptr() for b in bs]),
                act=(ctypes.c_int * nl)(*[a for *_, a, _ in chain]),
                alpha=(ctypes.c_float * nl)(*[al for *_, al in chain]),
                out_dim=chain[-1][0].shape[0], in_dim=chain[0][0].shape[1], out=None)

    graph_safe = True     # stateless: get_action is pure device work

    def get_action(self, state):
        t = self.torch
        s = t.as_tensor(state, dtype=t.float32, device=self.device)
        single = s.dim() == 1
        x = s.unsqueeze(0) if single else s
        f = self._fused
        if f is not None and x.shape[1] == f["in_dim"]:
            x = x.contiguous()
            if f["out"] is None or f["out"].shape[0] != x.shape[0]:
                f["out"] = t.empty((x.shape[0], f["out_dim"]), dtype=t.float32, device=self.device)
            rc = f["L"].cosim_mlp_forward(x.data_ptr(), x.shape[0], f["nl"], f["dims"], f["w"], f["b"], f["act"], f["alpha"], 1.0,
                                          f["out"].data_ptr(), t.cuda.current_stream(self.device).cuda_stream)
            if rc != 0:
                raise RuntimeError(f["L"].cosim_last_error().decode())
            out = f["out"]
        else:
            out = self.graph.run({self.input_name: x})[0].clamp(-1.0, 1.0)
        return out.squeeze(0) if single else out


    def get_action_into(self, state_rows, out_rows):
        """``out_rows[:] = get_action(state_rows)`` on the CURRENT stream without allocating: for callers that evaluate the policy per
        env range on the range's own stream (``Runner.test_pipelined``).  Both are contiguous row slices of ``[N, ...]`` tensors."""
        f = self._fused
        if f is None or state_rows.shape[1] != f["in_dim"] or not (state_rows.is_contiguous() and out_rows.is_contiguous()):
            out_rows.copy_(self.get_action(state_rows))
            return
        rc = f["L"].cosim_mlp_forward(state_rows.data_ptr(), state_rows.shape[0], f["nl"], f["dims"], f["w"], f["b"], f["act"], f["alpha"], 1.0,
                                      out_rows.data_ptr(), self.torch.cuda.current_stream(self.device).cuda_stream)
        if rc != 0:
            raise RuntimeError(f["L"].cosim_last_error().decode())


class LSTMPolicy:
    """``core/policy.py:24-47``: inputs (state, "h_in", "c_in"), outputs (action, h_out, c_out); h/c kept per env."""

    def __init__(self, config: dict, policy_path: str, num_envs: int = 1, device=None):
        import torch
        self.torch = torch
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.graph = OnnxGraph(read_onnx(policy_path), self.device)
        names = self.graph.inputs
        assert len(names) >= 3 and names[1] == "h_in" and names[2] == "c_in", \
            "The input names of ONNX policy must include 'h_in' and 'c_in'"
        self.input_name = names[0]
        self.h_in = torch.zeros((1, num_envs, config["policy"]["h_in_dim"]), dtype=torch.float32, device=self.device)
        self.c_in = torch.zeros((1, num_envs, config["policy"]["c_in_dim"]), dtype=torch.float32, device=self.device)

    graph_safe = True     # get_action is pure device work on persistent tensors (Runner.test_graphed)

    def reset(self, mask=None):
        """Zero the recurrent state (of the masked envs): what re-creating the policy does in the reference
        (core/tester.py builds a fresh policy per episode).  Branch-free on the device, so it can sit inside a captured graph."""
        if mask is None:
            self.h_in.zero_(); self.c_in.zero_()
        else:
            # masked_fill, not a multiply by a 0 / 1 mask: NaN * 0 is NaN, and a non-finite recurrent state must not survive the
            # reset of its env (it would emit NaN actions and be NaN-reset every step from then on)
            done = (self.torch.as_tensor(mask, device=self.device) != 0)[None, :, None]
            self.h_in.masked_fill_(done, 0.0)
            self.c_in.masked_fill_(done, 0.0)

    def state(self) -> dict:
        """The recurrent state ``h`` / ``c`` ``[N, H]`` (copies) for a ``Snapshot``."""
        return {"h": self.h_in[0].clone(), "c": self.c_in[0].clone()}

    def load_state(self, state: dict, src=None, mask=None):
        """Counterpart of ``BatchedEnv.restore``: env ``d`` takes row ``src[d]`` of ``state["h"]`` / ``["c"]`` (``None``: row ``d``);
        envs with ``mask[d] == 0`` keep theirs.  In place, so a captured graph keeps seeing the same tensors."""
        t = self.torch
        for name, dst in (("h", self.h_in), ("c", self.c_in)):
            x = t.as_tensor(state[name], dtype=t.float32, device=self.device)
            if src is not None:
                x = x[t.as_tensor(src, device=self.device).long()]
            if tuple(x.shape) != tuple(dst.shape[1:]):
                raise ValueError(f"LSTMPolicy.load_state: {name} has shape {tuple(x.shape)}, expected {tuple(dst.shape[1:])}")
            if mask is not None:
                x = t.where((t.as_tensor(mask, device=self.device) != 0)[:, None], x, dst[0])
            dst[0].copy_(x)

    def get_action(self, state):
        t = self.torch
        s = t.as_tensor(state, dtype=t.float32, device=self.device)
        single = s.dim() == 1
        action, h_out, c_out = self.graph.run({self.input_name: s.unsqueeze(0) if single else s, "h_in": self.h_in, "c_in": self.c_in})[:3]
        # in place: the recurrent state lives in two persistent tensors, so a HIP-graph replay of this call feeds it back
        self.h_in.copy_(h_out.reshape(self.h_in.shape))
        self.c_in.copy_(c_out.reshape(self.c_in.shape))
        action = action.reshape(-1, action.shape[-1]).clamp(-1.0, 1.0)
        return action.squeeze(0) if single else action


class _FleetTable:
    """What the tables of this module share: the files and their names, the assignment of envs to policies and the env ranges."""

    def _setup_fleet(self, policy_paths, num_envs, device, env_id0, scenarios, names):
        import torch
        self.torch = torch
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        who = type(self).__name__
        paths = [str(p) for p in policy_paths]
        K, N = len(paths), int(num_envs)
        if K < 1:
            raise ValueError(f"{who}: no policy file")
        if N < 1:
            raise ValueError(f"{who}: num_envs {N} is not positive")
        self.paths, self.num_envs, self.env_id0, self.scenarios = paths, N, int(env_id0), int(scenarios)
        self.names = [os.path.splitext(os.path.basename(p))[0] for p in paths] if names is None else [str(x) for x in names]
        if len(self.names) != K or len(set(self.names)) != K:
            raise ValueError(f"{who}: names must be {K} different strings, got {self.names}")

    def _setup_assign(self, assign, ranges):
        who, K, N = type(self).__name__, len(self.paths), self.num_envs
        self.assign = assign if isinstance(assign, str) else "explicit"
        if isinstance(assign, str):
            if assign not in ("interleave", "cross"):
                raise ValueError(f"{who}: assign '{assign}': interleave, cross or an int array")
            if assign == "cross" and self.scenarios < 1:
                raise ValueError(f"{who}: assign 'cross' needs scenarios >= 1 (the scenario count of the table)")
            self._explicit = None
        else:
            a = np.asarray(assign)
            if a.shape != (N,) or not np.issubdtype(a.dtype, np.integer):
                raise ValueError(f"{who}: an explicit assign has one integer per local env ({N}), got shape {a.shape} {a.dtype}")
            if a.min() < 0 or a.max() >= K:
                raise ValueError(f"{who}: assign holds {int(a.min())}..{int(a.max())}, outside [0, {K})")
            self._explicit = a.astype(np.int32)
        self.policy_of_env = self._base_of(np.arange(self.env_id0, self.env_id0 + N, dtype=np.int64))
        self.ranges = [(0, N)] if ranges is None else [(int(f), int(c)) for f, c in ranges]
        nxt = 0
        for f, c in self.ranges:
            if f != nxt or c < 1:
                raise ValueError(f"{who}: ranges {self.ranges} do not tile [0, {N}) in order")
            nxt = f + c
        if nxt != N:
            raise ValueError(f"{who}: ranges {self.ranges} do not tile [0, {N}) in order")

    def _policy_rows(self):
        """Per policy the int64 row tensors of its envs, and the same per range: what the torch twins index with."""
        t, K = self.torch, len(self.paths)
        idx = [np.nonzero(self.policy_of_env == k)[0] for k in range(K)]
        rows = [t.as_tensor(i, dtype=t.int64, device=self.device) for i in idx]
        range_rows = [[t.as_tensor(i[(i >= f) & (i < f + c)], dtype=t.int64, device=self.device) for i in idx] for f, c in self.ranges]
        return rows, range_rows

    def _base_of(self, global_env_ids) -> np.ndarray:
        """The static assignment: the policy index int32 of each global env id (an explicit assignment knows this rank's envs only)."""
        g = np.asarray(global_env_ids, dtype=np.int64)
        K = len(self.paths)
        if self._explicit is not None:
            loc = g - self.env_id0
            if loc.size and (loc.min() < 0 or loc.max() >= self.num_envs):
                raise ValueError(f"{type(self).__name__}.policy_of: an explicit assignment covers env ids {self.env_id0}..{self.env_id0 + self.num_envs - 1}")
            return self._explicit[loc]
        return ((g % K) if self.assign == "interleave" else ((g // self.scenarios) % K)).astype(np.int32)

    def policy_of(self, global_env_ids, episodes=None) -> np.ndarray:
        """The policy index int32 of each global env id; of a rotating table in the env's episode number ``episodes[i]`` (the episodes
        it had ended before: a ledger record's ordinal), ``(base + episodes // rotate_every) mod K``."""
        base = self._base_of(global_env_ids)
        if self.rotate_every is None:
            return base
        if episodes is None:
            raise ValueError(f"{type(self).__name__}.policy_of: the table rotates every {self.rotate_every} episode(s), so an env's policy depends on "
                             "its episode: pass episodes= (policy_of_env is the assignment of episode 0)")
        e = np.broadcast_to(np.asarray(episodes, dtype=np.int64), base.shape)
        K = len(self.paths)
        return ((base + (np.maximum(e, 0) // self.rotate_every) % K) % K).astype(np.int32)

    rotate_every = None   # None: the assignment holds for the whole run

    def _setup_rotate(self, rotate_every):
        """``rotate_every`` checked; a rotating table gets its counters: ``episode`` (ended episodes per env) and ``policy_now`` (the
        policy each env was last evaluated with), ``[N]`` int32 on the table's device, persistent."""
        t, who = self.torch, type(self).__name__
        if rotate_every is None:
            return
        if isinstance(rotate_every, bool) or not isinstance(rotate_every, (int, np.integer)) or int(rotate_every) < 1:
            raise ValueError(f"{who}: rotate_every {rotate_every!r}: an integer >= 1 (episodes a checkpoint keeps an env), or None")
        self.rotate_every = int(rotate_every)
        self._base = t.as_tensor(self.policy_of_env, dtype=t.int32, device=self.device)
        self.episode = t.zeros(self.num_envs, dtype=t.int32, device=self.device)
        self.policy_now = self._base.clone()

    def _arm(self, rotate_fn):
        if self.rotate_every is not None and self._handle is not None:
            with self.torch.cuda.device(self.device):
                if rotate_fn(self._handle, self.rotate_every) != 0:
                    raise RuntimeError(self._lib.cosim_last_error().decode())

    def _advance(self, mask):
        """The masked envs ended an episode: their counters go up by one (held at INT32_MAX).  Device work on persistent tensors: an
        add and a maximum -- a counter that would wrap comes out below the old one, and the old one is kept."""
        t = self.torch
        ended = t.as_tensor(mask, device=self.device)
        if ended.dtype != t.bool:
            ended = ended != 0
        t.maximum(self.episode, self.episode + ended, out=self.episode)

    def curve_groups(self):
        """``(group, K, names)`` for ``BatchedEnv.set_curve_groups``: ``group`` is an int32 device tensor ``[N]`` with each env's policy
        index, which the curves' fold reads when an episode ends.  A rotating table hands out ``policy_now`` itself -- it is rewritten
        only by the table's forward, so behind the step that ended an episode it still names the policy that drove it; a static table
        a persistent tensor of ``policy_of_env``, created once.  The table must drive the env from its first step."""
        t = self.torch
        if self.device.type != "cuda":
            raise ValueError(f"{type(self).__name__}.curve_groups: the table is on '{self.device}'; the curves' fold reads the group words on the "
                             "GPU that runs the env")
        if self.rotate_every is not None:
            return self.policy_now, len(self.paths), list(self.names)
        if getattr(self, "_curve_group", None) is None:
            self._curve_group = t.as_tensor(np.ascontiguousarray(self.policy_of_env, dtype=np.int32), device=self.device)
        return self._curve_group, len(self.paths), list(self.names)

    def rewind(self):
        """Back to episode 0 for every env: the counters of a rotating table are zeroed (``reset()`` without a mask leaves them)."""
        if self.rotate_every is not None:
            self.episode.zero_()
            self.policy_now.copy_(self._base)

    def _twin_rows(self, i, done):
        """The torch twin of the regroup launch for range ``i`` (-1: all): counters advanced by ``done``, ``policy_now`` from the rule, and
        per policy the int64 rows it drives now."""
        t, K = self.torch, len(self.paths)
        first, count = (0, self.num_envs) if i < 0 else self.ranges[i]
        sl = slice(first, first + count)
        if done is not None:
            ended = (done[0][sl] != 0) | (done[1][sl] != 0)
            self.episode[sl] += (ended & (self.episode[sl] < 2147483647)).to(t.int32)
        now = (self._base[sl] + (self.episode[sl].clamp(min=0) // self.rotate_every) % K) % K
        self.policy_now[sl] = now
        return [first + t.nonzero(now == k)[:, 0] for k in range(K)]

    def _check_done(self, done):
        t, who = self.torch, type(self).__name__
        if done is not None:
            for d in done:
                if d.shape != (self.num_envs,) or d.dtype not in (t.uint8, t.bool) or not d.is_contiguous() or d.device != self._out.device:
                    raise ValueError(f"{who}: done is (terminated, truncated), contiguous uint8 [{self.num_envs}] tensors on the table's device")

    def _load_counters(self, state, src, mask):
        """``load_state`` for the counters of a rotating table: env ``d`` takes ``state["episode"][src[d]]``, masked as the rest."""
        t, who = self.torch, type(self).__name__
        if self.rotate_every is None:
            return
        if state is None or "episode" not in state:
            raise ValueError(f"{who}.load_state: the state carries no episode counters (it was taken from a table that does not rotate)")
        x = t.as_tensor(state["episode"], dtype=t.int32, device=self.device)
        if src is not None:
            x = x[t.as_tensor(src, device=self.device).long()]
        if tuple(x.shape) != (self.num_envs,):
            raise ValueError(f"{who}.load_state: episode has shape {tuple(x.shape)}, expected ({self.num_envs},)")
        if mask is not None:
            x = t.where(t.as_tensor(mask, device=self.device) != 0, x, self.episode)
        self.episode.copy_(x)

    def _check_range(self, i):
        if not 0 <= int(i) < len(self.ranges):
            raise ValueError(f"{type(self).__name__}.get_action_range: range {i} outside 0..{len(self.ranges) - 1}")


class PolicyTable(_FleetTable):
    """K actor checkpoints over ONE fleet: env ``g`` (global id) is driven by policy ``policy_of(g)`` for the whole run, and one launch
    of the grouped kernel (``cosim_policy_table_forward``, csrc/cosim_mlp.hip) evaluates all of them -- every env gets the bits
    ``MLPPolicy(file, fused=True)`` gives it.  All policies meet the same terrain, spawn table, scenario table, fall rule and noise
    streams (those are keyed by global env id), so one run is the comparison; ``EpisodeLedger.by_policy`` / ``Verdicts.by_policy``
    break the outcomes down, and ``env.set_curve_groups(table)`` splits the response curves by policy (``curve_groups()``).

    ``assign``: ``"interleave"`` -- ``g mod K``; ``"cross"`` -- ``(g // S) mod K`` with ``S = scenarios`` (in scenario mode ``env``, where
    env ``g`` runs scenario ``g mod S``, every (scenario, policy) pair gets the same share of envs); or an int array with one entry per
    LOCAL env.  ``ranges``: the env's ``range_list`` (``get_action_range`` evaluates one of them on the current stream); default: one
    range.  Every file must be a Gemm / activation chain (``_mlp_chain``) with the first file's input and output width.  On a
    non-CUDA device, or with ``fused=False``, each policy's interpreter runs on its own rows and the results are scattered: the
    torch twin of the kernel.  Stateless: a ``Snapshot`` stores nothing for it.

    ``rotate_every=R`` (an integer >= 1; ``None``: everything above, unchanged) makes the design PAIRED: env ``g`` is driven by policy
    ``(policy_of_env + e // R) mod K`` in its episode number ``e``, so every robot meets every checkpoint and two checkpoints can be
    compared on the same robot, floor and noise slot.  ``episode`` (``[N]`` int32, the episodes each env has ended) and ``policy_now``
    (``[N]`` int32, the policy each env was last evaluated with) are persistent tensors; a device kernel regroups the envs ahead of
    every evaluation (``cosim_policy_table_forward_rotating``) and each env still gets the bits of ``MLPPolicy`` of the file that
    drives it now.  ``reset(mask)`` (a rotating table's only: a static one has no ``reset``) means "these envs ended an episode" and advances their counters (``Runner.test`` /
    ``test_graphed`` call it); ``get_action_range(..., done=(terminated, truncated))`` folds the same advance into the range's
    launch (``Runner.test_pipelined``); ``reset()`` leaves the counters alone, ``rewind()`` zeroes them; ``state()`` /
    ``load_state`` carry them, so a ``Snapshot`` continues the rotation.  ``policy_of(g, episodes)`` applies the rule;
    ``policy_of_env`` stays the assignment of episode 0.  The counter follows the ledger's episode ordinal when the table drives the
    env from its first step and the ledger is armed in the env's constructor.

    Out of scope: recurrent policies (``RecurrentPolicyTable``), files with different observation layouts, rotation keyed by anything
    but the table's own episode count."""

    graph_safe = True     # get_action is one launch on persistent tensors

    def __init__(self, policy_paths, num_envs: int, device=None, assign="interleave", env_id0: int = 0, scenarios: int = 0,
                 ranges=None, names=None, fused: Optional[bool] = None, rotate_every=None):
        import torch
        self._setup_fleet(policy_paths, num_envs, device, env_id0, scenarios, names)
        paths, K, N = self.paths, len(self.paths), self.num_envs
        chains, models = [], []
        for p in paths:
            model = read_onnx(p)
            if any(n["op"] == "LSTM" for n in model["nodes"]):
                raise ValueError(f"PolicyTable: {p}: an LSTM policy (recurrent policies in a table are out of scope)")
            chain = _mlp_chain(model)
            if chain is None:
                raise ValueError(f"PolicyTable: {p}: the graph is not a plain Gemm / activation chain (1..6 layers, widths up to 512, fp32)")
            i0, o0 = (chains[0][0][0].shape[1], chains[0][-1][0].shape[0]) if chains else (chain[0][0].shape[1], chain[-1][0].shape[0])
            if chain[0][0].shape[1] != i0:
                raise ValueError(f"PolicyTable: {p}: input width {chain[0][0].shape[1]} differs from {i0} of {paths[0]}")
            if chain[-1][0].shape[0] != o0:
                raise ValueError(f"PolicyTable: {p}: output width {chain[-1][0].shape[0]} differs from {o0} of {paths[0]}")
            chains.append(chain)
            models.append(model)
        self.in_dim, self.out_dim = int(chains[0][0][0].shape[1]), int(chains[0][-1][0].shape[0])
        self._setup_assign(assign, ranges)
        self._out = torch.zeros((N, self.out_dim), dtype=torch.float32, device=self.device)
        self._setup_rotate(rotate_every)
        if self.rotate_every is not None:
            self.reset = self._reset_rotating
        self._handle = None
        if fused is not False and self.device.type == "cuda":
            self._create(chains)
            self._arm(self._lib.cosim_policy_table_rotate)
        elif fused:
            raise ValueError("fused=True needs a GPU device")
        else:
            self._rows, self._range_rows = self._policy_rows()
            self._graphs = [OnnxGraph(m, self.device) for m in models]

    def _create(self, chains):
        import ctypes
        from .engine import load_library
        L = load_library()
        K, ML = len(chains), 6
        nl = (ctypes.c_int * K)(*[len(c) for c in chains])
        dims, act, alpha = (ctypes.c_int * (K * (ML + 1)))(), (ctypes.c_int * (K * ML))(), (ctypes.c_float * (K * ML))()
        w, b, keep = (ctypes.c_void_p * (K * ML))(), (ctypes.c_void_p * (K * ML))(), []
        for k, chain in enumerate(chains):
            dims[k * (ML + 1)] = chain[0][0].shape[1]
            for li, (wl, bl, a, al) in enumerate(chain):
                dims[k * (ML + 1) + li + 1] = wl.shape[0]
                act[k * ML + li], alpha[k * ML + li] = a, al
                wl = np.ascontiguousarray(wl, dtype=np.float32)
                keep.append(wl)
                w[k * ML + li] = wl.ctypes.data
                if bl is not None:
                    bl = np.ascontiguousarray(bl, dtype=np.float32)
                    keep.append(bl)
                    b[k * ML + li] = bl.ctypes.data
        por = np.ascontiguousarray(self.policy_of_env, dtype=np.int32)
        rng = np.ascontiguousarray(np.asarray(self.ranges, dtype=np.int32).reshape(-1, 2))
        handle = ctypes.c_void_p()
        with self.torch.cuda.device(self.device):
            rc = L.cosim_policy_table_create(K, nl, dims, act, alpha, w, b, self.num_envs, por.ctypes.data, len(self.ranges), rng.ctypes.data,
                                             ctypes.byref(handle))
        if rc != 0:
            raise RuntimeError(L.cosim_last_error().decode())
        self._lib, self._handle = L, handle

    def state(self):
        """Nothing for a static table: it is stateless, so ``env.snapshot(table)`` stores no policy state.  A rotating one: its episode
        counters (a copy)."""
        return None if self.rotate_every is None else {"episode": self.episode.clone()}

    def load_state(self, state, src=None, mask=None):
        """Counterpart of ``state()``, as ``LSTMPolicy.load_state``: env ``d`` takes the counter of row ``src[d]`` (``None``: row ``d``), envs
        with ``mask[d] == 0`` keep theirs; in place.  Nothing to do for a static table."""
        self._load_counters(state, src, mask)

    def _reset_rotating(self, mask=None):
        """``reset(mask)`` of a ROTATING table: the masked envs ended an episode, their counters advance (device work, graph-safe);
        ``reset()`` leaves the counters alone (``rewind()`` zeroes them).  A static table has no ``reset`` at all, so a runner that asks
        ``hasattr(policy, "reset")`` does for it exactly what it did before there was rotation."""
        if mask is not None:
            self._advance(mask)

    def close(self):
        if self._handle is not None:
            self._lib.cosim_policy_table_destroy(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass

    def _launch(self, x, out, i: int, done=None):
        t = self.torch
        if x.shape != (self.num_envs, self.in_dim) or out.shape != (self.num_envs, self.out_dim):
            raise ValueError(f"PolicyTable: state {tuple(x.shape)} / action {tuple(out.shape)}, expected ({self.num_envs}, {self.in_dim}) / "
                             f"({self.num_envs}, {self.out_dim})")
        rotating = self.rotate_every is not None
        if done is not None:
            self._check_done(done)
        if self._handle is not None:
            if not (x.is_cuda and out.is_cuda and x.dtype == t.float32 and out.dtype == t.float32 and x.is_contiguous() and out.is_contiguous()):
                raise ValueError("PolicyTable: state and action must be contiguous fp32 tensors on the table's device")
            stream = t.cuda.current_stream(self.device).cuda_stream
            if rotating:
                da, db = (None, None) if done is None else (done[0].data_ptr(), done[1].data_ptr())
                rc = self._lib.cosim_policy_table_forward_rotating(self._handle, x.data_ptr(), out.data_ptr(), self.episode.data_ptr(),
                                                                   self.policy_now.data_ptr(), da, db, i, 1.0, stream)
            else:
                rc = self._lib.cosim_policy_table_forward(self._handle, x.data_ptr(), out.data_ptr(), i, 1.0, stream)
            if rc != 0:
                raise RuntimeError(self._lib.cosim_last_error().decode())
            return
        rows = self._twin_rows(i, done) if rotating else (self._rows if i < 0 else self._range_rows[i])
        for g, idx in zip(self._graphs, rows):
            if idx.numel():
                out[idx] = g.run({g.inputs[0]: x[idx]})[0].clamp(-1.0, 1.0)

    def get_action(self, state):
        """``[N, action_dim]`` in [-1, 1]: the table's persistent output tensor (the next call overwrites it)."""
        t = self.torch
        x = t.as_tensor(state, dtype=t.float32, device=self.device).contiguous()
        self._launch(x, self._out, -1)
        return self._out

    def get_action_range(self, i: int, state, action, done=None):
        """Writes the rows of range ``i`` of ``ranges`` into ``action`` (``[N, action_dim]``) from ``state`` (``[N, in_dim]``), both whole-fleet
        contiguous fp32 tensors, on the CURRENT stream and without allocating; the other rows of ``action`` stay as they are.
        ``done=(terminated, truncated)`` (uint8 ``[N]``): a rotating table needs it -- an env of the range with either set has ended an
        episode, and its counter advances in this very launch; a static table ignores it."""
        self._check_range(i)
        if self.rotate_every is None:
            self._launch(state, action, int(i))
            return
        if done is None:
            raise ValueError("PolicyTable.get_action_range: the table rotates, pass done=(terminated, truncated) (the range's episode ends advance "
                             "its counters in this launch)")
        self._launch(state, action, int(i), done)


class RecurrentPolicyTable(_FleetTable):
    """K RECURRENT actor checkpoints over one fleet: ``PolicyTable`` for files of ``LSTMPolicy``'s kind (inputs ``(obs, "h_in", "c_in")``,
    outputs ``(action, h_out, c_out)``; the graph shape ``_recurrent_actor`` recognises).  One launch of the fused actor kernel
    (``cosim_recurrent_table_forward``, csrc/cosim_mlp.hip) runs encoder, LSTM cell and head of every env's own policy and updates the
    recurrent state in place -- every env gets the bits ``cosim_mlp_forward`` -> ``cosim_lstm_cell`` -> ``cosim_mlp_forward`` give it.

    The table owns the state: ``h`` and ``c``, ``[N, Hmax]`` with ``Hmax`` the largest hidden size; a policy with hidden size ``H`` uses
    columns ``0 .. H`` of its rows, the rest stay zero.  ``reset`` / ``state`` / ``load_state`` are ``LSTMPolicy``'s.  ``get_action_range``
    takes ``done=(terminated, truncated)`` (uint8 ``[N]``): an env with either set starts from a zero state in this very launch, the
    episode reset of ``Runner.test`` folded into the forward.  Constructor arguments as ``PolicyTable``.  On a non-CUDA device, or with
    ``fused=False``, each policy's interpreter runs on its own rows against slices of the state: the torch twin.

    ``rotate_every=R``: as ``PolicyTable`` -- the same rule, counters (``episode``, ``policy_now``), ``rewind()`` and ``policy_of``.  The done
    flags do both jobs: ``reset(mask)`` (or ``done=``) zeroes the masked envs' state and advances their counters, so the next policy of
    an env starts from ``h = c = 0``; ``state()`` / ``load_state`` carry ``h``, ``c`` and the counters.

    Out of scope: tables that mix MLP and recurrent files, GRU cells, stacked or multi-step LSTM nodes, rotation keyed by anything but
    the table's own episode count."""

    graph_safe = True     # one launch on persistent tensors
    recurrent = True      # Runner.test_pipelined hands get_action_range the env's done flags

    def __init__(self, policy_paths, num_envs: int, device=None, assign="interleave", env_id0: int = 0, scenarios: int = 0,
                 ranges=None, names=None, fused: Optional[bool] = None, rotate_every=None):
        import torch
        self._setup_fleet(policy_paths, num_envs, device, env_id0, scenarios, names)
        paths, N = self.paths, self.num_envs
        parts, models = [], []
        for p in paths:
            model = read_onnx(p)
            part, why = _recurrent_actor(model)
            if part is None:
                raise ValueError(f"RecurrentPolicyTable: {p}: not a recurrent actor: {why}")
            if parts and part["in_dim"] != parts[0]["in_dim"]:
                raise ValueError(f"RecurrentPolicyTable: {p}: input width {part['in_dim']} differs from {parts[0]['in_dim']} of {paths[0]}")
            if parts and part["out_dim"] != parts[0]["out_dim"]:
                raise ValueError(f"RecurrentPolicyTable: {p}: output width {part['out_dim']} differs from {parts[0]['out_dim']} of {paths[0]}")
            parts.append(part)
            models.append(model)
        self.in_dim, self.out_dim = parts[0]["in_dim"], parts[0]["out_dim"]
        self.hidden = [part["H"] for part in parts]
        self._setup_assign(assign, ranges)
        self.h = torch.zeros((N, max(self.hidden)), dtype=torch.float32, device=self.device)
        self.c = torch.zeros_like(self.h)
        self._out = torch.zeros((N, self.out_dim), dtype=torch.float32, device=self.device)
        self._setup_rotate(rotate_every)
        self._handle = None
        if fused is not False and self.device.type == "cuda":
            self._create(parts)
            self._arm(self._lib.cosim_recurrent_table_rotate)
        elif fused:
            raise ValueError("fused=True needs a GPU device")
        else:
            self._rows, self._range_rows = self._policy_rows()
            self._graphs = [OnnxGraph(m, self.device) for m in models]

    def _create(self, parts):
        import ctypes
        from .engine import load_library
        L = load_library()
        K, ML = len(parts), 3
        ci, cf, vp = ctypes.c_int, ctypes.c_float, ctypes.c_void_p
        keep = []

        def host(a):
            a = np.ascontiguousarray(a, dtype=np.float32)
            keep.append(a)
            return a.ctypes.data

        def layers(key, first_width):
            n, dims, act, alpha = (ci * K)(), (ci * (K * (ML + 1)))(), (ci * (K * ML))(), (cf * (K * ML))()
            w, b = (vp * (K * ML))(), (vp * (K * ML))()
            for k, part in enumerate(parts):
                n[k] = len(part[key])
                dims[k * (ML + 1)] = part[first_width]
                for li, (wl, bl, a, al) in enumerate(part[key]):
                    dims[k * (ML + 1) + li + 1] = wl.shape[0]
                    act[k * ML + li], alpha[k * ML + li] = a, al
                    w[k * ML + li] = host(wl)
                    if bl is not None:
                        b[k * ML + li] = host(bl)
            return n, dims, act, alpha, w, b
        enc, head = layers("enc", "in_dim"), layers("head", "H")
        lstm_in, hidden = (ci * K)(*[p["I"] for p in parts]), (ci * K)(*[p["H"] for p in parts])
        W, R, B = (vp * K)(*[host(p["W"]) for p in parts]), (vp * K)(*[host(p["R"]) for p in parts]), (vp * K)()
        for k, part in enumerate(parts):
            if part["B"] is not None:
                B[k] = host(part["B"])
        por = np.ascontiguousarray(self.policy_of_env, dtype=np.int32)
        rng = np.ascontiguousarray(np.asarray(self.ranges, dtype=np.int32).reshape(-1, 2))
        handle = vp()
        with self.torch.cuda.device(self.device):
            rc = L.cosim_recurrent_table_create(K, *enc, lstm_in, hidden, W, R, B, *head, self.num_envs, por.ctypes.data, len(self.ranges),
                                                rng.ctypes.data, ctypes.byref(handle))
        if rc != 0:
            import re
            msg = L.cosim_last_error().decode()
            m = re.search(r": policy (\d+)", msg)              # the validator names the policy it refuses: name its file
            raise ValueError(f"RecurrentPolicyTable: {self.paths[int(m.group(1))] + ': ' if m else ''}{msg}")
        self._lib, self._handle = L, handle

    def close(self):
        if self._handle is not None:
            self._lib.cosim_recurrent_table_destroy(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass

    def reset(self, mask=None):
        """Zero the recurrent state (of the masked envs), as ``LSTMPolicy.reset``: a fill, so a non-finite state does not survive.  With a
        mask the envs ended an episode: a rotating table advances their counters too; ``reset()`` leaves the counters alone."""
        if mask is None:
            self.h.zero_(); self.c.zero_()
        else:
            done = (self.torch.as_tensor(mask, device=self.device) != 0)[:, None]
            self.h.masked_fill_(done, 0.0)
            self.c.masked_fill_(done, 0.0)
            if self.rotate_every is not None:
                self._advance(mask)

    def state(self) -> dict:
        """The recurrent state ``h`` / ``c`` ``[N, Hmax]`` (copies) for a ``Snapshot``; of a rotating table the episode counters too."""
        out = {"h": self.h.clone(), "c": self.c.clone()}
        if self.rotate_every is not None:
            out["episode"] = self.episode.clone()
        return out

    def load_state(self, state: dict, src=None, mask=None):
        """As ``LSTMPolicy.load_state``: env ``d`` takes row ``src[d]`` of ``state["h"]`` / ``["c"]`` (``None``: row ``d``); envs with
        ``mask[d] == 0`` keep theirs.  In place.  A row is only meaningful for an env of the same policy as the one it was taken from."""
        t = self.torch
        for name, dst in (("h", self.h), ("c", self.c)):
            x = t.as_tensor(state[name], dtype=t.float32, device=self.device)
            if src is not None:
                x = x[t.as_tensor(src, device=self.device).long()]
            if tuple(x.shape) != tuple(dst.shape):
                raise ValueError(f"RecurrentPolicyTable.load_state: {name} has shape {tuple(x.shape)}, expected {tuple(dst.shape)}")
            if mask is not None:
                x = t.where((t.as_tensor(mask, device=self.device) != 0)[:, None], x, dst)
            dst.copy_(x)
        self._load_counters(state, src, mask)

    def _launch(self, x, out, i: int, done=None):
        t = self.torch
        if x.shape != (self.num_envs, self.in_dim) or out.shape != (self.num_envs, self.out_dim):
            raise ValueError(f"RecurrentPolicyTable: state {tuple(x.shape)} / action {tuple(out.shape)}, expected ({self.num_envs}, {self.in_dim}) / "
                             f"({self.num_envs}, {self.out_dim})")
        if done is not None:
            for d in done:
                if d.shape != (self.num_envs,) or d.dtype not in (t.uint8, t.bool) or not d.is_contiguous() or d.device != self.h.device:
                    raise ValueError(f"RecurrentPolicyTable: done is (terminated, truncated), contiguous uint8 [{self.num_envs}] tensors on the table's device")
        if self._handle is not None:
            if not (x.is_cuda and out.is_cuda and x.dtype == t.float32 and out.dtype == t.float32 and x.is_contiguous() and out.is_contiguous()):
                raise ValueError("RecurrentPolicyTable: state and action must be contiguous fp32 tensors on the table's device")
            da, db = (None, None) if done is None else (done[0].data_ptr(), done[1].data_ptr())
            stream = t.cuda.current_stream(self.device).cuda_stream
            if self.rotate_every is not None:
                rc = self._lib.cosim_recurrent_table_forward_rotating(self._handle, x.data_ptr(), self.h.data_ptr(), self.c.data_ptr(), out.data_ptr(),
                                                                      self.episode.data_ptr(), self.policy_now.data_ptr(), da, db, i, 1.0, stream)
            else:
                rc = self._lib.cosim_recurrent_table_forward(self._handle, x.data_ptr(), self.h.data_ptr(), self.c.data_ptr(), out.data_ptr(), da, db, i, 1.0,
                                                             stream)
            if rc != 0:
                raise RuntimeError(self._lib.cosim_last_error().decode())
            return
        rows = self._twin_rows(i, done) if self.rotate_every is not None else (self._rows if i < 0 else self._range_rows[i])
        fresh = None if done is None else ((done[0] != 0) | (done[1] != 0))
        for g, idx, H in zip(self._graphs, rows, self.hidden):
            if not idx.numel():
                continue
            h, c = self.h[idx, :H], self.c[idx, :H]
            if fresh is not None:
                h, c = h.masked_fill(fresh[idx, None], 0.0), c.masked_fill(fresh[idx, None], 0.0)
            action, h_out, c_out = g.run({g.inputs[0]: x[idx], "h_in": h.unsqueeze(0), "c_in": c.unsqueeze(0)})[:3]
            self.h[idx, :H] = h_out.reshape(-1, H)
            self.c[idx, :H] = c_out.reshape(-1, H)
            out[idx] = action.reshape(-1, self.out_dim).clamp(-1.0, 1.0)

    def get_action(self, state):
        """``[N, action_dim]`` in [-1, 1]: the table's persistent output tensor (the next call overwrites it); ``h`` / ``c`` move one step."""
        t = self.torch
        x = t.as_tensor(state, dtype=t.float32, device=self.device).contiguous()
        self._launch(x, self._out, -1)
        return self._out

    def get_action_range(self, i: int, state, action, done=None):
        """One step of the envs of range ``i``: their rows of ``action`` and of ``h`` / ``c`` are written, every other row stays as it is.
        ``state`` / ``action`` as ``PolicyTable.get_action_range``; on the CURRENT stream, without allocating.  ``done``: see the class."""
        self._check_range(i)
        if self.rotate_every is not None and done is None:
            raise ValueError("RecurrentPolicyTable.get_action_range: the table rotates, pass done=(terminated, truncated) (the range's episode "
                             "ends advance its counters in this launch)")
        self._launch(state, action, int(i), done)


def open_policy_table(policy_paths, **table_args):
    """A table over several files, its kind taken from the files: ``RecurrentPolicyTable`` if every file has the inputs
    ``(obs, "h_in", "c_in")``, ``PolicyTable`` if none has; a mix is refused (a table is all one kind)."""
    paths = [str(p) for p in policy_paths]
    kinds = [read_onnx(p)["inputs"][1:3] == ["h_in", "c_in"] for p in paths]
    if kinds and any(k != kinds[0] for k in kinds):
        other = paths[kinds.index(not kinds[0])]
        raise ValueError(f"open_policy_table: {other}: {'a recurrent' if not kinds[0] else 'an MLP'} actor among "
                         f"{'MLP' if not kinds[0] else 'recurrent'} ones ({paths[0]}); a table is all one kind")
    return (RecurrentPolicyTable if kinds and kinds[0] else PolicyTable)(paths, **table_args)


def build_policy(config: dict, policy_path: str = None, num_envs: int = 1, device=None, **table_args):
    """``core/policy.py:49-53``.  With a list of files in ``config["policy"]["onnx_files"]``: a table over them -- ``PolicyTable`` or,
    for recurrent files, ``RecurrentPolicyTable``; the kind is detected from the files (``open_policy_table``), ``use_lstm`` belongs to
    a single file (``config["policy"]["assign"]``, default interleave; ``config["policy"]["rotate"]``: the table's ``rotate_every``, default
    none; ``table_args``: ``env_id0``, ``scenarios``, ``ranges``, ``names``)."""
    files = config["policy"].get("onnx_files")
    if files:
        if config["policy"].get("use_lstm"):
            raise ValueError("build_policy: a policy table takes MLP actors only (recurrent policies in a table are out of scope)")
        if config["policy"].get("rotate") is not None:
            table_args = {"rotate_every": config["policy"]["rotate"], **table_args}
        return open_policy_table(list(files), num_envs=num_envs, device=device, assign=config["policy"].get("assign", "interleave"), **table_args)
    if config["policy"]["use_lstm"]:
        return LSTMPolicy(config, policy_path, num_envs=num_envs, device=device)
    return MLPPolicy(policy_path, device=device)


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
                     bias_scale: float = 0.0):
    """A random-weight actor with the usual export shape (Gemm + activation ... Gemm): stands in for the missing policy files.
    Biases are ``bias_scale * standard_normal`` from a generator of their own: the default 0 writes all-zero biases and exactly the
    weights (and bytes) earlier versions wrote for the same seed."""
    rng = np.random.default_rng(seed)
    brng = np.random.default_rng([seed, 1])
    dims = [state_dim, *hidden, action_dim]
    nodes, init, x = [], {}, "obs"
    for li in range(len(dims) - 1):
        w = (rng.standard_normal((dims[li + 1], dims[li])) / np.sqrt(dims[li])).astype(np.float32)
        b = (bias_scale * brng.standard_normal(dims[li + 1])).astype(np.float32) if bias_scale else np.zeros(dims[li + 1], dtype=np.float32)
        init[f"w{li}"], init[f"b{li}"] = w, b
        y = f"h{li}" if li < len(dims) - 2 else "actions"
        nodes.append({"op": "Gemm", "inputs": [x, f"w{li}", f"b{li}"], "outputs": [y + "_lin" if li < len(dims) - 2 else y], "attrs": {"transB": 1}})
        if li < len(dims) - 2:
            nodes.append({"op": activation, "inputs": [y + "_lin"], "outputs": [y]})
        x = y
    write_onnx(path, nodes, init, ["obs"], ["actions"])
