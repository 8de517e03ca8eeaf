"""Batched on-device policies: the counterpart of the reference's ``core/policy.py:5-54`` for N environments.

The reference runs an ONNX file through onnxruntime on the CPU, one state at a time (``MLPPolicy.get_action`` :11-21,
``LSTMPolicy.get_action`` :34-47, ``build_policy`` :49-53).  Here the same contract — ``get_action(state) -> action``
clipped to [-1, 1], LSTM ``h``/``c`` carried between calls — is kept over ``[N, state_dim]`` device tensors, so the
rollout loop never leaves the GPU.  onnxruntime and the ``onnx`` package are not available in this
build, so the file is read with a small protobuf wire-format decoder (``read_onnx``) and the graph is run by a tiny
interpreter over the operator subset RL policy exports use (Gemm / MatMul / Add / activations / LSTM / shape glue);
both, and the writer of synthetic policies, live in ``onnx_io.py`` and are re-exported here.
The GEMMs go through torch (rocBLAS / hipBLASLt): plain library matrix products, not part of the §8 hot path.

Two rules the tests pin.  Non-finite values: a NaN that reaches the output stays NaN on both paths (the interpreter's ``clamp``, like
the reference's ``np.clip``, propagates it; the fused kernel's Relu and final clip do the same), +-inf is clipped to +-1, and a bad
row never touches another row.  Initialisers stored as fp16 or fp64 are cast to fp32 when the graph is loaded (such a graph runs
through the interpreter; the fused kernel takes fp32 files only).

PARITY UNPINNED against onnxruntime (no policy file ships with the reference; onnxruntime is absent): the
tests compare with a numpy evaluation of the same graph.
"""
from __future__ import annotations

import ctypes
import os
from typing import Optional

import numpy as np

from .onnx_io import (OnnxGraph, _enc, _enc_varint, read_onnx, write_onnx, write_random_lstm, write_random_mlp,  # noqa: F401 (re-exported)
                      write_recurrent_actor)

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


_STAGE_OP = {"Add": 1, "Sub": 2, "Mul": 3, "Div": 4, "Clip": 5}      # the op codes of cosim_mlp_extras_t (include/cosim_actor.h)


def _actor_graph(model: dict):
    """The graph as an EXTENDED actor -- what ``cosim_mlp_forward_ex`` and ``cosim_policy_table_create_ex`` evaluate in one launch:

        actor  := input{0..4} [LN] layer{1..6} output{0..4}
        input  := Sub(x, c) | Div(x, c) | Add | Mul (either operand order) | Clip(x, lo, hi)
        layer  := linear [LN] [act]  |  linear act LN            (the last layer carries no LN)
        linear := Gemm(transB=1, alpha=beta=1)  |  MatMul(x, Wt) [Add(., b)]
        output := Mul | Add | Sub(y, c) | Div(y, c) | Clip(y, lo, hi)

    ``c``: an fp32 initialiser or ``Constant`` output of shape ``[]``, ``[1]``, ``[W]`` or ``[1, W]``; ``LN``: ``LayerNormalization`` over the
    last axis with a scale; activations: those of ``_ACT``; widths 1..512.  Returns ``(description, None)`` or ``(None, reason)`` with
    the reason naming the node.  ``description``: ``layers`` -- what ``_mlp_chain`` returns (for every graph it accepts: exactly that,
    and nothing else below); ``input`` / ``output`` -- stage items ``(code, vector [W] or None, lo, hi)``; ``ln`` -- ``{slot: (where, scale,
    bias or None, eps)}``, slot 0 the observation, ``l + 1`` layer ``l``, where 1 ahead of the activation and 2 behind it."""
    if len(model["inputs"]) != 1 or len(model["outputs"]) != 1:
        return None, f"{len(model['inputs'])} graph inputs and {len(model['outputs'])} outputs, not one of each"
    init = dict(model["init"])
    body = []
    for n in model["nodes"]:
        if n["op"] == "Constant" and isinstance(n["attrs"].get("value"), np.ndarray):
            init[n["outputs"][0]] = n["attrs"]["value"]
        else:
            body.append(n)
    used = {name for n in body for name in n["inputs"]} | set(model["outputs"])

    def tag(n):
        return f"node '{n['op']}' -> '{n['outputs'][0] if n['outputs'] else ''}'"

    def stage_item(n, cur):
        """A stage item on ``cur``: ``((code, constant or None, lo, hi), None)`` or ``(None, reason)``."""
        ins = [i for i in n["inputs"]]
        if n["op"] == "Clip":
            if not ins or ins[0] != cur:
                return None, f"{tag(n)} does not clip the tensor before it"
            bounds = []
            for k, key in ((1, "min"), (2, "max")):
                v = n["attrs"].get(key)
                if len(ins) > k and ins[k]:
                    if ins[k] not in init or np.asarray(init[ins[k]]).size != 1:
                        return None, f"{tag(n)}: bound '{ins[k]}' is not a constant scalar"
                    if np.asarray(init[ins[k]]).dtype != np.float32:
                        return None, f"{tag(n)}: bound '{ins[k]}' is {np.asarray(init[ins[k]]).dtype}, not fp32"
                    v = float(np.asarray(init[ins[k]]).ravel()[0])
                bounds.append(v)
            lo, hi = (-np.inf if bounds[0] is None else float(bounds[0])), (np.inf if bounds[1] is None else float(bounds[1]))
            return (5, None, lo, hi), None
        if len(ins) != 2 or cur not in ins:
            return None, f"{tag(n)} does not take the tensor before it and a constant"
        other = ins[1] if ins[0] == cur else ins[0]
        if n["op"] in ("Sub", "Div") and ins[0] != cur:
            return None, f"{tag(n)}: {'c - x' if n['op'] == 'Sub' else 'c / x'} (the constant on the left) is outside the fused subset"
        if other not in init:
            return None, f"{tag(n)}: operand '{other}' is not a constant"
        c = np.asarray(init[other])
        if c.dtype != np.float32:
            return None, f"{tag(n)}: constant '{other}' is {c.dtype}, not fp32"
        return (_STAGE_OP[n["op"]], c, 0.0, 0.0), None

    def widen(items, W, what):
        """The items' constants broadcast to vectors ``[W]``: ``(items, None)`` or ``(None, reason)``."""
        out = []
        for code, c, lo, hi in items:
            if c is not None:
                if c.shape not in ((), (1,), (W,), (1, W)):
                    return None, f"a constant of shape {c.shape} in the {what} stage, whose width is {W}"
                c = np.ascontiguousarray(np.broadcast_to(c.reshape(-1), (W,)), dtype=np.float32)
            out.append((code, c, lo, hi))
        return out, None

    def layer_norm(n, cur, W):
        a, ins = n["attrs"], n["inputs"]
        if not ins or ins[0] != cur:
            return None, f"{tag(n)} does not normalise the tensor before it"
        if a.get("axis", -1) not in (-1, 1):
            return None, f"{tag(n)}: axis {a.get('axis')} (the last axis only)"
        if len(ins) < 2 or not ins[1]:
            return None, f"{tag(n)}: LayerNormalization without scale"
        if any(o and o in used for o in n["outputs"][1:]):
            return None, f"{tag(n)}: its Mean / InvStdDev outputs are used"
        g = init.get(ins[1])
        b = init.get(ins[2]) if len(ins) > 2 and ins[2] else None
        if g is None or (len(ins) > 2 and ins[2] and b is None):
            return None, f"{tag(n)}: scale or bias is not an initialiser"
        if g.dtype != np.float32 or (b is not None and b.dtype != np.float32):
            return None, f"{tag(n)}: scale or bias is not fp32"
        if W is not None and (g.shape != (W,) or (b is not None and b.shape != (W,))):
            return None, f"{tag(n)}: scale {g.shape} / bias {None if b is None else b.shape} for width {W}"
        eps = float(np.float32(a.get("epsilon", 1e-5)))
        if not (np.isfinite(eps) and eps > 0):
            return None, f"{tag(n)}: epsilon {eps}"
        return (g, b, eps), None

    i, cur = 0, model["inputs"][0]
    raw_in, ln, layers = [], {}, []
    while i < len(body) and body[i]["op"] in _STAGE_OP:
        if len(raw_in) == 4:
            return None, f"{tag(body[i])}: a fifth item in the input stage (at most 4)"
        item, why = stage_item(body[i], cur)
        if item is None:
            return None, why
        raw_in.append(item)
        cur, i = body[i]["outputs"][0], i + 1
    if i < len(body) and body[i]["op"] == "LayerNormalization":
        got, why = layer_norm(body[i], cur, None)
        if got is None:
            return None, why
        ln[0] = (1, *got)
        cur, i = body[i]["outputs"][0], i + 1
    while i < len(body) and body[i]["op"] in ("Gemm", "MatMul"):
        n = body[i]
        a, ins = n["attrs"], n["inputs"]
        if n["op"] == "Gemm":
            if ins[0] != cur or a.get("transB", 0) != 1 or a.get("transA", 0) or a.get("alpha", 1.0) != 1.0 or a.get("beta", 1.0) != 1.0:
                return None, f"{tag(n)}: not Gemm(transB=1, alpha=beta=1, transA=0) on the tensor before it"
            if ins[1] not in model["init"]:
                return None, f"{tag(n)}: weight '{ins[1]}' is not an initialiser"
            w = model["init"][ins[1]]
            b = model["init"].get(ins[2]) if len(ins) > 2 and ins[2] else None
            if w.ndim != 2 or w.dtype != np.float32 or (b is not None and (b.shape != (w.shape[0],) or b.dtype != np.float32)) or \
                    (len(ins) > 2 and ins[2] and b is None):
                return None, f"{tag(n)}: weight or bias is not an fp32 initialiser of shape [O, I] / [O]"
            cur, i = n["outputs"][0], i + 1
        else:
            if len(ins) != 2 or ins[0] != cur or ins[1] not in model["init"]:
                return None, f"{tag(n)}: MatMul with a non-initialiser weight (x @ Wt with Wt an initialiser [I, O] only)"
            wt = model["init"][ins[1]]
            if wt.ndim != 2 or wt.dtype != np.float32:
                return None, f"{tag(n)}: weight '{ins[1]}' is {wt.dtype} {wt.shape}, not fp32 [I, O]"
            w, b = np.ascontiguousarray(wt.T), None
            cur, i = n["outputs"][0], i + 1
            if i < len(body) and body[i]["op"] == "Add" and cur in body[i]["inputs"] and len(body[i]["inputs"]) == 2:
                other = [x for x in body[i]["inputs"] if x != cur]
                c = init.get(other[0]) if other else None
                if c is not None and c.dtype == np.float32 and c.shape == (w.shape[0],):
                    b = c
                    cur, i = body[i]["outputs"][0], i + 1
        if len(layers) == 6:
            return None, f"{tag(n)}: a seventh layer (1..6)"
        if max(w.shape) > 512:
            return None, f"{tag(n)}: width {max(w.shape)} (1..512)"
        if layers and w.shape[1] != layers[-1][0].shape[0]:
            return None, f"{tag(n)}: input width {w.shape[1]} differs from the layer before it ({layers[-1][0].shape[0]})"
        act, alpha, where, norm = 0, 1.0, 0, None
        for _ in range(2):
            if i < len(body) and body[i]["op"] in _ACT and body[i]["inputs"] == [cur] and act == 0:
                act = _ACT[body[i]["op"]]
                alpha = float(body[i]["attrs"].get("alpha", 1.0 if act == 3 else 0.01))
                cur, i = body[i]["outputs"][0], i + 1
            elif i < len(body) and body[i]["op"] == "LayerNormalization" and norm is None:
                norm, why = layer_norm(body[i], cur, w.shape[0])
                if norm is None:
                    return None, why
                where = 2 if act else 1
                cur, i = body[i]["outputs"][0], i + 1
        if norm is not None:
            ln[len(layers) + 1] = (where, *norm)
        layers.append((w, b, act, alpha))
    if not layers:
        return None, (f"{tag(body[i])} is not part of the fused actor grammar" if i < len(body) else "no linear layer")
    raw_out = []
    while i < len(body) and body[i]["op"] in _STAGE_OP:
        if len(raw_out) == 4:
            return None, f"{tag(body[i])}: a fifth item in the output stage (at most 4)"
        item, why = stage_item(body[i], cur)
        if item is None:
            return None, why
        raw_out.append(item)
        cur, i = body[i]["outputs"][0], i + 1
    if i < len(body):
        return None, f"{tag(body[i])} is not part of the fused actor grammar"
    if cur != model["outputs"][0]:
        return None, f"the graph output '{model['outputs'][0]}' is not the end of the chain ('{cur}')"
    if len(layers) in ln:
        return None, "LayerNormalization on the last layer"
    in_dim = layers[0][0].shape[1]
    if 0 in ln and (ln[0][1].shape != (in_dim,) or (ln[0][2] is not None and ln[0][2].shape != (in_dim,))):
        return None, f"LayerNormalization on the observation: scale {ln[0][1].shape} for width {in_dim}"
    stage_in, why = widen(raw_in, in_dim, "input")
    if stage_in is None:
        return None, why
    stage_out, why = widen(raw_out, layers[-1][0].shape[0], "output")
    if stage_out is None:
        return None, why
    return {"layers": layers, "input": stage_in, "output": stage_out, "ln": ln}, None


class _Extras(ctypes.Structure):
    """``cosim_mlp_extras_t`` (include/cosim_actor.h)."""
    _fields_ = [("n_in", ctypes.c_int32), ("n_out", ctypes.c_int32), ("in_op", ctypes.c_int32 * 4), ("out_op", ctypes.c_int32 * 4),
                ("in_vec", ctypes.c_void_p * 4), ("out_vec", ctypes.c_void_p * 4),
                ("in_lo", ctypes.c_float * 4), ("in_hi", ctypes.c_float * 4), ("out_lo", ctypes.c_float * 4), ("out_hi", ctypes.c_float * 4),
                ("ln_where", ctypes.c_int32 * 7), ("ln_eps", ctypes.c_float * 7), ("ln_gamma", ctypes.c_void_p * 7), ("ln_beta", ctypes.c_void_p * 7)]


def _has_extras(desc: dict) -> bool:
    return bool(desc["input"] or desc["output"] or desc["ln"])


def _fill_extras(e: "_Extras", desc: dict, place):
    """One actor's extras into ``e``; ``place(array) -> address`` puts a vector where the callee reads it (device or host) and keeps it."""
    e.n_in, e.n_out = len(desc["input"]), len(desc["output"])
    for items, op, vec, lo, hi in ((desc["input"], e.in_op, e.in_vec, e.in_lo, e.in_hi), (desc["output"], e.out_op, e.out_vec, e.out_lo, e.out_hi)):
        for k, (code, c, l, h) in enumerate(items):
            op[k], lo[k], hi[k] = code, l, h
            vec[k] = None if c is None else place(c)
    for slot, (where, g, b, eps) in desc["ln"].items():
        e.ln_where[slot], e.ln_eps[slot] = where, eps
        e.ln_gamma[slot], e.ln_beta[slot] = place(g), None if b is None else place(b)


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

    A graph of the fused actor grammar (``_actor_graph``: a Gemm / activation chain, optionally with an observation normaliser,
    LayerNorm, MatMul + Add layers and an output stage) runs as ONE launch of the engine's fused MFMA kernel (``cosim_mlp_forward``, or
    ``cosim_mlp_forward_ex`` when it has any of the extras; csrc/cosim_mlp.hip) when the policy lives on a GPU; anything else goes
    through the interpreter.  ``_fused`` is not None exactly when the fused path runs."""

    def __init__(self, policy_path: str, device=None, fused: Optional[bool] = None):
        import torch
        self.torch = torch
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        model = read_onnx(policy_path)
        self.graph = OnnxGraph(model, self.device)
        self.input_name = self.graph.inputs[0]
        desc, why = _actor_graph(model) if (fused is not False and self.device.type == "cuda") else (None, f"the device is '{self.device}', not a GPU")
        if fused and desc is None:
            raise ValueError(f"fused=True needs a graph of the fused actor grammar (a Gemm/activation chain and its extras) on a GPU device: {why}")
        self._fused = None
        if desc is not None:
            from .engine import load_library
            chain = desc["layers"]
            ws = [torch.as_tensor(np.ascontiguousarray(w), device=self.device) for w, *_ in chain]
            bs = [None if b is None else torch.as_tensor(np.ascontiguousarray(b), device=self.device) for _, b, *_ in chain]
            nl = len(chain)
            extras, vecs = None, []
            if _has_extras(desc):
                def place(a):
                    vecs.append(torch.as_tensor(np.array(a, dtype=np.float32), device=self.device))
                    return vecs[-1].data_ptr()
                extras = _Extras()
                _fill_extras(extras, desc, place)
            self._fused = dict(
                L=load_library(), nl=nl, keep=(ws, bs, vecs), extras=extras,
                dims=(ctypes.c_int * (nl + 1))(chain[0][0].shape[1], *[w.shape[0] for w, *_ in chain]),
                w=(ctypes.c_void_p * nl)(*[w.data_ptr() for w in ws]),
                b=(ctypes.c_void_p * nl)(*[None if b is None else b.data_ptr() for b in bs]),
                act=(ctypes.c_int * nl)(*[a for *_, a, _ in chain]),
                alpha=(ctypes.c_float * nl)(*[al for *_, al in chain]),
                out_dim=chain[-1][0].shape[0], in_dim=chain[0][0].shape[1], out=None)

    graph_safe = True     # stateless: get_action is pure device work

    def _forward(self, x, out):
        """One launch of the fused kernel on the CURRENT stream: ``out[:] = actor(x)``, both contiguous fp32 rows on the policy's device."""
        f = self._fused
        stream = self.torch.cuda.current_stream(self.device).cuda_stream
        if f["extras"] is None:
            rc = f["L"].cosim_mlp_forward(x.data_ptr(), x.shape[0], f["nl"], f["dims"], f["w"], f["b"], f["act"], f["alpha"], 1.0, out.data_ptr(), stream)
        else:
            rc = f["L"].cosim_mlp_forward_ex(x.data_ptr(), x.shape[0], f["nl"], f["dims"], f["w"], f["b"], f["act"], f["alpha"], ctypes.byref(f["extras"]),
                                             1.0, out.data_ptr(), stream)
        if rc != 0:
            raise RuntimeError(f["L"].cosim_last_error().decode())

    def get_action(self, state):
        t = self.torch
        s = t.as_tensor(state, dtype=t.float32, device=self.device)
        single = s.dim() == 1
        x = s.unsqueeze(0) if single else s
        f = self._fused
        if f is not None and x.shape[1] == f["in_dim"]:
            if f["out"] is None or f["out"].shape[0] != x.shape[0]:
                f["out"] = t.empty((x.shape[0], f["out_dim"]), dtype=t.float32, device=self.device)
            out = f["out"]
            self._forward(x.contiguous(), out)
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
        self._forward(state_rows, out_rows)


def _take_rows(t, dst, stored, src, mask, name: str):
    """Env ``d`` takes row ``src[d]`` of the stored ``[N, ...]`` tensor (``src`` None: row ``d``) into ``dst``; envs with ``mask[d] == 0`` keep
    theirs.  In place, so a captured graph keeps seeing the same tensor.  A shape other than ``dst``'s is refused under ``name``."""
    x = t.as_tensor(stored, dtype=dst.dtype, device=dst.device)
    if src is not None:
        x = x[t.as_tensor(src, device=dst.device).long()]
    if tuple(x.shape) != tuple(dst.shape):
        raise ValueError(f"{name} has shape {tuple(x.shape)}, expected {tuple(dst.shape)}")
    if mask is not None:
        x = t.where((t.as_tensor(mask, device=dst.device) != 0)[(...,) + (None,) * (dst.dim() - 1)], x, dst)
    dst.copy_(x)


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
        for name, dst in (("h", self.h_in), ("c", self.c_in)):
            _take_rows(self.torch, dst[0], state[name], src, mask, f"LSTMPolicy.load_state: {name}")

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

    _entry = None         # the subclass's family of entry points: "cosim_policy_table" has _create, _rotate, _destroy ...
    _create_suffix = "_create"   # "_create_ex": a PolicyTable with an extended actor among its files
    recurrent = False     # a recurrent table's done flags also zero the state, so its static launch takes them too

    @staticmethod
    def _pack_layers(chains, first_widths, max_layers):
        """K chains of ``(w, b, act, alpha)`` layers as a create entry point takes them: ``((n, dims, act, alpha, w, b), keep)`` -- the ctypes
        arrays ``[K]``, ``[K][max_layers + 1]`` and four times ``[K][max_layers]`` (a null ``b``: no bias), and the host arrays they point
        into.  ``first_widths[k]``: the input width of chain ``k`` (a chain may be empty)."""
        K, ML = len(chains), max_layers
        ci, cf, vp = ctypes.c_int, ctypes.c_float, ctypes.c_void_p
        n, dims, act, alpha = (ci * K)(*[len(c) for c in chains]), (ci * (K * (ML + 1)))(), (ci * (K * ML))(), (cf * (K * ML))()
        w, b, keep = (vp * (K * ML))(), (vp * (K * ML))(), []
        for k, chain in enumerate(chains):
            dims[k * (ML + 1)] = first_widths[k]
            for li, (wl, bl, a, al) in enumerate(chain):
                q = k * ML + li
                dims[k * (ML + 1) + li + 1] = wl.shape[0]
                act[q], alpha[q] = a, al
                for arr, ptrs in ((wl, w), (bl, b)):
                    if arr is not None:
                        keep.append(np.ascontiguousarray(arr, dtype=np.float32))
                        ptrs[q] = keep[-1].ctypes.data
        return (n, dims, act, alpha, w, b), keep

    def _open(self, *policy_args):
        """The create entry point on the policies' arrays and the fleet's; arms a rotating table.  The library's words if create refuses."""
        from .engine import load_library
        L = load_library()
        por = np.ascontiguousarray(self.policy_of_env, dtype=np.int32)
        rng = np.ascontiguousarray(np.asarray(self.ranges, dtype=np.int32).reshape(-1, 2))
        handle = ctypes.c_void_p()
        with self.torch.cuda.device(self.device):
            if getattr(L, self._entry + self._create_suffix)(len(self.paths), *policy_args, self.num_envs, por.ctypes.data, len(self.ranges), rng.ctypes.data,
                                                    ctypes.byref(handle)) != 0:
                return L.cosim_last_error().decode()
            self._lib, self._handle = L, handle
            if self.rotate_every is not None and getattr(L, self._entry + "_rotate")(handle, self.rotate_every) != 0:
                raise RuntimeError(L.cosim_last_error().decode())

    def _setup_eval(self, fused, models, layers):
        """How the table evaluates: the library's table on a GPU (``_create(layers)``), else the torch twin over ``models``."""
        self._handle = None
        if fused is not False and self.device.type == "cuda":
            self._create(layers)
        elif fused:
            raise ValueError("fused=True needs a GPU device")
        else:
            self._rows, self._range_rows = self._policy_rows()
            self._graphs = [OnnxGraph(m, self.device) for m in models]

    def close(self):
        if self._handle is not None:
            getattr(self._lib, self._entry + "_destroy")(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass

    def _launch(self, x, out, i: int, done=None):
        """One evaluation of range ``i`` (-1: all): the rotating or the static library call, or the torch twin on the rows of each policy."""
        t = self.torch
        if x.shape != (self.num_envs, self.in_dim) or out.shape != (self.num_envs, self.out_dim):
            raise ValueError(f"{type(self).__name__}: state {tuple(x.shape)} / action {tuple(out.shape)}, expected ({self.num_envs}, {self.in_dim}) / "
                             f"({self.num_envs}, {self.out_dim})")
        if done is not None:
            self._check_done(done)
        rotating = self.rotate_every is not None
        if self._handle is None:
            self._twin(x, out, self._twin_rows(i, done) if rotating else (self._rows if i < 0 else self._range_rows[i]), done)
            return
        if not (x.is_cuda and out.is_cuda and x.dtype == t.float32 and out.dtype == t.float32 and x.is_contiguous() and out.is_contiguous()):
            raise ValueError(f"{type(self).__name__}: state and action must be contiguous fp32 tensors on the table's device")
        da, db = (None, None) if done is None else (done[0].data_ptr(), done[1].data_ptr())
        forward = self._forward_rotating if rotating else self._forward
        if forward(x.data_ptr(), out.data_ptr(), da, db, i, t.cuda.current_stream(self.device).cuda_stream) != 0:
            raise RuntimeError(self._lib.cosim_last_error().decode())

    def get_action(self, state):
        """``[N, action_dim]`` in [-1, 1]: the table's persistent output tensor (the next call overwrites it); a recurrent table's ``h`` /
        ``c`` move one step."""
        t = self.torch
        x = t.as_tensor(state, dtype=t.float32, device=self.device).contiguous()
        self._launch(x, self._out, -1)
        return self._out

    def get_action_range(self, i: int, state, action, done=None):
        """Writes the rows of range ``i`` of ``ranges`` into ``action`` (``[N, action_dim]``) from ``state`` (``[N, in_dim]``), both whole-fleet
        contiguous fp32 tensors, on the CURRENT stream and without allocating; the other rows of ``action`` (and of a recurrent table's
        ``h`` / ``c``) stay as they are.  ``done=(terminated, truncated)`` (uint8 ``[N]``): a rotating table needs it -- an env of the range
        with either set has ended an episode, and its counter advances in this very launch; a recurrent table starts such an env from
        a zero state; a static ``PolicyTable`` ignores it."""
        if not 0 <= int(i) < len(self.ranges):
            raise ValueError(f"{type(self).__name__}.get_action_range: range {i} outside 0..{len(self.ranges) - 1}")
        if self.rotate_every is None:
            self._launch(state, action, int(i), done if self.recurrent else None)
            return
        if done is None:
            raise ValueError(f"{type(self).__name__}.get_action_range: the table rotates, pass done=(terminated, truncated) (the range's episode "
                             "ends advance its counters in this launch)")
        self._launch(state, action, int(i), done)

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
        t = self.torch
        for d in done:
            if d.shape != (self.num_envs,) or d.dtype not in (t.uint8, t.bool) or not d.is_contiguous() or d.device != self._out.device:
                raise ValueError(f"{type(self).__name__}: done is (terminated, truncated), contiguous uint8 [{self.num_envs}] tensors on the table's device")

    def _load_counters(self, state, src, mask):
        """``load_state`` for the counters of a rotating table: env ``d`` takes ``state["episode"][src[d]]``, masked as the rest."""
        who = type(self).__name__
        if self.rotate_every is None:
            return
        if state is None or "episode" not in state:
            raise ValueError(f"{who}.load_state: the state carries no episode counters (it was taken from a table that does not rotate)")
        _take_rows(self.torch, self.episode, state["episode"], src, mask, f"{who}.load_state: episode")


class PolicyTable(_FleetTable):
    """K actor checkpoints over ONE fleet: env ``g`` (global id) is driven by policy ``policy_of(g)`` for the whole run, and one launch
    of the grouped kernel (``cosim_policy_table_forward``, csrc/cosim_mlp.hip) evaluates all of them -- every env gets the bits
    ``MLPPolicy(file, fused=True)`` gives it.  All policies meet the same terrain, spawn table, scenario table, fall rule and noise
    streams (those are keyed by global env id), so one run is the comparison; ``EpisodeLedger.by_policy`` / ``Verdicts.by_policy``
    break the outcomes down, and ``env.set_curve_groups(table)`` splits the response curves by policy (``curve_groups()``).

    ``assign``: ``"interleave"`` -- ``g mod K``; ``"cross"`` -- ``(g // S) mod K`` with ``S = scenarios`` (in scenario mode ``env``, where
    env ``g`` runs scenario ``g mod S``, every (scenario, policy) pair gets the same share of envs); or an int array with one entry per
    LOCAL env.  ``ranges``: the env's ``range_list`` (``get_action_range`` evaluates one of them on the current stream); default: one
    range.  Every file must be an actor of the fused grammar (``_actor_graph``: a Gemm / activation chain, optionally with an observation
    normaliser, LayerNorm, MatMul + Add layers and an output stage; plain and extended files may share a table) with the first file's
    input and output width.  On a
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
        chains, models, descs = [], [], []
        for p in paths:
            model = read_onnx(p)
            if any(n["op"] == "LSTM" for n in model["nodes"]):
                raise ValueError(f"PolicyTable: {p}: an LSTM policy (recurrent policies in a table are out of scope)")
            desc, why = _actor_graph(model)
            if desc is None:
                raise ValueError(f"PolicyTable: {p}: the graph is not a plain Gemm / activation chain (1..6 layers, widths up to 512, fp32) nor one with "
                                 f"the extras of the fused actor grammar: {why}")
            chain = desc["layers"]
            i0, o0 = (chains[0][0][0].shape[1], chains[0][-1][0].shape[0]) if chains else (chain[0][0].shape[1], chain[-1][0].shape[0])
            if chain[0][0].shape[1] != i0:
                raise ValueError(f"PolicyTable: {p}: input width {chain[0][0].shape[1]} differs from {i0} of {paths[0]}")
            if chain[-1][0].shape[0] != o0:
                raise ValueError(f"PolicyTable: {p}: output width {chain[-1][0].shape[0]} differs from {o0} of {paths[0]}")
            chains.append(chain)
            models.append(model)
            descs.append(desc)
        self._descs = descs
        self.in_dim, self.out_dim = int(chains[0][0][0].shape[1]), int(chains[0][-1][0].shape[0])
        self._setup_assign(assign, ranges)
        self._out = torch.zeros((N, self.out_dim), dtype=torch.float32, device=self.device)
        self._setup_rotate(rotate_every)
        if self.rotate_every is not None:
            self.reset = self._reset_rotating
        self._setup_eval(fused, models, chains)

    _entry = "cosim_policy_table"

    def _create(self, chains):
        layers, keep = self._pack_layers(chains, [c[0][0].shape[1] for c in chains], 6)   # keep: alive until create has copied them
        if any(_has_extras(d) for d in self._descs):      # one record per policy (all zero for a plain file), host vectors
            def place(a):
                keep.append(np.ascontiguousarray(a, dtype=np.float32))
                return keep[-1].ctypes.data
            extras = (_Extras * len(chains))()
            for e, d in zip(extras, self._descs):
                _fill_extras(e, d, place)
            self._create_suffix = "_create_ex"
            layers = (*layers, extras)
        msg = self._open(*layers)
        if msg is not None:
            raise RuntimeError(msg)

    def _forward(self, x, out, da, db, i, stream):
        return self._lib.cosim_policy_table_forward(self._handle, x, out, i, 1.0, stream)

    def _forward_rotating(self, x, out, da, db, i, stream):
        return self._lib.cosim_policy_table_forward_rotating(self._handle, x, out, self.episode.data_ptr(), self.policy_now.data_ptr(), da, db, i, 1.0,
                                                             stream)

    def _twin(self, x, out, rows, done):
        for g, idx in zip(self._graphs, rows):
            if idx.numel():
                out[idx] = g.run({g.inputs[0]: x[idx]})[0].clamp(-1.0, 1.0)

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
        self._setup_eval(fused, models, parts)

    _entry = "cosim_recurrent_table"

    def _create(self, parts):
        K, vp = len(parts), ctypes.c_void_p
        enc, keep_e = self._pack_layers([p["enc"] for p in parts], [p["in_dim"] for p in parts], 3)
        head, keep_h = self._pack_layers([p["head"] for p in parts], [p["H"] for p in parts], 3)
        cell = {key: [None if p[key] is None else np.ascontiguousarray(p[key], dtype=np.float32) for p in parts] for key in "WRB"}
        lstm_in, hidden = (ctypes.c_int * K)(*[p["I"] for p in parts]), (ctypes.c_int * K)(*[p["H"] for p in parts])
        W, R, B = ((vp * K)(*[None if a is None else a.ctypes.data for a in cell[key]]) for key in "WRB")
        msg = self._open(*enc, lstm_in, hidden, W, R, B, *head)
        if msg is not None:
            import re
            m = re.search(r": policy (\d+)", msg)              # the validator names the policy it refuses: name its file
            raise ValueError(f"RecurrentPolicyTable: {self.paths[int(m.group(1))] + ': ' if m else ''}{msg}")

    def _forward(self, x, out, da, db, i, stream):
        return self._lib.cosim_recurrent_table_forward(self._handle, x, self.h.data_ptr(), self.c.data_ptr(), out, da, db, i, 1.0, stream)

    def _forward_rotating(self, x, out, da, db, i, stream):
        return self._lib.cosim_recurrent_table_forward_rotating(self._handle, x, self.h.data_ptr(), self.c.data_ptr(), out, self.episode.data_ptr(),
                                                                self.policy_now.data_ptr(), da, db, i, 1.0, stream)

    def _twin(self, x, out, rows, done):
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
        for name, dst in (("h", self.h), ("c", self.c)):
            _take_rows(self.torch, dst, state[name], src, mask, f"RecurrentPolicyTable.load_state: {name}")
        self._load_counters(state, src, mask)


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
