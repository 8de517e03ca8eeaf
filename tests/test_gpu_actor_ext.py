"""Extended actors on the device: ``cosim_mlp_forward_ex`` (mlp_forward_ext_kernel, csrc/cosim_mlp.hip) through ``MLPPolicy`` against
plain fp64 numpy and against the interpreter on the same device -- observation normaliser, LayerNorm ahead of and behind the activation
and on the observation, MatMul + Add layers, the output stage -- at the tile edges; unclipped outputs; the input stage bit for bit;
row independence and non-finite rows; which path runs; and that empty extras leave a plain chain's bits alone.

Tolerances are the project's: 2e-5 absolute against fp64 (rtol 2e-5 on top for unclipped outputs).  The cases, their seeds and the
fp64 reference live in tests/actor_ext_graphs.py."""
import ctypes

import numpy as np
import pytest

import actor_ext_graphs as G
from actor_ext_graphs import ATOL, BATCHES
from cosim_amd.policy import MLPPolicy, write_onnx

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _policies(tmp_path, spec, **how):
    p = str(tmp_path / "actor.onnx")
    G.write_actor(p, spec, **how)
    fused, interp = MLPPolicy(p, device=DEV, fused=True), MLPPolicy(p, device=DEV, fused=False)
    assert fused._fused is not None and interp._fused is None
    assert MLPPolicy(p, device=DEV)._fused is not None                # the default takes the fused path too
    return fused, interp


def _forward_ex(f, xd, clip, extras="own"):
    """cosim_mlp_forward_ex called directly on a policy's arrays; ``extras``: the policy's own, or a ctypes pointer / None."""
    import torch
    out = torch.full((xd.shape[0], f["out_dim"]), 7.0, dtype=torch.float32, device=DEV)
    ex = (ctypes.byref(f["extras"]) if f["extras"] is not None else None) if isinstance(extras, str) else extras
    rc = f["L"].cosim_mlp_forward_ex(xd.data_ptr(), xd.shape[0], f["nl"], f["dims"], f["w"], f["b"], f["act"], f["alpha"], ex, clip, out.data_ptr(),
                                     torch.cuda.current_stream().cuda_stream)
    assert rc == 0, f["L"].cosim_last_error()
    return out


# ---------------------------------------------------------------------------------------------- 1: against fp64 and the interpreter
@pytest.mark.parametrize("name", list(G.CASES))
def test_fused_extended_actor_matches_fp64_and_the_interpreter(tmp_path, name):
    """Every case at n = 1, 31, 32, 33, 65: fused against fp64, the interpreter on the GPU against fp64, fused against the interpreter,
    all at 2e-5.  The errors are printed per batch size (pytest -s) before they are asserted."""
    import torch
    dims, spec = G.make_case(name)
    fused, interp = _policies(tmp_path, spec)
    assert (fused._fused["extras"] is None) == (name == "matmul_add")     # MatMul + Add is a plain chain once it is matched: the plain kernel
    for n in BATCHES:
        x = G.inputs(n, dims[0], seed=n + 17)
        ref = G.ref_actor(x, spec)
        inside = np.mean(np.abs(ref) < 1.0)
        assert inside >= 0.5, (name, n, inside)                          # saturated outputs would hide errors
        ref = np.clip(ref, -1.0, 1.0)
        xd = torch.tensor(x, device=DEV)
        a, b = fused.get_action(xd).cpu().numpy(), interp.get_action(xd).cpu().numpy()
        print(f"{name} n={n}: inside={inside:.2f} fused-fp64={np.abs(a - ref).max():.2e} interp-fp64={np.abs(b - ref).max():.2e} "
              f"fused-interp={np.abs(a - b).max():.2e}")
        assert a.shape == (n, dims[-1])
        np.testing.assert_allclose(a, ref, rtol=0, atol=ATOL, err_msg=f"{name} n={n} fused vs fp64")
        np.testing.assert_allclose(b, ref, rtol=0, atol=ATOL, err_msg=f"{name} n={n} interpreter vs fp64")
        np.testing.assert_allclose(a, b, rtol=0, atol=ATOL, err_msg=f"{name} n={n} fused vs interpreter")
    if name == "normaliser_clip_float4":                                 # the row scaled by 10 reaches the input clip
        z = G.stage64(G.inputs(33, dims[0], seed=50).astype(np.float64), spec["input"][:2])
        assert np.abs(z).max() > 5.0


# ---------------------------------------------------------------------------------------------- 2: unclipped
@pytest.mark.parametrize("name", ["normaliser", "layernorm_before_and_after"])
def test_fused_extended_actor_unclipped_outputs_match_fp64(tmp_path, name):
    """cosim_mlp_forward_ex called directly with clip = 0: the row scaled by 10 is compared at its full size."""
    import torch
    dims, spec = G.make_case(name)
    fused, _ = _policies(tmp_path, spec)
    x = G.inputs(33, dims[0], seed=5)
    ref = G.ref_actor(x, spec)
    out = _forward_ex(fused._fused, torch.tensor(x, device=DEV), 0.0).cpu().numpy()
    print(f"{name}: unclipped max |error| = {np.abs(out - ref).max():.2e}, max |ref| = {np.abs(ref).max():.2f}")
    if name == "normaliser":
        assert np.abs(ref).max() > 1.0                                   # the clip would have changed the result
    np.testing.assert_allclose(out, ref, rtol=2e-5, atol=ATOL)


# ---------------------------------------------------------------------------------------------- 3: the input stage alone
def test_input_stage_alone_is_the_interpreters_bit_for_bit(tmp_path):
    """Identity weight (width 8, no bias, no activation) behind Sub, Div, Clip: with clip = 0 the fused output is the input stage's, and
    each of its items is the one fp32 operation the node names -- so it equals the interpreter's Sub / Div / Clip to the bit (the
    identity product adds exact zeros: x * 1 + 0 * ...).  Also Mul and Add in a row (no contraction into an FMA), non-finite inputs."""
    import torch
    rng = np.random.default_rng(8)
    W = 8
    for items in ([("Sub", rng.standard_normal(W)), ("Div", rng.uniform(0.5, 2.0, W)), ("Clip", (-5.0, 5.0))],
                  [("Mul", rng.uniform(0.5, 2.0, W)), ("Add", rng.standard_normal(W)), ("Div", rng.uniform(0.5, 2.0, W)), ("Clip", (None, 1.5))]):
        spec = {"input": [(op, c if op == "Clip" else np.asarray(c, np.float32)) for op, c in items], "ln0": None, "output": [],
                "layers": [{"w": np.eye(W, dtype=np.float32), "b": None, "act": None, "alpha": 1.0, "alpha_attr": None, "ln": None, "matmul": False}]}
        fused, interp = _policies(tmp_path, spec)
        x = G.inputs(65, W, seed=9)
        x[3, 2], x[7, 0] = np.nan, np.inf
        if items[-1][1][0] is not None:                                  # with a lower bound -inf becomes finite again ahead of the product
            x[40, 5] = -np.inf
        xd = torch.tensor(x, device=DEV)
        got = _forward_ex(fused._fused, xd, 0.0)
        want = interp.graph.run({interp.input_name: xd})[0]
        assert np.abs(want[torch.isfinite(want)].cpu().numpy()).max() > 1.4          # nothing here was clipped to [-1, 1]
        assert torch.equal(torch.isnan(got), torch.isnan(want)) and bool(torch.isnan(got).any())
        assert torch.equal(got.nan_to_num(nan=123.0), want.nan_to_num(nan=123.0))


# ---------------------------------------------------------------------------------------------- 4: rows are independent
def test_row_slices_and_non_finite_rows_do_not_touch_other_rows(tmp_path):
    """A row's LayerNorm statistics are a function of its own columns: get_action_into on slices that cut the 32-row tiles gives the
    rows of the full forward bit for bit, and a NaN row and a +inf row among 65 leave every other row's bits alone; the bad rows' NaN
    pattern is the interpreter's."""
    import torch
    dims, spec = G.make_case("layernorm_before_and_after")
    fused, interp = _policies(tmp_path, spec)
    x = G.inputs(65, dims[0], seed=3)
    xd = torch.tensor(x, device=DEV)
    full = fused.get_action(xd).clone()
    np.testing.assert_allclose(full.cpu().numpy(), np.clip(G.ref_actor(x, spec), -1.0, 1.0), rtol=0, atol=ATOL)
    for lo, hi in ((0, 31), (31, 64), (64, 65)):
        out = torch.full((65, dims[-1]), 7.0, dtype=torch.float32, device=DEV)
        fused.get_action_into(xd[lo:hi], out[lo:hi])
        assert torch.equal(out[lo:hi], full[lo:hi])
        assert bool((out[:lo] == 7.0).all()) and bool((out[hi:] == 7.0).all())
    r_nan, r_inf = 3, 35
    bad = x.copy()
    bad[r_nan] = np.nan
    bad[r_inf, 0] = np.inf
    bd = torch.tensor(bad, device=DEV)
    a, b = fused.get_action(bd).clone(), interp.get_action(bd)
    good = torch.tensor([r for r in range(65) if r not in (r_nan, r_inf)], device=DEV)
    assert torch.equal(a[good], full[good])
    an, bn = a.cpu().numpy(), b.cpu().numpy()
    print("fused bad rows:", an[[r_nan, r_inf]], "interpreter:", bn[[r_nan, r_inf]])
    assert np.isnan(an[r_nan]).all() and np.array_equal(np.isnan(an), np.isnan(bn))
    np.testing.assert_allclose(an[[r_nan, r_inf]], bn[[r_nan, r_inf]], rtol=0, atol=ATOL, equal_nan=True)


# ---------------------------------------------------------------------------------------------- 5: which path runs
def test_decomposed_layernorm_stays_with_the_interpreter(tmp_path):
    import torch
    p = str(tmp_path / "decomposed.onnx")
    dims, spec = G.decomposed_layernorm_actor(p)
    pol = MLPPolicy(p, device=DEV)
    assert pol._fused is None
    with pytest.raises(ValueError, match="fused=True.*'ReduceMean'"):
        MLPPolicy(p, device=DEV, fused=True)
    x = G.inputs(33, dims[0], seed=9) * np.float32(0.5)
    ref = G.ref_actor(x, spec)
    assert np.mean(np.abs(ref) < 1.0) >= 0.5
    np.testing.assert_allclose(pol.get_action(torch.tensor(x, device=DEV)).cpu().numpy(), np.clip(ref, -1.0, 1.0), rtol=0, atol=ATOL)


def test_forward_ex_refuses_what_the_validator_refuses(tmp_path):
    """The C entry point on bad extras: COSIM_EINVAL, the field in cosim_last_error, and the output is not touched."""
    import torch
    from cosim_amd.policy import _Extras
    dims, spec = G.make_case("layernorm_before_and_after")
    fused, _ = _policies(tmp_path, spec)
    f = fused._fused
    xd = torch.tensor(G.inputs(5, dims[0], seed=1), device=DEV)
    out = torch.full((5, dims[-1]), 7.0, dtype=torch.float32, device=DEV)

    def call(e):
        return f["L"].cosim_mlp_forward_ex(xd.data_ptr(), 5, f["nl"], f["dims"], f["w"], f["b"], f["act"], f["alpha"], ctypes.byref(e), 1.0, out.data_ptr(),
                                           torch.cuda.current_stream().cuda_stream)
    for change, want in ((lambda e: setattr(e, "n_in", 5), "cosim_mlp_forward_ex: input stage: 5 items, outside 0..4"),
                         (lambda e: (setattr(e, "n_out", 1), e.out_op.__setitem__(0, 7)), "output stage, item 0: unknown op code 7"),
                         (lambda e: (setattr(e, "n_in", 1), e.in_op.__setitem__(0, 2)), "input stage, item 0: null vector"),
                         (lambda e: e.ln_eps.__setitem__(1, 0.0), "LayerNorm slot 1: eps 0.000000 is not a positive finite number"),
                         (lambda e: (e.ln_where.__setitem__(3, 1), e.ln_eps.__setitem__(3, 1e-5)), "LayerNorm slot 3: LayerNorm on the last layer"),
                         (lambda e: e.ln_gamma.__setitem__(2, None), "LayerNorm slot 2: null scale vector")):
        e = _Extras.from_buffer_copy(f["extras"])
        change(e)
        assert call(e) == -1 and want in f["L"].cosim_last_error().decode(), want
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


# ---------------------------------------------------------------------------------------------- 6: plain chains are untouched
PLAIN = {"leaky_elu_float4": ((12, 40, 36, 4), [("LeakyRelu", 0.2), ("Elu", 0.3), None], 0.1),
         "six_layers": ((9, 34, 31, 33, 30, 35, 2), ["Relu", None, "Tanh", "Sigmoid", "Elu", "Tanh"], 0.5)}


@pytest.mark.parametrize("name", list(PLAIN))
def test_empty_extras_give_the_bits_of_the_plain_entry_point(tmp_path, name):
    """Two chains of tests/test_gpu_policy_kernels.py: cosim_mlp_forward_ex with null and with all-zero extras against cosim_mlp_forward."""
    import torch
    from cosim_amd.policy import _Extras
    dims, acts, last_scale = PLAIN[name]
    layers = G.make_layers(dims, [a if a is None or isinstance(a, str) else a[0] for a in acts], seed=sum(map(ord, name)), last_scale=last_scale)
    for L, a in zip(layers, acts):
        if isinstance(a, tuple):
            L["alpha"], L["alpha_attr"] = float(np.float32(a[1])), a[1]
    spec = {"layers": layers}
    fused, _ = _policies(tmp_path, spec)
    f = fused._fused
    assert f["extras"] is None
    for n in (33, 65):
        xd = torch.tensor(G.inputs(n, dims[0], seed=n), device=DEV)
        for clip in (1.0, 0.0):
            want = torch.full((n, dims[-1]), 7.0, dtype=torch.float32, device=DEV)
            assert f["L"].cosim_mlp_forward(xd.data_ptr(), n, f["nl"], f["dims"], f["w"], f["b"], f["act"], f["alpha"], clip, want.data_ptr(),
                                            torch.cuda.current_stream().cuda_stream) == 0
            zero = _Extras()
            assert torch.equal(_forward_ex(f, xd, clip, extras=None), want) and torch.equal(_forward_ex(f, xd, clip, extras=ctypes.byref(zero)), want)
        np.testing.assert_allclose(want.cpu().numpy(), G.ref_actor(xd.cpu().numpy(), spec), rtol=2e-5, atol=ATOL)
