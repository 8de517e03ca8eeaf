"""Policy tables with extended actors on the device: ``cosim_policy_table_create_ex`` / mlp_grouped_ext_kernel (csrc/cosim_mlp.hip).
One table of four files of the same widths -- a plain chain, a normaliser with clip, LayerNorm ahead of the activation, LayerNorm behind
it plus an output stage -- over 100 envs in two ranges: every env gets the bits of ``MLPPolicy(its file, fused=True)``, static and
rotating; the CPU-device twin agrees within the project's 2e-5; a file outside the grammar is refused by name."""
import numpy as np
import pytest

import actor_ext_graphs as G
from actor_ext_graphs import ATOL
from cosim_amd.policy import MLPPolicy, PolicyTable

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N, IN, OUT = 100, 12, 4
RANGES = [(0, 37), (37, 63)]


def _specs():
    f32 = np.float32
    rng = np.random.default_rng(123)

    def ln(w):
        return f32(1.0 + 0.3 * rng.standard_normal(w)), f32(0.2 * rng.standard_normal(w)), 1e-5

    def spec(dims, acts, seed):
        return {"input": [], "ln0": None, "output": [], "layers": G.make_layers(dims, acts, seed, last_scale=0.5)}
    plain = spec((IN, 40, 36, OUT), ["LeakyRelu", "Elu", None], 1)
    norm = spec((IN, 33, OUT), ["Elu", None], 2)
    norm["input"] = [("Sub", f32(0.5 * rng.standard_normal(IN))), ("Div", f32(rng.uniform(0.5, 2.0, IN))), ("Clip", (-5.0, 5.0))]
    before = spec((IN, 34, 31, OUT), ["Elu", "Tanh", None], 3)
    before["layers"][0]["ln"] = ("before", *ln(34))
    before["layers"][1]["ln"] = ("before", *ln(31))
    after = spec((IN, 20, OUT), ["Tanh", "Tanh"], 4)
    after["layers"][0]["ln"] = ("after", *ln(20))
    after["output"] = [("Mul", f32(rng.uniform(0.5, 1.5, OUT))), ("Add", f32(0.2 * rng.standard_normal(OUT))), ("Clip", (-0.8, 0.9))]
    return {"plain": plain, "normaliser_clip": norm, "ln_before": before, "ln_after_output": after}


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """The files, the single policies and what each of them gives on the whole batch: computed once, left unchanged."""
    import torch
    tmp = tmp_path_factory.mktemp("table_ext")
    specs = _specs()
    files = []
    for name, spec in specs.items():
        files.append(str(tmp / f"{name}.onnx"))
        G.write_actor(files[-1], spec)
    singles = [MLPPolicy(f, device=DEV, fused=True) for f in files]
    assert [s._fused["extras"] is not None for s in singles] == [False, True, True, True]
    xs = [torch.tensor(G.inputs(N, IN, seed=70 + t), device=DEV) for t in range(5)]
    alone = [[s.get_action(x).clone() for s in singles] for x in xs]      # alone[t][k]: policy k on batch t
    ref = np.clip(G.ref_actor(xs[0].cpu().numpy(), specs["ln_before"]), -1.0, 1.0)
    np.testing.assert_allclose(alone[0][2].cpu().numpy(), ref, rtol=0, atol=ATOL)
    return {"files": files, "xs": xs, "alone": alone, "specs": list(specs.values())}


def _expected(alone_t, policy_of):
    import torch
    idx = torch.as_tensor(np.asarray(policy_of), dtype=torch.int64, device=DEV)
    return torch.stack(alone_t, dim=0)[idx, torch.arange(N, device=DEV)]


def _assignments():
    """interleave, and an explicit array that gives policy 3 33 rows: the first 32 of range 0 (a full tile) and one of range 1 (a tile of a
    single row); the other rows go round the other three policies."""
    explicit = np.arange(N) % 3
    explicit[:32] = 3
    explicit[37] = 3
    assert (explicit == 3).sum() == 33 and (explicit[37:] == 3).sum() == 1
    return {"interleave": "interleave", "explicit_33": explicit.astype(np.int32)}


@pytest.mark.parametrize("how", ["interleave", "explicit_33"])
def test_table_rows_equal_each_files_single_policy(world, how):
    import torch
    assign = _assignments()[how]
    tab = PolicyTable(world["files"], num_envs=N, device=DEV, assign=assign, ranges=RANGES)
    assert tab._handle is not None and tab._create_suffix == "_create_ex"
    if how == "explicit_33":
        counts = np.bincount(tab.policy_of_env, minlength=4)
        assert counts[3] == 33 and all(counts > 0)
        assert np.bincount(tab.policy_of_env[37:], minlength=4)[3] == 1    # one tile holds a single row
    x, alone = world["xs"][0], world["alone"][0]
    want = _expected(alone, tab.policy_of_env)
    got = tab.get_action(x)
    assert torch.equal(got, want)
    for k in range(4):                                                     # the plain file's rows too
        rows = torch.as_tensor(np.nonzero(tab.policy_of_env == k)[0], device=DEV)
        assert len(rows) and torch.equal(got[rows], alone[k][rows])
    side = torch.cuda.Stream(device=DEV)
    for i, (first, count) in enumerate(RANGES):
        out = torch.full((N, OUT), 7.0, dtype=torch.float32, device=DEV)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            tab.get_action_range(i, x, out)
        torch.cuda.current_stream().wait_stream(side)
        assert torch.equal(out[first:first + count], want[first:first + count])
        inside = torch.zeros(N, dtype=torch.bool, device=DEV)
        inside[first:first + count] = True
        assert bool((out[~inside] == 7.0).all())
    tab.close()


def test_rotating_table_follows_policy_of_bit_for_bit(world):
    import torch
    tab = PolicyTable(world["files"], num_envs=N, device=DEV, ranges=RANGES, rotate_every=1)
    rng = np.random.default_rng(5)
    episodes = np.zeros(N, np.int64)
    term, trunc = torch.zeros(N, dtype=torch.uint8, device=DEV), torch.zeros(N, dtype=torch.uint8, device=DEV)
    out = torch.zeros((N, OUT), dtype=torch.float32, device=DEV)
    seen = set()
    for t in range(5):
        done_t, done_r = rng.random(N) < 0.3, rng.random(N) < 0.1
        if t == 0:
            done_t[:], done_r[:] = False, False
        if t == 2:
            done_t[:37] = True                                             # a whole range moves on at once
        term.copy_(torch.as_tensor(done_t.astype(np.uint8)))
        trunc.copy_(torch.as_tensor(done_r.astype(np.uint8)))
        episodes += (done_t | done_r)
        for i in range(len(RANGES)):
            tab.get_action_range(i, world["xs"][t], out, done=(term, trunc))
        now = tab.policy_of(np.arange(N), episodes)
        assert np.array_equal(tab.policy_now.cpu().numpy(), now) and np.array_equal(tab.episode.cpu().numpy(), episodes)
        assert torch.equal(out, _expected(world["alone"][t], now)), t
        seen |= set(now.tolist())
    assert seen == {0, 1, 2, 3} and episodes.max() >= 2
    tab.close()


def test_cpu_device_twin_agrees_with_the_fused_table(world):
    import torch
    fused = PolicyTable(world["files"], num_envs=N, device=DEV, ranges=RANGES)
    twin = PolicyTable(world["files"], num_envs=N, device="cpu", ranges=RANGES)
    assert twin._handle is None
    x = world["xs"][1]
    a, b = fused.get_action(x).cpu().numpy(), twin.get_action(x.cpu()).numpy()
    assert np.mean(np.abs(a) < 1.0) >= 0.5
    np.testing.assert_allclose(a, b, rtol=0, atol=ATOL)
    for k, spec in enumerate(world["specs"]):
        rows = np.nonzero(fused.policy_of_env == k)[0]
        np.testing.assert_allclose(a[rows], np.clip(G.ref_actor(x.cpu().numpy()[rows], spec), -1.0, 1.0), rtol=0, atol=ATOL)
    fused.close()


def test_a_file_outside_the_grammar_is_refused_by_name(world, tmp_path):
    p = str(tmp_path / "decomposed.onnx")
    G.decomposed_layernorm_actor(p)
    with pytest.raises(ValueError, match=r"decomposed\.onnx: .*'ReduceMean'"):
        PolicyTable(world["files"][:2] + [p], num_envs=8, device=DEV)
