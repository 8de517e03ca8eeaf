"""Rotating policy tables without a GPU.  The rule and the tile-capacity bound of csrc/cosim_poltab.h through tests/polrot_host.cpp,
built plain and with AddressSanitizer / UBSan as a stand-alone child process; then the CPU torch twin of ``PolicyTable(rotate_every=)``
and ``RecurrentPolicyTable(rotate_every=)`` under a scripted sequence of done flags (counters, ``policy_now``, actions against
``MLPPolicy`` of each row's current file, ranges, ``reset`` / ``rewind`` / ``state`` / ``load_state``, the refusals word for word); and
``by_policy`` of the ledger and the verdicts on hand-built records whose episode ordinals differ per env."""
import os
import subprocess

import numpy as np
import pytest

from test_policy_table_host import _write_chain

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


@pytest.fixture(scope="module", params=["plain", "asan-ubsan"])
def exe(request, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("polrot") / ("polrot_host_" + request.param.replace("-", "_")))
    extra = [] if request.param == "plain" else ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
    subprocess.check_call([os.environ.get("CXX", "c++"), "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unknown-pragmas", *extra, "-I",
                           os.path.join(ROOT, "cosim_amd", "csrc"), "-o", out, os.path.join(ROOT, "tests", "polrot_host.cpp")])
    return out


def test_rule_and_capacity_bound(exe):
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0, (p.stdout[-3000:], p.stderr[-3000:])
    last = p.stdout.strip().splitlines()[-1].split()
    assert last[0] == "OK" and int(last[1]) > 5000 and int(last[2]) > 700 and int(last[3]) >= 62     # the single-row cases meet the bound


# ------------------------------------------------------------------------------------------------------------ the torch twin on the CPU
@pytest.fixture()
def files(tmp_path):
    return [_write_chain(str(tmp_path / "a.onnx"), (12, 40, 36, 4), ["LeakyRelu", "Elu", None], 1),
            _write_chain(str(tmp_path / "b.onnx"), (12, 33, 4), ["Sigmoid", None], 2, nobias=(0,)),
            _write_chain(str(tmp_path / "c.onnx"), (12, 4), [None], 3)]


N, RANGES, CALLS = 41, [(0, 17), (17, 1), (18, 23)], 8


def _script(seed):
    """CALLS rounds of (terminated, truncated) bytes: about a third of the envs end an episode per round, some by both flags."""
    rng = np.random.default_rng(seed)
    return [((rng.random(N) < 0.25).astype(np.uint8), (rng.random(N) < 0.15).astype(np.uint8)) for _ in range(CALLS)]


def _rule(base, e, every, K):
    return (base + e // every) % K


@pytest.mark.parametrize("every", [1, 2])
def test_twin_follows_the_rule_call_by_call(files, every):
    import torch
    from cosim_amd.policy import MLPPolicy, PolicyTable
    base = np.random.default_rng(4).integers(0, 3, N)
    tab = PolicyTable(files, num_envs=N, device="cpu", assign=base, ranges=RANGES, rotate_every=every)
    assert tab.rotate_every == every and tab.episode.dtype == torch.int32 and tab.policy_now.dtype == torch.int32
    assert (tab.policy_of_env == base).all() and not tab.episode.any() and (tab.policy_now.numpy() == base).all()
    singles = [MLPPolicy(f, device="cpu") for f in files]
    xs = torch.tensor(np.random.default_rng(5).standard_normal((CALLS, N, 12)).astype(np.float32) * 2.0)
    e = np.zeros(N, np.int64)
    ep_ptr, now_ptr = tab.episode.data_ptr(), tab.policy_now.data_ptr()
    for call, (term, trunc) in enumerate(_script(7)):
        got = tab.get_action(xs[call]).clone()
        now = _rule(base, e, every, 3)
        assert (tab.episode.numpy() == e).all() and (tab.policy_now.numpy() == now).all(), call       # get_action moves no counter
        for k, pol in enumerate(singles):
            idx = torch.as_tensor(np.nonzero(now == k)[0])
            if len(idx):
                assert torch.equal(got[idx], pol.get_action(xs[call][idx])), (call, k)
        tab.reset(torch.tensor(term | trunc))                                                          # what Runner.test does after the step
        e += (term | trunc)
        assert (tab.episode.numpy() == e).all(), call                                                  # the cumulative sums
    assert e.max() >= 3 and len(set(e.tolist())) > 2                                                   # the envs are out of step with each other
    assert (tab.episode.data_ptr(), tab.policy_now.data_ptr()) == (ep_ptr, now_ptr)                   # persistent tensors
    assert (tab.policy_of(np.arange(N), e) == _rule(base, e, every, 3)).all()
    assert (tab.policy_of(np.arange(N), 5) == _rule(base, 5, every, 3)).all()                          # a scalar ordinal broadcasts
    tab.reset()                                                                                        # no mask: the counters stay
    assert (tab.episode.numpy() == e).all()
    tab.rewind()
    assert not tab.episode.any() and (tab.policy_now.numpy() == base).all()


@pytest.mark.parametrize("every", [1, 2])
def test_twin_range_calls_touch_their_rows_only(files, every):
    import torch
    from cosim_amd.policy import MLPPolicy, PolicyTable
    tab = PolicyTable(files, num_envs=N, device="cpu", assign="interleave", env_id0=100, ranges=RANGES, rotate_every=every)
    base = (np.arange(100, 100 + N) % 3)
    singles = [MLPPolicy(f, device="cpu") for f in files]
    xs = torch.tensor(np.random.default_rng(6).standard_normal((CALLS, N, 12)).astype(np.float32))
    e = np.zeros(N, np.int64)
    for call, (term, trunc) in enumerate(_script(8)):
        done = (torch.tensor(term), torch.tensor(trunc))
        for i in (2, 0, 1):                                                                            # any order: a range knows its own rows only
            first, count = RANGES[i]
            inside = np.zeros(N, bool)
            inside[first:first + count] = True
            before_e, before_now = tab.episode.clone(), tab.policy_now.clone()
            out = torch.full((N, 4), 7.0)
            tab.get_action_range(i, xs[call], out, done=done)
            e[inside] += (term | trunc)[inside]
            now = _rule(base, e, every, 3)
            assert (tab.episode.numpy()[inside] == e[inside]).all() and (tab.policy_now.numpy()[inside] == now[inside]).all(), (call, i)
            assert torch.equal(tab.episode[~torch.tensor(inside)], before_e[~torch.tensor(inside)]), (call, i)
            assert torch.equal(tab.policy_now[~torch.tensor(inside)], before_now[~torch.tensor(inside)]), (call, i)
            assert bool((out[~torch.tensor(inside)] == 7.0).all()), (call, i)
            for k, pol in enumerate(singles):
                idx = torch.as_tensor(np.nonzero(inside & (now == k))[0])
                if len(idx):
                    # the CPU library GEMM picks its kernel by batch size: equal to rounding here, bit-equal on the device
                    assert torch.allclose(out[idx], pol.get_action(xs[call][idx]), rtol=0, atol=1e-6), (call, i, k)
        assert (tab.episode.numpy() == e).all(), call


def test_twin_state_round_trip_and_fork(files):
    import torch
    from cosim_amd.policy import PolicyTable
    tab = PolicyTable(files, num_envs=N, device="cpu", rotate_every=1)
    assert PolicyTable(files, num_envs=N, device="cpu").state() is None                                # a static table stays stateless
    for term, trunc in _script(9)[:3]:
        tab.reset(torch.tensor(term | trunc))
    st = tab.state()
    assert set(st) == {"episode"} and st["episode"].data_ptr() != tab.episode.data_ptr()               # a copy
    kept = st["episode"].clone()
    tab.reset(torch.ones(N, dtype=torch.uint8))
    assert torch.equal(tab.episode, kept + 1) and torch.equal(st["episode"], kept)
    mask = torch.tensor((np.arange(N) % 2).astype(np.uint8))
    tab.load_state(st, mask=mask)                                                                       # the odd envs go back, the even ones keep theirs
    assert torch.equal(tab.episode, torch.where(mask != 0, kept, kept + 1))
    tab.load_state(st)
    assert torch.equal(tab.episode, kept)
    tab.load_state(st, src=torch.full((N,), 5, dtype=torch.int32))                                      # a fork: every env takes env 5's counter
    assert bool((tab.episode == kept[5]).all())
    with pytest.raises(ValueError, match=r"episode has shape \(40,\), expected \(41,\)"):
        tab.load_state({"episode": kept[:-1]})
    with pytest.raises(ValueError, match="carries no episode counters"):
        tab.load_state(None)


def test_counter_is_held_at_the_top(files):
    import torch
    from cosim_amd.policy import PolicyTable
    tab = PolicyTable(files, num_envs=4, device="cpu", rotate_every=1)
    top = 2 ** 31 - 1
    tab.episode.copy_(torch.tensor([top, top - 1, 5, top], dtype=torch.int32))
    tab.reset(torch.tensor([1, 1, 1, 0], dtype=torch.uint8))
    assert tab.episode.tolist() == [top, top, 6, top]
    tab.reset(torch.tensor([True, True, False, True]))
    assert tab.episode.tolist() == [top, top, 6, top]
    tab.get_action(torch.zeros((4, 12)))
    assert tab.policy_now.tolist() == [(int(b) + e) % 3 for b, e in zip(tab.policy_of_env, [top, top, 6, top])]


def test_refusals_name_the_value(files):
    import torch
    from cosim_amd.policy import PolicyTable, build_policy, open_policy_table
    for bad in (0, -2, 1.5, "2", True):
        with pytest.raises(ValueError, match=r"PolicyTable: rotate_every %s: an integer >= 1" % repr(bad).replace(".", r"\.")):
            PolicyTable(files, num_envs=8, device="cpu", rotate_every=bad)
    with pytest.raises(ValueError, match="rotate_every 0: an integer >= 1"):
        open_policy_table(files, num_envs=8, device="cpu", rotate_every=0)
    with pytest.raises(ValueError, match="rotate_every 0: an integer >= 1"):
        build_policy({"policy": {"use_lstm": False, "onnx_files": files, "rotate": 0}}, num_envs=8, device="cpu")
    tab = build_policy({"policy": {"use_lstm": False, "onnx_files": files, "rotate": 2}}, num_envs=8, device="cpu")
    assert tab.rotate_every == 2
    assert build_policy({"policy": {"use_lstm": False, "onnx_files": files}}, num_envs=8, device="cpu").rotate_every is None
    with pytest.raises(ValueError, match=r"PolicyTable\.policy_of: the table rotates every 2 episode\(s\).*pass episodes="):
        tab.policy_of([0, 1])
    x, out = torch.zeros((8, 12)), torch.zeros((8, 4))
    with pytest.raises(ValueError, match=r"PolicyTable\.get_action_range: the table rotates, pass done=\(terminated, truncated\)"):
        tab.get_action_range(0, x, out)
    with pytest.raises(ValueError, match=r"done is \(terminated, truncated\), contiguous uint8 \[8\] tensors"):
        tab.get_action_range(0, x, out, done=(torch.zeros(7, dtype=torch.uint8), torch.zeros(8, dtype=torch.uint8)))
    static = PolicyTable(files, num_envs=8, device="cpu")
    static.get_action_range(0, x, out)                                                                  # a static table needs no done
    static.rewind()
    assert not hasattr(static, "reset") and hasattr(tab, "reset")                                      # a runner calls reset only where there is one
    assert not hasattr(static, "episode") and (static.policy_of([3, 4, 5]) == [0, 1, 2]).all()


class _Env:
    auto_reset, command_dim, num_envs = False, 0, 8


def test_runner_refuses_rotation_without_auto_reset(files):
    from cosim_amd.policy import PolicyTable
    from cosim_amd.runner import Runner
    with pytest.raises(ValueError, match=r"PolicyTable\(rotate_every=1\).*needs an env built with auto_reset=True"):
        Runner(_Env(), PolicyTable(files, num_envs=8, device="cpu", rotate_every=1))
    Runner(_Env(), PolicyTable(files, num_envs=8, device="cpu"))


def test_cli_refuses_a_bad_rotation(capsys):
    from cosim_amd import cli
    for argv, want in ((["--policy", "a.onnx", "b.onnx", "--policy-rotate", "0"], "0 is not an integer >= 1"),
                       (["--policy", "a.onnx", "--policy-rotate", "1"], "--policy-rotate needs several --policy files")):
        with pytest.raises(SystemExit) as e:
            cli.main(argv)
        assert e.value.code == 2 and want in capsys.readouterr().err, argv


def test_recurrent_twin_rotates_and_zeroes_state(tmp_path):
    import torch
    from cosim_amd.policy import LSTMPolicy, RecurrentPolicyTable, write_random_lstm
    Hs = (8, 20)
    paths = [write_random_lstm(str(tmp_path / f"r{k}.onnx"), 12, 4, hidden=H, head=(16,), seed=40 + k) or str(tmp_path / f"r{k}.onnx") for k, H in enumerate(Hs)]
    n = 9
    tab = RecurrentPolicyTable(paths, num_envs=n, device="cpu", rotate_every=1)
    base = np.arange(n) % 2
    rng = np.random.default_rng(3)
    e = np.zeros(n, np.int64)
    # one single-env LSTMPolicy per env and per file is the reference: a fresh one at each episode start
    def fresh(i, k):
        return LSTMPolicy({"policy": {"h_in_dim": Hs[k], "c_in_dim": Hs[k]}}, paths[k], num_envs=1, device="cpu")
    ref = [fresh(i, base[i]) for i in range(n)]
    for call in range(6):
        x = torch.tensor(rng.standard_normal((n, 12)).astype(np.float32))
        got = tab.get_action(x).clone()
        now = _rule(base, e, 1, 2)
        assert (tab.policy_now.numpy() == now).all()
        for i in range(n):
            assert torch.allclose(got[i], ref[i].get_action(x[i:i + 1])[0], rtol=0, atol=1e-6), (call, i)
        done = rng.random(n) < 0.4
        tab.reset(torch.tensor(done.astype(np.uint8)))
        e += done
        for i in np.nonzero(done)[0]:
            ref[i] = fresh(i, _rule(base[i], e[i], 1, 2))
        assert (tab.episode.numpy() == e).all()
    st = tab.state()
    assert set(st) == {"h", "c", "episode"}
    tab.rewind()
    tab.load_state(st)
    assert (tab.episode.numpy() == e).all()


# ---------------------------------------------------------------------------------------------------------------------- by_policy
class _RotTab:
    """What by_policy needs of a rotating table: names, rotate_every and the rule (interleaved over three, every 2 episodes)."""
    names = ["a", "b", "c"]
    rotate_every = 2

    @staticmethod
    def policy_of(g, episodes=None):
        assert episodes is not None
        return ((np.asarray(g) % 3 + np.asarray(episodes) // 2) % 3).astype(np.int32)


#        env  episode length flags(1 terminated, 2 truncated, 16 open) scenario
RECS = [(100, 0, 10, 1, 0), (100, 1, 50, 2, 1), (100, 2, 30, 1, 0), (100, 3, 3, 16, 1),
        (101, 4, 20, 1, 1), (101, 5, 30, 1, 0),                                                        # its ring lost episodes 0..3
        (102, 0, 50, 2, 0),
        (103, 7, 50, 2, 1), (103, 8, 40, 1, 0), (103, 9, 50, 2, 1)]


def test_ledger_by_policy_attributes_by_env_and_ordinal():
    from cosim_amd.ledger import OPEN, WORDS, EpisodeLedger
    w = np.zeros((len(RECS), WORDS), np.int32)
    for r, (_, ep, ln, fl, sc) in enumerate(RECS):
        w[r, 0], w[r, 1], w[r, 2], w[r, 13] = ep, ln, fl, sc + 1
        w[r, 5:13] = np.full(8, float(ln), np.float32).view(np.int32)
    led = EpisodeLedger(w, [r[0] for r in RECS], np.zeros(4, np.int64), slots=4, env_id0=100)
    want, cells = {}, {}
    for g, ep, ln, fl, sc in RECS:
        if fl & OPEN:
            continue
        name = _RotTab.names[(g % 3 + ep // 2) % 3]
        want.setdefault(name, []).append(ln)
        cells.setdefault((name, sc), []).append(ln)
    by = led.by_policy(_RotTab)
    assert {k: v["episodes"] for k, v in by.items()} == {k: len(v) for k, v in want.items()}
    assert {k: v["length"]["mean"] for k, v in by.items()} == {k: float(np.mean(v)) for k, v in want.items()}
    assert sum(v["episodes"] for v in by.values()) == led.counts()["episodes"] == 9
    # env 100 alone shows the rotation: episodes 0, 1 with policy 1 ("b"), episode 2 with policy 2 ("c")
    assert by["b"]["episodes"] >= 2 and set(by) == {"a", "b", "c"}
    mat = led.by_policy(_RotTab, scenario=True)
    assert set(mat) == set(cells) and {k: v["episodes"] for k, v in mat.items()} == {k: len(v) for k, v in cells.items()}
    from cosim_amd.ledger import policy_of_records
    with pytest.raises(ValueError, match="the table rotates.*pass the records' ordinals"):
        policy_of_records(_RotTab, led.env, 100)


def test_verdicts_by_policy_attributes_by_env_and_ordinal():
    from cosim_amd.checks import HDR, Verdicts
    I = 1
    item_mode, item_t = np.zeros((2, I), np.int32), np.zeros((2, I, 2), np.int32)
    item_t[:, :, 1] = 10
    w = np.zeros((len(RECS), HDR + 2 * I), np.int32)
    for r, (_, ep, ln, fl, sc) in enumerate(RECS):
        w[r, 0], w[r, 1], w[r, 2], w[r, 3] = ep, ln, fl, sc + 1
    v = Verdicts(w, [r[0] for r in RECS], np.zeros(4, np.int64), [["upright"], ["upright"]], item_mode, item_t, slots=4, env_id0=100)
    want, cells = {}, {}
    for g, ep, ln, fl, sc in RECS:
        if fl & 16:
            continue
        name = _RotTab.names[(g % 3 + ep // 2) % 3]
        want[name] = want.get(name, 0) + 1
        cells[(name, sc)] = cells.get((name, sc), 0) + 1
    assert {k: c["episodes"] for k, c in v.by_policy(_RotTab).items()} == want
    assert {k: c["episodes"] for k, c in v.by_policy(_RotTab, scenario=True).items()} == cells
    assert sum(want.values()) == v.counts()["episodes"]
