"""The shared pieces under the Python layer: the record core of cosim_amd/records.py against a brute-force loop and
against the containers built on it, the ABI table of cosim_amd/engine.py against the prototypes of include/cosim.h, the CSR helper
under the ``Engine.scenario_*_set`` wrappers against a stub library, and the two helpers of cosim_amd/cli.py.  No GPU, no shared
library."""
import ctypes
import os
import re

import numpy as np
import pytest

from cosim_amd import cli, records
from cosim_amd.checks import Verdicts
from cosim_amd.engine import ABI, EXPORTS, Engine, _ABI_ROWS
from cosim_amd.ledger import EpisodeLedger
from cosim_amd.scenario import ScenarioTable

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
COUNTS = [0, 1, 5]   # with 2 slots: an empty ring, a partly filled one, one that wrapped twice with an odd count


def _rings(slots, W, counts=COUNTS, seed=0):
    """Rings ``[N, slots, W]`` as a device that closed ``counts[i]`` records of env i leaves them (word 0 the ordinal, every other
    word different everywhere), and the open rows ``[N, W]`` carrying each env's next ordinal."""
    rng = np.random.default_rng(seed)
    N = len(counts)
    rec = np.zeros((N, slots, W), dtype=np.int32)
    for i, c in enumerate(counts):
        for o in range(c):
            rec[i, o % slots] = rng.integers(1000, 1 << 30, W)
            rec[i, o % slots, 0] = o
    opn = rng.integers(1000, 1 << 30, (N, W)).astype(np.int32)
    opn[:, 0] = counts
    return rec, np.asarray(counts, dtype=np.int32), opn


def _brute(rec, counts, opn):
    words, env, lost = [], [], []
    for i in range(rec.shape[0]):
        c, slots = int(counts[i]), rec.shape[1]
        kept = min(c, slots)
        lost.append(c - kept)
        for o in range(c - kept, c):        # oldest kept first
            words.append(rec[i, o % slots])
            env.append(i)
        if opn is not None:
            words.append(opn[i])
            env.append(i)
    return np.array(words, dtype=np.int32).reshape(-1, rec.shape[2]), np.array(env, dtype=np.int64), np.array(lost, dtype=np.int64)


@pytest.mark.parametrize("with_open", [False, True])
@pytest.mark.parametrize("slots", [2, 1])
def test_unroll_rings_against_a_loop(slots, with_open):
    rec, cnt, opn = _rings(slots, 4)
    opn = opn if with_open else None
    words, env, lost = records.unroll_rings(rec, cnt, opn)
    bw, be, bl = _brute(rec, cnt, opn)
    assert words.dtype == np.int32 and env.dtype == np.int64 and lost.dtype == np.int64
    assert np.array_equal(words, bw) and np.array_equal(env, be) and np.array_equal(lost, bl)
    assert lost.tolist() == [0, 0, 5 - slots]
    assert len(words) == sum(min(c, slots) for c in COUNTS) + (3 if with_open else 0)
    assert words[env == 2, 0].tolist() == list(range(5 - slots, 5)) + ([5] if with_open else [])   # sorted by ordinal, the open row last


@pytest.mark.parametrize("with_open", [False, True])
@pytest.mark.parametrize("slots", [2, 1])
def test_containers_unroll_as_the_core_does(slots, with_open):
    """``EpisodeLedger.from_raw`` and ``Verdicts.from_raw`` on rings of the same N, slots and counts, each at its own record width
    (16 words; 8 + 2 I = 12 words for a table with one check): words, env and lost are the core's, which are the loop's."""
    table = ScenarioTable([{"checks": [[0, 10, "torque_max", 0, "always", "<", 1.0]]}], command_dim=0)
    for W, make in ((16, lambda r, c, o: EpisodeLedger.from_raw(r, c, o, env_id0=7)),
                    (12, lambda r, c, o: Verdicts.from_raw(r, c, o, table, env_id0=7))):
        rec, cnt, opn = _rings(slots, W, seed=W)
        rec[:, :, 3], opn[:, 3] = 1, 1                  # (a verdict's scenario word: row 0)
        opn = opn if with_open else None
        got = make(rec, cnt, opn)
        words, env, lost = records.unroll_rings(rec, cnt, opn)
        bw, be, bl = _brute(rec, cnt, opn)
        assert np.array_equal(words, bw) and np.array_equal(env, be) and np.array_equal(lost, bl)
        assert np.array_equal(got.words, bw) and np.array_equal(got.env, be + 7) and np.array_equal(got.lost, bl)
        assert got.slots == slots and got.env_id0 == 7


def _prototypes():
    """name -> parameter count of every ``cosim_name(args);`` in include/cosim.h, comments stripped."""
    hdr = open(os.path.join(ROOT, "include", "cosim.h")).read()
    hdr = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    hdr = re.sub(r"//[^\n]*", " ", hdr)
    out = {}
    for name, args in re.findall(r"\b(cosim_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", hdr):
        assert name not in out, f"{name} is declared twice"
        out[name] = 0 if args.strip() in ("", "void") else args.count(",") + 1
    return out


def test_abi_table_matches_the_header():
    protos = _prototypes()
    assert len(protos) == 63
    assert len(_ABI_ROWS) == len(ABI), "a name appears twice in the ABI table"
    assert set(ABI) == set(protos), set(ABI) ^ set(protos)
    for name, n in protos.items():
        assert len(ABI[name][1]) == n, f"{name}: {len(ABI[name][1])} argtypes, the prototype has {n} parameters"
    assert (protos["cosim_fleet_stats"], protos["cosim_fleet_hist"], protos["cosim_last_error"]) == (9, 11, 0)
    assert set(EXPORTS) == set(ABI) and len(EXPORTS) == len(ABI)
    assert ABI["cosim_last_error"][0] is ctypes.c_char_p
    assert all(r is ctypes.c_int for name, (r, _) in ABI.items() if name != "cosim_last_error")


class _StubLibrary:
    """Stands in for the loaded library: every entry point records its arguments and succeeds (``cosim_query`` answers 0)."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args))
            return 0
        return fn


def _stub_engine():
    e = Engine.__new__(Engine)
    e.L, e.h = _StubLibrary(), 1234
    return e


def test_csr_setters_clear_with_todays_calls():
    e = _stub_engine()
    e.scenario_set(None, 0, None, None, 99)
    e.scenario_params_set(None)
    e.scenario_checks_set(None)
    e.scenario_curves_set(None)
    assert e.L.calls == [("cosim_scenario_set", (1234, 0) + (None,) * 6 + (0, None, None, 99)),
                         ("cosim_scenario_params_set", (1234, 0) + (None,) * 6),
                         ("cosim_scenario_checks_set", (1234, 0) + (None,) * 7 + (0,)),
                         ("cosim_scenario_curves_set", (1234, 0) + (None,) * 7)]
    for name, args in e.L.calls:
        assert len(args) == len(ABI[name][1]), name


def test_csr_setters_pass_the_columns_and_refuse_short_ones():
    e = _stub_engine()
    i32, f32 = np.int32, np.float32
    adr = np.array([0, 2], dtype=i32)
    col = lambda dt: np.zeros(2, dtype=dt)   # noqa: E731
    cases = (("scenario_params_set", e.scenario_params_set, 2, (i32, i32, i32, f32), ()),
             ("scenario_checks_set", e.scenario_checks_set, 2, (i32, i32, i32, i32, f32), (5,)),
             ("scenario_curves_set", e.scenario_curves_set, 3, (i32, i32, f32, f32, i32), ()))
    for who, setter, t_width, dtypes, tail in cases:
        good = [adr, np.zeros((2, t_width), dtype=np.int64)] + [col(np.float64) for _ in dtypes]   # (converted on the way)
        del e.L.calls[:]
        setter(good, *tail)
        (name, args), = e.L.calls
        assert name == "cosim_" + who and args[:2] == (1234, 1) and len(args) == len(ABI[name][1]) and args[len(args) - len(tail):] == tail
        assert all(isinstance(a, int) and a != 0 for a in args[2:2 + 2 + len(dtypes)])
        for k in range(1, len(good)):                  # t, then every column, one element short
            bad = list(good)
            bad[k] = bad[k].reshape(-1)[:-1]
            with pytest.raises(ValueError) as err:
                setter(bad, *tail)
            assert str(err.value) == f"{who}: the item arrays are shorter than their row addresses (2 items)"
        with pytest.raises(ValueError) as err:
            setter([np.zeros((2, 2), dtype=i32)] + good[1:], *tail)
        assert str(err.value) == f"{who}: adr must be [S + 1]"
        assert len(e.L.calls) == 1                     # no refused table reached the library
    # the keyframe / push table: its own two refusals, command_dim from the (stub's) query: 0
    ka, pa = np.array([0, 1], dtype=i32), np.array([0, 0], dtype=i32)
    empty = np.zeros(0, dtype=f32)
    del e.L.calls[:]
    e.scenario_set((ka, np.zeros(1, dtype=i32), empty, pa, empty, empty), 1, 11, 22, 33)
    assert e.L.calls[-1][0] == "cosim_scenario_set" and e.L.calls[-1][1][:2] == (1234, 1) and e.L.calls[-1][1][8:] == (1, 11, 22, 33)
    with pytest.raises(ValueError) as err:
        e.scenario_set((ka, np.zeros(0, dtype=i32), empty, pa, empty, empty), 1, 11, 22, 33)
    assert str(err.value) == "scenario_set: the table arrays are shorter than their row addresses (1 keyframes, 0 push windows)"
    with pytest.raises(ValueError) as err:
        e.scenario_set((ka, np.zeros(1, dtype=i32), empty, pa[:1], empty, empty), 1, 11, 22, 33)
    assert str(err.value) == "scenario_set: key_adr and push_adr must both be [S + 1]"


def test_opt_precedence():
    opt = cli.session_opt({"ledger": 3, "engine": {"ledger": 4, "check_slots": 5}})
    assert opt(2, "ledger", 0) == 2                    # the flag
    assert opt(None, "ledger", 0) == 3                 # the session's top level
    assert opt(None, "check_slots", 0) == 5            # session["engine"]
    assert opt(None, "curves", False) is False         # the default
    assert opt(0, "ledger", 9) == 0                    # a flag of 0 is a flag
    for falsy in (0, False):                           # a top-level 0 / False wins over the engine's value: `is not None`
        assert cli.session_opt({"curves": falsy, "engine": {"curves": True}})(None, "curves", None) is falsy
    assert cli.session_opt({"curves": None, "engine": {"curves": True}})(None, "curves", None) is True
    assert cli.session_opt({"engine": None})(None, "ledger", 7) == 7
    assert cli.session_opt({})(None, "ledger", 7) == 7


def test_rank_path():
    assert cli.rank_path("out/episodes.npz", 0, 1) == "out/episodes.npz"
    assert cli.rank_path("out/episodes.npz", 2, 4) == "out/episodes.rank2.npz"
    assert cli.rank_path("out.d/episodes", 2, 4) == "out.d/episodes.rank2"
    assert cli.rank_path("episodes.v2.npz", 0, 4) == "episodes.v2.rank0.npz"
