"""Ranges, groups and the stream rule on the host (no GPU): csrc/cosim_ranges.h compiled as plain C++ (tests/range_groups.cpp), once
plainly and once with the address and undefined-behaviour sanitizers, and the program itself is run.  The rules as DESIGN 4.6 states
them are written out again here: group g of P over R ranges holds ranges [g R / P, (g + 1) R / P); streams = min(R, max(1, Q / 2))."""
import os
import subprocess

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
BUILDS = {"plain": ["-O0"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}


@pytest.fixture(scope="module", params=sorted(BUILDS))
def exe(request, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("range_groups_" + request.param) / "range_groups")
    cxx = os.environ.get("CXX", "c++")
    p = subprocess.run([cxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", *BUILDS[request.param], "-I", os.path.join(ROOT, "cosim_amd", "csrc"),
                        "-o", path, os.path.join(ROOT, "tests", "range_groups.cpp")], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    return path


def run(exe, *args):
    p = subprocess.run([exe, *map(str, args)], capture_output=True, text=True)
    assert p.returncode == 0, (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    return p.stdout


def test_partitions(exe):
    """R in 1..16, P in 1..R, twelve fleet sizes, unit 1 and 2: ranges and groups partition in order, none empty, sizes within one,
    group unions even under unit 2 (checked inside the program, which prints the number of (fleet, R, unit) cases it went through)."""
    out = run(exe).split()
    assert out[0] == "ok" and int(out[1]) > 300, out


def test_rule_table(exe):
    rows = [tuple(map(int, line.split())) for line in run(exe, "table").splitlines()]
    assert len(rows) == 16 * 9
    for R, Q, P in rows:
        assert P == min(R, max(1, Q // 2)), (R, Q, P)
    got = {(R, Q): P for R, Q, P in rows}
    # the arrangements measured so far (four ranges): 4 queues carry two chains, 8 carry four
    assert [got[4, Q] for Q in (1, 2, 4, 8, 32)] == [1, 1, 2, 4, 4]
    assert [got[1, Q] for Q in (1, 2, 4, 8, 32)] == [1, 1, 1, 1, 1]
    assert [got[16, Q] for Q in (1, 2, 4, 8, 32)] == [1, 1, 2, 4, 16]


@pytest.mark.parametrize("value, queues", [(None, 4), ("", 4), ("1", 1), ("2", 2), ("4", 4), ("8", 8), ("32", 32), (" 8", 8), ("8 ", 8),
                                           ("0", 4), ("-2", 4), ("eight", 4), ("8q", 4), ("4.5", 4), ("0x10", 4),
                                           ("99999999999999999999", 4)])
def test_hw_queues_from_env(exe, value, queues):
    """GPU_MAX_HW_QUEUES as a whole positive number, anything else (unset, empty, garbage, overflow) as the HIP default of 4."""
    assert int(run(exe, "env", *([] if value is None else [value]))) == queues


@pytest.mark.parametrize("asked, R, Q, P", [(0, 4, 4, 2), (0, 4, 8, 4), (0, 4, 1, 1), (1, 4, 8, 1), (2, 4, 8, 2), (3, 4, 4, 3), (4, 4, 4, 4),
                                            (9, 4, 4, 4), (0, 1, 32, 1), (3, 1, 4, 1), (-1, 4, 4, 2)])
def test_streams_in_use(exe, asked, R, Q, P):
    """"range_streams": a value >= 1 is clamped to R, 0 (and anything below) is the rule's answer."""
    assert int(run(exe, "use", asked, R, Q)) == P
