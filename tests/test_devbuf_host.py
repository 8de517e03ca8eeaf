"""The owning buffer of the engine's host code (csrc/cosim_devbuf.h) without a GPU: tests/devbuf_host.cpp instantiates DevBuf over
a counting allocator on std::malloc that fails the k-th request on command, built plain and with AddressSanitizer / UBSan as a
stand-alone child process.  Under the sanitizer build a double free or a leak fails the child's exit status.  (The shape
cosim_engine.hip has with it -- one place that allocates, one that frees -- is held in tests/test_tables_host.py.)"""
import os
import subprocess

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CSRC = os.path.join(ROOT, "cosim_amd", "csrc")
CASES = ["empty", "alloc_destruct", "zeroed", "moves", "self_move", "reset_twice", "failed_alloc", "build_then_commit", "drop_first"]


@pytest.fixture(scope="module", params=["plain", "asan-ubsan"])
def exe(request, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("devbuf") / ("devbuf_host_" + request.param.replace("-", "_")))
    extra = [] if request.param == "plain" else ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
    subprocess.check_call([os.environ.get("CXX", "c++"), "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", *extra, "-I", CSRC, "-o", out,
                           os.path.join(ROOT, "tests", "devbuf_host.cpp")])
    return out


@pytest.mark.parametrize("case", CASES)
def test_devbuf(exe, case):
    p = subprocess.run([exe, case], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.strip() == "ok " + case, (p.stdout + p.stderr)[-3000:]


def test_an_unknown_case_is_no_pass(exe):
    assert subprocess.run([exe, "no_such_case"], capture_output=True, text=True).returncode == 2
