"""The headline kernel (the step-only dense plane kernel of flamingo_light_v1) with the solver's LDS reads batched (KTraits::LDSB),
compiled alone for gfx950 and read as assembly text: the mat-vecs and the triangular solves of a Newton iteration issue the reads of
a site together ahead of one wait, and the kernel as a whole waits for LDS less often than its parent did.  No GPU."""
import os
import re
import shutil
import subprocess

import pytest

HEADLINE = "cosim::env_kernel<18, 14, 1, false, 11, false, false, 1, 0, 0>"
# `s_waitcnt lgkmcnt(0)` in this kernel at commit dca13fc ("Step kernel: packed Cholesky updates, pivot look-ahead, register solves"),
# same compiler and flags: one per pair of terms in M v, J v and the substitutions
PARENT_LGKMCNT0 = 222


def _hipcc():
    h = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    return h if os.path.isfile(h) else shutil.which("hipcc")


def _read_dwords(op):
    """LDS dwords per lane that a ds_read* instruction returns."""
    n = 2 if "read2" in op else 1
    m = re.search(r"_b(\d+)$", op)
    return n * max(1, int(m.group(1)) // 32)


@pytest.mark.skipif(_hipcc() is None, reason="no hipcc")
def test_headline_kernel_reads_a_solver_site_behind_one_wait(tmp_path):
    from cosim_amd.engine import CSRC, HIPCC_TUNING
    src = tmp_path / "headline.hip"
    src.write_text('#include <math.h>\n#include <stdio.h>\n#include <stdlib.h>\n#include <string.h>\n#include "cosim_kernels.hip"\n'
                   f"template __global__ void {HEADLINE}(cosim::KArgs);\n")
    inc = os.path.join(os.path.dirname(CSRC), "..", "include")
    out = tmp_path / "headline.s"
    p = subprocess.run([_hipcc(), "--offload-arch=gfx950", "--cuda-device-only", "-S", "-O3", "-std=c++17", "-Wno-unused-value", *HIPCC_TUNING,
                        "-I", CSRC, "-I", inc, "-o", str(out), str(src)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    body, inside = [], False
    for line in out.read_text().splitlines():
        if re.match(r"_ZN5cosim10env_kernelILi18E\w*:", line):
            inside = True
        if inside:
            t = line.split(";")[0].strip()
            if t:
                body.append(t)
            if t == "s_endpgm":
                break
    assert body and body[-1] == "s_endpgm"
    waits0 = sum(1 for t in body if t.startswith("s_waitcnt") and "lgkmcnt(0)" in t)
    print("s_waitcnt lgkmcnt(0):", waits0, "parent:", PARENT_LGKMCNT0)
    assert waits0 < PARENT_LGKMCNT0
    # the Newton loop: from the Hessian's first matrix instruction to the wave-priority update that ends an iteration.  The text
    # between the two is the loop's body from the Hessian build on (factorisation, both substitutions, line search, move, constraint
    # update); the mat-vecs of qacc ahead of the loop and implicitfast behind it are outside and are not counted
    mfma = [i for i, t in enumerate(body) if t.startswith("v_mfma")]
    prio = [i for i, t in enumerate(body) if t.startswith("s_setprio")]
    assert mfma and prio and mfma[0] < prio[-1]
    runs, cur = [], 0
    for t in body[mfma[0]:prio[-1]]:
        op = t.split()[0]
        if op.startswith("ds_read"):
            cur += _read_dwords(op)
        elif op == "s_waitcnt" and "lgkmcnt" in t:               # a wait for LDS ends a run; a vmcnt-only wait does not
            runs.append(cur)
            cur = 0
    big = [r for r in runs if r >= 17]
    print("read-dwords between consecutive waits, Newton loop:", [r for r in runs if r])
    assert len(big) >= 3      # M s and J s (36 each), the backward substitution (18); the forward one where a factor is reused (18)
    # and they are the named sites: two runs of a whole row and vector (2 x 18 dwords), two of a factor row / column (18)
    assert sum(1 for r in runs if r in (36, 37)) == 2 and sum(1 for r in runs if r == 18) == 2
    # the parent's shape is gone from the loop: no run of nine waits in a row with exactly one pair of reads (4 dwords) before each
    assert not any(runs[i:i + 9] == [4] * 9 for i in range(len(runs)))
