"""Resources of the headline kernel (the step-only dense plane kernel of flamingo_light_v1) with the batched row loops: compiled
alone for gfx950, the way tools/kres.py reads a build.  Sixteen more values live across a wait must not cost the kernel its fourth
wave per SIMD (128 registers), a spilled register or scratch, and the batch needs no LDS of its own.  Resource numbers only."""
import os
import re
import shutil
import subprocess

import pytest

HEADLINE = "cosim::env_kernel<18, 14, 1, false, 11, false, false, 1, 0, 0>"


def _hipcc():
    h = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    return h if os.path.isfile(h) else shutil.which("hipcc")


@pytest.mark.skipif(_hipcc() is None, reason="no hipcc")
def test_headline_kernel_keeps_its_registers_and_lds(tmp_path):
    from cosim_amd.engine import CSRC, HIPCC_TUNING
    src = tmp_path / "headline.hip"
    src.write_text('#include <math.h>\n#include <stdio.h>\n#include <stdlib.h>\n#include <string.h>\n#include "cosim_kernels.hip"\n'
                   f"template __global__ void {HEADLINE}(cosim::KArgs);\n")
    inc = os.path.join(os.path.dirname(CSRC), "..", "include")
    p = subprocess.run([_hipcc(), "--offload-arch=gfx950", "--cuda-device-only", "-c", "-O3", "-std=c++17", "-Wno-unused-value", *HIPCC_TUNING,
                        "-I", CSRC, "-I", inc, "-Rpass-analysis=kernel-resource-usage", "-o", str(tmp_path / "headline.o"), str(src)],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    kernels, cur = {}, None
    for line in p.stderr.splitlines():                               # tools/kres.py's reading of the remarks
        m = re.search(r"remark:\s+(.*?) \[-Rpass", line)
        if not m:
            continue
        t = m.group(1).strip()
        if t.startswith("Function Name:"):
            cur = kernels.setdefault(t.split(":", 1)[1].strip(), {})
        elif cur is not None and ":" in t:
            k, v = t.split(":", 1)
            cur[k.strip()] = v.strip()
    mine = [v for k, v in kernels.items() if "env_kernel" in k]
    assert len(mine) == 1, sorted(kernels)
    r = mine[0]
    assert int(r["VGPRs"]) <= 128 and int(r["Occupancy [waves/SIMD]"]) == 4
    assert int(r["VGPRs Spill"]) == 0 and int(r["ScratchSize [bytes/lane]"]) == 0
    assert int(r["LDS Size [bytes/block]"]) == 10232
