#!/usr/bin/env python3
"""Code bytes per kernel of the HIP engine (gfx950), largest first.  Needs no GPU.

    python tools/ksize.py [flags]         # compile cosim_engine.hip device-only and read the kernel symbol sizes
                                          # (extra hipcc flags replace the product build's tuning flags, engine.HIPCC_TUNING)
    python tools/ksize.py --lib [PATH]    # the same table from the code object inside an already built libcosim_hip.so

AMD's CDNA3 documentation gives the instruction cache as 64 KiB per pair of compute units.  A kernel's symbol size overstates what
its waves execute: measured on MI355X, the 76 KB headline kernel hits that cache on 99.8 % of its fetches.
"""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LLVM = os.environ.get("ROCM_LLVM", "/opt/rocm/llvm/bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
BUNDLE_MAGICS = (b"__CLANG_OFFLOAD_BUNDLE__", b"CCOB")


def run(cmd):
    p = subprocess.run(cmd, capture_output=True, text=True)
    if p.returncode:
        sys.stderr.write(p.stdout + p.stderr)
        sys.exit(p.returncode)
    return p.stdout


def unbundle(path, out):
    """gfx950 code object of a clang offload bundle (a plain code object is passed through)."""
    with open(path, "rb") as f:
        head = f.read(24)
    if not head.startswith(BUNDLE_MAGICS):
        return path
    run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", f"--targets={TARGET}", f"--input={path}", f"--output={out}"])
    return out


def kernel_sizes(code_object):
    """{mangled kernel name: code bytes}: the function symbols that have a kernel descriptor (<name>.kd) beside them."""
    text = run([os.path.join(LLVM, "llvm-readelf"), "--symbols", "--wide", code_object])
    size, kd = {}, set()
    for line in text.splitlines():
        m = re.match(r"\s*\d+:\s+[0-9a-fA-F]+\s+(\d+)\s+(\w+)\s+\w+\s+\w+\s+\S+\s+(\S+)", line)
        if not m:
            continue
        n, typ, name = int(m.group(1)), m.group(2), m.group(3)
        if typ == "OBJECT" and name.endswith(".kd"):
            kd.add(name[:-3])
        elif typ == "FUNC":
            size[name] = n
    return {k: v for k, v in size.items() if k in kd}


def main():
    from cosim_amd.engine import CSRC, HIPCC_TUNING, LIB_PATH
    args = sys.argv[1:]
    with tempfile.TemporaryDirectory() as tmp:
        if args and args[0] == "--lib":
            lib = args[1] if len(args) > 1 else LIB_PATH
            fat = os.path.join(tmp, "fatbin")
            run([os.path.join(LLVM, "llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", lib, fat])
            src, what = fat, f"code object of {os.path.relpath(lib, ROOT)}"
        else:
            hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
            flags = args if args else HIPCC_TUNING
            src = os.path.join(tmp, "engine.dev")
            run([hipcc, "--offload-arch=gfx950", "--cuda-device-only", "-c", "-O3", "-std=c++17", "-Wno-unused-value", *flags, "-o", src,
                 os.path.join(CSRC, "cosim_engine.hip")])
            what = "hipcc --offload-arch=gfx950 --cuda-device-only -O3 " + " ".join(flags)
        sizes = kernel_sizes(unbundle(src, os.path.join(tmp, "engine.co")))
    names = list(sizes)
    dem = run(["c++filt"] + names).splitlines() if names else []
    print(f"# code bytes per kernel, gfx950: {what}")
    print(f"{'bytes':>8s}  kernel")
    for name, d in sorted(zip(names, dem), key=lambda nd: (-sizes[nd[0]], nd[1])):
        d = d.replace("cosim::", "").replace("(KArgs)", "")
        if d.startswith("void "):
            d = d[5:]
        print(f"{sizes[name]:8d}  {d}")


if __name__ == "__main__":
    main()
