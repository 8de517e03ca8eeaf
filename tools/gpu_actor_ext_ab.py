#!/usr/bin/env python3
"""What the extended actor kernels cost (52 -> 256 -> 128 -> 4 Elu actor, 4096 envs, the policy side alone: no physics):

    python tools/gpu_actor_ext_ab.py [--iters K] [--warmup W] [--repeats R] [--timeout S] [--parent-lib LIB.so] [--json OUT.json]

Legs, microseconds per evaluation of the whole fleet:
  plain            cosim_mlp_forward on the plain file, this build's library
  plain_parent     the same call into --parent-lib (libcosim_hip.so built from the parent commit): the plain instantiation is meant to
                   be unchanged, so the two agree within the spread of the session
  ext              cosim_mlp_forward_ex on write_random_mlp(normaliser=True, layer_norm=True): Sub, Div, Clip and LayerNorm on both
                   hidden layers
  ext_norm, ext_ln the same call on a file with the normaliser alone / the two LayerNorms alone: where ext's cost over plain goes
  ext_interp       ext's file through the interpreter on the same device (what it cost before)
  plain_interp     the plain file through the interpreter
  table_plain      PolicyTable over 4 plain files, 4 ranges, one get_action
  table_ext        the same over 4 extended files (mlp_grouped_ext_kernel)
The legs are interleaved R times, each run in a child process of its own under `timeout -k 10 S`; the first run that fails ends the
tool, nothing is retried.  A run times K evaluations behind W warm-up ones between two device events on one stream.  Information
only: one machine, one session; no threshold."""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, OBS, ACT = 4096, 52, 4
LEGS = ["plain", "plain_parent", "ext", "ext_norm", "ext_ln", "ext_interp", "plain_interp", "table_plain", "table_ext"]


def leg(name, iters, warmup, parent_lib):
    import torch
    from cosim_amd.policy import MLPPolicy, PolicyTable, write_random_mlp
    dev = torch.device("cuda", 0)
    d = tempfile.mkdtemp(prefix="cosim_actor_ab_")
    ext = name in ("ext", "ext_norm", "ext_ln", "ext_interp", "table_ext")
    files = [os.path.join(d, f"actor{k}.onnx") for k in range(4)]
    for k, f in enumerate(files):
        write_random_mlp(f, OBS, ACT, hidden=(256, 128), seed=50 + k, bias_scale=0.1, normaliser=ext and name != "ext_ln", layer_norm=ext and name != "ext_norm")
    x = torch.randn((N, OBS), dtype=torch.float32, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    out = torch.zeros((N, ACT), dtype=torch.float32, device=dev)
    if name.startswith("table"):
        tab = PolicyTable(files, num_envs=N, device=dev, ranges=[(i * (N // 4), N // 4) for i in range(4)])
        assert tab._handle is not None and (tab._create_suffix == "_create_ex") == ext

        def call():
            tab.get_action(x)
    elif name.endswith("interp"):
        pol = MLPPolicy(files[0], device=dev, fused=False)

        def call():
            pol.get_action(x)
    elif name == "plain_parent":
        pol = MLPPolicy(files[0], device=dev, fused=True)
        f = pol._fused
        L = ctypes.CDLL(parent_lib)
        vp, ci, cf = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
        L.cosim_mlp_forward.restype, L.cosim_mlp_forward.argtypes = ci, [vp, ci, ci] + [vp] * 5 + [cf, vp, vp]
        stream = torch.cuda.current_stream(dev).cuda_stream

        def call():
            assert L.cosim_mlp_forward(x.data_ptr(), N, f["nl"], f["dims"], f["w"], f["b"], f["act"], f["alpha"], 1.0, out.data_ptr(), stream) == 0
    else:
        pol = MLPPolicy(files[0], device=dev, fused=True)
        assert (pol._fused["extras"] is not None) == ext

        def call():
            pol.get_action_into(x, out)
    for _ in range(warmup):
        call()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        call()
    t1.record()
    torch.cuda.synchronize()
    print(json.dumps({"leg": name, "envs": N, "iters": iters, "warmup": warmup, "us_per_eval": 1000.0 * t0.elapsed_time(t1) / iters,
                      "device": torch.cuda.get_device_name(0)}))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--iters", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=60, help="seconds one run may take")
    ap.add_argument("--parent-lib", default="", help="libcosim_hip.so of the parent commit; without it the plain_parent leg is left out")
    ap.add_argument("--json", default="")
    ap.add_argument("--leg", default="", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.leg:
        leg(args.leg, args.iters, args.warmup, args.parent_lib)
        return 0
    legs = [name for name in LEGS if name != "plain_parent" or args.parent_lib]
    runs = []
    for r in range(args.repeats):
        for name in legs:
            p = subprocess.run(["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--leg", name, "--iters", str(args.iters),
                                "--warmup", str(args.warmup), "--parent-lib", os.path.abspath(args.parent_lib) if args.parent_lib else ""],
                               capture_output=True, text=True)
            if p.returncode != 0:
                print(f"{name} (repeat {r}) ended with status {p.returncode}: stopping\n{p.stderr[-2000:]}", file=sys.stderr)
                return 1
            runs.append({**json.loads(p.stdout.strip().splitlines()[-1]), "repeat": r})
            print(json.dumps(runs[-1]), flush=True)
    summary = {}
    for name in legs:
        v = sorted(x["us_per_eval"] for x in runs if x["leg"] == name)
        summary[name] = {"median": v[len(v) // 2], "min": v[0], "max": v[-1], "spread": (v[-1] - v[0]) / v[len(v) // 2]}
    m = {k: v["median"] for k, v in summary.items()}
    ratios = {"ext / plain": m["ext"] / m["plain"], "ext_norm / plain": m["ext_norm"] / m["plain"], "ext_ln / plain": m["ext_ln"] / m["plain"], "ext_interp / ext": m["ext_interp"] / m["ext"], "plain_interp / plain": m["plain_interp"] / m["plain"],
              "table_ext / table_plain": m["table_ext"] / m["table_plain"]}
    if "plain_parent" in m:
        ratios["plain / plain_parent"] = m["plain"] / m["plain_parent"]
    out = {"workload": f"actor {OBS} -> 256 -> 128 -> {ACT} (Elu), {N} envs, policy side alone; tables: 4 files, 4 ranges", "iters": args.iters,
           "warmup": args.warmup, "repeats": args.repeats, "us_per_eval": summary, "ratios_of_medians": ratios, "runs": runs}
    print(json.dumps({k: out[k] for k in ("workload", "us_per_eval", "ratios_of_medians")}, indent=1))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
