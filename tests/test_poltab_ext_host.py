"""The extended half of the policy table's host code without a GPU (csrc/cosim_poltab.h: PolExtRaw, check_extras,
pack_policy_extras) through tests/poltab_ext_host.cpp, built plain and with AddressSanitizer / UBSan as a stand-alone child process:
the image and both records of a three-policy table word for word against a packing written here in numpy, every refusal of the
validator, and that a table without extras packs to what it always did."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
i32 = np.int32
ML, MS = 6, 4
FN = "cosim_policy_table_create_ex"


def _build(tmp, source, variant):
    out = str(tmp / (source.replace(".cpp", "_") + variant.replace("-", "_")))
    extra = [] if variant == "plain" else ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
    subprocess.check_call([os.environ.get("CXX", "c++"), "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unknown-pragmas", *extra, "-I",
                           os.path.join(ROOT, "cosim_amd", "csrc"), "-o", out, os.path.join(ROOT, "tests", source)])
    return out


@pytest.fixture(scope="module", params=["plain", "asan-ubsan"])
def exe(request, tmp_path_factory):
    return _build(tmp_path_factory.mktemp("poltab_ext"), "poltab_ext_host.cpp", request.param)


def _ints(a):
    a = np.asarray(a, dtype=np.int64).ravel()
    return [str(a.size)] + [str(int(x)) for x in a]


def extras(n_in=0, n_out=0, in_op=(), out_op=(), in_vec=None, out_vec=None, in_lohi=(), out_lohi=(), ln=None):
    """One policy's extras.  in_vec / out_vec: which items get a vector (default: every op but a clip); lohi: (lo, hi) per item;
    ln: {slot: (where, eps, has_scale, has_bias)}."""
    e = {"n_in": n_in, "n_out": n_out, "in_op": list(in_op) + [0] * (MS - len(in_op)), "out_op": list(out_op) + [0] * (MS - len(out_op))}
    e["in_vec"] = [int(op in (1, 2, 3, 4)) for op in e["in_op"]] if in_vec is None else list(in_vec)
    e["out_vec"] = [int(op in (1, 2, 3, 4)) for op in e["out_op"]] if out_vec is None else list(out_vec)
    for key, lohi in (("in", in_lohi), ("out", out_lohi)):
        lohi = list(lohi) + [(0.0, 0.0)] * (MS - len(lohi))
        e[key + "_lo"], e[key + "_hi"] = [p[0] for p in lohi], [p[1] for p in lohi]
    e["ln"] = dict(ln or {})
    return e


def table(policies, ext, assign):
    """policies: per policy (dims, acts, has_bias per layer); ext: None, or per policy an ``extras(...)``."""
    K, n = len(policies), len(assign)
    dims, act, hb = np.zeros((K, ML + 1), i32), np.zeros((K, ML), i32), np.zeros((K, ML), i32)
    for k, (d, a, b) in enumerate(policies):
        dims[k, :len(d)], act[k, :len(a)], hb[k, :len(b)] = d, a, b
    return {"K": K, "nl": np.array([len(p[0]) - 1 for p in policies], i32), "dims": dims, "act": act, "has_bias": hb, "n": n, "por": np.asarray(assign, i32),
            "ranges": np.array([(0, n)], i32), "ext": ext}


def _f(x):
    return repr(float(x)) if np.isfinite(x) else ("nan" if np.isnan(x) else ("inf" if x > 0 else "-inf"))


def run(exe, t):
    tok = [str(t["K"])] + _ints(t["nl"]) + _ints(t["dims"]) + _ints(t["act"]) + _ints(t["has_bias"]) + [str(t["n"])] + _ints(t["por"]) + ["1"] + _ints(t["ranges"])
    tok.append("0" if t["ext"] is None else "1")
    for e in t["ext"] or []:
        tok += [str(e["n_in"]), str(e["n_out"])] + [str(v) for key in ("in_op", "out_op", "in_vec", "out_vec") for v in e[key]]
        tok += [_f(v) for key in ("in_lo", "in_hi", "out_lo", "out_hi") for v in e[key]]
        ln = [e["ln"].get(s, (0, 0.0, 0, 0)) for s in range(ML + 1)]
        tok += [str(x[0]) for x in ln] + [_f(x[1]) for x in ln] + [str(x[2]) for x in ln] + [str(x[3]) for x in ln]
    p = subprocess.run([exe], input=" ".join(tok), capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = p.stdout.splitlines()
    if lines[0].startswith("ERR "):
        return "ERR", lines[0][4:]
    assert lines[0] == "OK"
    out = {"desc": [], "ext": [], "lines": lines}
    for ln in lines[1:]:
        f = ln.split()
        v = [int(x) for x in f[1:]]
        if f[0] == "image":
            assert v[0] == len(v) - 1
            out["image"] = np.array(v[1:], dtype=np.int64)
        elif f[0] in ("maxd", "next"):
            out[f[0]] = v[0]
        elif f[0] == "ext":
            out["ext"].append(np.array(v, dtype=np.int64).astype(i32))
        else:
            out["desc"].append({"nl": v[0], "dims": v[1:8], "act": v[8:14], "woff": v[14:20], "boff": v[20:26]})
    return "OK", out


def _pack(policies, ext):
    """The image and the two records per policy as the header documents them, written independently: per policy its layers (a matrix
    begins at a multiple of 4 words, the bias follows), then item by item the input and the output vector of that position, then slot
    by slot scale and bias -- every vector begun at a multiple of 4 words; a record is 64 words."""
    img, descs, recs = [], [], []

    def aligned(words):
        while len(img) % 4:
            img.append(0)
        off = len(img)
        img.extend(words)
        return off
    for k, ((dims, acts, hb), e) in enumerate(zip(policies, ext)):
        nl = len(dims) - 1
        woff, boff = [-1] * ML, [-1] * ML
        for l in range(nl):
            woff[l] = aligned([64 * k + 8 * l + 1] * (dims[l] * dims[l + 1]))
            if hb[l]:
                boff[l] = len(img)
                img.extend([64 * k + 8 * l + 2] * dims[l + 1])
        descs.append({"nl": nl, "dims": list(dims) + [0] * (ML + 1 - len(dims)), "act": list(acts) + [0] * (ML - nl), "woff": woff, "boff": boff})
        rec = np.zeros(64, i32)
        fl = rec.view(np.float32)
        rec[0], rec[1] = e["n_in"], e["n_out"]
        for i in range(MS):
            for side, base, count, width, value in (("in", 4, e["n_in"], dims[0], 10000), ("out", 20, e["n_out"], dims[-1], 20000)):
                q = base + 4 * i
                rec[q + 1] = -1
                if i < count:
                    rec[q] = e[side + "_op"][i]
                    fl[q + 2], fl[q + 3] = e[side + "_lo"][i], e[side + "_hi"][i]
                    if e[side + "_op"][i] != 5:
                        rec[q + 1] = aligned([value + 100 * k + i] * width)
        for s in range(ML + 1):
            rec[43 + s] = rec[50 + s] = -1
            where, eps, has_g, has_b = e["ln"].get(s, (0, 0.0, 0, 0))
            if s < nl and where:
                rec[36 + s], fl[57 + s] = where, eps
                rec[43 + s] = aligned([30000 + 100 * k + s] * dims[s])
                off = aligned([40000 + 100 * k + s] * dims[s] if has_b else [])
                rec[50 + s] = off if has_b else -1
        recs.append(rec)
    return np.array(img, dtype=np.int64), descs, recs


POLICIES = [((12, 40, 36, 4), (5, 3, 0), (1, 1, 1)),             # plain
            ((12, 33, 4), (4, 0), (0, 1)),                       # normaliser: Sub, Div, Clip
            ((12, 7, 5, 4), (3, 2, 2), (1, 0, 1))]               # LN on obs, before layer 0's act, behind layer 1's; output Mul, Add, Clip
EXT = [extras(),
       extras(n_in=3, in_op=(2, 4, 5), in_lohi=((0, 0), (0, 0), (-5.0, 5.0))),
       extras(n_out=3, out_op=(3, 1, 5), out_lohi=((0, 0), (0, 0), (-0.8, float("inf"))),
              ln={0: (1, 1e-5, 1, 1), 1: (1, 1e-3, 1, 0), 2: (2, 1e-5, 1, 1)})]


def test_image_and_records_equal_the_numpy_packing(exe):
    status, got = run(exe, table(POLICIES, EXT, [0, 1, 2, 2, 1]))
    assert status == "OK" and got["maxd"] == 40 and got["next"] == 3
    img, descs, recs = _pack(POLICIES, EXT)
    assert got["desc"] == descs
    assert np.array_equal(got["image"], img), np.argwhere(got["image"][:len(img)] != img[:len(got["image"])])[:5]
    for k in range(3):
        assert np.array_equal(got["ext"][k], recs[k]), (k, np.argwhere(got["ext"][k] != recs[k]).ravel())
    # what the numbers mean: every vector begins at a multiple of 4 words and holds its own value; the plain policy's record is empty
    assert (recs[0][[5, 9, 13, 17, 21, 25, 29, 33]] == -1).all() and not recs[0][:4].any() and not recs[0][36:43].any()
    r1, r2 = recs[1], recs[2]
    assert r1[4] == 2 and r1[5] % 4 == 0 and (img[r1[5]:r1[5] + 12] == 10100).all() and (img[r1[9]:r1[9] + 12] == 10101).all() and r1[13] == -1
    assert r1.view(np.float32)[14] == -5.0 and r1.view(np.float32)[15] == 5.0
    assert (img[r2[21]:r2[21] + 4] == 20200).all() and np.isinf(r2.view(np.float32)[31]) and r2[29] == -1
    assert (img[r2[43]:r2[43] + 12] == 30200).all() and (img[r2[44]:r2[44] + 7] == 30201).all() and r2[51] == -1 and (img[r2[52]:r2[52] + 5] == 40202).all()
    assert all(o % 4 == 0 for o in list(r2[43:46]) + [r2[50], r2[52]])


def test_a_table_without_extras_packs_to_what_it_always_did(exe, tmp_path):
    none = run(exe, table(POLICIES, None, [0, 1, 2, 2, 1]))[1]
    zero = run(exe, table(POLICIES, [extras()] * 3, [0, 1, 2, 2, 1]))[1]
    assert none["next"] == 0 and zero["next"] == 0 and none["lines"] == zero["lines"]
    # and to what pack_policy_image gives the plain driver (tests/poltab_host.cpp) for the same table
    old = _build(tmp_path, "poltab_host.cpp", "plain")
    t = table(POLICIES, None, [0, 1, 2, 2, 1])
    tok = [str(t["K"])] + _ints(t["nl"]) + _ints(t["dims"]) + _ints(t["act"]) + _ints(t["has_bias"]) + [str(t["n"])] + _ints(t["por"]) + ["1"] + _ints(t["ranges"])
    lines = subprocess.run([old], input=" ".join(tok), capture_output=True, text=True, check=True).stdout.splitlines()
    keep = [ln for ln in lines if ln.split()[0] in ("desc", "image")]
    assert keep == [ln for ln in none["lines"] if ln.split()[0] in ("desc", "image")] and len(keep) == 4
    # with extras in the table, the layers of the policies ahead of the first vector still sit where they did
    ext = run(exe, table(POLICIES, EXT, [0, 1, 2, 2, 1]))[1]
    first_vec = int(ext["ext"][1][5])
    assert ext["desc"][:2] == none["desc"][:2] and np.array_equal(ext["image"][:first_vec], none["image"][:first_vec])


def test_every_refusal_of_the_extras_validator(exe):
    good = table(POLICIES, EXT, [0, 1, 2, 2, 1])
    assert run(exe, good)[0] == "OK"

    def refused(want, k, **over):
        ext = [dict(e) for e in EXT]
        ext[k] = {**ext[k], **over}
        assert run(exe, {**good, "ext": ext}) == ("ERR", f"{FN}: policy {k}: {want}")
    refused("input stage: 5 items, outside 0..4", 1, n_in=5)
    refused("output stage: -1 items, outside 0..4", 2, n_out=-1)
    for code in (0, 6, -3):
        refused(f"input stage, item 1: unknown op code {code} (1 add, 2 sub, 3 mul, 4 div, 5 clip)", 1, in_op=[2, code, 5, 0])
    refused("output stage, item 0: unknown op code 9 (1 add, 2 sub, 3 mul, 4 div, 5 clip)", 2, out_op=[9, 1, 5, 0])
    refused("input stage, item 0: null vector", 1, in_vec=[0, 1, 0, 0])
    refused("output stage, item 1: null vector", 2, out_vec=[1, 0, 0, 0])
    for eps, text in ((0.0, "0.000000"), (-1e-5, "-0.000010"), (float("inf"), "inf"), (float("nan"), "nan")):
        refused(f"LayerNorm slot 1: eps {text} is not a positive finite number", 2, ln={**EXT[2]["ln"], 1: (1, eps, 1, 0)})
    refused("LayerNorm slot 3: LayerNorm on the last layer", 2, ln={**EXT[2]["ln"], 3: (1, 1e-5, 1, 1)})
    refused("LayerNorm slot 2: LayerNorm on the last layer", 1, ln={2: (2, 1e-5, 1, 1)})
    refused("LayerNorm slot 0: null scale vector", 2, ln={**EXT[2]["ln"], 0: (1, 1e-5, 0, 1)})
    refused("LayerNorm slot 1: unknown placement 3 (0 none, 1 before the activation, 2 behind it)", 2, ln={**EXT[2]["ln"], 1: (3, 1e-5, 1, 0)})
    # a clip needs no vector, a slot behind the last layer is not read, and the table's own checks come first and keep the entry point's name
    ext = [dict(e) for e in EXT]
    ext[1] = {**ext[1], "ln": {5: (7, -1.0, 0, 0)}}
    assert run(exe, {**good, "ext": ext})[0] == "OK"
    # such a stray slot alone does not make a table an extended one: no second record, the plain image
    stray = run(exe, {**good, "ext": [extras(), extras(ln={5: (1, 1e-5, 1, 1)}), extras(ln={3: (0, 0.0, 0, 0), 6: (2, 1e-5, 1, 0)})]})[1]
    assert stray["next"] == 0 and stray["lines"] == run(exe, {**good, "ext": None})[1]["lines"]
    assert run(exe, {**good, "K": 0}) == ("ERR", f"{FN}: 0 policies, outside 1..64")
