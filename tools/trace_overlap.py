#!/usr/bin/env python3
"""How many step kernels were in flight at once, from a rocprofv3 kernel trace:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python3 bench.py --steps 60 --warmup 10
    python tools/trace_overlap.py DIR [--match env_kernel] [--title TEXT] [--out FILE]

Reads every *kernel_trace.csv under DIR (or the files given).  The step kernel is the most-launched kernel whose name contains
--match and not "fixup".  Reports the hardware queue ids it ran on with the launches of each, its durations, and the share of the
traced span (first start to last end of a step kernel) during which at least 1, 2, 3 and 4 of them were running -- range chains that
share a queue never overlap, so "4 streams" on fewer queues shows as a small share at the higher counts -- and, per queue pair, whether
two launches ever overlapped.  Then the per-kernel table of the whole trace.  Plain text; no GPU needed to run it."""
import argparse
import collections
import csv
import glob
import os
import sys


def load(paths):
    files = []
    for p in paths:
        files += sorted(glob.glob(os.path.join(p, "**", "*kernel_trace.csv"), recursive=True)) if os.path.isdir(p) else [p]
    rows = []
    for f in files:
        with open(f, newline="") as fh:
            for r in csv.DictReader(fh):
                rows.append((r["Kernel_Name"], r.get("Queue_Id", "?"), int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
    return rows


def in_flight_shares(spans, most=4):
    """spans: (start, end) -> share of [min start, max end] with at least k = 1..most of them open."""
    ev = sorted([(s, 1) for s, _ in spans] + [(e, -1) for _, e in spans])   # at equal times an end (-1) sorts before a start
    t0, t1 = min(s for s, _ in spans), max(e for _, e in spans)
    at_least = [0] * (most + 1)
    level, last = 0, t0
    for t, d in ev:
        for k in range(1, min(level, most) + 1):
            at_least[k] += t - last
        level, last = level + d, t
    return [at_least[k] / max(1, t1 - t0) for k in range(1, most + 1)], t1 - t0


def report(rows, match, title):
    out = [title] if title else []
    calls = collections.Counter(n for n, _, _, _ in rows if match in n and "fixup" not in n)
    if not calls:
        return "\n".join(out + [f"no kernel matching {match!r} in the trace"])
    name = calls.most_common(1)[0][0]
    k = [(q, s, e) for n, q, s, e in rows if n == name]
    dur = [e - s for _, s, e in k]
    out.append(f"step kernel: {name}")
    out.append(f"launches {len(k)}, duration us: mean {sum(dur) / len(dur) / 1e3:.2f} min {min(dur) / 1e3:.2f} max {max(dur) / 1e3:.2f}")
    queues = sorted({q for q, _, _ in k}, key=lambda q: (len(q), q))
    out.append(f"distinct hardware queue ids of the step kernel: {len(queues)}  (" +
               ", ".join(f"queue {q}: {sum(1 for x in k if x[0] == q)} launches" for q in queues) + ")")
    shares, span = in_flight_shares([(s, e) for _, s, e in k])
    out.append(f"traced span {span / 1e6:.3f} ms; step kernels per ms of span {len(k) / (span / 1e6):.2f}")
    for i, s in enumerate(shares):
        out.append(f"  share of the span with {'>= ' if i < 3 else '   '}{i + 1} step kernel{'s' if i else ''} in flight: {100 * s:6.2f} %")
    # do launches on one queue, and on each pair of queues, ever overlap?
    for a in range(len(queues)):
        for b in range(a, len(queues)):
            xa = sorted((s, e) for q, s, e in k if q == queues[a])
            xb = sorted((s, e) for q, s, e in k if q == queues[b])
            if a == b:
                ov = sum(max(0, xa[i][1] - xa[i + 1][0]) for i in range(len(xa) - 1))
            else:
                ov, j = 0, 0
                for s, e in xa:
                    while j < len(xb) and xb[j][1] <= s:
                        j += 1
                    i = j
                    while i < len(xb) and xb[i][0] < e:
                        ov += max(0, min(e, xb[i][1]) - max(s, xb[i][0]))
                        i += 1
            out.append(f"  overlap of launches on queue {queues[a]} with queue {queues[b]}: {ov / 1e6:8.3f} ms")
    by = collections.defaultdict(list)
    for n, _, s, e in rows:
        by[n].append(e - s)
    out.append("")
    out.append(f"{'kernel':110s} {'calls':>6s} {'avg_us':>10s} {'min_us':>10s} {'max_us':>10s} {'total_ms':>10s}")
    for n, v in sorted(by.items(), key=lambda kv: -sum(kv[1]))[:12]:
        out.append(f"{n[:110]:110s} {len(v):6d} {sum(v) / len(v) / 1e3:10.2f} {min(v) / 1e3:10.2f} {max(v) / 1e3:10.2f} {sum(v) / 1e6:10.3f}")
    return "\n".join(out)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("paths", nargs="+", help="rocprofv3 output directory, or kernel_trace.csv files")
    ap.add_argument("--match", default="env_kernel")
    ap.add_argument("--title", default="")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = load(a.paths)
    if not rows:
        print("no kernel_trace.csv rows found", file=sys.stderr)
        return 1
    text = report(rows, a.match, a.title)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
