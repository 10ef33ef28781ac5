#!/usr/bin/env python3
"""Overlap summary of the conv + op_sigs section of one benchmark step from a rocprofv3 kernel trace.

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python bench.py --steps 3 --warmup 1
    python tools/lanes_trace.py DIR/**/*_kernel_trace.csv

The last replayed step is found as the shortest tail of the trace (by start time) whose kernel names
repeat, as a multiset, in the kernels just before it (the steps launch the same kernels; with capture
lanes their start order may differ). Its section is what starts after the step's longest kernel: the
sgemm set runs first, in ascending size, and its last op (12288^3) is wide, so every lane is joined
behind it. Prints one
JSON line: span (first start to last end), sum of kernel durations, kernels that overlap another."""
import collections
import csv
import json
import sys


def load(path):
    rows = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    return rows


def last_step(rows, min_len=50):
    names = [r[2] for r in rows]
    n = len(names)
    for p in range(min_len, n // 2 + 1):
        if collections.Counter(names[n - p:]) == collections.Counter(names[n - 2 * p:n - p]):
            return rows[n - p:]
    raise SystemExit("no repeating step found in %d kernels" % n)


def summary(rows):
    step = last_step(rows)
    t0 = max(step, key=lambda r: r[1] - r[0])[1]
    sec = [r for r in step if r[0] >= t0]
    overl = 0
    for i, (s, e, _) in enumerate(sec):
        # sorted by start: overlaps a neighbour iff an earlier kernel still runs or the next starts early
        if any(pe > s for _, pe, _ in sec[max(0, i - 8):i]) or (i + 1 < len(sec) and sec[i + 1][0] < e):
            overl += 1
    return {"step_kernels": len(step), "section_kernels": len(sec),
            "span_us": round((max(r[1] for r in sec) - sec[0][0]) / 1e3, 1),
            "sum_kernel_us": round(sum(r[1] - r[0] for r in sec) / 1e3, 1),
            "kernels_overlapping_another": overl}


if __name__ == "__main__":
    print(json.dumps(summary(load(sys.argv[1]))))
