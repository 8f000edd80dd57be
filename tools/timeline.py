#!/usr/bin/env python3
"""Timeline of a rocprofv3 --kernel-trace --memory-copy-trace run of bench.py: the last steps'
kernels and copies in start order with their offsets and durations, and per-step spacing
(k_front to k_front; k_classify in traces of older trees).

usage: timeline.py TRACE_DIR [steps_to_show] [first_step]
first_step: index of the first k_front launch shown (default: the last steps_to_show steps;
bench.py runs the PCIe-inclusive pass before the resident one, so its steps come first)."""
import csv
import glob
import os
import sys


def main():
    root = sys.argv[1]
    show = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    first = int(sys.argv[3]) if len(sys.argv) > 3 else None
    ev = []
    for p in glob.glob(os.path.join(root, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(p)):
            name = r["Kernel_Name"].replace("(anonymous namespace)::", "").split("(")[0]
            ev.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), "K", name[-40:], r.get("Queue_Id", "")))
    for p in glob.glob(os.path.join(root, "**", "*memory_copy_trace.csv"), recursive=True):
        for r in csv.DictReader(open(p)):
            kind = r.get("Direction", r.get("Operation", "copy"))
            size = r.get("Size", r.get("Bytes", ""))
            ev.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), "C", f"{kind} {size}", ""))
    ev.sort()
    cls = [e for e in ev if e[2] == "K" and ("k_front" in e[3] or "k_classify" in e[3])]
    if len(cls) < show + 1:
        print("too few steps", len(cls))
        return
    gaps = [(cls[i + 1][0] - cls[i][0]) / 1e3 for i in range(len(cls) - 1)]
    print("front-to-front (us):", [round(g) for g in gaps])
    # batches may overlap (consecutive batches on two streams): per search, the idle time before the
    # next search starts (negative: they run side by side), whether the next front end started
    # while it ran, and when the tail that follows it ended against the next search's end
    se = [e for e in ev if e[2] == "K" and "k_search_" in e[3]]
    ta = [e for e in ev if e[2] == "K" and "k_nn_" in e[3] and "tail" in e[3]]
    print("search end -> next search start (us):", [round((b[0] - a[1]) / 1e3, 1) for a, b in zip(se, se[1:])][-show - 8:])
    early = sum(1 for f in cls if any(a[0] < f[0] < a[1] for a in se))
    print(f"front ends that start while a search runs: {early} of {len(cls)}")
    late = []
    for a, b in zip(se, se[1:]):
        t = next((x for x in ta if x[0] >= a[1]), None)   # the first tail that starts after this search ends
        if t:
            late.append(round((t[1] - b[1]) / 1e3, 1))
    print("tail end - next search end (us; negative: the tail is over first):", late[-show - 8:])
    i0 = len(cls) - show - 1 if first is None else first
    t0 = cls[i0][0]
    t1 = cls[min(i0 + show, len(cls) - 1)][0]
    for s, e, k, name, q in ev:
        if t0 <= s <= t1 or t0 <= e <= t1:
            print(f"{(s - t0) / 1e3:9.1f} {(e - s) / 1e3:8.1f} us  {k} {name} {q}")


if __name__ == "__main__":
    main()
