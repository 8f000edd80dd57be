#!/usr/bin/env python3
"""The hand-over table of profiles/r13_handover.txt from a rocprofv3 --kernel-trace run of
`python bench.py --no-pcie --steps 20 --warmup 5`: over the last N searches of the run (default 20)
the period, the search's length, the idle time between searches split into even and odd steps,
where the front end and the tail start relative to the searches, the drain, the dispatches per
batch and the hardware queues.

usage: handover_table.py TRACE_DIR [N]
All times in microseconds, medians (min - max)."""
import csv
import glob
import os
import statistics
import sys


def mmm(v):
    if not v:
        return "-"
    return f"{statistics.median(v):8.1f}  ({min(v):.1f} - {max(v):.1f})"


def main():
    root = sys.argv[1]
    last = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    ev = []
    for p in glob.glob(os.path.join(root, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(p)):
            name = r["Kernel_Name"].replace("(anonymous namespace)::", "").split("(")[0].split("<")[0].split("::")[-1]
            ev.append((int(r["Start_Timestamp"]) / 1e3, int(r["End_Timestamp"]) / 1e3, name, r.get("Queue_Id", "")))
    ev.sort()
    se = [e for e in ev if e[2].startswith("k_search_")][-last:]
    if len(se) < 3:
        print("too few searches", len(se))
        return
    t0, t1 = se[0][0], se[-1][1]
    win = [e for e in ev if t0 <= e[0] <= t1]
    print(f"searches in the window: {len(se)}")
    print(f"search start to next search start   {mmm([b[0] - a[0] for a, b in zip(se, se[1:])])}")
    print(f"{se[0][2]:35s} {mmm([e[1] - e[0] for e in se])}")
    gaps = [b[0] - a[1] for a, b in zip(se, se[1:])]
    print(f"search end to next search start     {mmm(gaps)}")
    print(f"  even steps                        {mmm(gaps[0::2])}")
    print(f"  odd steps                         {mmm(gaps[1::2])}")
    period = statistics.median([b[0] - a[0] for a, b in zip(se, se[1:])])
    d = abs(statistics.median(gaps[0::2]) - statistics.median(gaps[1::2]))
    print(f"  the two populations' medians differ by {d:.1f} us = {100 * d / period:.1f} % of the period")

    def running(t):   # the search that runs at time t, or the last one that ended before it
        cur = None
        for s in se:
            if s[0] <= t:
                cur = s
        return cur

    for kn in ("k_put_tables", "k_front", "k_nn_tail", "k_nn_deep_tail"):
        ks = [e for e in win if e[2] == kn]
        if not ks:
            continue
        print(f"{kn:35s} {mmm([e[1] - e[0] for e in ks])}   ({len(ks)} launches)")
        rs, re_, inside = [], [], 0
        for e in ks:
            s = running(e[0])
            if s is None:
                continue
            rs.append(e[0] - s[0])
            re_.append(e[0] - s[1])
            inside += s[0] <= e[0] < s[1]
        print(f"  start after the last search's start {mmm(rs)}")
        print(f"  start after that search's end       {mmm(re_)}   ({inside} of {len(ks)} start while it runs)")
    # the drain: from the first front-end kernel that gets a slot while a search runs to that search's end
    drain = []
    for s in se:
        fe = [e for e in win if e[2] in ("k_put_tables", "k_front") and s[0] <= e[0] < s[1]]
        if fe:
            drain.append(s[1] - fe[0][0])
    print(f"drain (first front-end kernel with a slot to the end of the search it waited behind) {mmm(drain)}   ({len(drain)} searches)")
    other = [e for e in win if not e[2].startswith("k_search_")]
    print(f"dispatches per batch (search included): {(len(other) + len(se)) / len(se):.2f}")
    qs = {}
    for e in win:
        qs.setdefault(e[2], set()).add(e[3])
    print("hardware queues: " + ", ".join(f"{k} {sorted(v)}" for k, v in sorted(qs.items())))
    print("search queue sequence: " + " ".join(e[3] for e in se))
    print("# first kernels of the window (start, duration, kernel, queue):")
    for e in win[:14]:
        print(f"# {e[0] - t0:9.1f} {e[1] - e[0]:8.1f}  {e[2]}  q{e[3]}")


if __name__ == "__main__":
    main()
