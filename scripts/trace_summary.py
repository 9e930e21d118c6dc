"""Summarise rocprofv3 --kernel-trace output (kernel_trace.csv): per kernel, the launches at its largest grid size (the
set-up phase of bench.py launches the solve kernel on small batches as well) and within a factor of two of the longest -- calls, average / min / max duration.
Launches of one handle may overlap (two launch lanes, DESIGN.md 5.1 "Work distribution"): each of two overlapped launches then shows a longer
duration than it would alone, so next to the mean the table has, over the same launches,
  busy_us   the union of their [start, end] intervals divided by their number: the time the card was busy with the kernel per launch;
  ovl_%     the share of that union during which at least two of them ran;
  idle_%    the share of the time from the first start to the last end during which none of them ran; a gap of a millisecond or more is
            the host's (set-up, a fence between the warm-up and the timed steps) and is left out of both sides of the ratio.
Usage: python scripts/trace_summary.py gpurun_out/prof_xxx [more dirs] > profiles/xxx_kernel_trace_summary.txt"""
import collections
import csv
import glob
import sys


HOST_GAP_NS = 1_000_000


def union_and_overlap(intervals):
    """(ns covered by at least one interval, ns covered by at least two, ns of the gaps shorter than HOST_GAP_NS) of [(start, end)]"""
    ev = sorted([(s, 1) for s, _ in intervals] + [(e, -1) for _, e in intervals], key=lambda p: (p[0], p[1]))
    depth, last, one, two, idle = 0, ev[0][0], 0, 0, 0
    for t, d in ev:
        if depth >= 1:
            one += t - last
        if depth >= 2:
            two += t - last
        if depth == 0 and t - last < HOST_GAP_NS:
            idle += t - last
        depth, last = depth + d, t
    return one, two, idle


if __name__ == "__main__":
    for d in sys.argv[1:]:
        for f in glob.glob(d + "/**/*kernel_trace.csv", recursive=True):
            rows = list(csv.DictReader(open(f)))
            per = collections.defaultdict(list)
            for r in rows:
                grid = int(r.get("Grid_Size", r.get("Grid_Size_X", 0)) or 0)
                per[r["Kernel_Name"]].append((grid, int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
            print(f"# {f}")
            print(f"{'kernel':70s} {'grid':>8s} {'calls':>6s} {'avg_us':>10s} {'min_us':>10s} {'max_us':>10s} {'busy_us':>10s} {'ovl_%':>7s} {'idle_%':>7s}")
            for name, v in sorted(per.items(), key=lambda kv: -sum(e - s for _, s, e in kv[1])):
                gmax = max(g for g, _, _ in v)
                iv = [(s, e) for g, s, e in v if g == gmax]
                # (round 4: the first work items of a launch are dealt wave-major, so every batch of at least one item per CU has the full grid;
                # the full-size launches are then the ones within a factor of two of the longest)
                tmax = max(e - s for s, e in iv)
                iv = [(s, e) for s, e in iv if 2 * (e - s) >= tmax]
                t = [e - s for s, e in iv]
                one, two, idle = union_and_overlap(iv)
                short = name.split("(tmpc::")[0].replace("void ", "").replace("(anonymous namespace)::", "")[:70]
                print(f"{short:70s} {gmax:8d} {len(t):6d} {sum(t) / len(t) / 1e3:10.2f} {min(t) / 1e3:10.2f} {max(t) / 1e3:10.2f} "
                      f"{one / len(t) / 1e3:10.2f} {100.0 * two / max(one, 1):7.1f} {100.0 * idle / max(one + idle, 1):7.1f}")
