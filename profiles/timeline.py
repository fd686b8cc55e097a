#!/usr/bin/env python3
"""Timeline of the forked decode + E-step call from a rocprofv3 --kernel-trace CSV.

A step runs from a kw_prepass launch to the kw_mstep launch that follows it.  It is a forked step (decode and
E-step in one call, on two streams) when it holds one kw_bwd, one kw_fwd and one backtrace launch and the backtrace
ends after kw_fwd has started; in the benchmark's profiling pass the decode is a call of its own and ends first.
For every kernel that starts between the step's kw_prepass and its kw_mstep the table gives
the median, over the forked steps, of start and end relative to the END of kw_bwd, the duration, and the gap
to the end of the previous launch of the decode branch (launches of the same name inside one step are
numbered in launch order).

usage: timeline.py <b_kernel_trace.csv> <out.md> [title]
"""
import csv
import statistics
import sys

sys.path.insert(0, __import__("os").path.dirname(__file__))
from summarize import short  # noqa: E402

ESTEP = {"kw_prepass", "kw_fwd", "kw_bwd", "kw_fb_check", "kw_stats_final", "kw_mstep", "kw_gsum"}


def main():
    src, dst = sys.argv[1:3]
    title = sys.argv[3] if len(sys.argv) > 3 else src
    rows = []
    for r in csv.DictReader(open(src)):
        rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), short(r["Kernel_Name"])))
    rows.sort()
    # steps: from one kw_prepass to the kw_mstep that follows it
    steps, cur = [], None
    for s, e, n in rows:
        if n == "kw_prepass":
            cur = []
        if cur is not None:
            cur.append((s, e, n))
            if n == "kw_mstep":
                steps.append(cur)
                cur = None
    def is_forked(st):   # decode and E-step in one call: the backtrace ends after the forward sweep has started
        if sum(n == "kw_bwd" for _, _, n in st) != 1:
            return False
        bt = [e for _, e, n in st if n.startswith("kw_backtrace")]
        fw = [s for s, _, n in st if n == "kw_fwd"]
        return len(bt) == 1 and len(fw) == 1 and bt[0] > fw[0]

    forked = [st for st in steps if is_forked(st)]
    if len(forked) > 4:
        forked = forked[len(forked) // 4:]     # the first quarter is warm-up
    acc, order = {}, []
    bwd_dur, step_dur = [], []
    for st in forked:
        bend = [e for _, e, n in st if n == "kw_bwd"][0]
        bwd_dur.append([e - s for s, e, n in st if n == "kw_bwd"][0])
        step_dur.append(st[-1][1] - st[0][0])
        seen, prev_end = {}, None
        for s, e, n in st:
            seen[n] = seen.get(n, 0) + 1
            key = "%s #%d" % (n, seen[n]) if n not in ESTEP else n
            gap = None
            if n not in ESTEP:
                gap = s - prev_end if prev_end is not None else None
                prev_end = e
            if key not in acc:
                acc[key] = ([], [], [], [])
                order.append(key)
            a = acc[key]
            a[0].append(s - bend); a[1].append(e - bend); a[2].append(e - s)
            if gap is not None:
                a[3].append(gap)
    med = lambda v: statistics.median(v) / 1e3 if v else float("nan")   # noqa: E731
    with open(dst, "w") as f:
        f.write("# %s\n\n" % title)
        f.write("%d forked steps (warm-up quarter dropped).  Times in microseconds relative to the end of kw_bwd; "
                "medians over the steps.  kw_bwd itself: median %.1f us (min %.1f, max %.1f); kw_prepass start to "
                "kw_mstep end: median %.1f us.\n\n" % (len(forked), med(bwd_dur), min(bwd_dur) / 1e3,
                                                        max(bwd_dur) / 1e3, med(step_dur)))
        f.write("| launch | seen in steps | start | end | duration | gap to previous decode launch |\n|---|---|---|---|---|---|\n")
        for k in sorted(order, key=lambda k: statistics.median(acc[k][0])):
            a = acc[k]
            f.write("| %s | %d | %.1f | %.1f | %.1f | %s |\n" % (
                k, len(a[0]), med(a[0]), med(a[1]), med(a[2]), ("%.1f" % med(a[3])) if a[3] else "-"))
    print(open(dst).read())


if __name__ == "__main__":
    main()
