#!/usr/bin/env python3
"""How much of a search step runs beside an int8 prefilter scan, from a kernel trace (`rocprofv3 --kernel-trace --output-format csv`) of
`bench.py --gpus 1`: with four batches in flight every small kernel of one batch is meant to run while another batch's scan holds the CUs.

Prints, over the middle half of the trace's second-launch scans (the timed region without its ends):
  * the time per step in which NO scan_i8copy_kernel_res* dispatch is open (the union of the scans' intervals taken out of the window);
  * per sample pre-scan (scan_f32_mfma_kernel), sample scan over the int8 copy (scan_i8copy_sample_kernel, option i8_sample_scan) and sample top-k (custom_topk_*) dispatch: whether its interval lies inside one scan's, overlaps one
    partly, or meets none, and its mean duration (the trace has start and end times only: how long a dispatch waited for a CU is not in it);
  * the mean duration of the first and second scan launches;
  * the conditional exact passes at the end of a search (scan_f32_mfma16_kernel, merge_keys_kernel; option fallback_beside_scan): per kernel the
    interval from dispatch to end - a dispatch's interval opens when its packet is taken up, so a block that waits for room on a CU shows as a long
    interval of a kernel that does nothing - and how many of those intervals end within END_SLACK_US after the end of a scan: a dispatch that
    waited for a hand-over between two scans;
  * per lane (the trace's stream, or queue where it has no stream column): the time between the end of the lane's second scan launch and the
    dispatch of the first kernel of the lane's next step (the first dispatch behind the step's last tail kernel), and what share of it the
    conditional passes' intervals cover.
usage: tools/scan_overlap.py <kernel_trace.csv>"""
import bisect
import csv
import sys

END_SLACK_US = 5.0
LONG_US = 100.0      # a conditional pass that does nothing ends within microseconds of getting a CU: a longer interval is a wait
# what follows the second scan launch in a step's chain; the next step starts with the first dispatch of the lane that is none of these
TAIL = ("sp_regroup_kernel", "sp_i8_probe_kernel", "pair_kernel", "sp_i8_bound_kernel", "sp_select_kernel", "sort_scored_kernel", "sp_plan_kernel",
        "scan_f32_mfma16_kernel", "merge_keys_kernel")


def lane_key(rows):
    """the column that tells the batches in flight apart: the stream where the trace has one with several values, else the queue"""
    for col in ("Stream_Id", "Queue_Id"):
        if rows and col in rows[0] and len({r[col] for r in rows}) > 1:
            return col
    return None


def stats_us(xs):
    xs = sorted(xs)
    if not xs:
        return "none"
    return "mean %.1f us, median %.1f, min %.1f, max %.1f" % (sum(xs) / len(xs) / 1e3, xs[len(xs) // 2] / 1e3, xs[0] / 1e3, xs[-1] / 1e3)


def fallback_report(rows, scans, second, w0, w1, steps):
    scan_ends = sorted(b for _, b in scans)
    slack = int(END_SLACK_US * 1000)
    for what in ("scan_f32_mfma16_kernel", "merge_keys_kernel"):
        items = [(int(r["Start_Timestamp"]), int(r["End_Timestamp"])) for r in rows if what in r["Kernel_Name"]]
        items = [x for x in items if x[0] >= w0 and x[1] <= w1]
        at_end = 0
        for _, t1 in items:
            i = bisect.bisect_right(scan_ends, t1) - 1          # the last scan end at or before this dispatch's end
            if i >= 0 and t1 - scan_ends[i] <= slack:
                at_end += 1
        durs = [t1 - t0 for t0, t1 in items]
        long_ones = sum(1 for d in durs if d > LONG_US * 1000)
        print("%s: %d dispatches (%.1f per step), dispatch to end %s; %d longer than %.0f us (%.2f per step); %d (%.0f %%) end within %.0f us after a "
              "scan's end; %.4f ms per step in all"
              % (what, len(items), len(items) / steps, stats_us(durs), long_ones, LONG_US, long_ones / steps, at_end, 100.0 * at_end / max(len(items), 1),
                 END_SLACK_US, sum(durs) / steps / 1e6))
    col = lane_key(rows)
    if col is None:
        print("lane wait: the trace tells no lanes apart (one stream, one queue)")
        return
    lanes = {}
    for r in rows:
        lanes.setdefault(r[col], []).append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    second_set = set(second)
    waits, cond_share = [], []
    for items in lanes.values():
        items.sort()
        for i, (t0, t1, name) in enumerate(items):
            if (t0, t1) not in second_set or "scan_i8copy_kernel" not in name or t0 < w0 or t1 > w1:
                continue
            cond = 0
            for u0, u1, nm in items[i + 1:]:
                if not any(k in nm for k in TAIL):
                    waits.append(u0 - t1)
                    cond_share.append(cond)
                    break
                if "scan_f32_mfma16_kernel" in nm or "merge_keys_kernel" in nm:
                    cond += u1 - u0
    print("lane wait (%s, %d lanes): from the end of a lane's second scan launch to the dispatch of its next step's first kernel: %d steps, %s; "
          "of it inside the conditional passes' intervals: %s"
          % (col, len(lanes), len(waits), stats_us(waits), stats_us(cond_share)))


def main():
    scans, small = [], {"pre-scan": [], "sample scan": [], "top-k": []}
    rows = list(csv.DictReader(open(sys.argv[1])))
    for r in rows:
        name, t0, t1 = r["Kernel_Name"], int(r["Start_Timestamp"]), int(r["End_Timestamp"])
        if "scan_i8copy_sample_kernel" in name:
            small["sample scan"].append((t0, t1, name))
        elif "scan_i8copy_kernel" in name:
            scans.append((t0, t1, "res_dense" in name))
        elif "scan_f32_mfma_kernel" in name:
            small["pre-scan"].append((t0, t1, name))
        elif "custom_topk_" in name:
            small["top-k"].append((t0, t1, name))
    # which launch: the first one has a kernel of its own (option i8_dense_epilogue); without it the strided sixteenth is the one under 0.3 ms
    by_name = any(d for _, _, d in scans)
    is_first = lambda s: s[2] if by_name else s[1] - s[0] < 300_000
    second = sorted(s[:2] for s in scans if not is_first(s))
    firsts = [s[:2] for s in scans if is_first(s)]
    scans = [s[:2] for s in scans]
    if len(second) < 8:
        print("fewer than 8 second-launch scans in", sys.argv[1])
        return 1
    lo, hi = second[len(second) // 4], second[(3 * len(second)) // 4]
    w0, w1 = lo[0], hi[0]                                             # from the start of one second launch to the start of a later one: whole steps
    steps = (3 * len(second)) // 4 - len(second) // 4
    inside = sorted((max(a, w0), min(b, w1)) for a, b in scans if b > w0 and a < w1)
    covered, end = 0, w0
    for a, b in inside:                                               # the union of the scans' intervals inside the window
        if b > end:
            covered += b - max(a, end)
            end = b
    print("window: %d steps, %.3f ms per step; no scan open for %.4f ms per step (%.2f %%)"
          % (steps, (w1 - w0) / steps / 1e6, (w1 - w0 - covered) / steps / 1e6, 100.0 * (w1 - w0 - covered) / (w1 - w0)))
    first = [b - a for a, b in firsts if a >= w0 and b <= w1]
    sec = [b - a for a, b in second if a >= w0 and b <= w1]
    print("first scan launch : %d dispatches, mean %.4f ms" % (len(first), sum(first) / max(len(first), 1) / 1e6))
    print("second scan launch: %d dispatches, mean %.4f ms" % (len(sec), sum(sec) / max(len(sec), 1) / 1e6))
    for what, items in small.items():
        items = [x for x in items if x[0] >= w0 and x[1] <= w1]
        full = part = none = 0
        beside_ns = 0
        for t0, t1, _ in items:
            ov = 0
            whole = False
            for a, b in scans:
                if a <= t0 and t1 <= b:
                    whole = True
                ov = max(ov, min(b, t1) - max(a, t0))
            if whole:
                full += 1
            elif ov > 0:
                part += 1
            else:
                none += 1
            beside_ns += max(ov, 0)
        durs = [t1 - t0 for t0, t1, _ in items]
        names = sorted({n.split("(")[0] for _, _, n in items})
        print("%s: %d dispatches (%d per step), mean %.1f us (min %.1f max %.1f); inside one scan's interval %d, partly %d, beside none %d; "
              "%.0f %% of their time beside a scan\n    %s"
              % (what, len(items), round(len(items) / steps), sum(durs) / max(len(durs), 1) / 1e3, min(durs, default=0) / 1e3, max(durs, default=0) / 1e3,
                 full, part, none, 100.0 * beside_ns / max(sum(durs), 1), "; ".join(names)))
    fallback_report(rows, scans, second, w0, w1, steps)
    return 0


if __name__ == "__main__":
    sys.exit(main())
