#!/usr/bin/env python3
"""How much of a search step runs beside an int8 prefilter scan, from a kernel trace (`rocprofv3 --kernel-trace --output-format csv`) of
`bench.py --gpus 1`: with four batches in flight every small kernel of one batch is meant to run while another batch's scan holds the CUs.

Prints, over the middle half of the trace's second-launch scans (the timed region without its ends):
  * the time per step in which NO scan_i8copy_kernel_res* dispatch is open (the union of the scans' intervals taken out of the window);
  * per sample pre-scan (scan_f32_mfma_kernel), sample scan over the int8 copy (scan_i8copy_sample_kernel, option i8_sample_scan) and sample top-k (custom_topk_*) dispatch: whether its interval lies inside one scan's, overlaps one
    partly, or meets none, and its mean duration (the trace has start and end times only: how long a dispatch waited for a CU is not in it);
  * the mean duration of the first and second scan launches.
usage: tools/scan_overlap.py <kernel_trace.csv>"""
import csv
import sys


def main():
    scans, small = [], {"pre-scan": [], "sample scan": [], "top-k": []}
    for r in csv.DictReader(open(sys.argv[1])):
        name, t0, t1 = r["Kernel_Name"], int(r["Start_Timestamp"]), int(r["End_Timestamp"])
        if "scan_i8copy_kernel" in name:
            scans.append((t0, t1, "res_dense" in name))
        elif "scan_f32_mfma_kernel" in name:
            small["pre-scan"].append((t0, t1, name))
        elif "scan_i8copy_sample_kernel" in name:
            small["sample scan"].append((t0, t1, name))
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
    return 0


if __name__ == "__main__":
    sys.exit(main())
