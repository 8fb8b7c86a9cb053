#!/usr/bin/env python3
"""The two launches of the int8 prefilter scan in a kernel trace (`rocprofv3 --kernel-trace --output-format csv`): mean duration of the first-launch
dispatches (the strided sixteenth: under 0.3 ms) and of the second-launch ones, and the first launch's time over its stream time - its bytes at the
rate the second launch reaches in the same trace.   usage: tools/i8_launch_split.py <kernel_trace.csv> [rows dim stride]"""
import csv
import sys


def main():
    path = sys.argv[1]
    n, dim, stride = (int(x) for x in sys.argv[2:5]) if len(sys.argv) >= 5 else (10_000_000, 768, 16)
    tiles = (n + 255) // 256
    first_tiles = (tiles + stride - 1) // stride
    first_bytes, second_bytes = first_tiles * 256 * dim, (tiles - first_tiles) * 256 * dim
    first, second, names = [], [], set()
    for r in csv.DictReader(open(path)):
        if "scan_i8copy_kernel" not in r["Kernel_Name"]:
            continue
        ms = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6
        (first if ms < 0.3 else second).append(ms)
        names.add(r["Kernel_Name"].split("(")[0] + (" [first]" if ms < 0.3 else " [second]"))
    if not first or not second:
        print("no int8 scan launches of both kinds in", path)
        return 1
    m1, m2 = sum(first) / len(first), sum(second) / len(second)
    med1, med2 = sorted(first)[len(first) // 2], sorted(second)[len(second) // 2]
    rate = second_bytes / (m2 * 1e-3)
    stream_ms = first_bytes / rate * 1e3
    print("kernels: %s" % "; ".join(sorted(names)))
    print("first launch : %4d dispatches, mean %.4f ms (median %.4f min %.4f max %.4f), %.3f GB" % (len(first), m1, med1, min(first), max(first), first_bytes / 1e9))
    print("second launch: %4d dispatches, mean %.4f ms (median %.4f min %.4f max %.4f), %.3f GB, %.2f TB/s" % (len(second), m2, med2, min(second), max(second), second_bytes / 1e9, rate / 1e12))
    print("first launch over its stream time (%.4f ms at the second launch's rate): %.2f  (by the medians: %.2f)"
          % (stream_ms, m1 / stream_ms, med1 / (first_bytes / (second_bytes / med2))))
    return 0


if __name__ == "__main__":
    sys.exit(main())
