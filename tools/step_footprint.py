#!/usr/bin/env python3
"""What every kernel of the headline step (C2: 10 M x 768 f32 cosine over the int8 copy, top 10, 128 queries) needs of a CU, and whether a block of it
starts on a CU whose other tenant is a block of the resident int8 scan - the question the four batches in flight depend on.

No GPU: the translation units of those kernels are compiled for gfx950 with -Rpass-analysis=kernel-resource-usage (device side only) and the remarks
are parsed: VGPRs (+ AGPRs: one file on CDNA3 / 4), scratch, static LDS.  Threads per block and the dynamic LDS at the headline shape are the
launchers' (file and function named per row; the formulas are repeated here).

A resident scan block (scan_i8copy_kernel_res<1> / _res_dense<1>: 512 threads = 2 waves per SIMD, registers allocated in units of 8, LDS
sp8r_lds_bytes(dim / 128)) leaves on its CU: 163 840 B - its LDS, and 512 - 2 x its allocation registers per SIMD.  A block of w waves per SIMD
(threads / 256, rounded up) at r registers (rounded up to 8) fits when w * r and its LDS are within that - and it has no scratch to speak of.

With --i8-sample-scan 1 (the default, as the option) the sample's bound comes from the int8 copy: scan_i8copy_sample_kernel<NQ> with NQ as
scan_i8copy.hip split_i8_sample_queries picks it, the picks and the sample's bound kernel; 0 lists the f32 pre-scan.

With --fallback-beside-scan 1 (the default, as the option) the conditional exact pass at the end of the step is the one-launch form of
scan_mfma16.hip launch_scan_f32_mfma16_groups where its LDS fits beside the scan's (api_search.hip fallback_groups_fit); 0, and where it does not
fit, lists the 16-query pass and the 64- (32-) query passes.  The closing line says whether every launch of a step without overflow fits.

usage: tools/step_footprint.py [--prescan-beside-scan 0|1] [--i8-sample-scan 0|1] [--fallback-beside-scan 0|1] [--rows N] [--dim D] [--queries Q] [--top K] [--keep DIR]      (prints markdown)"""
import argparse
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
UNITS = ("preprocess", "scan_mfma", "custom_query", "scan_i8copy", "split_select", "scan_dense", "topk_merge", "scan_mfma16")
LDS_PER_CU, REGS_PER_SIMD, REG_UNIT = 163840, 512, 8


def compile_remarks(unit, keep):
    out = os.path.join(keep, unit + ".remarks.txt")
    if not os.path.exists(out):
        cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fvisibility=hidden", "-Wall", "-Wno-unused-function",
               "-Iinclude", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", "qdrant_amd/csrc/%s.hip" % unit, "-o", os.devnull]
        r = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if r.returncode != 0:
            sys.exit("compiling %s failed:\n%s" % (unit, r.stdout[-2000:]))
        with open(out, "w") as f:
            f.write(r.stdout)
    return open(out).read()


def parse(text):
    """mangled kernel name -> {vgprs, agprs, scratch, lds}"""
    kernels, cur = {}, None
    for line in text.splitlines():
        m = re.search(r"remark: \s*(.*?)\s*\[-Rpass-analysis=kernel-resource-usage\]", line)
        if not m:
            continue
        t = m.group(1)
        if t.startswith("Function Name:"):
            cur = kernels.setdefault(t.split(":", 1)[1].strip(), {})
            continue
        for key, pat in (("vgprs", r"^VGPRs: (\d+)"), ("agprs", r"^AGPRs: (\d+)"), ("scratch", r"^ScratchSize \[bytes/lane\]: (\d+)"),
                         ("lds", r"^LDS Size \[bytes/block\]: (\d+)")):
            mm = re.match(pat, t)
            if mm and cur is not None:
                cur[key] = int(mm.group(1))
    return kernels


def targs(*vals):
    """Itanium mangling of integer / bool template arguments, as they stand in the kernel's symbol"""
    return "I" + "".join("Lb%dE" % v if isinstance(v, bool) else "Li%dE" % v for v in vals) + "E"


def lds_tile_stride(b):          # api_internal.hpp
    return b + (16 + 256 - b % 256) % 256


def step_kernels(a):
    """(what, kernel label, regex on the mangled name, threads, dynamic LDS, where the launch is)"""
    dim, nq, top = a.dim, a.queries, a.top
    nseg = dim * 4 // 128
    S = min(a.rows, max(a.rows >> 11, 8192))                       # api_search.hip prefilter_begin / split_begin (prescan_shift 10, + 1 over a derived copy)
    q_stride = lds_tile_stride(dim * 4 + 64)                         # query entry: the row + the 64-byte aux block
    fast = nseg % 12 == 0
    rows = [
        ("preprocess", "cosine_preprocess_lds_kernel", r"cosine_preprocess_lds_kernelE", 256, dim * 16, "preprocess.hip launch_cosine_preprocess_f32"),
        ("pack", "pack_queries_kernel", r"pack_queries_kernelE", 64, 0, "preprocess.hip launch_pack_queries"),
    ]
    res_lds = (dim // 128) * (128 * 2 * 4) * 16 + 2 * 128 * 4        # scan_i8copy.hip sp8r_lds_bytes
    if a.i8_sample_scan:
        S = S // 16 * 16
        nch = dim // 128                                               # scan_i8copy.hip split_i8_sample_queries
        group = 16
        for c in (32, 64):
            if nch <= 8 and nch * (c // 16) * 2048 <= LDS_PER_CU - res_lds and c // 2 < nq:
                group = c
        rows += [
            ("sp_i8_pack", "sp_i8_pack_kernel", r"sp_i8_pack_kernelE", 256, dim * 4, "scan_i8copy.hip launch_split_i8_pack"),
            ("sample scan", "scan_i8copy_sample_kernel<%d>" % group, r"scan_i8copy_sample_kernel" + targs(group), 256, nch * (group // 16) * 2048,
             "scan_i8copy.hip launch_scan_i8copy_sample"),
        ]
    elif a.prescan_beside_scan and S <= 16384 and nq >= 16:
        d = 6
        rows.append(("pre-scan", "scan_f32_mfma_kernel<16,1,%d,nt,4 waves,%s,ids,scores>" % (d, "fast" if fast else "generic"),
                     r"scan_f32_mfma_kernel" + targs(16, 1, d, True, 4, fast, False, True, 1), 256, (16 * q_stride + 256 + 15) & ~15,
                     "scan_mfma.hip launch_scan_f32_mfma_beside"))
    else:
        d = 6 if fast else 12
        rows.append(("pre-scan", "scan_f32_mfma_kernel<16,2,%d,nt,8 waves,%s,ids,scores>" % (d, "fast" if fast else "generic"),
                     r"scan_f32_mfma_kernel" + targs(16, 2, d, True, 8, fast, False, True, 1), 512, (32 * q_stride + 256 + 15) & ~15,
                     "scan_mfma.hip launch_scan_f32_mfma"))
    if a.prescan_beside_scan and S <= 16384 and top <= 64:
        rows.append(("top-k", "custom_topk_beside_kernel<%d>" % (32 if S <= 8192 else 64), r"custom_topk_beside_kernel" + targs(32 if S <= 8192 else 64), 256, 0,
                     "custom_query.hip launch_custom_topk"))
    else:
        rows.append(("top-k", "custom_topk_small_kernel", r"custom_topk_small_kernelE", 1024, S * 8, "custom_query.hip launch_custom_topk"))
    if a.i8_sample_scan:
        rows += [
            ("sample picks", "sp_i8_picks_kernel", r"sp_i8_picks_kernelE", 64, 0, "scan_i8copy.hip launch_split_i8_picks"),
            ("sample bound", "sp_i8_sample_bound_kernel", r"sp_i8_sample_bound_kernelE", 64, 0, "scan_i8copy.hip launch_split_i8_sample_bound"),
        ]
    # scan_mfma16.hip M16Shape::LDS (ring stages of 16 rows x 1 KiB at pitch 1040; the half stages of odd row lengths come to the same)
    m16 = lambda nw, nt, ring=0: (ring or (4 if nw == 4 else 7)) * 16 * 1040 + nw * nt * 4 * 64 * 4 + 16 * 16 * 4
    ks = dim // 128
    fqt = 64 if ks <= 6 else 32                                        # api_internal.hpp split_fallback_qt
    # option fallback_beside_scan: the one-launch form where a block of it fits beside the scan (api_search.hip fallback_groups_fit decides from the
    # kernels' attributes; here: the LDS, which is what rules it out at 1 024 coordinates - the table's last column shows the registers)
    groups = a.fallback_beside_scan and m16(4, 1, 3) + res_lds <= LDS_PER_CU
    if not a.i8_sample_scan:
        rows.append(("sp_i8_pack", "sp_i8_pack_kernel", r"sp_i8_pack_kernelE", 256, dim * 4, "scan_i8copy.hip launch_split_i8_pack"))
    rows += [
        ("first scan", "scan_i8copy_kernel_res_dense<1>", r"scan_i8copy_kernel_res_denseILi1EE", 512, res_lds, "scan_i8copy.hip launch_scan_i8copy"),
        ("second scan", "scan_i8copy_kernel_res<1>", r"scan_i8copy_kernel_resILi1EE", 512, res_lds, "scan_i8copy.hip launch_scan_i8copy"),
        ("regroup", "sp_regroup_kernel", r"sp_regroup_kernelE", 256, 0, "split_select.hip launch_split_regroup"),
        ("probe", "sp_i8_probe_kernel", r"sp_i8_probe_kernelE", 512, 0, "split_select.hip launch_split_i8_probe"),
        ("pair kernel", "pair_kernel<RowF32<dot>>", r"pair_kernelINS_6RowF32ILi0EEEE", 256, 0, "scan_common.hpp launch_pairs"),
        ("bound", "sp_i8_bound_kernel", r"sp_i8_bound_kernelE", 64, 0, "scan_i8copy.hip launch_split_i8_bound"),
        ("select", "sp_select_kernel", r"sp_select_kernelE", 512, 0, "split_select.hip launch_split_select"),
        ("sort", "sort_scored_kernel", r"sort_scored_kernelE", 256, 0, "topk_merge.hip launch_sort_scored"),
        ("plan", "sp_plan_kernel", r"sp_plan_kernelE", 256, 0, "split_select.hip launch_split_plan"),
    ]
    if groups:
        rows += [
            ("fallback scan, block rows of 16 queries (conditional)", "scan_f32_mfma16_kernel<%d,4 waves,1 tile,ring 3,groups>" % ks,
             r"scan_f32_mfma16_kernel" + targs(ks, 4, 1, 0, False, False, 3, True, False), 256, m16(4, 1, 3), "scan_mfma16.hip launch_scan_f32_mfma16_groups"),
            ("fallback merge (conditional)", "merge_keys_kernel", r"merge_keys_kernelE", 256, 0, "topk_merge.hip launch_merge_keys"),
        ]
    else:
        nw, nt = (8, 4) if fqt == 64 else (8, 2)                       # scan_mfma16.hip launch_scan_f32_mfma16: 64 queries, or 32 at more than 6 K-steps
        rows += [
            ("fallback scan, 16 queries (conditional)", "scan_f32_mfma16_kernel<%d,4 waves,1 tile>" % ks,
             r"scan_f32_mfma16_kernel" + targs(ks, 4, 1, 0, False, False, 0, False, False), 256, m16(4, 1), "scan_mfma16.hip launch_m16"),
            ("fallback scans, %d queries (conditional, %d)" % (fqt, (nq + fqt - 1) // fqt), "scan_f32_mfma16_kernel<%d,%d waves,%d tiles>" % (ks, nw, nt),
             r"scan_f32_mfma16_kernel" + targs(ks, nw, nt, 0, (nw, nt, ks) == (8, 4, 6), False, 0, False, False), 512, m16(nw, nt), "scan_mfma16.hip launch_m16"),
            ("fallback merges (conditional)", "merge_keys_kernel", r"merge_keys_kernelE", 256, 0, "topk_merge.hip launch_merge_keys"),
        ]
    return rows, S


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--prescan-beside-scan", type=int, default=1)
    ap.add_argument("--i8-sample-scan", type=int, default=1)
    ap.add_argument("--fallback-beside-scan", type=int, default=1)
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--queries", type=int, default=128)
    ap.add_argument("--top", type=int, default=10)
    ap.add_argument("--keep", default=None, help="directory for the compiler's remarks (kept and reused)")
    a = ap.parse_args()
    keep = a.keep or tempfile.mkdtemp(prefix="step_footprint_")
    os.makedirs(keep, exist_ok=True)
    with ThreadPoolExecutor(max_workers=min(len(UNITS), os.cpu_count() or 1, 8)) as ex:
        texts = list(ex.map(lambda u: compile_remarks(u, keep), UNITS))
    kernels = {}
    for t in texts:
        kernels.update(parse(t))
    rows, S = step_kernels(a)

    def find(pattern, optional=False):
        hits = [(k, v) for k, v in kernels.items() if re.search(r"^_ZN3qmx\d+(?:%s)" % pattern, k)]
        if not hits and optional:      # (a conditional fallback scan whose shape is not instantiated at this row length)
            return None
        if len(hits) != 1:
            sys.exit("kernel pattern %r matches %d symbols: %s" % (pattern, len(hits), [k for k, _ in hits][:6]))
        return hits[0][1]

    up = lambda v, u: (v + u - 1) // u * u
    scans = [find(r[2]) for r in rows if r[0] in ("first scan", "second scan")]
    scan_lds = max(s["lds"] for s in scans) + [r[4] for r in rows if r[0] == "second scan"][0]
    scan_regs = 2 * max(up(s["vgprs"] + s["agprs"], REG_UNIT) for s in scans)
    free_lds, free_regs = LDS_PER_CU - scan_lds, REGS_PER_SIMD - scan_regs
    print("# Footprint of the headline step's kernels (prescan_beside_scan = %d, i8_sample_scan = %d, fallback_beside_scan = %d)\n"
          % (a.prescan_beside_scan, a.i8_sample_scan, a.fallback_beside_scan))
    print("%d rows x %d f32, %d queries, top %d; sample of %d rows.  Compiler remarks of gfx950 code (`tools/step_footprint.py`), no GPU involved.\n"
          % (a.rows, a.dim, a.queries, a.top, S))
    print("A resident scan block takes %d B of LDS and %d registers per SIMD (2 waves): beside it a CU has **%d B of LDS and %d registers per SIMD** left.\n"
          % (scan_lds, scan_regs, free_lds, free_regs))
    print("| step | kernel | threads | VGPRs (+AGPRs) | static LDS | dynamic LDS | scratch | fits beside a resident scan |")
    print("|---|---|---:|---:|---:|---:|---:|---|")
    misfits = []
    for what, label, pattern, threads, dyn, where in rows:
        k = find(pattern, optional="conditional" in what)
        if k is None:
            print("| %s | `%s` (%s) | %d | - | - | %d | - | (no such instantiation in the build) |" % (what, label, where, threads, dyn))
            continue
        regs = k["vgprs"] + k["agprs"]
        need_regs = (threads + 255) // 256 * up(regs, REG_UNIT)
        why = []
        if k["lds"] + dyn > free_lds:
            why.append("LDS %d B" % (k["lds"] + dyn))
        if need_regs > free_regs:
            why.append("registers %d per SIMD" % need_regs)
        if k["scratch"]:
            why.append("scratch")
        fits = "yes" if not why else "no (%s)" % ", ".join(why)
        if what in ("first scan", "second scan"):
            fits = "(the scan)"
        elif why:
            misfits.append(what)
        print("| %s | `%s` (%s) | %d | %d | %d | %d | %d | %s |" % (what, label, where, threads, regs, k["lds"], dyn, k["scratch"], fits))
    # (the conditional launches are part of every step: they are enqueued whether or not a query overflowed)
    if misfits:
        print("\n**%d coordinates: NOT every launch of a step without overflow fits beside a resident scan block** - these wait for a CU without one: %s."
              % (a.dim, "; ".join(misfits)))
    else:
        print("\n**%d coordinates: every launch of a step without overflow fits beside a resident scan block.**" % a.dim)


if __name__ == "__main__":
    main()
