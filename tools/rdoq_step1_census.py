"""Census of the four-lane RDOQ walk's blocks at the bench's settled state (run on the GPU):

    python tools/rdoq_step1_census.py                 # CHAIN=600 passes, QP=32
    HIST=0 rocprofv3 --pmc SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_THREAD_CYCLES_VALU \\
        --kernel-include-regex quant_rdo_packed4 --output-format csv -d DIR -o pmc -- \\
        python tools/rdoq_step1_census.py             # counters in a run of their own, no tracing
    python tools/rdoq_step1_census.py --pmc DIR       # ... and their mean over the last fifth of the launches

One picture chain of CHAIN frame passes at 1080p in bench.py's frame cycle (frames 1..8 and back, every
picture coded against the previous reconstruction).  Prints the class-list counts of the last cycle's
passes and, for the exact 16x16 luma and 8x8 chroma blocks of the last pass (a 1080p picture's other
blocks are the 120 16x8 luma blocks of its bottom row and their 8x4 chroma blocks): the candidates (plain
quantised value != 0) per block, the highest sub-block anti-diagonal that holds one, the occupied
(sub-block, anti-diagonal) pairs and the final levels.  XVCGPU_LIB selects another build of the library.
profiles/rdoq_step1_{before,after}.txt were made with it."""
import collections
import csv
import glob
import ctypes as C
import os
import sys

import numpy as np


def pmc_summary(d):
    acc = collections.defaultdict(list)
    for f in sorted(glob.glob(d + "/**/*counter_collection.csv", recursive=True)):
        for row in csv.DictReader(open(f)):
            if "quant_rdo_packed4" in row["Kernel_Name"]:
                acc[row["Counter_Name"]].append(float(row["Counter_Value"]))
    for k in sorted(acc):
        v = acc[k]
        n = max(1, len(v) // 5)
        print("%-24s launches %d  mean of the last %d: %.0f  (min %.0f max %.0f)" %
              (k, len(v), n, sum(v[-n:]) / n, min(v[-n:]), max(v[-n:])))
    if "SQ_INSTS_VALU" in acc and "SQ_THREAD_CYCLES_VALU" in acc:
        n = max(1, len(acc["SQ_INSTS_VALU"]) // 5)
        va = sum(acc["SQ_INSTS_VALU"][-n:]) / n
        tc = sum(acc["SQ_THREAD_CYCLES_VALU"][-n:]) / n
        print("active lanes: %.1f %%" % (100.0 * tc / 64.0 / va))


if len(sys.argv) > 2 and sys.argv[1] == "--pmc":
    pmc_summary(sys.argv[2])
    sys.exit(0)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from xvc_amd import api, pipeline, synth  # noqa: E402

W, H, bd, border = 1920, 1080, 10, 128
CHAIN = int(os.environ.get("CHAIN", 600))
QP = int(os.environ.get("QP", 32))
F = 8
ctx = api.Context(0)
clip = synth.SyntheticClip(W, H, bd)
pad = lambda pl: [np.ascontiguousarray(np.pad(p, border >> (1 if c else 0), mode="edge"))
                  for c, p in enumerate(pl)]
origs = []
for f in range(1, F + 1):
    p = ctx.picture(W, H, bd)
    p.upload(pad(clip.frame(f)), border)
    origs.append(p)
recs = [ctx.picture(W, H, bd), ctx.picture(W, H, bd)]
recs[0].upload(pad(clip.frame(0)), border)
fp = pipeline.FramePass(ctx, W, H, bd, qp=QP, rdoq=True)
cyc = 2 * F - 2
counts_log = []
for j in range(CHAIN):
    k = j % cyc
    fp.run(origs[k if k < F else cyc - k], recs[j % 2], recs[(j + 1) % 2], ref_poc=j)
    if j >= CHAIN - cyc:
        ctx.sync()
        out = (C.c_int32 * 3)()
        ctx._check(ctx.lib.xvcgpu_quant_rdo_class_counts(ctx.h, out))
        counts_log.append(list(out))
ctx.sync()
print("chain of %d passes, 1080p QP %d; class-list counts [<=4 sub-blocks, <=16, general] of the last %d passes:"
      % (CHAIN, QP, cyc))
print("  ", counts_log)
a = np.array(counts_log)
print("   mean per pass: %s of %d blocks" % (a.mean(axis=0).round(1).tolist(), len(fp.desc.tx)))
if os.environ.get("HIST", "1") == "1":
    d = fp.desc
    cf = fp.d_coeffs.to_array(np.int16, fp.n_levels)
    lv = fp.d_levels.to_array(np.int16, fp.n_levels)
    off, _ = ctx.level_offsets(d.tx)
    SCALES = [26214, 23302, 20560, 18396, 16384, 14564]
    for comp, size in ((0, 16), (1, 8), (2, 8)):
        sel = np.flatnonzero((d.tx["comp"] == comp) & (d.tx["w"] == size) & (d.tx["h"] == size))
        nq, nl, lastsb, ndiag = [], [], [], []
        g = size // 4
        for i in sel:
            qp = int(d.tx[i]["qp"]) + 6 * (bd - 8)
            shift = 14 + qp // 6 + (15 - bd - int(np.log2(size)))
            c = np.abs(cf[off[i]:off[i] + size * size].astype(np.int64)).reshape(size, size)
            q = (c * SCALES[qp % 6] + (1 << (shift - 1))) >> shift
            n = int((q != 0).sum())
            nq.append(n)
            nl.append(int((lv[off[i]:off[i] + size * size] != 0).sum()))
            if n:
                sb = (q != 0).reshape(g, 4, g, 4).any(axis=(1, 3))
                sy, sx = np.nonzero(sb)
                lastsb.append(int((sx + sy).max()))
                # occupied anti-diagonals (x + y inside a sub-block) summed over the sub-blocks
                yy, xx = np.nonzero(q)
                ndiag.append(len(set(zip((yy // 4).tolist(), (xx // 4).tolist(), ((yy % 4) + (xx % 4)).tolist()))))
        nq, nl = np.array(nq), np.array(nl)
        has = nq > 0
        print("comp %d %dx%d: %d blocks, %d with a candidate, %d end with a level" %
              (comp, size, size, len(nq), int(has.sum()), int((nl > 0).sum())))
        print("   candidates per block with one: hist[1..16, 17+] %s  mean %.2f p50 %d p90 %d max %d" %
              (np.bincount(np.minimum(nq[has], 17), minlength=18)[1:].tolist(), nq[has].mean(),
               *np.percentile(nq[has], [50, 90]), nq.max()))
        print("   highest sub-block anti-diagonal with a candidate: hist %s" %
              np.bincount(np.array(lastsb), minlength=2 * g - 1).tolist())
        print("   occupied (sub-block, anti-diagonal) pairs per block with a candidate: mean %.2f p50 %d p90 %d" %
              (np.mean(ndiag), *np.percentile(ndiag, [50, 90])))
        print("   levels per coded block: hist[1..12, 13+] %s" %
              np.bincount(np.minimum(nl[nl > 0], 13), minlength=14)[1:].tolist())
