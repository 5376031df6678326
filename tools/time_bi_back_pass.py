#!/usr/bin/env python3
"""Times the frame pass of a B picture with only back references
(pipeline.BiRefsFramePass(low_delay=True), xvcgpu_frame_pass_bi_back) at 1080p, 10 bit, QP
32, form residual_rdoq, on the 16-sample grid: the low-delay default (L0 {16, 12}, L1 {16,
12} at POC 20) per pass and per launch - the predictor-cost kernel and the two folds alone
among them - beside the two-directional pass (xvcgpu_frame_pass_bi_refs) on a set with the
same picture counts (L0 {16, 24}, L1 {24, 16}: both list-1 pictures re-used), in the same run.

    python tools/time_bi_back_pass.py [--out profiles/bi_back_frame_pass_time.txt]
                                      [--repeats 30] [--warmup 5] [--inner 8]

What to compare against: both passes run two list-0 searches and no list-1 search, and two
refinement jobs per CU; the low-delay pass adds one predictor-cost launch over 2 x 8160 jobs.
Device events around `inner` back-to-back calls, divided by inner; `warmup` untimed rounds,
then `repeats` timed ones, the two passes taking turns round by round: median and
inter-quartile range, in microseconds.  A launch is timed alone, after the launches before it
ran once untimed.  There is no target.  profiles/bi_back_frame_pass_time.txt holds a run of
this tool and, behind it, the paired bench.py runs of DESIGN section 12: give --out another
name to keep that record."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from time_bi_refs_pass import per_launch, timed    # noqa: E402

CUR_POC = 20
LOW_DELAY = ((16, 12), (16, 12))
TWO_WAY = ((16, 24), (24, 16))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles",
                                                  "bi_back_frame_pass_time.txt"))
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--inner", type=int, default=8)
    a = ap.parse_args()
    from xvc_amd import api, pipeline, synth
    w, h, bd, qp = 1920, 1080, 10, 32
    ctx = api.Context(0)
    clip = synth.SyntheticClip(w, h, bd)
    O, Rec = ctx.picture(w, h, bd), ctx.picture(w, h, bd)
    by_poc = {}
    for k, poc in enumerate((12, 16, 20, 24)):     # four frames of the clip, POC 20 coded
        pic = O if poc == CUR_POC else ctx.picture(w, h, bd)
        pic.upload([np.ascontiguousarray(np.pad(p, 128 if c == 0 else 64, mode="edge"))
                    for c, p in enumerate(clip.frame(k))], 128)
        if poc != CUR_POC:
            by_poc[poc] = pic
    passes = []
    for lists, low_delay in ((LOW_DELAY, True), (TWO_WAY, False)):
        fr = pipeline.BiRefsFramePass(ctx, w, h, bd, qp, rdoq=True, rdoq_packed=False,
                                      cur_poc=CUR_POC, ref_pocs=lists, low_delay=low_delay)
        passes.append((fr, lists, [[by_poc[p] for p in lists[l]] for l in range(2)]))
    lines = ["B frame pass with only back references, %dx%d, %d bit, QP %d, form %s"
             % (w, h, bd, qp, passes[0][0].form),
             "device events, inner %d, warm-up %d, repeats %d: median (IQR) in us"
             % (a.inner, a.warmup, a.repeats), ""]
    meds = timed(ctx, [(lambda fr=fr, refs=refs: fr.run(O, refs, Rec)) for fr, _, refs in passes],
                 a)
    ctx.sync()
    for (fr, lists, refs), (med, iqr) in zip(passes, meds):
        choice = fr.results()[4]
        dirs = np.bincount(choice["inter_dir"], minlength=3)
        entry = "xvcgpu_frame_pass_bi_back" if fr.low_delay else "xvcgpu_frame_pass_bi_refs"
        lines += ["%s: L0 %s, L1 %s at POC %d, %d CUs (L0 / L1 / bi chosen: %d / %d / %d)"
                  % ("low delay" if fr.low_delay else "two directions", list(lists[0]),
                     list(lists[1]), CUR_POC, fr.desc.n_cus, dirs[0], dirs[1], dirs[2]),
                  "  %s, one call  fused tail %-5s %9.1f (%.1f)"
                  % (entry, bool(fr.p.fused_tail), med, iqr)]
        rows = per_launch(ctx, lambda fr=fr, refs=refs: fr.kernel_steps(O, refs, Rec), a)
        lines.append("  per launch (sum %.1f)" % sum(r[1] for r in rows))
        lines += ["    %-18s %9.1f (%.1f)" % r for r in rows]
        lines.append("")
    lines.append("low delay - two directions, one call: %+.1f us"
                 % (meds[0][0] - meds[1][0]))
    for fr, _, _ in passes:
        fr.destroy()
    for p in [O, Rec] + list(by_poc.values()):
        p.destroy()
    ctx.close()
    text = "\n".join(lines).rstrip("\n")
    print(text)
    with open(a.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
