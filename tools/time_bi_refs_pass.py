#!/usr/bin/env python3
"""Times the frame pass of a B picture (pipeline.BiRefsFramePass,
xvcgpu_frame_pass_bi_refs) at 1080p, 10 bit, QP 32, packed RDOQ - on the 16-sample grid and
on one real partition (`c1` picture 1) - for the picture sets D (L0 {4}, L1 {12}), B (L0
{4, 12}, L1 {12, 4}) and A (L0 {4, 0}, L1 {12, 16}) around POC 8, per pass and per launch.
profiles/bi_refs_frame_pass_time.txt is a run of an earlier version, which also timed the
retired one-reference pass beside set D: give --out another name to keep that record.

    python tools/time_bi_refs_pass.py [--out profiles/bi_refs_frame_pass_time.txt]
                                      [--repeats 30] [--warmup 5] [--inner 8]

On the partition the planned refinement is timed against the whole-list launches per class.
Device events around `inner` back-to-back calls, divided by inner; `warmup` untimed rounds,
then `repeats` timed ones: median and inter-quartile range, in microseconds.  A launch is
timed alone, after the launches before it ran once untimed.  There is no target."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CUR_POC = 8
SETS = (("D", ((4,), (12,))), ("B", ((4, 12), (12, 4))), ("A", ((4, 0), (12, 16))))


def stats(us):
    q1, med, q3 = np.percentile(np.asarray(us, float), [25, 50, 75])
    return float(med), float(q3 - q1)


def timed_round(ctx, fn, inner):
    ctx.timer_begin()
    for _ in range(inner):
        fn()
    return ctx.timer_end() * 1000.0 / inner


def timed(ctx, fns, a):
    """Median and IQR per callable of fns, the callables taking turns round by round."""
    for _ in range(a.warmup):
        for fn in fns:
            for _ in range(a.inner):
                fn()
    ctx.sync()
    out = [[] for _ in fns]
    for _ in range(a.repeats):
        for k, fn in enumerate(fns):
            out[k].append(timed_round(ctx, fn, a.inner))
    return [stats(o) for o in out]


def per_launch(ctx, steps_of, a):
    """(name, median, iqr) per launch of steps_of() (a fresh list of (name, callable))."""
    rows = []
    for k, (name, _) in enumerate(steps_of()):
        for _, fn in steps_of()[:k]:
            fn()
        (med, iqr), = timed(ctx, [steps_of()[k][1]], a)
        rows.append((name, med, iqr))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles",
                                                  "bi_refs_frame_pass_time.txt"))
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--inner", type=int, default=8)
    a = ap.parse_args()
    from partition_fixture import luma_partition
    from xvc_amd import api, pipeline, synth
    w, h, bd, qp = 1920, 1080, 10, 32
    ctx = api.Context(0)
    clip = synth.SyntheticClip(w, h, bd)
    O, Rec = ctx.picture(w, h, bd), ctx.picture(w, h, bd)
    by_poc = {}
    for k, poc in enumerate((0, 4, 8, 12, 16)):     # five frames of the clip, POC 8 coded
        pic = O if poc == CUR_POC else ctx.picture(w, h, bd)
        pic.upload([np.ascontiguousarray(np.pad(p, 128 if c == 0 else 64, mode="edge"))
                    for c, p in enumerate(clip.frame(k))], 128)
        if poc != CUR_POC:
            by_poc[poc] = pic
    lines = ["B frame pass, %dx%d, %d bit, QP %d, packed RDOQ" % (w, h, bd, qp),
             "device events, inner %d, warm-up %d, repeats %d: median (IQR) in us"
             % (a.inner, a.warmup, a.repeats), ""]
    for name, parts in (("grid 16x16", None), ("partition c1 picture 1", luma_partition("c1", 1))):
        for which, lists in SETS:
            refs = [[by_poc[p] for p in lists[l]] for l in range(2)]
            fr = pipeline.BiRefsFramePass(ctx, w, h, bd, qp, rdoq=True, partition=parts,
                                          cur_poc=CUR_POC, ref_pocs=lists)
            meds = timed(ctx, [lambda: fr.run(O, refs, Rec)], a)
            ctx.sync()
            choice = fr.results()[4]
            dirs = np.bincount(choice["inter_dir"], minlength=3)
            lines += ["%s, set %s (L0 %s, L1 %s): %d CUs (L0 / L1 / bi chosen: %d / %d / %d; "
                      "ref_idx > 0 in L0 / L1: %d / %d)"
                      % (name, which, list(lists[0]), list(lists[1]), fr.desc.n_cus, dirs[0],
                         dirs[1], dirs[2], (choice["ref_idx"][:, 0] > 0).sum(),
                         (choice["ref_idx"][:, 1] > 0).sum()),
                      "  xvcgpu_frame_pass_bi_refs, one call  form %-14s fused tail %-5s "
                      "%9.1f (%.1f)" % (fr.form, bool(fr.p.fused_tail), meds[0][0], meds[0][1])]
            rows = per_launch(ctx, lambda: fr.kernel_steps(O, refs, Rec), a)
            lines.append("  per launch (sum %.1f)" % sum(r[1] for r in rows))
            lines += ["    %-18s %9.1f (%.1f)" % r for r in rows]
            if parts is not None:
                rows = [r for r in per_launch(
                    ctx, lambda: fr.kernel_steps(O, refs, Rec, planned=False), a)
                    if r[0].startswith("bipred_c")]
                lines.append("  the refinement as whole-list launches per class (sum %.1f)"
                             % sum(r[1] for r in rows))
                lines += ["    %-18s %9.1f (%.1f)" % r for r in rows]
            lines.append("")
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
