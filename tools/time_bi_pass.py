#!/usr/bin/env python3
"""Times the frame pass of a B picture (pipeline.BiFramePass, xvcgpu_frame_pass_bi) at
1080p, 10 bit, QP 32, packed RDOQ - on the 16-sample grid and on one real partition (`c1`
picture 1) - per pass and per launch, with the P pass of the same CUs beside it, measured
in the same process in alternating rounds (profiles/bi_frame_pass_time.txt is a run of it).

    python tools/time_bi_pass.py [--out profiles/bi_frame_pass_time.txt]
                                 [--repeats 30] [--warmup 5] [--inner 8]

Device events around `inner` back-to-back calls, divided by inner; `warmup` untimed
rounds, then `repeats` timed ones: median and inter-quartile range, in microseconds.  A
launch is timed alone, after the launches before it ran once untimed (it needs their
results).  There is no target: this is where the pass's first measured numbers live."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bi_frame_pass_time.txt"))
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--inner", type=int, default=8)
    a = ap.parse_args()
    from partition_fixture import luma_partition
    from xvc_amd import api, pipeline, synth
    w, h, bd, qp = 1920, 1080, 10, 32
    ctx = api.Context(0)
    clip = synth.SyntheticClip(w, h, bd)
    R0, O, R1, Rec = (ctx.picture(w, h, bd) for _ in range(4))
    for k, pic in enumerate((R0, O, R1)):       # the original between its two references
        pic.upload([np.ascontiguousarray(np.pad(p, 128 if c == 0 else 64, mode="edge"))
                    for c, p in enumerate(clip.frame(k))], 128)
    lines = ["B frame pass beside the P pass, %dx%d, %d bit, QP %d, packed RDOQ" % (w, h, bd, qp),
             "device events, inner %d, warm-up %d, repeats %d: median (IQR) in us"
             % (a.inner, a.warmup, a.repeats), ""]
    for name, parts in (("grid 16x16", None), ("partition c1 picture 1", luma_partition("c1", 1))):
        fb = pipeline.BiFramePass(ctx, w, h, bd, qp, rdoq=True, partition=parts)
        fp = pipeline.FramePass(ctx, w, h, bd, qp, rdoq=True, partition=parts)
        (b_med, b_iqr), (p_med, p_iqr) = timed(
            ctx, [lambda: fb.run(O, R0, R1, Rec), lambda: fp.run(O, R0, Rec)], a)
        ctx.sync()
        choice = fb.results()[4]
        dirs = np.bincount(choice["inter_dir"], minlength=3)
        lines += ["%s: %d CUs (L0 / L1 / bi chosen: %d / %d / %d)"
                  % (name, fb.desc.n_cus, dirs[0], dirs[1], dirs[2]),
                  "  B pass, one call  form %-14s fused tail %-5s %9.1f (%.1f)"
                  % (fb.form, bool(fb.p.fused_tail), b_med, b_iqr),
                  "  P pass, one call  form %-14s fused tail %-5s %9.1f (%.1f)"
                  % (fp.form, bool(fp.fused_tail), p_med, p_iqr),
                  "  B / P %.2f" % (b_med / p_med)]
        for title, rows in (("B pass", per_launch(ctx, lambda: fb.kernel_steps(O, R0, R1, Rec), a)),
                            ("P pass", per_launch(ctx, lambda: fp.kernel_steps(O, R0, Rec), a))):
            lines.append("  %s per launch (sum %.1f)" % (title, sum(r[1] for r in rows)))
            lines += ["    %-16s %9.1f (%.1f)" % r for r in rows]
        lines.append("")
        fb.destroy()
        fp.destroy()
    for p in (R0, O, R1, Rec):
        p.destroy()
    ctx.close()
    text = "\n".join(lines).rstrip("\n")
    print(text)
    with open(a.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
