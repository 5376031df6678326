#!/usr/bin/env python3
"""Times the P frame pass with and without merge mode (pipeline.FramePass(merge_cands=...),
xvcgpu_frame_pass_merge) at 1080p, 10 bit, QP 32 on the 16-sample grid, forms `residual_rdoq`
and `fwd_from_me` (the benchmark's), and the rank kernel alone beside the two small launches.

    python tools/time_merge_pass.py [--out profiles/merge_frame_pass_time.txt]
                                    [--repeats 30] [--warmup 5] [--inner 4]

Every CU is listed.  Its five candidates, from a seeded generator: zero, three vectors within
+-4 samples, one within +-64 samples.  Device events around `inner` back-to-back calls,
divided by inner; `warmup` untimed rounds, then `repeats` timed ones, the flat pass, the pass
with merge and the rank kernel taking turns round by round in the same run: median and
inter-quartile range, in microseconds.  These are first measurements, not targets: what a
five-candidate ranking over a whole 1080p grid costs had not been measured."""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def stats(us):
    q1, med, q3 = np.percentile(np.asarray(us, float), [25, 50, 75])
    return float(med), float(q3 - q1)


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
            ctx.timer_begin()
            for _ in range(a.inner):
                fn()
            out[k].append(ctx.timer_end() * 1000.0 / a.inner)
    return [stats(o) for o in out]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "merge_frame_pass_time.txt"))
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--inner", type=int, default=4)
    a = ap.parse_args()
    from xvc_amd import api, pipeline, synth
    w, h, bd, qp = 1920, 1080, 10, 32
    ctx = api.Context(0)
    clip = synth.SyntheticClip(w, h, bd)
    O, R, Rec = (ctx.picture(w, h, bd) for _ in range(3))
    for pic, k in ((R, 0), (O, 1)):
        pic.upload([np.ascontiguousarray(np.pad(p, 128 if c == 0 else 64, mode="edge"))
                    for c, p in enumerate(clip.frame(k))], 128)
    lines = ["P frame pass with and without merge mode, %dx%d, %d bit, QP %d, 16x16 grid"
             % (w, h, bd, qp),
             "device events, inner %d, warm-up %d, repeats %d: median (IQR) in us"
             % (a.inner, a.warmup, a.repeats), ""]
    for form, kw in (("residual_rdoq", dict(rdoq=True, fused=False)),
                     ("fwd_from_me", dict(rdoq=True))):
        flat = pipeline.FramePass(ctx, w, h, bd, qp, **kw)
        n = flat.desc.n_cus
        rng = np.random.default_rng(1)
        mv = np.zeros((n, api.FP_MERGE_CANDS, 2), np.int32)
        mv[:, 1:4] = rng.integers(-4 * 16, 4 * 16 + 1, (n, 3, 2))
        mv[:, 4] = rng.integers(-64 * 16, 64 * 16 + 1, (n, 2))
        mrg = pipeline.FramePass(ctx, w, h, bd, qp, merge_cands=mv, **kw)
        assert flat.form == mrg.form == form
        fm, lib, d = mrg.merge, ctx.lib, mrg.desc
        m = fm.args()
        steps = [
            ("xvcgpu_frame_pass, one call", lambda: flat.run(O, R, Rec)),
            ("xvcgpu_frame_pass_merge, one call", lambda: mrg.run(O, R, Rec)),
            ("fp_merge_rank alone (%d CUs x 5)" % n, lambda: ctx._check(lib.xvcgpu_fp_merge_rank(
                ctx.h, O.h_pic, R.h_pic, mrg.d_me.ptr, n, C.byref(m)))),
            ("fp_merge_choice alone", lambda: ctx._check(lib.xvcgpu_fp_merge_choice(
                ctx.h, mrg.d_me.ptr, mrg.d_res.ptr, n, C.byref(m)))),
            ("fp_merge_skip alone", lambda: ctx._check(lib.xvcgpu_fp_merge_skip(
                ctx.h, mrg.d_nnz.ptr, mrg.d_luma_idx.ptr, n, fm.d_choice.ptr)))]
        rows = timed(ctx, [fn for _, fn in steps], a)
        mrg.run(O, R, Rec)
        ctx.sync()
        choice = mrg.merge_choice()
        (f_med, f_iqr), (m_med, _) = rows[0], rows[1]
        lines.append("form %s, %d CUs, every CU listed, fused tail %s"
                     % (form, d.n_cus, bool(mrg.fused_tail)))
        lines += ["  %-38s %9.1f (%.1f)" % (n_, r[0], r[1]) for (n_, _), r in zip(steps, rows)]
        lines += ["  merge - flat %+.1f us = %+.2f %% (the flat pass's IQR %.1f us)"
                  % (m_med - f_med, 100.0 * (m_med - f_med) / f_med, f_iqr),
                  "  CUs that chose merge: %d of %d, skip among them: %d; first rank by merge "
                  "index: %s" % (int((choice["use_merge"] == 1).sum()), n,
                                 int((choice["skip"] == 1).sum()),
                                 np.bincount(mrg.merge_rank()["order"][:, 0], minlength=5).tolist()),
                  ""]
        flat.destroy()
        mrg.destroy()
    for p in (O, R, Rec):
        p.destroy()
    ctx.close()
    with open(a.out, "w") as f_:
        f_.write("\n".join(lines).rstrip("\n") + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
