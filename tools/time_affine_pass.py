#!/usr/bin/env python3
"""Times the P frame pass with and without affine motion (pipeline.FramePass(affine=True),
xvcgpu_frame_pass_affine) at 1080p, 10 bit, QP 32, form `residual_rdoq`: on the 16-sample grid
(8040 of its 8160 CUs are capable) and on the partition of a real picture
(tests/partition_fixture: c1, picture 1), and the listed affine search alone per height
class, beside the added small launches.

    python tools/time_affine_pass.py [--out profiles/affine_frame_pass_time.txt]
                                     [--repeats 30] [--warmup 5] [--inner 4]

Device events around `inner` back-to-back calls, divided by inner; `warmup` untimed rounds,
then `repeats` timed ones, the flat and the affine pass taking turns round by round: median
and inter-quartile range, in microseconds.  These are first measurements, not targets: what
an affine search over every capable CU of a 1080p grid costs had not been measured."""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "affine_frame_pass_time.txt"))
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--inner", type=int, default=4)
    a = ap.parse_args()
    from partition_fixture import luma_partition
    from xvc_amd import api, pipeline, synth
    w, h, bd, qp = 1920, 1080, 10, 32
    ctx = api.Context(0)
    clip = synth.SyntheticClip(w, h, bd)
    O, R, Rec = (ctx.picture(w, h, bd) for _ in range(3))
    for pic, k in ((R, 0), (O, 1)):
        pic.upload([np.ascontiguousarray(np.pad(p, 128 if c == 0 else 64, mode="edge"))
                    for c, p in enumerate(clip.frame(k))], 128)
    lines = ["P frame pass with and without affine motion, %dx%d, %d bit, QP %d, form residual_rdoq"
             % (w, h, bd, qp),
             "device events, inner %d, warm-up %d, repeats %d: median (IQR) in us"
             % (a.inner, a.warmup, a.repeats), ""]
    for name, part in (("16x16 grid", None), ("partition c1 picture 1", luma_partition("c1", 1))):
        kw = dict(rdoq=True, fused=False, partition=part)
        flat = pipeline.FramePass(ctx, w, h, bd, qp, **kw)
        aff = pipeline.FramePass(ctx, w, h, bd, qp, affine=True, **kw)
        assert flat.form == aff.form == "residual_rdoq"
        (fm, fi), (am, ai) = timed(ctx, [lambda: flat.run(O, R, Rec), lambda: aff.run(O, R, Rec)], a)
        ctx.sync()
        fa, d, lib = aff.affine, aff.desc, ctx.lib
        choice = aff.affine_choice()
        listed = sum(fa.n_class)
        lines += ["%s, %d CUs, %d capable (height 16 / 32 / 64: %d / %d / %d), fused tail %s"
                  % ((name, d.n_cus, listed) + tuple(fa.n_class) + (bool(aff.fused_tail),)),
                  "  %-38s %9.1f (%.1f)"
                  % ("xvcgpu_frame_pass%s, one call" % ("_planned" if part is not None else ""),
                     fm, fi),
                  "  %-38s %9.1f (%.1f)" % ("xvcgpu_frame_pass_affine, one call", am, ai),
                  "  affine - flat %+.1f us = %+.2f %% (the flat pass's IQR %.1f us)"
                  % (am - fm, 100.0 * (am - fm) / fm, fi),
                  "  CUs that chose affine: %d of %d capable"
                  % (int((choice["use_affine"] == 1).sum()), listed)]
        # the added launches alone, on this pass's arrays (as the last run left them)
        f = fa.args()
        refs = (C.c_void_p * 1)(R.h_pic)
        steps = [("fp_affine_boot", lambda: ctx._check(lib.xvcgpu_fp_affine_boot(
            ctx.h, aff.d_res.ptr, fa.d_order.ptr, listed, w, h, fa.d_affine.ptr)))]
        first = 0
        for k, cu_h in enumerate((16, 32, 64)):
            if not fa.n_class[k]:
                continue
            cls = (C.c_int32 * 3)(*[fa.n_class[k] if j == k else 0 for j in range(3)])
            at = fa.d_order.ptr + 4 * first
            steps.append(("affine_me_listed h=%d (%d CUs)" % (cu_h, fa.n_class[k]),
                          lambda cls=cls, at=at: ctx._check(lib.xvcgpu_affine_me_listed(
                              ctx.h, O.h_pic, R.h_pic, fa.d_affine.ptr, d.n_cus, at, cls,
                              fa.d_affine_res.ptr))))
            first += fa.n_class[k]
        steps += [
            ("fp_affine_choice", lambda: ctx._check(lib.xvcgpu_fp_affine_choice(
                ctx.h, aff.d_me.ptr, aff.d_res.ptr, d.n_cus, C.byref(f)))),
            ("inter_pred_batch", lambda: ctx._check(lib.xvcgpu_inter_pred_batch(
                ctx.h, refs, 1, Rec.h_pic, aff.pred.h_pic, fa.d_inter.ptr, 3 * d.n_cus))),
            ("mc_from_me (the flat pass's)", lambda: ctx.mc_from_me_dev(
                R, flat.pred, flat.d_me.ptr, flat.d_res.ptr, d.n_cus)),
            ("cu_info_from_affine_choice", lambda: ctx._check(lib.xvcgpu_cu_info_from_affine_choice(
                ctx.h, aff.d_me.ptr, fa.d_choice.ptr, aff.d_nnz.ptr, aff.d_luma_idx.ptr, d.n_cus,
                d.qp, d.qp_c, 0, aff.d_cus_own)))]
        rows = timed(ctx, [fn for _, fn in steps], a)
        lines.append("  launches alone")
        lines += ["    %-34s %9.1f (%.1f)" % (n_, r[0], r[1]) for (n_, _), r in zip(steps, rows)]
        lines.append("")
        flat.destroy()
        aff.destroy()
    for p in (O, R, Rec):
        p.destroy()
    ctx.close()
    with open(a.out, "w") as f_:
        f_.write("\n".join(lines).rstrip("\n") + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
