#!/usr/bin/env python3
"""Times the B frame pass with and without affine motion (pipeline.BiRefsFramePass(affine=True),
xvcgpu_frame_pass_bi_refs_affine) at 1080p, 10 bit, QP 32, form `residual_rdoq`, lists L0 {4, 0},
L1 {12, 16} at POC 8 (five frames of the synthetic clip as POC 0, 4, 8, 12, 16): on the
16-sample grid and on the partition of a real picture (tests/partition_fixture: c1, picture 1),
each launch of the new ones alone, and the listed-refs class launch that holds every searched
picture against the same jobs issued as one xvcgpu_affine_me_listed launch per picture.

    python tools/time_bi_affine_pass.py [--out profiles/bi_affine_frame_pass_time.txt]
                                        [--repeats 30] [--warmup 5] [--inner 4]

Device events around `inner` back-to-back calls, divided by inner; `warmup` untimed rounds,
then `repeats` timed ones, the callables of a comparison taking turns round by round: median
and inter-quartile range, in microseconds.  These are first measurements, not targets: nobody
had measured an affine search over two lists of a whole picture."""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CUR_POC, LISTS = 8, ((4, 0), (12, 16))


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bi_affine_frame_pass_time.txt"))
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--inner", type=int, default=4)
    a = ap.parse_args()
    from partition_fixture import luma_partition
    from xvc_amd import api, pipeline, synth
    w, h, bd, qp = 1920, 1080, 10, 32
    ctx = api.Context(0)
    clip = synth.SyntheticClip(w, h, bd)
    pics = {}
    for k, poc in enumerate((0, 4, 8, 12, 16)):
        pics[poc] = ctx.picture(w, h, bd)
        pics[poc].upload([np.ascontiguousarray(np.pad(p, 128 if c == 0 else 64, mode="edge"))
                          for c, p in enumerate(clip.frame(k))], 128)
    O, Rec = pics[CUR_POC], ctx.picture(w, h, bd)
    refs = [[pics[poc] for poc in LISTS[l]] for l in range(2)]
    lines = ["B frame pass with and without affine motion, %dx%d, %d bit, QP %d, form residual_rdoq,"
             % (w, h, bd, qp),
             "L0 %s, L1 %s at POC %d" % (list(LISTS[0]), list(LISTS[1]), CUR_POC),
             "device events, inner %d, warm-up %d, repeats %d: median (IQR) in us; first "
             "measurements, no target" % (a.inner, a.warmup, a.repeats), ""]
    for name, part in (("16x16 grid", None), ("partition c1 picture 1", luma_partition("c1", 1))):
        kw = dict(rdoq=True, rdoq_packed=False, partition=part, cur_poc=CUR_POC, ref_pocs=LISTS)
        plain = pipeline.BiRefsFramePass(ctx, w, h, bd, qp, **kw)
        aff = pipeline.BiRefsFramePass(ctx, w, h, bd, qp, affine=True, **kw)
        assert plain.form == aff.form == "residual_rdoq"
        (pm, pi), (am, ai) = timed(ctx, [lambda: plain.run(O, refs, Rec),
                                         lambda: aff.run(O, refs, Rec)], a)
        ctx.sync()
        fa, d, lib = aff.affine, aff.desc, ctx.lib
        choice = aff.affine_choice()
        listed = sum(fa.n_class)
        won = choice[choice["use_affine"] == 1]
        lines += ["%s, %d CUs, %d capable (height 16 / 32 / 64: %d / %d / %d), planned %s"
                  % ((name, d.n_cus, listed) + tuple(fa.n_class) + (part is not None,)),
                  "  %-44s %9.1f (%.1f)" % ("xvcgpu_frame_pass_bi_refs, one call", pm, pi),
                  "  %-44s %9.1f (%.1f)" % ("xvcgpu_frame_pass_bi_refs_affine, one call", am, ai),
                  "  affine - plain %+.1f us = %+.2f %% (the plain pass's IQR %.1f us)"
                  % (am - pm, 100.0 * (am - pm) / pm, pi),
                  "  CUs that chose affine: %d of %d capable (L0 / L1 / bi: %d / %d / %d)"
                  % ((len(won), listed) + tuple(int((won["inter_dir"] == k).sum()) for k in range(3)))]
        # each launch of the pass alone, on the pass's arrays as the last run left them
        steps = aff.kernel_steps(O, refs, Rec)
        rows = timed(ctx, [fn for _, fn in steps], a)
        lines.append("  launches alone (affine_uni / affine_bi: one call = one launch per height class)")
        lines += ["    %-34s %9.1f (%.1f)" % (n_, r[0], r[1]) for (n_, _), r in zip(steps, rows)]
        # the class launch over every searched picture against one launch per picture
        e = 2 * aff.rmax
        jobs, slots = aff.affine_jobs(), fa.slots
        handles = (C.c_void_p * len(aff.distinct))(*[pics[poc].h_pic for poc in aff.distinct])
        n_class = (C.c_int32 * 3)(*fa.n_class)
        per_pic = []
        for k in range(e):
            if slots[0, k, 0] == api.FP_BI_NO_JOB:
                continue
            per_pic.append((pics[aff.distinct[int(slots[0, k, 0])]],
                            ctx.buffer(np.ascontiguousarray(jobs[:, k])),
                            ctx.buffer(np.zeros(d.n_cus, api.AFFINE_ME_RESULT_DTYPE))))

        def one_launch_per_class():
            ctx._check(lib.xvcgpu_affine_me_listed_refs(
                ctx.h, O.h_pic, handles, len(aff.distinct), fa.d_uni.ptr, fa.d_uni_slots.ptr,
                d.n_cus, e, fa.d_order.ptr, n_class, fa.d_uni_res.ptr))

        def one_launch_per_picture():
            for ref, d_jobs, d_out in per_pic:
                ctx._check(lib.xvcgpu_affine_me_listed(ctx.h, O.h_pic, ref.h_pic, d_jobs.ptr,
                                                       d.n_cus, fa.d_order.ptr, n_class, d_out.ptr))
        (cm, ci), (qm, qi) = timed(ctx, [one_launch_per_class, one_launch_per_picture], a)
        ctx.sync()
        got = aff.affine_uni_results()
        k = 0
        for col in range(e):       # the same answers both ways
            if slots[0, col, 0] == api.FP_BI_NO_JOB:
                continue
            out = per_pic[k][2].to_array(api.AFFINE_ME_RESULT_DTYPE, d.n_cus)
            assert out[fa.order].tobytes() == np.ascontiguousarray(got[fa.order, col]).tobytes()
            k += 1
        lines += ["  the uni-directional affine jobs, %d pictures, %d jobs" % (len(per_pic), listed * len(per_pic)),
                  "    %-44s %9.1f (%.1f)" % ("xvcgpu_affine_me_listed_refs, all pictures", cm, ci),
                  "    %-44s %9.1f (%.1f)" % ("xvcgpu_affine_me_listed, one call per picture", qm, qi),
                  "    per picture / all pictures = %.2f (above 1: the class launch over all pictures is faster)"
                  % (qm / cm), ""]
        for _, d_jobs, d_out in per_pic:
            d_jobs.free()
            d_out.free()
        plain.destroy()
        aff.destroy()
    for p in list(pics.values()) + [Rec]:
        p.destroy()
    ctx.close()
    with open(a.out, "w") as f_:
        f_.write("\n".join(lines).rstrip("\n") + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
