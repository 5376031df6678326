#!/usr/bin/env python3
"""Times the B frame pass with and without merge mode (pipeline.BiRefsFramePass(merge_cands=...),
xvcgpu_frame_pass_bi_refs_merge) at 1080p, 10 bit, QP 32 on the 16-sample grid with list 0 =
POC {4, 0} and list 1 = POC {12, 16} around POC 8, with RDOQ (the pass's packed form,
`fwd_transform`); the rank kernel alone
with the candidate mix below, with bi-directional candidates only and with list-0 candidates
only, beside the P pass's xvcgpu_fp_merge_rank over the same CUs and list-0 vectors in the
same run (the yardstick: a bi-directional candidate does two interpolations); and the two
small launches.

    python tools/time_bi_merge_pass.py [--out profiles/bi_merge_frame_pass_time.txt]
                                       [--repeats 30] [--warmup 5] [--inner 4]

Every CU is listed.  Its five candidates, from a seeded generator: list 0 zero; list 1 within
+-4 samples; both lists within +-4 samples, pictures 0 and 0; the same into pictures 1 and 1;
both lists within +-64 samples.  Device events around `inner` back-to-back calls, divided by
inner; `warmup` untimed rounds, then `repeats` timed ones, the callables taking turns round
by round in the same run: median and inter-quartile range, in microseconds.  First
measurements, not targets."""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from time_merge_pass import timed     # noqa: E402  (tools/ is the script's directory)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bi_merge_frame_pass_time.txt"))
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--inner", type=int, default=4)
    a = ap.parse_args()
    from xvc_amd import api, pipeline, synth
    w, h, bd, qp = 1920, 1080, 10, 32
    lists, cur = ((4, 0), (12, 16)), 8
    ctx = api.Context(0)
    clip = synth.SyntheticClip(w, h, bd)

    def picture(k):
        pic = ctx.picture(w, h, bd)
        pic.upload([np.ascontiguousarray(np.pad(p, 128 if c == 0 else 64, mode="edge"))
                    for c, p in enumerate(clip.frame(k))], 128)
        return pic
    O, Rec = picture(cur // 4), ctx.picture(w, h, bd)
    by_poc = {poc: picture(poc // 4) for l in lists for poc in l}
    refs = [[by_poc[poc] for poc in l] for l in lists]
    kw = dict(rdoq=True, cur_poc=cur, ref_pocs=lists)
    plain = pipeline.BiRefsFramePass(ctx, w, h, bd, qp, **kw)
    n = plain.desc.n_cus
    rng = np.random.default_rng(1)
    ref_idx = np.zeros((n, api.FP_MERGE_CANDS, 2), np.int32)
    mv = rng.integers(-4 * 16, 4 * 16 + 1, (n, api.FP_MERGE_CANDS, 2, 2)).astype(np.int32)
    ref_idx[:, 0], mv[:, 0] = (0, -1), 0
    ref_idx[:, 1], mv[:, 1, 0] = (-1, 0), 0
    ref_idx[:, 3] = (1, 1)
    mv[:, 4] = rng.integers(-64 * 16, 64 * 16 + 1, (n, 2, 2))
    mrg = pipeline.BiRefsFramePass(ctx, w, h, bd, qp, merge_cands=(ref_idx, mv), **kw)
    assert plain.form == mrg.form
    lib, fm = ctx.lib, mrg.merge
    args, m = mrg._call_args(O, refs, Rec), fm.args()
    # the rank kernel on other candidate mixes, and the P kernel over list 0's vectors
    only = {}
    for name, r in (("bi", (0, 0)), ("l0", (0, -1))):
        c = fm.cands.copy()
        c["ref_idx"] = r
        only[name] = ctx.buffer(c)
    p_cands = ctx.buffer(pipeline.merge_cand_array(mv[:, :, 0, :], n))
    p_rank = ctx.buffer(np.zeros(n, api.FP_MERGE_RANK_DTYPE))
    pm = pipeline.merge_args(n, 1, 1, fm.lambda_sqrt, p_cands.ptr, None, p_rank.ptr)

    def rank_with(d_cands):
        mm_ = fm.args()
        mm_.d_cands = d_cands.ptr
        return lambda: ctx._check(lib.xvcgpu_fp_bi_merge_rank(ctx.h, C.byref(args), C.byref(mm_)))
    steps = [
        ("xvcgpu_frame_pass_bi_refs, one call", lambda: plain.run(O, refs, Rec)),
        ("xvcgpu_frame_pass_bi_refs_merge, one call", lambda: mrg.run(O, refs, Rec)),
        ("fp_bi_merge_rank alone (%d CUs x 5)" % n, rank_with(fm.d_cands)),
        ("  ... five bi-directional candidates", rank_with(only["bi"])),
        ("  ... five list-0 candidates", rank_with(only["l0"])),
        ("fp_merge_rank (P), list 0's vectors", lambda: ctx._check(lib.xvcgpu_fp_merge_rank(
            ctx.h, O.h_pic, refs[0][0].h_pic, mrg.d_me[0][0].ptr, n, C.byref(pm)))),
        ("fp_bi_merge_choice alone", lambda: ctx._check(lib.xvcgpu_fp_bi_merge_choice(
            ctx.h, C.byref(args), C.byref(m)))),
        ("fp_bi_merge_skip alone", lambda: ctx._check(lib.xvcgpu_fp_bi_merge_skip(
            ctx.h, mrg.p.d_nnz.ptr, mrg.p.d_luma_idx.ptr, n, fm.d_choice.ptr)))]
    mrg.run(O, refs, Rec)       # (the small launches read a whole pass's arrays)
    rows = timed(ctx, [fn for _, fn in steps], a)
    mrg.run(O, refs, Rec)
    ctx.sync()
    won = mrg.merge_choice()
    use = won["use_merge"] == 1
    (f_med, f_iqr), (m_med, _) = rows[0], rows[1]
    lines = ["B frame pass with and without merge mode, %dx%d, %d bit, QP %d, 16x16 grid, "
             "L0 POC %s, L1 POC %s" % (w, h, bd, qp, list(lists[0]), list(lists[1])),
             "device events, inner %d, warm-up %d, repeats %d: median (IQR) in us"
             % (a.inner, a.warmup, a.repeats), "",
             "form %s, %d CUs, every CU listed, fused tail %s" % (mrg.form, n, bool(mrg.p.fused_tail))]
    lines += ["  %-44s %9.1f (%.1f)" % (n_, r[0], r[1]) for (n_, _), r in zip(steps, rows)]
    lines += ["  merge - plain %+.1f us = %+.2f %% (the plain pass's IQR %.1f us)"
              % (m_med - f_med, 100.0 * (m_med - f_med) / f_med, f_iqr),
              "  bi-directional / list-0 ranking: %.2f; list-0 ranking / the P kernel: %.2f"
              % (rows[3][0] / rows[4][0], rows[4][0] / rows[5][0]),
              "  CUs that chose merge: %d of %d (L0 %d, L1 %d, bi %d), skip among them: %d; first "
              "rank by merge index: %s"
              % (int(use.sum()), n, *[int((use & (won["inter_dir"] == d)).sum()) for d in range(3)],
                 int((won["skip"] == 1).sum()),
                 np.bincount(mrg.merge_rank()["order"][:, 0], minlength=5).tolist())]
    for b in list(only.values()) + [p_cands, p_rank]:
        b.free()
    plain.destroy()
    mrg.destroy()
    for p in [O, Rec] + list(by_poc.values()):
        p.destroy()
    ctx.close()
    with open(a.out, "w") as f_:
        f_.write("\n".join(lines).rstrip("\n") + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
