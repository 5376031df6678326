#!/usr/bin/env python3
"""Times the P frame pass with and without adaptive QP (pipeline.FramePass(aqp_strength=...),
xvcgpu_frame_pass_aqp) at 1080p, 10 bit, QP 32 on the 16-sample grid, for the forms
`residual_rdoq` and `fwd_transform`, and the three launches adaptive QP adds
(xvcgpu_variance_map, xvcgpu_aqp_apply, xvcgpu_cu_info_set_qp) alone.

    python tools/time_aqp_pass.py [--out profiles/aqp_frame_pass_time.txt]
                                  [--repeats 30] [--warmup 5] [--inner 8]
                                  [--parent DIR [--pairs 5] [--steps 1000] [--bench-warmup 100]]

Device events around `inner` back-to-back calls, divided by inner; `warmup` untimed rounds,
then `repeats` timed ones, the flat and the adaptive pass taking turns round by round: median
and inter-quartile range, in microseconds.  There is no target: the expectation to confirm or
refute is that the added launches cost a few microseconds each beside a pass of several
hundred.

--parent DIR: a built checkout of the parent commit.  The flat passes must not move, so
`python bench.py --gpus 1` is run `pairs` times in DIR and here, alternating, each in a process
of its own; both medians, the spread of each and the difference go into the same file."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STRENGTH = 13       # the reference's default aqp_strength (encoder_settings.h:90)


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


def bench_pairs(a):
    """bench.py in the parent checkout and here, alternating: lines for the file."""
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", str(a.steps), "--warmup",
           str(a.bench_warmup)]
    values = {"parent": [], "this": []}
    for _ in range(a.pairs):
        for name, cwd in (("parent", a.parent), ("this", ROOT)):
            out = subprocess.run(cmd, cwd=cwd, capture_output=True, text=True, check=True).stdout
            line = [l for l in out.splitlines() if l.startswith("{")][-1]
            values[name].append(float(json.loads(line)["value"]))
            print("bench.py (%s): %.1f" % (name, values[name][-1]), flush=True)
    lines = ["", "python bench.py --gpus 1 --steps %d --warmup %d, %d paired runs (parent, this, "
             "parent, ...), each a process of its own: frame passes/s" % (a.steps, a.bench_warmup,
                                                                           a.pairs)]
    med = {}
    for name in ("parent", "this"):
        v = values[name]
        med[name] = float(np.median(v))
        lines.append("  %-7s median %9.1f  min %9.1f  max %9.1f  spread (max - min) %6.1f = %.2f %%"
                     % (name, med[name], min(v), max(v), max(v) - min(v),
                        100.0 * (max(v) - min(v)) / med[name]))
        lines.append("          runs " + " ".join("%.1f" % x for x in v))
    diff = med["this"] - med["parent"]
    spread = max(values["parent"]) - min(values["parent"])
    lines.append("  this - parent %+.1f passes/s = %+.2f %%; the parent's own run-to-run spread %.1f: "
                 "the difference is %s it" % (diff, 100.0 * diff / med["parent"], spread,
                                              "within" if abs(diff) <= spread else "LARGER than"))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "aqp_frame_pass_time.txt"))
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--inner", type=int, default=8)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--bench-warmup", type=int, default=100)
    a = ap.parse_args()
    from xvc_amd import api, pipeline, synth
    w, h, bd, qp = 1920, 1080, 10, 32
    ctx = api.Context(0)
    clip = synth.SyntheticClip(w, h, bd)
    O, R, Rec = (ctx.picture(w, h, bd) for _ in range(3))
    for pic, k in ((R, 0), (O, 1)):
        pic.upload([np.ascontiguousarray(np.pad(p, 128 if c == 0 else 64, mode="edge"))
                    for c, p in enumerate(clip.frame(k))], 128)
    lines = ["P frame pass with and without adaptive QP, %dx%d, %d bit, QP %d, aqp_strength %d, "
             "16x16 grid" % (w, h, bd, qp, STRENGTH),
             "device events, inner %d, warm-up %d, repeats %d: median (IQR) in us"
             % (a.inner, a.warmup, a.repeats), ""]
    for form, kw in (("residual_rdoq", dict(rdoq=True, fused=False)),
                     ("fwd_transform", dict(rdoq=True, form="fwd_transform"))):
        flat = pipeline.FramePass(ctx, w, h, bd, qp, **kw)
        aqp = pipeline.FramePass(ctx, w, h, bd, qp, aqp_strength=STRENGTH, **kw)
        assert flat.form == aqp.form == form
        (fm, fi), (am_, ai) = timed(ctx, [lambda: flat.run(O, R, Rec), lambda: aqp.run(O, R, Rec)], a)
        ctx.sync()
        dqp = aqp.ctu_delta_qp()
        hist = np.bincount(dqp.ravel().astype(int) - api.AQP_DELTA_MIN, minlength=api.AQP_DELTAS)
        lines += ["form %s, %d CUs, fused tail %s" % (form, aqp.desc.n_cus, bool(aqp.fused_tail)),
                  "  xvcgpu_frame_pass, one call       %9.1f (%.1f)" % (fm, fi),
                  "  xvcgpu_frame_pass_aqp, one call   %9.1f (%.1f)" % (am_, ai),
                  "  aqp - flat %+.1f us = %+.2f %% (the flat pass's IQR %.1f us)"
                  % (am_ - fm, 100.0 * (am_ - fm) / fm, fi),
                  "  CTUs per delta -3 .. 7: " + " ".join(str(int(v)) for v in hist),
                  "  (the adaptive pass codes at the map's QPs: the difference holds the changed "
                  "load of the search and the quantiser beside the added launches)"]
        if form == "fwd_transform":     # the added launches alone, on this pass's arrays
            q, d, lib = aqp.aqp, aqp.desc, ctx.lib
            jobs = (C.c_void_p * 1)(aqp.d_me.ptr)
            prm = aqp.d_rdoq_prm.ptr
            steps = [
                ("variance_map", lambda: ctx._check(lib.xvcgpu_variance_map(
                    ctx.h, O.h_pic, q.d_var16.ptr, q.ctu_size, q.d_ctu_var.ptr))),
                ("aqp_apply", lambda: ctx._check(lib.xvcgpu_aqp_apply(
                    ctx.h, C.byref(q.table), q.d_ctu_var.ptr, jobs, 1, aqp.d_tx.ptr, prm,
                    aqp.d_luma_idx.ptr, d.n_cus, q.d_cu_qp.ptr, q.d_ctu_dqp.ptr))),
                ("cu_info_set_qp", lambda: ctx._check(lib.xvcgpu_cu_info_set_qp(
                    ctx.h, aqp.d_cus_own, q.d_cu_qp.ptr, d.n_cus)))]
            rows = timed(ctx, [fn for _, fn in steps], a)
            lines.append("  the added launches alone (sum %.1f; variance_map is two kernels)"
                         % sum(r[0] for r in rows))
            lines += ["    %-18s %9.1f (%.1f)" % (name, r[0], r[1])
                      for (name, _), r in zip(steps, rows)]
        lines.append("")
        flat.destroy()
        aqp.destroy()
    for p in (O, R, Rec):
        p.destroy()
    ctx.close()
    if a.parent:
        lines += bench_pairs(a)
    with open(a.out, "w") as f:
        f.write("\n".join(lines).rstrip("\n") + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
