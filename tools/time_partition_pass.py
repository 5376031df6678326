#!/usr/bin/env python3
"""Times the search plan and the frame pass on a real CU partition (one JSON object on
stdout; profiles/partition_pass.json is a run of it).

    python tools/time_partition_pass.py [--parent-lib /path/to/parent/libxvcgpu.so]
                                        [--repeats 30] [--warmup 5] [--inner 8]

* search of the `c1` picture-1 list (1133 CUs of a 1080p luma tree) and of an all-8x8
  1080p list: xvcgpu_me_search_planned against xvcgpu_me_search_sized of this build on
  the same lists - and, with --parent-lib, against xvcgpu_me_search_sized of a library
  built from the parent commit (measured in child processes of its own, once before and
  once after this build's searches: one library per process);
* the whole partition pass at 1080p (`c1` 1, `c1x` 3; 10 bit, QP 32, RDOQ) per kernel and
  in total, beside the uniform 16x16 pass of the same build;
* xvcgpu_me_plan_create, host wall time (it synchronises).

Device events around `inner` back-to-back calls, divided by inner; `warmup` untimed
rounds, then `repeats` timed ones: median and inter-quartile range, in microseconds."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def stats(us):
    q1, med, q3 = np.percentile(np.asarray(us, float), [25, 50, 75])
    return {"median_us": round(float(med), 2), "iqr_us": round(float(q3 - q1), 2),
            "n": len(us)}


def timed(ctx, fn, a):
    for _ in range(a.warmup):
        for _ in range(a.inner):
            fn()
    ctx.sync()
    out = []
    for _ in range(a.repeats):
        ctx.timer_begin()
        for _ in range(a.inner):
            fn()
        out.append(ctx.timer_end() * 1000.0 / a.inner)
    return stats(out)


def search_lists():
    from partition_fixture import luma_partition
    from xvc_amd import api, pipeline
    w, h = 1920, 1080
    real = pipeline.FrameDescriptors(w, h, 32, partition=luma_partition("c1", 1)).me
    sq8 = pipeline.FrameDescriptors(w, h, 32, cu=8).me
    return {"c1_picture1": (real, 64), "all_8x8_1080p": (sq8, 16)}


def pictures(ctx, w, h, bd, n):
    from xvc_amd import synth
    clip = synth.SyntheticClip(w, h, bd)
    pics = [ctx.picture(w, h, bd) for _ in range(n)]
    for k in (0, 1):
        planes = [np.ascontiguousarray(np.pad(p, 128 if c == 0 else 64, mode="edge"))
                  for c, p in enumerate(clip.frame(k))]
        pics[k].upload(planes, 128)
    return pics     # [ref, orig, ...]


def measure_searches(a, planned):
    from xvc_amd import api
    ctx = api.Context(0)
    R, O = pictures(ctx, 1920, 1080, 10, 2)
    out = {}
    for name, (me, mbs) in search_lists().items():
        n = len(me)
        d_me, d_res = ctx.buffer(me), ctx.alloc(api.MERES_DTYPE.itemsize * n)
        fl = api.ME_FULLPEL | api.ME_SUBPEL
        r = {"jobs": n}
        r["sized"] = timed(ctx, lambda: ctx.me_search_dev(O, R, fl, d_me.ptr, n, d_res.ptr, mbs), a)
        if planned:
            t0 = time.perf_counter()
            plan = ctx.me_plan(d_me.ptr, n, mbs)
            r["plan_create_us"] = round((time.perf_counter() - t0) * 1e6, 1)
            r["plan_counts"] = dict(zip(api.ME_PLAN_BIN_NAMES, plan.counts.tolist()))
            r["planned"] = timed(ctx, lambda: ctx.me_search_planned(O, R, fl, plan, d_res.ptr), a)
            plan.destroy()
        out[name] = r
        d_me.free()
        d_res.free()
    O.destroy()
    R.destroy()
    ctx.close()
    return out


def measure_passes(a):
    from partition_fixture import luma_partition
    from xvc_amd import api, pipeline
    ctx = api.Context(0)
    w, h, bd = 1920, 1080, 10
    R, O, Rec = pictures(ctx, w, h, bd, 3)
    out = {}
    cases = [("c1_picture1", luma_partition("c1", 1)), ("c1x_picture3", luma_partition("c1x", 3)),
             ("uniform_16x16", None)]
    for name, parts in cases:
        fp = pipeline.FramePass(ctx, w, h, bd, qp=32, rdoq=True, partition=parts)
        r = {"cus": fp.desc.n_cus, "form": fp.form, "fused_tail": bool(fp.fused_tail)}
        r["total"] = timed(ctx, lambda: fp.run(O, R, Rec), a)
        steps = {}
        for k, (step, _) in enumerate(fp.kernel_steps(O, R, Rec)):
            # the launches before step k untimed (it needs their results), then k alone
            def one(k=k):
                fp.kernel_steps(O, R, Rec)[k][1]()
            for _, fn in fp.kernel_steps(O, R, Rec)[:k]:
                fn()
            steps[step] = timed(ctx, one, a)
        r["kernels"] = steps
        out[name] = r
        fp.destroy()
    for p in (O, R, Rec):
        p.destroy()
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib")
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--inner", type=int, default=8)
    ap.add_argument("--only-sized-of", help="(child) measure me_search_sized of this library")
    a = ap.parse_args()
    if a.only_sized_of:
        from xvc_amd import api
        api.LIB_PATH = a.only_sized_of
        # (the parent's library does not have the plan's entry points)
        api.load_library(allow_missing=("xvcgpu_me_plan_create", "xvcgpu_me_plan_counts",
                                        "xvcgpu_me_plan_destroy", "xvcgpu_me_search_planned",
                                        "xvcgpu_frame_pass_planned"))
        print(json.dumps(measure_searches(a, planned=False)))
        return
    res = {"repeats": a.repeats, "warmup": a.warmup, "inner": a.inner}
    def parent_run():
        child = subprocess.run(
            [sys.executable, os.path.abspath(__file__), "--only-sized-of", a.parent_lib,
             "--repeats", str(a.repeats), "--warmup", str(a.warmup), "--inner", str(a.inner)],
            capture_output=True, text=True, timeout=600)
        if child.returncode != 0:
            sys.exit("parent library run failed:\n" + child.stdout + child.stderr)
        return json.loads(child.stdout.strip().splitlines()[-1])

    # the parent's library before AND after this build's (one library per process; this
    # process holds no context while a child runs): drift of the machine between the two
    # parent runs shows in their difference
    if a.parent_lib:
        res["parent_search"] = parent_run()
    res["search"] = measure_searches(a, planned=True)
    if a.parent_lib:
        res["parent_search_again"] = parent_run()
    res["pass"] = measure_passes(a)
    if a.parent_lib:
        verdict = {}
        for name, r in res["search"].items():
            runs = [res[k][name]["sized"] for k in ("parent_search", "parent_search_again")]
            p = min(runs, key=lambda t: t["median_us"])     # the faster parent run
            verdict[name] = {
                "planned_minus_parent_us": round(r["planned"]["median_us"] - p["median_us"], 2),
                "parent_iqr_us": p["iqr_us"],
                "parent_medians_us": [t["median_us"] for t in runs],
                "no_slower_beyond_spread": r["planned"]["median_us"] <= p["median_us"] + p["iqr_us"]}
        res["planned_vs_parent"] = verdict
    print(json.dumps(res))


if __name__ == "__main__":
    main()
