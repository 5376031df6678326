"""Isolated timings of xvcgpu_picture_convert_to (decoder output formats) at
1080p and 2160p, 10-bit 4:2:0 pictures, with the algorithmic bandwidth (bytes
of the source planes read + bytes written) / time, beside the plain export
(xvcgpu_picture_export to 8 bit, tools/time_kernels.py's export8).

    python tools/time_output.py [reps]
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
from xvc_amd import api  # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 200
BD = 10
ctx = api.Context(0)


def timed(fn, reps=REPS):
    fn()
    ctx.sync()
    ctx.timer_begin()
    for _ in range(reps):
        fn()
    return 1e3 * ctx.timer_end() / reps


print("%-34s %10s %10s %8s" % ("case", "MB moved", "us", "GB/s"))
for W, H in ((1920, 1080), (3840, 2160)):
    rng = np.random.default_rng(W)
    P = ctx.picture(W, H, BD)
    P.upload([rng.integers(0, 1 << BD, size=(h, w), dtype=np.uint16)
              for w, h in ((W, H), (W // 2, H // 2), (W // 2, H // 2))])
    src_bytes = W * H * 3 // 2 * 2
    cases = [
        ("export8 (xvcgpu_picture_export)", None, W * H * 3 // 2),
        ("4:2:0 8-bit dither", api.OutputFormat(0, 0, 1, 0, 8, 1), None),
        ("4:2:0 8-bit", api.OutputFormat(0, 0, 1, 0, 8, 0), None),
        ("ARGB 8-bit (709)", api.OutputFormat(0, 0, 4, 0, 8), None),
        ("ARGB 10-bit (2020)", api.OutputFormat(0, 0, 4, 3, 10), None),
        ("-> 1280x720 4:2:0 8-bit", api.OutputFormat(1280, 720, 1, 0, 8), None),
        ("-> 3840x2160 4:4:4 10-bit", api.OutputFormat(3840, 2160, 3, 0, 10), None),
    ]
    print("-- %dx%d, %d-bit 4:2:0 source" % (W, H, BD))
    d = ctx.alloc(3840 * 2160 * 8)
    for name, fmt, out_bytes in cases:
        if fmt is None:
            fn = lambda: ctx._check(ctx.lib.xvcgpu_picture_export(  # noqa: E731
                ctx.h, P.h_pic, d.ptr, W, H, 8, 0))
        else:
            out_bytes = api.output_bytes(fmt.resolved(W, H, BD))
            fn = lambda fmt=fmt: ctx.picture_convert_to(P, W, H, fmt, d.ptr)  # noqa: E731
        us = timed(fn)
        moved = src_bytes + out_bytes
        print("%-34s %10.2f %10.2f %8.0f" % (name, moved / 1e6, us, moved / us / 1e3))
    d.free()
    P.destroy()
ctx.close()
