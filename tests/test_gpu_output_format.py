"""Decoder output formats on the device (xvcgpu_picture_convert_to): every
chroma format, size, bit depth and matrix of Resampler::ConvertTo against the
numpy model (tests/output_model.py), byte for byte."""
import os

import numpy as np
import pytest

import output_model as om
import stream_fixture as sf
from helpers import rnd_samples

pytestmark = pytest.mark.gpu
BORDER = 16


@pytest.fixture(scope="module")
def gpu():
    from xvc_amd import api
    ctx = api.Context(0)
    yield api, ctx
    ctx.close()


def make_picture(ctx, rng, w, h, bd, smooth):
    """A picture whose border holds noise: the conversion must not read it."""
    planes = [rnd_samples(rng, bd, hh, ww, smooth) for ww, hh in
              ((w, h), (w // 2, h // 2), (w // 2, h // 2))]
    padded = []
    for c, p in enumerate(planes):
        b = BORDER >> (c > 0)
        q = rng.integers(0, 1 << bd, size=(p.shape[0] + 2 * b, p.shape[1] + 2 * b),
                         dtype=np.uint16)
        q[b:-b, b:-b] = p
        padded.append(q)
    P = ctx.picture(w, h, bd)
    P.upload(padded, BORDER)
    return P, planes


def fmt_dict(f):
    return {n: getattr(f, n) for n, _ in f._fields_}


def check(api, ctx, P, planes, dw, dh, f):
    """Convert on the device and compare with the model; a combination the
    reference leaves undefined must be refused."""
    try:
        exp = om.convert_to(planes, P.bd, dw, dh, fmt_dict(f))
    except AssertionError:
        with pytest.raises(api.XvcGpuError):
            ctx.picture_convert_to(P, dw, dh, f)
        return
    got = ctx.picture_convert_to(P, dw, dh, f)
    assert len(got) == len(exp), (dw, dh, f)
    if got != exp:
        a, b = np.frombuffer(got, np.uint8), np.frombuffer(exp, np.uint8)
        bad = np.flatnonzero(a != b)
        raise AssertionError("%r %dx%d: %d bytes differ, first at %s" % (
            f, dw, dh, len(bad), bad[:8].tolist()))


SAME_SIZE = [dict(chroma_format=cf, bitdepth=bd, dither=d)
             for cf in (0, 1, 2, 3) for bd in (0, 8, 10, 16) for d in (0, 1)]
ARGB = [dict(chroma_format=4, bitdepth=bd, color_matrix=m) for bd in (8, 10, 16)
        for m in (0, 1, 2, 3)]
RESIZED = [dict(width=w, height=h, chroma_format=cf, bitdepth=bd, color_matrix=m)
           for (w, h) in ((68, 36), (101, 37), (272, 144), (2, 2), (3, 5), (200, 100),
                          (50, 140), (408, 216))
           for cf, bd, m in ((1, 8, 0), (2, 10, 0), (3, 12, 0), (4, 8, 1), (4, 10, 3),
                             (0, 16, 0), (1, 16, 0))]


@pytest.mark.parametrize("bd", [8, 10, 12])
@pytest.mark.parametrize("disp", ["full", "cropped", "odd"])
def test_convert_synthetic(gpu, bd, disp):
    api, ctx = gpu
    rng = np.random.default_rng(7000 + bd + len(disp))
    w, h = 136, 72
    dw, dh = {"full": (w, h), "cropped": (w - 6, h - 10), "odd": (w - 5, h - 3)}[disp]
    P, planes = make_picture(ctx, rng, w, h, bd, smooth=bd == 12)
    try:
        for kw in SAME_SIZE + ARGB + RESIZED:
            check(api, ctx, P, planes, dw, dh, api.OutputFormat(**kw))
    finally:
        P.destroy()


@pytest.mark.parametrize("w,h,dw,dh,out", [
    (1920, 1080, 1920, 1080, (2, 2)),
    (1920, 1080, 1918, 1078, (1280, 720)),
    (136, 72, 136, 72, (4096, 2160)),
    (136, 72, 136, 72, (4096, 3)),
    (1920, 1080, 1920, 1080, (3840, 2160)),
    (352, 288, 352, 288, (1920, 1080)),
])
def test_convert_extreme_ratios(gpu, w, h, dw, dh, out):
    api, ctx = gpu
    rng = np.random.default_rng(w + h + out[0])
    P, planes = make_picture(ctx, rng, w, h, 10, smooth=False)
    try:
        for cf, bd, m in ((1, 8, 0), (3, 10, 0), (4, 8, 2), (2, 16, 0)):
            check(api, ctx, P, planes, dw, dh,
                  api.OutputFormat(out[0], out[1], cf, m, bd))
    finally:
        P.destroy()


def test_convert_writes_device_buffer(gpu):
    api, ctx = gpu
    rng = np.random.default_rng(5)
    P, planes = make_picture(ctx, rng, 64, 48, 10, smooth=False)
    f = api.OutputFormat(100, 60, 4, 1, 8)
    n = api.output_bytes(f.resolved(64, 48, 10))
    assert n == 100 * 60 * 4
    d = ctx.alloc(n + 64)
    try:
        ctx.lib.xvcgpu_memset(ctx.h, d.ptr, 0x5a, n + 64)
        ctx.picture_convert_to(P, 64, 48, f, d.ptr)
        got = d.to_array(np.uint8, n + 64)
        assert got[:n].tobytes() == om.convert_to(planes, 10, 64, 48, fmt_dict(f))
        assert (got[n:] == 0x5a).all()  # nothing beyond the output
    finally:
        d.free()
        P.destroy()


INVALID = [
    (64, 48, dict(width=1)), (64, 48, dict(height=1)), (64, 48, dict(width=40000)),
    (64, 48, dict(height=-3)), (64, 48, dict(chroma_format=5)),
    (64, 48, dict(chroma_format=-1)), (64, 48, dict(color_matrix=4)),
    (64, 48, dict(bitdepth=7)), (64, 48, dict(bitdepth=17)),
    (66, 48, dict()), (64, 50, dict()), (1, 48, dict()), (64, 0, dict()),
    (64, 48, dict(chroma_format=3, bitdepth=11)),       # 4:4:4 at bd + 1
    (64, 48, dict(width=32768, height=32768, chroma_format=4)),  # > INT_MAX samples
]


@pytest.mark.parametrize("dw,dh,kw", INVALID)
def test_convert_invalid_argument(gpu, dw, dh, kw):
    api, ctx = gpu
    P = ctx.picture(64, 48, 10)
    n = 1 << 16
    d = ctx.alloc(n)
    try:
        ctx.lib.xvcgpu_memset(ctx.h, d.ptr, 0x33, n)
        st = ctx.lib.xvcgpu_picture_convert_to(ctx.h, P.h_pic, dw, dh,
                                               api.C.byref(api.OutputFormat(**kw)), d.ptr)
        assert st == 10  # XVCGPU_INVALID_ARGUMENT
        ctx.sync()
        assert (d.to_array(np.uint8, n) == 0x33).all()
    finally:
        d.free()
        P.destroy()


def test_argb_from_11_bit_refused(gpu):
    api, ctx = gpu
    P = ctx.picture(64, 48, 11)
    d = ctx.alloc(64 * 48 * 8)
    try:
        st = ctx.lib.xvcgpu_picture_convert_to(ctx.h, P.h_pic, 64, 48,
                                               api.C.byref(api.OutputFormat(chroma_format=4)),
                                               d.ptr)
        assert st == 10
    finally:
        d.free()
        P.destroy()


# -- the decoder's Postprocess: real streams against the reference's output ---

def decode_with_outputs(api, ctx, fx, fmt, lanes=1, outs=True):
    """decode_sequence of the whole stream with every picture converted to
    `fmt`; returns (the output bytes per picture, the decoder's launch count,
    the reconstructed planes)."""
    from xvc_amd import decoder
    w, h, bd = (int(fx.info[0][k]) for k in ("width", "height", "bitdepth"))
    dec = decoder.PictureDecoder(ctx, w, h, bd)
    lane_ctxs = [api.Context(0) for _ in range(lanes - 1)]
    for c in lane_ctxs:
        dec.add_lane(c)
    infos = [fx.info[i] for i in range(fx.n)]
    pos = {int(infos[i]["poc"]): i for i in range(fx.n)}
    ref_index = np.full((fx.n, 2, 5), -1, np.int32)
    pictures = []
    for i, info in enumerate(infos):
        ps, cs = sf.to_syntax(info, fx.cus(i))
        pictures.append((ps, cs, np.ascontiguousarray(fx.levels(i))))
        for l in range(2):
            for k in range(int(info["num_ref"][l])):
                ref_index[i, l, k] = pos[int(info["ref_poc"][l][k])]
    recs = [ctx.picture(w, h, bd) for _ in range(fx.n)]
    n = api.output_bytes(fmt.resolved(w, h, bd)) if outs else 0
    bufs = [ctx.alloc(n) for _ in range(fx.n)] if outs else []
    try:
        if outs:
            dec.set_output_format(fmt, w, h)
            dec.decode_sequence(pictures, ref_index, recs, outs=[b.ptr for b in bufs])
        else:
            dec.decode_sequence(pictures, ref_index, recs)
        ctx.sync()
        data = [b.to_array(np.uint8, n).tobytes() for b in bufs]
        planes = [r.download(0) for r in recs]
        return data, dec.launches, planes
    finally:
        for b in bufs:
            b.free()
        dec.destroy()
        for c in lane_ctxs:
            c.close()
        for p in recs:
            p.destroy()


@pytest.mark.parametrize("clip,lanes", [("tiny", 1), ("tiny", 3), ("c0", 2), ("c1", 1)])
def test_decode_sequence_outputs_equal_reference(gpu, clip, lanes):
    """Every picture the reference padded hashes to the reference decoder's
    output; tiny's unpadded pictures equal it wherever no tap reaches beyond the
    picture, and the model everywhere.  The reconstruction itself is unchanged."""
    import hashlib
    api, ctx = gpu
    fx = sf.StreamFixture(clip)
    g = np.load(os.path.join(sf.GOLDEN, "output", "output_%s.npz" % clip))
    z = np.load(os.path.join(sf.GOLDEN, "stream_%s.npz" % clip))
    w, h, bd = (int(fx.info[0][k]) for k in ("width", "height", "bitdepth"))
    step = 5 if lanes > 1 and clip == "tiny" else 1   # with lanes: every fifth case
    for i in range(0, len(g["cases"]), step):
        fmt = api.OutputFormat(*(int(v) for v in g["cases"][i]))
        data, _, planes = decode_with_outputs(api, ctx, fx, fmt, lanes)
        for j in range(fx.n):
            assert np.array_equal(sf.picture_md5(planes[j], bd), fx.info[j]["md5"])
            if fx.info[j]["padded"]:
                assert hashlib.sha256(data[j]).digest() == g["sha256"][i, j].tobytes(), \
                    (clip, i, j, fmt)
                continue
            ref_planes = [z["post_%d_%d" % (j, c)] for c in range(3)] \
                if "post_%d_0" % j in z.files else None
            if ref_planes is not None:
                assert data[j] == om.convert_to(ref_planes, bd, w, h, fmt_dict(fmt)), (i, j)
            if "full_%d_%d" % (i, j) in g.files:
                full = g["full_%d_%d" % (i, j)]
                m = om.interior_mask(fmt_dict(fmt), w, h, bd, w, h)
                got = np.frombuffer(data[j], np.uint8)
                assert np.array_equal(got[m], full[m]), (clip, i, j, fmt)


@pytest.mark.parametrize("clip", ["t8", "t12"])
@pytest.mark.parametrize("kw", [
    dict(chroma_format=1, bitdepth=0),                      # 4:2:0 at the internal depth
    dict(chroma_format=3, bitdepth=8, dither=1),            # 4:4:4, 8 bit, dithered
    dict(chroma_format=4, bitdepth=8, color_matrix=2),      # ARGB, 8 bit, BT.709
    dict(width=101, height=37, chroma_format=1, bitdepth=16),
], ids=["420", "444d8", "argb709", "resized16"])
def test_decode_sequence_outputs_at_other_depths(gpu, clip, kw):
    """Streams of 8 and 12 bit internal depth: every picture's output equals the
    model's conversion of the planes of the same run, and those planes hash to
    the stream's MD5."""
    api, ctx = gpu
    fx = sf.StreamFixture(clip)
    w, h, bd = (int(fx.info[0][k]) for k in ("width", "height", "bitdepth"))
    assert bd == {"t8": 8, "t12": 12}[clip]
    fmt = api.OutputFormat(**kw)
    data, _, planes = decode_with_outputs(api, ctx, fx, fmt)
    for j in range(fx.n):
        assert np.array_equal(sf.picture_md5(planes[j], bd), fx.info[j]["md5"]), (clip, j)
        exp = om.convert_to(planes[j], bd, w, h, fmt_dict(fmt))
        assert len(data[j]) == len(exp) and data[j] == exp, (clip, j, fmt)


def test_decode_sequence_without_format_unchanged(gpu):
    """No output format: the same planes and launch count as with one (the
    conversion is not one of the decoder's counted launches)."""
    api, ctx = gpu
    fx = sf.StreamFixture("tiny")
    _, launches_plain, planes_plain = decode_with_outputs(api, ctx, fx, None, outs=False)
    _, launches_out, planes_out = decode_with_outputs(
        api, ctx, fx, api.OutputFormat(100, 60, 4, 1, 8))
    assert launches_plain == launches_out
    for a, b in zip(planes_plain, planes_out):
        for c in range(3):
            assert np.array_equal(a[c], b[c])
