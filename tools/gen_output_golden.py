#!/usr/bin/env python3
"""Decoder output-format fixtures (authoring container only: needs
oracle/_ref/libxvcref.so, i.e. the reference sources).

    python tools/gen_output_golden.py [tiny] [c0] [c1]

For each clip: feed the committed bitstream of tests/golden/stream_<clip>.npz
(4-byte LE size + NAL) to the REFERENCE decoder's public C API
(xvc_decoder_api_get: parameters_set_default, threads = 0, the output fields
set per case) and record, per (case, picture in decoding order), the SHA-256
of the output bytes.  The full bytes are kept only for the pictures the
reference did not pad (tiny's poc 1 and 3), only for cases that read past
the picture edge (a resampled plane, or the bilinear chroma of 4:4:4 / ARGB)
and only up to FULL_MAX bytes per picture, for the interior comparison.
Written to tests/golden/output/output_<clip>.npz, with its MD5 in
tests/golden/output/MANIFEST.md5 (checked by tests/test_output_format.py).

simd_mask = 0: the reference's SSE2 error-feedback down-shift keeps eight
accumulators, one per column lane, carried down the rows, while its C
function (and Resampler::SimdFunc's default, which the project's export pins)
carries one remainder through the plane in raster order.  The scalar
functions give the definition; every other output is the same either way.

Asserts that the resized cases cover every downsampling filter
(GetFilterFromScale 0..7) and upsampling on luma and on chroma.
"""
import ctypes as C
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import output_model as om  # noqa: E402
import stream_fixture as sf  # noqa: E402

REF_LIB = os.path.join(ROOT, "oracle", "_ref", "libxvcref.so")
OUT_DIR = os.path.join(sf.GOLDEN, "output")
FULL_MAX = 30000  # full bytes kept for outputs up to this size (fixture budget)
CASE_FIELDS = ("width", "height", "chroma_format", "color_matrix", "bitdepth", "dither")


def case(w=0, h=0, cf=255, cm=0, bd=0, dither=1):
    return (w, h, cf, cm, bd, dither)


SAME = [case(cf=cf, bd=bd, dither=d) for cf in (0, 1, 2, 3)
        for bd, d in ((8, 0), (8, 1), (10, 1), (16, 1))]
ARGB = [case(cf=4, bd=bd, cm=m) for bd in (8, 10) for m in (0, 1, 2, 3)]
# 136x72: widths whose luma (136 / w) and 4:2:0 chroma (68 / (w >> 1)) ratios
# fall in every GetFilterFromScale band; upsampling; odd sizes
TINY_RESIZED = [case(w, h, 1, bd=8) for w, h in ((135, 71), (120, 64), (100, 50), (75, 40),
                                                 (60, 36), (50, 30), (40, 24), (20, 10))] + [
    case(272, 144), case(68, 36, bd=8), case(13, 9, 1, bd=8), case(101, 37, 2, bd=8),
    case(100, 60, 2, bd=10), case(200, 100, 3, bd=12), case(137, 73, 3, bd=16),
    case(100, 60, 4), case(30, 18, 4, 3, 10), case(272, 144, 4, 1, 8), case(48, 24, 0, bd=8)]
CLIPS = {
    "tiny": SAME + ARGB + TINY_RESIZED,
    "c0": [case(cf=1, bd=8), case(cf=3, bd=10), case(cf=4, bd=8), case(cf=2, bd=8, dither=0),
           case(1920, 1080, 4, 0, 8), case(176, 144, 1, bd=8), case(704, 576, 3, bd=10),
           case(333, 277, 2, bd=16)],
    "c1": [case(cf=1, bd=8), case(cf=4, bd=8, cm=2), case(1280, 720, 1, bd=8),
           case(3840, 2160, 3, bd=10)],
}


class Params(C.Structure):  # xvc_decoder_parameters (xvcdec.h)
    _fields_ = [("output_width", C.c_int), ("output_height", C.c_int),
                ("output_chroma_format", C.c_int), ("output_color_matrix", C.c_int),
                ("output_bitdepth", C.c_int), ("max_framerate", C.c_double),
                ("threads", C.c_int), ("simd_mask", C.c_uint32), ("dither", C.c_int),
                ("additional_decoder_buffers", C.c_int)]


class Stats(C.Structure):  # xvc_dec_pic_stats
    _fields_ = [("nal_unit_type", C.c_uint32), ("poc", C.c_uint32), ("doc", C.c_uint32),
                ("soc", C.c_uint32), ("tid", C.c_uint32), ("l0", C.c_int32 * 5),
                ("l1", C.c_int32 * 5), ("bitdepth", C.c_int32),
                ("bitstream_bitdepth", C.c_int32), ("width", C.c_int32),
                ("height", C.c_int32), ("qp", C.c_int32), ("chroma_format", C.c_int),
                ("color_matrix", C.c_int), ("framerate", C.c_double),
                ("bitstream_framerate", C.c_double), ("conforming", C.c_int32),
                ("profile", C.c_int32)]


class Pic(C.Structure):  # xvc_decoded_picture
    _fields_ = [("bytes", C.c_void_p), ("size", C.c_size_t), ("planes", C.c_void_p * 3),
                ("stride", C.c_int * 3), ("stats", Stats), ("user_data", C.c_int64)]


_vp = C.c_void_p
_P, _Q = C.POINTER(Params), C.POINTER(Pic)


class Api(C.Structure):  # xvc_decoder_api
    _fields_ = [("parameters_create", C.CFUNCTYPE(_P)),
                ("parameters_destroy", C.CFUNCTYPE(C.c_int, _P)),
                ("parameters_set_default", C.CFUNCTYPE(C.c_int, _P)),
                ("parameters_check", C.CFUNCTYPE(C.c_int, _P)),
                ("picture_create", C.CFUNCTYPE(_Q, _vp)),
                ("picture_destroy", C.CFUNCTYPE(C.c_int, _Q)),
                ("decoder_create", C.CFUNCTYPE(_vp, _P)),
                ("decoder_destroy", C.CFUNCTYPE(C.c_int, _vp)),
                ("decoder_update_parameters", C.CFUNCTYPE(C.c_int, _vp, _P)),
                ("decoder_decode_nal", C.CFUNCTYPE(C.c_int, _vp, C.c_char_p, C.c_size_t,
                                                   C.c_int64)),
                ("decoder_get_picture", C.CFUNCTYPE(C.c_int, _vp, _Q)),
                ("decoder_flush", C.CFUNCTYPE(C.c_int, _vp)),
                ("decoder_check_conformance", C.CFUNCTYPE(C.c_int, _vp, C.POINTER(C.c_int))),
                ("error_text", _vp)]


def ref_api():
    lib = C.CDLL(REF_LIB)
    lib.xvc_decoder_api_get.restype = C.POINTER(Api)
    return lib, lib.xvc_decoder_api_get().contents


def decode(api, stream, c):
    """{poc: output bytes} of the reference decoder with output format c."""
    p = api.parameters_create()
    api.parameters_set_default(p)
    q = p.contents
    (q.output_width, q.output_height, q.output_chroma_format, q.output_color_matrix,
     q.output_bitdepth, q.dither) = c
    q.threads = 0
    q.simd_mask = 0
    assert api.parameters_check(p) == 0, c
    d = api.decoder_create(p)
    pic = api.picture_create(d)
    out = {}

    def drain():
        while api.decoder_get_picture(d, pic) == 0:
            r = pic.contents
            out[int(r.stats.poc)] = C.string_at(r.bytes, r.size)

    b, o = bytes(stream), 0
    while o < len(b):
        n = int.from_bytes(b[o:o + 4], "little")
        api.decoder_decode_nal(d, b[o + 4:o + 4 + n], n, 0)
        o += 4 + n
        drain()
    api.decoder_flush(d)
    drain()
    api.picture_destroy(pic)
    api.decoder_destroy(d)
    api.parameters_destroy(p)
    return out


def plane_kinds(c, disp_w, disp_h):
    """CopyToWithResize's choice per plane: 'shift', 'bilinear' or a
    ('resample', filter_x, filter_y) with -1 = upsampling, None = same size."""
    f = om.resolve(dict(zip(CASE_FIELDS, c)), disp_w, disp_h, 10)
    cf = f["chroma_format"]
    kinds = []
    for p in range(1 if cf == 0 else 3):
        sw, sh = (disp_w, disp_h) if p == 0 else (disp_w >> 1, disp_h >> 1)
        dw, dh = om.plane_size(f["width"], f["height"], 3 if cf == 4 else cf, p)
        if (dw, dh) == (sw, sh):
            kinds.append("shift")
        elif p and (dw, dh) == (2 * sw, 2 * sh):
            kinds.append("bilinear")
        else:
            def band(s, d):
                sc = om.scale_of(s, d)
                return -1 if sc < om.SCALE_ONE else (None if sc == om.SCALE_ONE
                                                     else om.filter_from_scale(sc))
            kinds.append(("resample", band(sw, dw), band(sh, dh)))
    return kinds


def check_coverage(cases, disp_w, disp_h):
    want = set(range(-1, 8))
    for comp in (0, 1):
        seen = set()
        for c in cases:
            k = plane_kinds(c, disp_w, disp_h)
            if len(k) > comp and isinstance(k[comp], tuple):
                seen |= {k[comp][1], k[comp][2]} - {None}
        assert want <= seen, ("filter coverage", comp, sorted(want - seen))


def update_manifest(fname):
    mpath = os.path.join(OUT_DIR, "MANIFEST.md5")
    lines = [ln for ln in (open(mpath).read().split("\n") if os.path.exists(mpath) else [])
             if ln.strip() and ln.split()[1] != fname]
    digest = hashlib.md5(open(os.path.join(OUT_DIR, fname), "rb").read()).hexdigest()
    lines.append("%s  %s" % (digest, fname))
    open(mpath, "w").write("\n".join(sorted(lines, key=lambda ln: ln.split()[1])) + "\n")


def generate(clip):
    _, api = ref_api()
    z = np.load(os.path.join(sf.GOLDEN, "stream_%s.npz" % clip))
    info = z["info"].view(sf.STREAM_INFO_DTYPE).reshape(-1)
    disp_w, disp_h = int(info["width"][0]), int(info["height"][0])
    cases = CLIPS[clip]
    if clip == "tiny":
        check_coverage(cases, disp_w, disp_h)
    pocs = [int(p) for p in info["poc"]]
    arrays = {"cases": np.array(cases, np.int32), "poc": np.array(pocs, np.int32),
              "padded": info["padded"].astype(np.uint8)}
    sha = np.zeros((len(cases), len(pocs), 32), np.uint8)
    nbytes = np.zeros(len(cases), np.int64)
    for i, c in enumerate(cases):
        out = decode(api, z["stream"], c)
        assert sorted(out) == sorted(pocs), (c, sorted(out))
        nbytes[i] = len(out[pocs[0]])
        edge = any(k != "shift" for k in plane_kinds(c, disp_w, disp_h))
        for j, poc in enumerate(pocs):
            sha[i, j] = np.frombuffer(hashlib.sha256(out[poc]).digest(), np.uint8)
            if clip == "tiny" and edge and not info["padded"][j] and \
                    len(out[poc]) <= FULL_MAX:
                arrays["full_%d_%d" % (i, j)] = np.frombuffer(out[poc], np.uint8)
        print(clip, i, c, nbytes[i], flush=True)
    arrays["sha256"] = sha
    arrays["nbytes"] = nbytes
    fname = "output_%s.npz" % clip
    os.makedirs(OUT_DIR, exist_ok=True)
    np.savez_compressed(os.path.join(OUT_DIR, fname), **arrays)
    update_manifest(fname)
    print(fname, os.path.getsize(os.path.join(OUT_DIR, fname)), "bytes")


if __name__ == "__main__":
    for clip in sys.argv[1:] or list(CLIPS):
        generate(clip)
