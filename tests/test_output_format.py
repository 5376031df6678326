"""CPU checks of the decoder output formats (Resampler::ConvertTo): the numpy
model (tests/output_model.py) against the reference decoder's recorded output
(tests/golden/output/output_*.npz) and against the reference's own filter functions,
the byte counts of xvcgpu_output_bytes, and the layout of xvcgpu_output_format."""
import ctypes as C
import hashlib
import os
import subprocess
import tempfile

import numpy as np
import pytest

import output_model as om
import stream_fixture as sf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_LIB = os.path.join(ROOT, "oracle", "_ref", "libxvcref.so")
FIELDS = ("width", "height", "chroma_format", "color_matrix", "bitdepth", "dither")


def golden(clip):
    return np.load(os.path.join(sf.GOLDEN, "output", "output_%s.npz" % clip))


def stream(clip):
    z = np.load(os.path.join(sf.GOLDEN, "stream_%s.npz" % clip))
    return z, z["info"].view(sf.STREAM_INFO_DTYPE).reshape(-1)


def fmt_of(row):
    return dict(zip(FIELDS, (int(v) for v in row)))


@pytest.mark.parametrize("clip", ["tiny", "c0"])
def test_model_reproduces_reference_output(clip):
    """Every picture the reference padded: the model's bytes hash to the
    reference decoder's.  The others (tiny's poc 1 and 3): equal wherever no
    filter tap reaches beyond the picture."""
    g = golden(clip)
    z, info = stream(clip)
    n_padded = n_interior = 0
    for i, row in enumerate(g["cases"]):
        fmt = fmt_of(row)
        for j in range(len(info)):
            if "post_%d_0" % j not in z.files:
                continue
            planes = [z["post_%d_%d" % (j, c)] for c in range(3)]
            w, h, bd = (int(info[j][k]) for k in ("width", "height", "bitdepth"))
            out = om.convert_to(planes, bd, w, h, fmt)
            if info["padded"][j]:
                assert hashlib.sha256(out).digest() == g["sha256"][i, j].tobytes(), (i, j, fmt)
                n_padded += 1
            elif "full_%d_%d" % (i, j) in g.files:
                full = g["full_%d_%d" % (i, j)]
                m = om.interior_mask(fmt, w, h, bd, planes[0].shape[1], planes[0].shape[0])
                got = np.frombuffer(out, np.uint8)
                assert len(got) == len(full) == len(m)
                assert np.array_equal(got[m], full[m]), (i, j, fmt)
                n_interior += 1
    assert n_padded >= 3 * len(g["cases"])
    assert clip != "tiny" or n_interior > 20


def test_output_fixture_manifest():
    """tests/golden/output/: every fixture listed in its MANIFEST.md5 with the
    MD5 written at capture time (tools/gen_output_golden.py)."""
    d = os.path.join(sf.GOLDEN, "output")
    listed = {}
    for line in open(os.path.join(d, "MANIFEST.md5")).read().split("\n"):
        if line.strip():
            digest, name = line.split()
            listed[name] = digest
    assert set(listed) == {f for f in os.listdir(d) if f.endswith(".npz")}
    for name, digest in listed.items():
        assert hashlib.md5(open(os.path.join(d, name), "rb").read()).hexdigest() == digest, name


@pytest.mark.parametrize("clip", ["tiny", "c0", "c1"])
def test_output_bytes_match_reference(clip):
    from xvc_amd import api
    g = golden(clip)
    _, info = stream(clip)
    w, h, bd = (int(info[0][k]) for k in ("width", "height", "bitdepth"))
    for row, n in zip(g["cases"], g["nbytes"]):
        f = api.OutputFormat(*(int(v) for v in row)).resolved(w, h, bd)
        assert api.output_bytes(f) == n, f
        assert om.output_bytes(om.resolve(fmt_of(row), w, h, bd)) == n
    for bad in (api.OutputFormat(1, 8, 1, 0, 8), api.OutputFormat(8, 8, 5, 0, 8),
                api.OutputFormat(8, 8, 1, 0, 17), api.OutputFormat(8, 8, 1, 4, 8),
                api.OutputFormat(0, 8, 1, 0, 8)):
        assert api.output_bytes(bad) == 0, bad


def test_output_format_layout():
    from xvc_amd import api
    src = ("#include <stdio.h>\n#include <stddef.h>\n#include \"xvcgpu.h\"\nint main(){"
           "printf(\"%zu %zu %zu %zu %zu %zu %zu\\n\", sizeof(xvcgpu_output_format),"
           "offsetof(xvcgpu_output_format, width), offsetof(xvcgpu_output_format, height),"
           "offsetof(xvcgpu_output_format, chroma_format),"
           "offsetof(xvcgpu_output_format, color_matrix),"
           "offsetof(xvcgpu_output_format, bitdepth), offsetof(xvcgpu_output_format, dither));"
           "return 0;}")
    with tempfile.TemporaryDirectory() as d:
        cpp = os.path.join(d, "l.cc")
        open(cpp, "w").write(src)
        exe = os.path.join(d, "l")
        subprocess.check_call(["g++", "-I", os.path.join(ROOT, "include"), cpp, "-o", exe])
        got = [int(v) for v in subprocess.check_output([exe]).split()]
    O = api.OutputFormat
    assert got == [C.sizeof(O)] + [getattr(O, n).offset for n in FIELDS]


# -- the model's filters against the reference's own instances ----------------

def _ref():
    if not os.path.exists(REF_LIB):
        pytest.skip("oracle/_ref/libxvcref.so is not built (needs the reference sources)")
    return C.CDLL(REF_LIB)


def _ref_fn(lib, name, wide_out):
    sym = {"resample": "_ZN3xvc8resample8ResampleIt%sEEvPhiiliPKhiili",
           "bilinear": "_ZN3xvc8resample16BilinearResampleIt%sEEvPhiiliPKhiili"}[name]
    f = getattr(lib, sym % ("t" if wide_out else "h"))
    f.restype = None
    f.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_long, C.c_int,
                  C.c_void_p, C.c_int, C.c_int, C.c_long, C.c_int]
    return f


def _call(f, plane, dw, dh, src_bd, dst_bd, pad=16):
    """The reference function on `plane` padded by edge replication (what
    YuvPicture::PadBorder leaves around a picture)."""
    h, w = plane.shape
    p = np.ascontiguousarray(np.pad(plane.astype(np.uint16), pad, mode="edge"))
    dt = np.uint16 if dst_bd > 8 else np.uint8
    out = np.zeros((dh, dw), dt)
    f(out.ctypes.data, dw, dh, dw, dst_bd,
      p.ctypes.data + 2 * (pad * p.shape[1] + pad), w, h, p.shape[1], src_bd)
    return out


# destination sizes for a 136 x 72 source: every GetFilterFromScale band
# (136 / d: 1.007 .. 6.8), no resampling, upsampling, odd sizes
DST_W = [135, 120, 100, 75, 60, 50, 40, 20, 136, 272, 137, 3]
DST_H = [71, 64, 50, 40, 36, 30, 24, 10, 72, 144, 73, 2]


@pytest.mark.parametrize("src_bd", [8, 10, 12])
def test_model_resample_equals_reference(src_bd):
    lib = _ref()
    rng = np.random.default_rng(40 + src_bd)
    plane = rng.integers(0, 1 << src_bd, size=(72, 136))
    bands = set()
    for k, (dw, dh) in enumerate(zip(DST_W, DST_H)):
        for dst_bd in (8, 10, 12, 16):
            f = _ref_fn(lib, "resample", dst_bd > 8)
            for w2, h2 in ((dw, dh), (DST_W[-1 - k], dh)):
                exp = _call(f, plane, w2, h2, src_bd, dst_bd)
                got = om.resample(plane, 136, 72, w2, h2, src_bd, dst_bd)
                assert np.array_equal(got, exp), (w2, h2, src_bd, dst_bd)
        sc = om.scale_of(136, dw)
        bands.add(-1 if sc < om.SCALE_ONE else om.filter_from_scale(sc))
    assert bands >= set(range(-1, 8))


@pytest.mark.parametrize("src_bd", [8, 10, 12])
def test_model_bilinear_equals_reference(src_bd):
    lib = _ref()
    rng = np.random.default_rng(50 + src_bd)
    for h, w in ((36, 68), (9, 13), (2, 2)):
        plane = rng.integers(0, 1 << src_bd, size=(h, w))
        for dst_bd in (8, 10, 12, 16):
            if dst_bd - src_bd == 1:
                continue  # >> -1 in the reference
            f = _ref_fn(lib, "bilinear", dst_bd > 8)
            exp = _call(f, plane, 2 * w, 2 * h, src_bd, dst_bd)
            got = om.bilinear(plane, w, h, src_bd, dst_bd)
            assert np.array_equal(got, exp), (w, h, src_bd, dst_bd)
