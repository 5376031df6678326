"""The device's two deblocking implementations - the two-pass kernels (k_deblock.h) and the
fused tail (k_tail.h) - on the directed cases of tests/deblock_cases.py: QPs 0..63, offsets
-32..31, every table index clip, saturation at both ends, the strong filter's clip, all
outcomes of the boundary strength.  Bit exact against the oracle, which
tests/test_deblock_model.py pins to the counting model and to the reference on the same
cases (and shows that each of those classes is among them)."""
import functools

import numpy as np
import pytest

import deblock_cases as dc
import oracle_lib as ol

pytestmark = pytest.mark.gpu

BL, BC = 128, 64  # device borders
BORDERS = [BL, BC, BC]
NO_BORDER = [0, 0, 0]


@pytest.fixture(scope="module")
def gpu():
    from xvc_amd import api
    ctx = api.Context(0)
    yield api, ctx
    ctx.close()


@pytest.fixture(scope="module")
def xo():
    return ol.Lib("xo")


@functools.lru_cache(maxsize=None)
def _expected(xo, family, sub):
    """The oracle's filtered planes (no border) of the family's cases, computed once."""
    out = []
    for c in dc.cases(family):
        planes = [p.copy() for p in c["planes"]]
        xo.deblock(c["bd"], c["pw"], c["ph"], c["bipred"], c["beta"], c["tc"], sub, c["cus"],
                   c["cu_map"], planes, NO_BORDER)
        for p in planes:
            p.setflags(write=False)
        out.append(planes)
    return out


def cases_of(xo, family, sub, bd):
    got = [(c, e) for c, e in zip(dc.cases(family), _expected(xo, family, sub)) if c["bd"] == bd]
    assert got
    return got


def args(c):
    return c["bipred"], c["beta"], c["tc"]


def check_picture(pic, exp, what):
    got = pic.download()
    for k in range(3):
        assert np.array_equal(got[k], exp[k]), what + (k,)


@pytest.mark.parametrize("bd", dc.DEPTHS)
@pytest.mark.parametrize("family,sub", [("g4", 4), ("g8", 4), ("g8", 8)])
def test_deblock(gpu, xo, bd, family, sub):
    api, ctx = gpu
    changed = 0
    for c, exp in cases_of(xo, family, sub, bd):
        R = ctx.picture(c["pw"], c["ph"], bd)
        R.upload(dc.padded(c, BORDERS), BL)
        ctx.deblock(R, c["cus"], c["cu_map"], *args(c), sub)
        check_picture(R, exp, (c["name"], sub))
        changed += sum(int((e != p).sum()) for e, p in zip(exp, c["planes"]))
        R.destroy()
    assert changed > 0


@pytest.mark.parametrize("bd", dc.DEPTHS)
def test_tail(gpu, xo, bd):
    """xvcgpu_deblock_pad_ssd on the 8-grid cases - the low-delay-shaped ones among them:
    the destination with its border against the oracle's deblocking + PadBorder, whatever
    the source's border holds; the SSD at both shifts; the form without an original."""
    api, ctx = gpu
    rng = np.random.default_rng(8800 + bd)
    todo = cases_of(xo, "g8", 4, bd)
    assert bd == 9 or any(c["recipe"] == "lowdelay" for c, _ in todo)
    for c, filtered in todo:
        pw, ph = c["pw"], c["ph"]
        src = dc.padded(c, BORDERS, rng)
        exp = dc.padded(dict(c, planes=filtered), BORDERS)
        xo.pad_border(pw, ph, exp, BORDERS)
        orig = np.clip(filtered[0].astype(np.int64) + rng.integers(-7, 8, (ph, pw)), 0,
                       (1 << bd) - 1).astype(np.uint16)
        S, D, O = (ctx.picture(pw, ph, bd) for _ in range(3))
        S.upload(src, BL)
        O.upload(dc.padded(dict(c, planes=[orig] + list(c["planes"][1:])), BORDERS, rng), BL)
        for sbd in (8, bd, None):       # None: no original, no SSD
            D.upload([np.zeros_like(p) for p in src], BL)
            ssd = ctx.deblock_pad_ssd(S, D, O if sbd else None, c["cus"], c["cu_map"], *args(c),
                                      sbd or 8)
            got = D.download(BL)
            for k in range(3):
                assert np.array_equal(got[k], exp[k]), (c["name"], sbd, k)
            if sbd:
                e = xo.picture_ssd(sbd, orig, np.ascontiguousarray(filtered[0]))
                assert ssd == e, (c["name"], sbd, ssd, e)
            else:
                assert ssd is None
        for p in (S, D, O):
            p.destroy()


@pytest.mark.parametrize("bd", dc.DEPTHS)
def test_deblock_rows_split(gpu, xo, bd):
    """Each pass in two calls of xvcgpu_deblock_rows, split at a row off the 8 grid (the
    rule for the head of a chain of horizontal edges depends on y_begin), equals the
    whole-picture call."""
    api, ctx = gpu
    for c, exp in cases_of(xo, "g4", 4, bd):
        ph = c["ph"]
        R = ctx.picture(c["pw"], ph, bd)
        R.upload(dc.padded(c, BORDERS), BL)
        cus, cmap = np.ascontiguousarray(c["cus"]), np.ascontiguousarray(c["cu_map"], np.int32)
        dcu, dm = ctx.buffer(cus), ctx.buffer(cmap)
        for pass_, ys in ((0, ph // 2), (1, ph // 2 - 8)):
            assert ys % 8 == 4
            for y0, y1 in ((0, ys), (ys, ph)):
                ctx.deblock_rows_dev(R, dcu.ptr, len(cus), dm.ptr, cmap.shape[1], pass_, y0, y1,
                                     *args(c), 4)
        ctx.sync()
        check_picture(R, exp, (c["name"], "rows"))
        for b in (dcu, dm):
            b.free()
        R.destroy()


@pytest.mark.parametrize("bd", dc.DEPTHS)
@pytest.mark.parametrize("family,sub", [("g4", 4), ("g8", 8)])
def test_deblock_tree_masks(gpu, xo, bd, family, sub):
    """xvcgpu_deblock_tree: luma alone (mask 1) then chroma alone (mask 2) is mask 3, the
    whole filter; after mask 1 the chroma planes are untouched."""
    api, ctx = gpu
    for c, exp in cases_of(xo, family, sub, bd):
        cus, cmap = np.ascontiguousarray(c["cus"]), np.ascontiguousarray(c["cu_map"], np.int32)
        dcu, dm = ctx.buffer(cus), ctx.buffer(cmap)
        pics = []
        for masks in ((1, 2), (3,)):
            R = ctx.picture(c["pw"], c["ph"], bd)
            R.upload(dc.padded(c, BORDERS), BL)
            for mask in masks:
                ctx._check(ctx.lib.xvcgpu_deblock_tree(ctx.h, R.h_pic, dcu.ptr, len(cus), dm.ptr,
                                                       cmap.shape[1], *args(c), sub, mask))
                ctx.sync()
                if mask == 1:
                    check_picture(R, [exp[0], c["planes"][1], c["planes"][2]], (c["name"], mask))
            check_picture(R, exp, (c["name"], masks))
            pics.append(R)
        for b in (dcu, dm):
            b.free()
        for R in pics:
            R.destroy()
