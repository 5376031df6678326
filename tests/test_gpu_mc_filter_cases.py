"""Every case of the separable motion-compensation filter (csrc/k_interp.h),
enumerated instead of drawn: the four phase cases (copy, horizontal, vertical,
both) at the first, middle and last filter phase, all three components, block
shapes from 4x4 to 64x64 and a block in each picture corner whose vector ClipMv
clips in both directions - through one entry point per (team, output)
instantiation of the routine, each compared bit-exactly with the oracle:

  mc_batch         its own workgroup / Sample copy (k_misc.h), strided destination
  mc_bipred_batch  workgroup / 14-bit int16 (+ AddAvgBi)
  mc_metric_batch  wave / Sample (SAD of the prediction)
  bipred_search    wave / Sample in slabs (64x64: 8 slabs, 8x4: one)
  mc_affine_batch  three equal control vectors: the plain path = workgroup / Sample,
                   strided destination
  mc_lic_batch     the LIC model with above-only, left-only, both, no neighbours
  inter_pred_batch a bi-predicted CU with LIC and one without

The picture content puts 0 and the bit depth's maximum next to each other
(a checkerboard on a random half of the samples, random samples on the rest), so
that filter sums leave the sample range on both sides: the int16 narrowing of the
vertical Sample filter and both ends of the clip are exercised.
"""
import numpy as np
import pytest

import oracle_lib as ol
import oracle_lic

pytestmark = pytest.mark.gpu

PW = PH = 128
BL, BC = 128, 64  # device borders
SHAPES = [(4, 4), (64, 4), (4, 64), (8, 16), (64, 64)]
X0 = Y0 = 32      # the enumerated blocks' position (room for a 64x64 CU and its neighbours)
SAD = 0           # XVC_METRIC_SAD


@pytest.fixture(scope="module")
def gpu():
    from xvc_amd import api
    ctx = api.Context(0)
    yield api, ctx
    ctx.close()


@pytest.fixture(scope="module")
def xo():
    return ol.Lib("xo")


def phases(comp):
    """(fx, fy) of the four cases, k at the first, middle and last phase."""
    out = [(0, 0)]
    for k in ((1, 16, 31) if comp else (1, 8, 15)):
        out += [(k, 0), (0, k), (k, k)]
    return out


def vector(comp, fx, fy, full=(3, -2)):
    """1/16-pel luma vector with full-pel part `full` (in samples of the component)
    and phase (fx, fy) in the component's units (chroma: 1/32)."""
    unit = 32 if comp else 16
    return full[0] * unit + fx, full[1] * unit + fy


def corner_cases():
    """(x, y, mv) of an 8x16 CU in each picture corner, the vector far outside the
    picture towards and away from that corner."""
    out = []
    for x in (0, PW - 8):
        for y in (0, PH - 16):
            for sx in (-1, 1):
                for sy in (-1, 1):
                    out.append((x, y, (sx * 5003, sy * 4999)))
    return out


def harsh_plane(rng, bd, h, w):
    """random samples; on a random half of the positions a 0 / maximum checkerboard"""
    p = rng.integers(0, 1 << bd, (h, w)).astype(np.uint16)
    yy, xx = np.mgrid[0:h, 0:w]
    checker = (((yy + xx) & 1) * ((1 << bd) - 1)).astype(np.uint16)
    half = rng.random((h, w)) < 0.5
    p[half] = checker[half]
    return p


def harsh_planes(rng, bd):
    return [harsh_plane(rng, bd, PH + 2 * BL, PW + 2 * BL),
            harsh_plane(rng, bd, PH // 2 + 2 * BC, PW // 2 + 2 * BC),
            harsh_plane(rng, bd, PH // 2 + 2 * BC, PW // 2 + 2 * BC)]


_PLANES = {}


def planes(bd):
    """The padded planes of the two reference pictures, the original and the
    reconstruction (unpadded) of bit depth bd: made once, never modified."""
    if bd not in _PLANES:
        rng = np.random.default_rng(7100 + bd)
        ref0, ref1, orig = (harsh_planes(rng, bd) for _ in range(3))
        rec = [np.ascontiguousarray(p[b:-b, b:-b]) for p, b in zip(harsh_planes(rng, bd), (BL, BC, BC))]
        _PLANES[bd] = ref0, ref1, orig, rec
    return _PLANES[bd]


def border(comp):
    return BC if comp else BL


def block_of(plane, comp, x, y, w, h):
    cs = 1 if comp else 0
    return plane[y >> cs:(y + h) >> cs, x >> cs:(x + w) >> cs]


# ---- the enumerated jobs and what the oracle says about them ------------------------

def uni_cases():
    """(x, y, w, h, comp, mv): phases x components x shapes, then the corners"""
    out = []
    for (w, h) in SHAPES:
        for comp in range(3):
            out += [(X0, Y0, w, h, comp, vector(comp, fx, fy)) for fx, fy in phases(comp)]
    for (x, y, mv) in corner_cases():
        out += [(x, y, 8, 16, comp, mv) for comp in range(3)]
    return out


def expect_uni(xo, bd, case):
    x, y, w, h, comp, mv = case
    return xo.mc_block(bd, comp, x, y, w, h, mv[0], mv[1], PW, PH, planes(bd)[0][comp], border(comp))


def bi_cases():
    """(x, y, w, h, comp, mv0, mv1): list 0 walks the phases, list 1 walks them shifted"""
    out = []
    for (w, h) in SHAPES:
        for comp in range(3):
            ph = phases(comp)
            for i, (fx, fy) in enumerate(ph):
                gx, gy = ph[(i + 3) % len(ph)]
                out.append((X0, Y0, w, h, comp, vector(comp, fx, fy), vector(comp, gx, gy, (-1, 2))))
    for (x, y, mv) in corner_cases():
        out += [(x, y, 8, 16, comp, mv, (-mv[0], mv[1])) for comp in range(3)]
    return out


def expect_bi(xo, bd, case):
    x, y, w, h, comp, mv0, mv1 = case
    ref0, ref1 = planes(bd)[:2]
    return xo.mc_bipred_block(bd, comp, x, y, w, h, mv0, mv1, PW, PH, ref0[comp], ref1[comp],
                              border(comp))


def metric_cases():
    """(x, y, w, h, mv), luma"""
    out = [(X0, Y0, w, h, vector(0, fx, fy)) for (w, h) in SHAPES for fx, fy in phases(0)]
    return out + [(x, y, 8, 16, mv) for (x, y, mv) in corner_cases()]


def expect_metric(xo, bd, case):
    x, y, w, h, mv = case
    ref0, _, orig, _ = planes(bd)
    return xo.mc_metric(bd, SAD, 32, 16, x, y, w, h, mv, PW, PH, orig[0], ref0[0], BL)


def search_cases():
    """(x, y, w, h, other_mv): the other list's prediction walks the phases"""
    out = [(X0, Y0, w, h, vector(0, fx, fy)) for (w, h) in ((64, 64), (8, 4)) for fx, fy in phases(0)]
    return out + [(x, y, 8, 16, mv) for (x, y, mv) in corner_cases()]


def search_job(case):
    x, y, w, h, other = case
    j = ol.BiBlock()
    j.blk.x, j.blk.y, j.blk.w, j.blk.h = x, y, w, h
    j.blk.mvp_x, j.blk.mvp_y, j.blk.lambda16 = 20, -12, 498000
    j.blk.search_range = 96
    j.other_mv_x, j.other_mv_y = other
    j.boot_mv_x, j.boot_mv_y = 37, -21
    return j


def expect_search(xo, bd, case):
    ref0, ref1, orig, _ = planes(bd)
    return xo.bipred_search(bd, search_job(case), PW, PH, orig[0], ref0[0], ref1[0], BL)


def expect_affine(xo, bd, case):
    x, y, w, h, comp, mv = case
    return xo.mc_affine_block(bd, comp, x, y, w, h, [mv] * 3, PW, PH, planes(bd)[0][comp],
                              border(comp))


def lic_job(x, y, w, h, comp, mv, neighbors):
    j = np.zeros(1, oracle_lic.LIC_DTYPE)[0]
    j["x"], j["y"], j["w"], j["h"], j["comp"], j["neighbors"] = x, y, w, h, comp, neighbors
    j["mv_x"], j["mv_y"] = mv
    # the neighbouring CUs: 8 wide above, 8 high left, far enough inside for any vector here
    j["above_x"], j["above_y"], j["left_x"], j["left_y"] = x, y - 8, x - 8, y
    return j


BOTH = oracle_lic.HAS_ABOVE | oracle_lic.HAS_LEFT


def inside_neighbors(x, y):
    """the neighbours of a CU at (x, y) that lie inside the picture"""
    return (oracle_lic.HAS_ABOVE if y > 0 else 0) | (oracle_lic.HAS_LEFT if x > 0 else 0)


def lic_cases():
    """LIC jobs: neighbours x shapes x components x phases, then the corners (the clipped
    vector goes into the model) with the neighbours the picture has there"""
    out = []
    for nb in (oracle_lic.HAS_ABOVE, oracle_lic.HAS_LEFT, BOTH, 0):
        for (w, h) in SHAPES:
            for comp in range(3):
                out += [lic_job(X0, Y0, w, h, comp, vector(comp, fx, fy), nb)
                        for fx, fy in phases(comp)]
    for (x, y, mv) in corner_cases():
        out += [lic_job(x, y, 8, 16, comp, mv, inside_neighbors(x, y)) for comp in range(3)]
    return out


def expect_lic(xo, bd, job, ref=0):
    ref_planes, rec = planes(bd)[ref], planes(bd)[3]
    return oracle_lic.xo_mc_lic(xo, bd, job, PW, PH, ref_planes, [BL, BC, BC], rec)


def inter_cases():
    """(x, y, w, h, comp, mv0, mv1, lic, neighbors): bi-predicted CUs, with and without
    LIC: phases x components x shapes, then the corners"""
    out = []
    for lic in (0, 1):
        for (w, h) in SHAPES:
            for comp in range(3):
                ph = phases(comp)
                for i, (fx, fy) in enumerate(ph):
                    gx, gy = ph[(i + 3) % len(ph)]
                    out.append((X0, Y0, w, h, comp, vector(comp, fx, fy),
                                vector(comp, gx, gy, (-1, 2)), lic, BOTH))
        for (x, y, mv) in corner_cases():
            out += [(x, y, 8, 16, comp, mv, (-mv[0], mv[1]), lic, inside_neighbors(x, y))
                    for comp in range(3)]
    return out


def expect_inter(xo, bd, case):
    """MotionCompensation of a bi-predicted CU (inter_prediction.cc:710-738): without LIC
    the two lists at 14 bit; with LIC each list's compensated Sample prediction taken to
    14 bit by FilterCopyBipred; AddAvgBi."""
    x, y, w, h, comp, mv0, mv1, lic, neighbors = case
    if not lic:
        return expect_bi(xo, bd, (x, y, w, h, comp, mv0, mv1))
    p16 = []
    for l, mv in enumerate((mv0, mv1)):
        job = lic_job(x, y, w, h, comp, mv, neighbors)
        smp = np.ascontiguousarray(block_of(expect_lic(xo, bd, job, ref=l), comp, x, y, w, h))
        p16.append(xo.mc_uni(bd, comp != 0, smp.shape[1], smp.shape[0], 0, 0, smp, 0, 0, bipred=True))
    return xo.add_avg(bd, p16[0], p16[1])


# ---- the device against them ---------------------------------------------------------

class Pictures:
    def __init__(self, ctx, bd):
        ref0, ref1, orig, rec = planes(bd)
        self.R0, self.R1, self.O, self.C, self.P = (ctx.picture(PW, PH, bd) for _ in range(5))
        self.R0.upload(ref0, BL)
        self.R1.upload(ref1, BL)
        self.O.upload(orig, BL)
        self.C.upload(rec)

    def destroy(self):
        for p in (self.R0, self.R1, self.O, self.C, self.P):
            p.destroy()


@pytest.fixture(scope="module", params=[8, 10, 12])
def pics(request, gpu):
    p = Pictures(gpu[1], request.param)
    yield request.param, p
    p.destroy()


def test_mc_batch_cases(gpu, xo, pics):
    api, ctx = gpu
    bd, p = pics
    for case in uni_cases():
        x, y, w, h, comp, mv = case
        ctx.mc_batch(p.R0, p.P, np.array([(x, y, w, h, comp, 0, *mv)], api.MC_DTYPE))
        got = block_of(p.P.download()[comp], comp, x, y, w, h)
        assert np.array_equal(got, expect_uni(xo, bd, case)), case


def test_mc_bipred_batch_cases(gpu, xo, pics):
    api, ctx = gpu
    bd, p = pics
    for case in bi_cases():
        x, y, w, h, comp, mv0, mv1 = case
        ctx.mc_bipred_batch(p.R0, p.R1, p.P, np.array([(x, y, w, h, comp, 0, *mv0, *mv1)], api.MCBI_DTYPE))
        got = block_of(p.P.download()[comp], comp, x, y, w, h)
        assert np.array_equal(got, expect_bi(xo, bd, case)), case


def test_mc_metric_batch_cases(gpu, xo, pics):
    api, ctx = gpu
    bd, p = pics
    cases = metric_cases()
    cands = np.array([(x, y, w, h, SAD, 32, *mv) for (x, y, w, h, mv) in cases], api.MCM_DTYPE)
    got = ctx.mc_metric_batch(p.O, p.R0, cands, strength=16)
    for i, case in enumerate(cases):
        assert int(got[i]) == expect_metric(xo, bd, case), case


def test_bipred_search_cases(gpu, xo, pics):
    api, ctx = gpu
    bd, p = pics
    cases = search_cases()
    jobs = np.zeros(len(cases), api.BI_DTYPE)
    for j, case in zip(jobs, cases):
        s = search_job(case)
        for name in ol.ME_DTYPE.names:
            j["blk"][name] = getattr(s.blk, name)
        for name in ("other_mv_x", "other_mv_y", "boot_mv_x", "boot_mv_y"):
            j[name] = getattr(s, name)
    res = ctx.bipred_search(p.O, p.R0, p.R1, jobs)
    for i, case in enumerate(cases):
        got = ((int(res[i]["mv_x"]), int(res[i]["mv_y"])), int(res[i]["subpel_dist"]))
        assert got == expect_search(xo, bd, case), case


def test_mc_affine_batch_plain_cases(gpu, xo, pics):
    api, ctx = gpu
    bd, p = pics
    for case in uni_cases():
        x, y, w, h, comp, mv = case
        ctx.mc_affine_batch(p.R0, p.P, np.array([(x, y, w, h, comp, 0, [mv] * 3)], api.MCAFF_DTYPE))
        got = block_of(p.P.download()[comp], comp, x, y, w, h)
        assert np.array_equal(got, expect_affine(xo, bd, case)), case


def test_mc_lic_batch_cases(gpu, xo, pics):
    api, ctx = gpu
    bd, p = pics
    for job in lic_cases():
        ctx.mc_lic_batch(p.R0, p.C, p.P, np.array([job], api.LIC_DTYPE))
        comp = int(job["comp"])
        where = (comp, int(job["x"]), int(job["y"]), int(job["w"]), int(job["h"]))
        got = block_of(p.P.download()[comp], *where)
        assert np.array_equal(got, block_of(expect_lic(xo, bd, job), *where)), job


def test_inter_pred_batch_bi_cases(gpu, xo, pics):
    api, ctx = gpu
    bd, p = pics
    for case in inter_cases():
        x, y, w, h, comp, mv0, mv1, lic, neighbors = case
        j = np.zeros(1, api.INTER_DTYPE)
        j["x"], j["y"], j["w"], j["h"], j["comp"] = x, y, w, h, comp
        j["ref"] = [0, 1]
        j["mv"][0, 0, 0], j["mv"][0, 1, 0] = mv0, mv1
        if lic:
            nb = lic_job(x, y, w, h, comp, mv0, neighbors)
            j["flags"] = api.INTER_LIC
            for name in ("neighbors", "above_x", "above_y", "left_x", "left_y"):
                j[name] = nb[name]
        ctx.inter_pred_batch([p.R0, p.R1], p.C, p.P, j)
        got = block_of(p.P.download()[comp], comp, x, y, w, h)
        assert np.array_equal(got, expect_inter(xo, bd, case)), case
