"""The frame pass on a real CU partition and the search plan behind it, on the GPU:
the plan's counts against a numpy classification, xvcgpu_me_search_planned against
xvcgpu_me_search_sized record for record, and pipeline.FramePass(partition=...) against
the oracle's frame pass (pinned on partitions by tests/test_partition.py), and the C++
host program on a partition file."""
import os
import numpy as np
import pytest

import oracle_lib as ol
from partition_fixture import luma_partition, picture_size

pytestmark = pytest.mark.gpu

BL, BC = 128, 64  # device borders


@pytest.fixture(scope="module")
def gpu():
    from xvc_amd import api
    ctx = api.Context(0)
    yield api, ctx
    ctx.close()


@pytest.fixture(scope="module")
def xo():
    return ol.Lib("xo")


def pad_planes(planes):
    return [np.ascontiguousarray(np.pad(p, BL if c == 0 else BC, mode="edge"))
            for c, p in enumerate(planes)]


def numpy_bins(api, me, max_block_size):
    """The bin of every job, from the rules of include/xvcgpu_types.h."""
    w, h = me["w"].astype(int), me["h"].astype(int)
    mx = np.maximum(w, h)
    ml = 64 if max_block_size > 32 else (32 if max_block_size > 16 else 16)
    pow2 = ((w & (w - 1)) == 0) & ((h & (h - 1)) == 0)
    valid = pow2 & (w >= 4) & (h >= 4) & (w <= 64) & (h <= 64) & (mx <= ml)
    lic = (me["fullpel_mv"].astype(int) & 2) != 0
    cls = np.where(mx <= 16, 0, np.where(mx <= 32, 1, 2))
    names = list(api.ME_PLAN_BIN_NAMES)
    b = np.full(len(me), names.index("other16"))
    b[(w == 16) & (h == 16)] = names.index("16x16")
    b[(w == 16) & (h == 8)] = names.index("16x8")
    b[(w == 8) & (h == 8)] = names.index("8x8")
    b[cls == 1] = names.index("c32")
    b[(cls == 2) & (w >= 8) & (h >= 8)] = names.index("c64_team")
    b[(cls == 2) & ~((w >= 8) & (h >= 8))] = names.index("c64_wave")
    b[lic] = names.index("lic16") + cls[lic]
    b[~valid] = names.index("unsupported")
    return b


def me_list(parts, qp=32, search_range=96):
    from xvc_amd import api, pipeline
    me = np.zeros(len(parts), api.ME_DTYPE)
    for i, (x, y, w, h) in enumerate(parts):
        me[i]["x"], me[i]["y"], me[i]["w"], me[i]["h"] = x, y, w, h
    me["depth_nonzero"] = 1
    me["lambda16"] = pipeline.lambda16_for_qp(qp)
    me["search_range"] = search_range
    return me


def grid(w, h, cw, ch):
    return [(x, y, cw, ch) for y in range(0, h - ch + 1, ch) for x in range(0, w - cw + 1, cw)]


def test_plan_counts(gpu):
    """The counts per bin.  The lists themselves (every job once, list order inside a bin)
    are not read back - the C-ABI does not expose them -: that every job is in exactly one
    list of the right bin is what test_planned_search_equals_sized shows (a job missing
    from its list keeps the poisoned record, one in a wrong list gets another instance's
    answer or none), and the order inside a bin does not change a result."""
    api, ctx = gpu
    from xvc_amd import pipeline
    w, h = picture_size("c1x", 3)
    desc = pipeline.FrameDescriptors(w, h, 32, partition=luma_partition("c1x", 3))
    lists = {"c1x": (desc.me, 64), "c1x as 32": (desc.me, 32), "c1x as 16": (desc.me, 16)}
    odd = desc.me[:300].copy()
    odd["w"][5], odd["h"][7] = 12, 48           # sizes the search does not have
    odd["fullpel_mv"][10:40] |= 2               # XVC_ME_USE_LIC
    lists["odd"] = (odd, 64)
    lists["one"] = (desc.me[:1], 64)
    big = np.tile(desc.me, 20)[:30001]          # more than a few steps of the plan kernel
    lists["big"] = (big, 64)
    for name, (me, mbs) in lists.items():
        d_me = ctx.buffer(me)
        plan = ctx.me_plan(d_me.ptr, len(me), mbs)
        expect = np.bincount(numpy_bins(api, me, mbs), minlength=api.ME_PLAN_BINS)
        assert np.array_equal(plan.counts, expect), (name, plan.counts, expect)
        assert int(plan.counts.sum()) == len(me)
        if name == "c1x":   # the input is chosen so that these hold
            c = dict(zip(api.ME_PLAN_BIN_NAMES, plan.counts.tolist()))
            for k in ("16x16", "16x8", "8x8", "other16", "c32"):
                assert c[k] > 0, c
            assert c["c64_team"] > 0 or c["c64_wave"] > 0, c
        plan.destroy()
        d_me.free()
    empty = ctx.me_plan(None, 0, 64)
    assert int(empty.counts.sum()) == 0
    empty.destroy()


def _search_lists(w, h):
    """name -> (descriptors, max_block_size, LIC jobs announced)"""
    from xvc_amd import pipeline
    real = pipeline.FrameDescriptors(w, h, 32, partition=luma_partition("c1x", 3)).me
    rng = np.random.default_rng(5)
    for f in ("mvp_x", "mvp_y"):        # predictors off zero: the sub-pel cost prices them
        real[f] = rng.integers(-64, 65, len(real))
    real["prev_x"], real["prev_y"] = rng.integers(-3, 4, len(real)), rng.integers(-3, 4, len(real))
    odd = real[:400].copy()
    odd["w"][3], odd["h"][3] = 12, 16                   # a 12x16 job: unsupported record
    odd["w"][9], odd["h"][9] = 16, 48
    # an out-of-picture job: xvcgpu_me_search_sized has no picture test (the vectors are
    # clipped to the padded picture), so there is a searched record for it, and the same one
    odd["x"][11], odd["y"][11], odd["w"][11], odd["h"][11] = w + 16, 8, 16, 16
    lic = real[200:700].copy()
    lic["fullpel_mv"][::3] |= 2                         # XVC_ME_USE_LIC, every class
    fp = real[:300].copy()
    fp["fullpel_mv"][::2] |= 1                          # XVC_ME_FULLPEL_MV
    return {
        "real": (real, 64, False), "real as 32": (real, 32, False), "odd": (odd, 64, False),
        "lic": (lic, 64, True), "lic not announced": (lic, 64, False), "fullpel mv": (fp, 64, False),
        "16x16": (me_list(grid(w, h, 16, 16)[:2000]), 16, False),
        "8x8": (me_list(grid(w, h, 8, 8)[:3000]), 16, False),
        "16x8": (me_list(grid(w, h, 16, 8)[:500]), 64, False),
        "one": (real[:1].copy(), 64, False),
    }


# (the 10-bit cases keep the ids they had before there was a depth to choose)
@pytest.mark.parametrize("phases,bd", [
    pytest.param(ph, bd, id=ph if bd == 10 else "%s-bd%d" % (ph, bd))
    for bd in (10, 12) for ph in ("both", "fullpel", "subpel")])
def test_planned_search_equals_sized(gpu, phases, bd):
    """bd 12: the 64 class's sub-pel leaves the four-wave team kernel for the wave
    instance (the packed SATD sweep holds bd <= 10)."""
    api, ctx = gpu
    from xvc_amd import synth
    w, h = picture_size("c1x", 3)
    clip = synth.SyntheticClip(w, h, bd)
    O, R = ctx.picture(w, h, bd), ctx.picture(w, h, bd)
    O.upload(pad_planes(clip.frame(1)), BL)
    R.upload(pad_planes(clip.frame(0)), BL)
    flags = {"both": api.ME_FULLPEL | api.ME_SUBPEL, "fullpel": api.ME_FULLPEL,
             "subpel": api.ME_SUBPEL}[phases]
    item = api.MERES_DTYPE.itemsize
    for name, (me, mbs, lic) in _search_lists(w, h).items():
        n = len(me)
        fl = flags | (api.ME_LIC_JOBS if lic else 0)
        d_me = ctx.buffer(me)
        # sub-pel only starts from the records' full-pel vectors: the same ones for both
        start = np.zeros(n, api.MERES_DTYPE)
        rng = np.random.default_rng(9)
        start["fullpel_x"], start["fullpel_y"] = rng.integers(-8, 9, n), rng.integers(-8, 9, n)
        start["fullpel_cost"], start["subpel_dist"] = 0x55555555, 0x66666666
        d_a, d_b = ctx.buffer(start), ctx.buffer(start)
        ctx.me_search_dev(O, R, fl, d_me.ptr, n, d_a.ptr, mbs)
        plan = ctx.me_plan(d_me.ptr, n, mbs)
        ctx.me_search_planned(O, R, fl, plan, d_b.ptr)
        ctx.sync()
        a, b = d_a.to_array(api.MERES_DTYPE, n), d_b.to_array(api.MERES_DTYPE, n)
        bad = np.nonzero(a != b)[0]
        assert len(bad) == 0, (name, phases, bad[:8], a[bad[:4]], b[bad[:4]], me[bad[:4]])
        if name == "odd":
            assert a["subpel_dist"][3] == 0xffffffff and a["fullpel_cost"][3] == 0xffffffff
        assert item * n == a.nbytes
        plan.destroy()
        for d in (d_me, d_a, d_b):
            d.free()
    # n = 0: nothing to do, no error
    plan = ctx.me_plan(None, 0, 64)
    ctx.me_search_planned(O, R, flags, plan, None)
    plan.destroy()
    O.destroy()
    R.destroy()


BIN_SHAPES = {
    "16x16": [(16, 16)], "16x8": [(16, 8)], "8x8": [(8, 8)],
    "other16": [(4, 4), (8, 4), (4, 16), (8, 16), (16, 4)],
    "c32": [(32, 32), (32, 8), (16, 32)],
    "c64_team": [(64, 64), (64, 8), (32, 64)],
    "c64_wave": [(64, 4), (4, 64)],
}
BIN_SHAPES["lic16"] = [s for k in ("16x16", "16x8", "8x8", "other16") for s in BIN_SHAPES[k]]
BIN_SHAPES["lic32"] = BIN_SHAPES["c32"]
BIN_SHAPES["lic64"] = BIN_SHAPES["c64_team"] + BIN_SHAPES["c64_wave"]
BIN_JOBS = 48       # at most, per list
ME_USE_LIC = 2      # XVC_ME_USE_LIC (include/xvc_inter_bits.h; xvc_amd.api has no name for it)


def _one_bin_list(name, pw, ph):
    """(descriptors, the bin they fall into, LIC jobs announced): jobs of one plan bin only,
    spread over the picture, mvp = prev = 0, range 96.  "unsupported": 12x16 jobs and LIC
    jobs of every class that the search is not told about."""
    lic = name.startswith("lic")
    shapes = BIN_SHAPES["lic16"] + BIN_SHAPES["lic32"] + BIN_SHAPES["lic64"] + [(12, 16)] * 6 \
        if name == "unsupported" else BIN_SHAPES[name]
    n = max(len(shapes), BIN_JOBS // len(shapes) * len(shapes))
    parts = []
    for i in range(n):
        w, h = shapes[i % len(shapes)]
        parts.append(((i * 44) % (pw - w + 1) & ~3, (i * 28) % (ph - h + 1) & ~3, w, h))
    me = me_list(parts)
    if lic or name == "unsupported":
        me["fullpel_mv"] = np.where(me["w"] == 12, 0, ME_USE_LIC)
    return me, name, lic


@pytest.fixture(scope="module", params=[10, 12])
def one_bin_case(request, xo):
    """The pictures and, per bin, its list with the oracle's answers (computed once)."""
    import helpers
    from test_gpu_parity import to_me_struct
    bd, pw, ph = request.param, 320, 192
    orig, ref = helpers.make_pics(np.random.default_rng(4100 + bd), bd, pw, ph, BL, (40, 26))
    lists = []
    for name in list(BIN_SHAPES) + ["unsupported"]:
        me, bin_name, lic = _one_bin_list(name, pw, ph)
        want = None
        if name != "unsupported":
            want = []
            for b in me:
                s = to_me_struct(b)
                (fx, fy), cost = xo.tz_search(bd, s, pw, ph, orig, ref, BL)
                (sx, sy), sd = xo.subpel_search(bd, s, pw, ph, orig, ref, BL, (fx, fy))
                want.append((fx, fy, cost, sx, sy, sd))
            want = np.array(want, np.int64)
            # the step-5 grid and the record write are on the tested path: an answer 8 or
            # more samples from the start (mvp = prev = 0) in some component
            if not lic:
                assert (np.abs(want[:, :2]).max(axis=1) >= 8).any(), name
        lists.append((me, bin_name, lic, want))
    return bd, pw, ph, orig, ref, lists


def test_every_bin_alone(gpu, one_bin_case):
    """Every plan bin as the only one of its search - so it is the launch that keeps the
    straggler-first record -, every phase mask: the planned search twice with one plan (the
    second call rotates by the record the first one wrote) and the sized search give the
    same records; fused, they are the oracle's job by job; a job no instance takes reads
    0xffffffff in both fields."""
    api, ctx = gpu
    bd, pw, ph, orig, ref, lists = one_bin_case
    O, R = ctx.picture(pw, ph, bd), ctx.picture(pw, ph, bd)
    O.upload([orig, None, None], BL)
    R.upload([ref, None, None], BL)
    names = list(api.ME_PLAN_BIN_NAMES)
    for me, bin_name, lic, want in lists:
        n = len(me)
        assert n <= BIN_JOBS
        d_me = ctx.buffer(me)
        plan = ctx.me_plan(d_me.ptr, n, 64)
        if want is None:    # (the plan bins a LIC job as such: who was told is the search's)
            assert plan.counts[names.index("lic16"):].sum() == n and \
                plan.counts[names.index("unsupported")] > 0, plan.counts
        else:
            assert plan.counts[names.index(bin_name)] == n, (bin_name, plan.counts)
        start = np.zeros(n, api.MERES_DTYPE)
        rng = np.random.default_rng(11)
        start["fullpel_x"], start["fullpel_y"] = rng.integers(-8, 9, n), rng.integers(-8, 9, n)
        start["fullpel_cost"], start["subpel_dist"] = 0x55555555, 0x66666666
        for flags in (api.ME_FULLPEL | api.ME_SUBPEL, api.ME_FULLPEL, api.ME_SUBPEL):
            fl = flags | (api.ME_LIC_JOBS if lic else 0)
            got = []
            for form in ("planned", "planned again", "sized"):
                d_r = ctx.buffer(start)
                if form == "sized":
                    ctx.me_search_dev(O, R, fl, d_me.ptr, n, d_r.ptr, 64)
                else:
                    ctx.me_search_planned(O, R, fl, plan, d_r.ptr)
                ctx.sync()
                got.append(d_r.to_array(api.MERES_DTYPE, n))
                d_r.free()
            for form, g in zip(("planned again", "sized"), got[1:]):
                bad = np.nonzero(g != got[0])[0]
                assert len(bad) == 0, (bin_name, flags, form, bad[:8], got[0][bad[:4]], g[bad[:4]])
            g = got[0]
            if want is None:
                assert (g["fullpel_cost"] == 0xffffffff).all(), (bin_name, flags)
                assert (g["subpel_dist"] == 0xffffffff).all(), (bin_name, flags)
            elif flags == api.ME_FULLPEL | api.ME_SUBPEL:
                cols = ("fullpel_x", "fullpel_y", "fullpel_cost", "mv_x", "mv_y", "subpel_dist")
                have = np.stack([g[c].astype(np.int64) for c in cols], axis=1)
                bad = np.nonzero((have != want).any(axis=1))[0]
                assert len(bad) == 0, (bin_name, bad[:8], have[bad[:4]], want[bad[:4]], me[bad[:4]])
        plan.destroy()
        d_me.free()
    O.destroy()
    R.destroy()


def _run_partition_pass(api, ctx, xo, name, pic, bd, qp, rdoq, check_steps=False):
    import oracle_frame
    from xvc_amd import pipeline, synth
    w, h = picture_size(name, pic)
    parts = luma_partition(name, pic)
    clip = synth.SyntheticClip(w, h, bd)
    ref_host, orig_host = pad_planes(clip.frame(0)), pad_planes(clip.frame(1))
    O, R, Rec, Rec2 = (ctx.picture(w, h, bd) for _ in range(4))
    O.upload(orig_host, BL)
    R.upload(ref_host, BL)
    fp = pipeline.FramePass(ctx, w, h, bd, qp=qp, partition=parts, rdoq=rdoq)
    assert fp.plan is not None and int(fp.plan.counts.sum()) == len(parts)
    fp.run(O, R, Rec)
    ctx.sync()
    res, nnz, cus, ssd = fp.results()
    e_rec, e_res, e_nnz, e_cus, e_ssd = oracle_frame.frame_pass(fp.desc, bd, orig_host, ref_host,
                                                                BL, lib=xo)
    assert np.array_equal(res, e_res), np.nonzero(res != e_res)[0][:8]
    assert np.array_equal(nnz, e_nnz), np.nonzero(nnz != e_nnz)[0][:8]
    assert cus.tobytes() == e_cus.tobytes()
    got = Rec.download(BL)
    for c in range(3):
        assert np.array_equal(got[c], e_rec[c]), c
    assert (int(ssd[0]), int(ssd[1])) == e_ssd
    assert int(np.count_nonzero(nnz)) > 0
    if check_steps:
        # the launches one by one are the pass
        for _, fn in fp.kernel_steps(O, R, Rec2):
            fn()
        ctx.sync()
        res2, nnz2, cus2, ssd2 = fp.results()
        assert res2.tobytes() == res.tobytes() and nnz2.tobytes() == nnz.tobytes()
        assert cus2.tobytes() == cus.tobytes() and ssd2.tobytes() == ssd.tobytes()
        got2 = Rec2.download(BL)
        for c in range(3):
            assert np.array_equal(got2[c], got[c]), c
        # the decoder's side reproduces the reconstruction from the kept levels
        enc = pipeline.FramePass(ctx, w, h, bd, qp=qp, partition=parts, rdoq=rdoq,
                                 keep_levels=True)
        dec = pipeline.DecodePass(ctx, enc.desc, bd)
        enc.run(O, R, Rec2)
        dec.run(R, Rec, enc.d_res.ptr, enc.d_levels.ptr, enc.d_level_off.ptr, enc.d_nnz.ptr)
        ctx.sync()
        a, b = Rec.download(BL), Rec2.download(BL)
        for c in range(3):
            assert np.array_equal(a[c], e_rec[c]), c
            assert np.array_equal(b[c], e_rec[c]), c
        enc.destroy()
        dec.destroy()
    fp.destroy()
    for p in (O, R, Rec, Rec2):
        p.destroy()


@pytest.mark.parametrize("rdoq", [False, True])
@pytest.mark.parametrize("bd,qp", [(10, 32), (8, 27), (12, 32)])
@pytest.mark.parametrize("name,pic", [("tiny", 1), ("tiny", 3), ("c0", 1), ("c0q22", 1)])
def test_partition_pass_matches_oracle(gpu, xo, name, pic, bd, qp, rdoq):
    api, ctx = gpu
    _run_partition_pass(api, ctx, xo, name, pic, bd, qp, rdoq, check_steps=True)


@pytest.mark.parametrize("name,pic", [("c1", 1), ("c1x", 3)])
def test_partition_pass_1080p_matches_oracle(gpu, xo, name, pic):
    api, ctx = gpu
    _run_partition_pass(api, ctx, xo, name, pic, 10, 32, True, check_steps=True)


def test_grid_partition_pass_equals_grid_pass(gpu):
    """A partition that is the 16x16 grid takes the fused forms and gives the grid pass's
    bytes; a plan of another list is refused."""
    api, ctx = gpu
    from xvc_amd import pipeline, synth
    w, h, bd = 352, 288, 10
    clip = synth.SyntheticClip(w, h, bd)
    O, R, A, B = (ctx.picture(w, h, bd) for _ in range(4))
    O.upload(pad_planes(clip.frame(1)), BL)
    R.upload(pad_planes(clip.frame(0)), BL)
    for rdoq in (False, True):
        g = pipeline.FramePass(ctx, w, h, bd, qp=32, rdoq=rdoq)
        p = pipeline.FramePass(ctx, w, h, bd, qp=32, rdoq=rdoq,
                               partition=pipeline.cu_partition(w, h, 16))
        assert p.form == g.form and p.fused_tail == g.fused_tail
        g.run(O, R, A)
        p.run(O, R, B)
        ctx.sync()
        for x, y in zip(g.results(), p.results()):
            assert x.tobytes() == y.tobytes()
        a, b = A.download(BL), B.download(BL)
        for c in range(3):
            assert np.array_equal(a[c], b[c])
        other = ctx.me_plan(p.d_me.ptr, p.desc.n_cus - 1, 16)
        args = p._call_args(O, R, B)
        import ctypes as C
        st = ctx.lib.xvcgpu_frame_pass_planned(ctx.h, C.byref(args), other.h, 31)
        assert st == 10     # XVCGPU_INVALID_ARGUMENT
        other.destroy()
        g.destroy()
        p.destroy()
    for q in (O, R, A, B):
        q.destroy()


def small_partition(w, h):
    """All sides <= 16, with 4-wide, 4-tall and 4x4 CUs: the class-16 plan whose pass must
    not take the kernels that hold a CU whole (both sides >= 8)."""
    parts = []
    for y in range(0, h, 16):
        for x in range(0, w, 16):
            k = (x // 16 + 3 * (y // 16)) % 5
            if k == 0:
                parts.append((x, y, 16, 16))
            elif k == 1:
                parts += [(x, y, 4, 16), (x + 4, y, 4, 16), (x + 8, y, 8, 16)]
            elif k == 2:
                parts += [(x, y, 16, 4), (x, y + 4, 16, 4), (x, y + 8, 16, 8)]
            elif k == 3:
                parts += [(x, y, 8, 8), (x + 8, y, 8, 4), (x + 8, y + 4, 4, 4), (x + 12, y + 4, 4, 4),
                          (x, y + 8, 16, 8)]
            else:
                parts += [(x, y, 8, 16), (x + 8, y, 8, 16)]
    return parts


@pytest.mark.parametrize("rdoq,bd", [
    pytest.param(r, bd, id=str(r) if bd == 10 else "%s-bd%d" % (r, bd))
    for bd in (10, 12) for r in (False, True)])
def test_one_call_on_small_cus(gpu, xo, rdoq, bd):
    """xvcgpu_frame_pass_planned itself (run_phases: no Python choice in between) on a
    partition whose largest side is 16 and that holds 4-wide CUs: the plan knows, the call
    takes the any-size middle; against the oracle.  And a plan of another class is refused."""
    import ctypes as C
    import oracle_frame
    from xvc_amd import pipeline, synth
    api, ctx = gpu
    w, h, qp = 208, 112, 30
    parts = small_partition(w, h)
    clip = synth.SyntheticClip(w, h, bd)
    ref_host, orig_host = pad_planes(clip.frame(0)), pad_planes(clip.frame(1))
    O, R, Rec = (ctx.picture(w, h, bd) for _ in range(3))
    O.upload(orig_host, BL)
    R.upload(ref_host, BL)
    fp = pipeline.FramePass(ctx, w, h, bd, qp=qp, partition=parts, rdoq=rdoq)
    assert fp.desc.cu_size == 16 and fp.desc.min_side == 4
    fp.run_phases(O, R, Rec, api.FP_ENCODE | api.FP_DEBLOCK_V | api.FP_DEBLOCK_H | api.FP_PAD |
                  api.FP_SSD)
    ctx.sync()
    res, nnz, cus, ssd = fp.results()
    e_rec, e_res, e_nnz, e_cus, e_ssd = oracle_frame.frame_pass(fp.desc, bd, orig_host, ref_host,
                                                                BL, lib=xo)
    assert np.array_equal(res, e_res)
    assert np.array_equal(nnz, e_nnz), np.nonzero(nnz != e_nnz)[0][:8]
    assert cus.tobytes() == e_cus.tobytes()
    got = Rec.download(BL)
    for c in range(3):
        assert np.array_equal(got[c], e_rec[c]), c
    assert (int(ssd[0]), int(ssd[1])) == e_ssd
    assert int(np.count_nonzero(nnz)) > 0
    # a plan made for another class of max_block_size
    other = ctx.me_plan(fp.d_me.ptr, fp.desc.n_cus, 64)
    args = fp._call_args(O, R, Rec)
    assert ctx.lib.xvcgpu_frame_pass_planned(ctx.h, C.byref(args), other.h, 31) == 10
    other.destroy()
    fp.destroy()
    for p in (O, R, Rec):
        p.destroy()


def test_pass_refuses_a_cu_the_search_cannot_take(gpu):
    """check_partition lets a side cut by the picture edge to 24 through (the issue's rule);
    the pass, which has the plan's counts, refuses it instead of coding an unsearched CU."""
    api, ctx = gpu
    from xvc_amd import pipeline
    parts = [(0, 0, 64, 64), (64, 0, 24, 64)]
    assert pipeline.check_partition(88, 64, parts)
    with pytest.raises(ValueError) as e:
        pipeline.FramePass(ctx, 88, 64, 10, qp=32, partition=parts)
    assert "(64, 0, 24, 64)" in str(e.value)


def test_cpp_frame_pass_program_on_a_partition(gpu, tmp_path):
    """frame_pass_main with a partition file of `tiny` picture 1 prints the SSD the Python
    pass gets (QuantFast, 10 bit, QP 32, one picture), and refuses a file with a gap."""
    import subprocess
    from xvc_amd import pipeline, synth
    api, ctx = gpu
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    host = os.path.join(root, "xvc_amd", "host")
    obj, exe = str(tmp_path / "synth.o"), str(tmp_path / "frame_pass")
    subprocess.check_call(["gcc", "-O2", "-std=c99", "-Wall", "-Werror", "-c",
                           os.path.join(host, "xvc_synth.c"), "-o", obj])
    subprocess.check_call([
        "g++", "-std=c++11", "-O2", "-Wall", "-Wextra", "-Werror",
        "-I", os.path.join(root, "include"), "-I", host,
        os.path.join(host, "frame_pass_main.cc"), obj, "-o", exe,
        "-L", os.path.join(root, "xvc_amd"), "-lxvcgpu",
        "-Wl,-rpath," + os.path.join(root, "xvc_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    w, h = picture_size("tiny", 1)
    parts = luma_partition("tiny", 1)
    bd, qp = 10, 32
    pfile = tmp_path / "tiny1.txt"
    pfile.write_text("".join("%d %d %d %d\n" % tuple(p) for p in parts.tolist()))
    r = subprocess.run([exe, str(w), str(h), str(bd), str(qp), "1", str(pfile)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    line = [l.split() for l in r.stdout.splitlines() if l.startswith("frame ")]
    assert len(line) == 1
    clip = synth.SyntheticClip(w, h, bd)
    O, R, Rec = (ctx.picture(w, h, bd) for _ in range(3))
    O.upload(pad_planes(clip.frame(1)), BL)
    R.upload(pad_planes(clip.frame(0)), BL)
    fp = pipeline.FramePass(ctx, w, h, bd, qp=qp, partition=parts)
    fp.run(O, R, Rec)
    ctx.sync()
    ssd = fp.results()[3]
    assert (int(line[0][3]), int(line[0][5])) == (int(ssd[0]), int(ssd[1]))
    assert ("%d CUs per picture" % len(parts)) in r.stdout
    fp.destroy()
    for p in (O, R, Rec):
        p.destroy()
    gap = tmp_path / "gap.txt"
    gap.write_text("".join("%d %d %d %d\n" % tuple(p) for p in parts.tolist()[:-1]))
    r = subprocess.run([exe, str(w), str(h), str(bd), str(qp), "1", str(gap)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "partition" in r.stdout, r.stdout + r.stderr


def mixed_8_16_partition(w, h):
    """Sides of 8 and 16 only: the shapes the fused kernels hold, class 16, no 4-wide CU."""
    parts = []
    for y in range(0, h, 16):
        for x in range(0, w, 16):
            k = (x // 16 + 2 * (y // 16)) % 4
            if k == 0:
                parts.append((x, y, 16, 16))
            elif k == 1:
                parts += [(x, y, 8, 16), (x + 8, y, 8, 16)]
            elif k == 2:
                parts += [(x, y, 16, 8), (x, y + 8, 8, 8), (x + 8, y + 8, 8, 8)]
            else:
                parts += [(x, y, 8, 8), (x + 8, y, 8, 8), (x, y + 8, 16, 8)]
    return parts


@pytest.mark.parametrize("kind", ["grid16", "mixed"])
def test_keep_levels_on_cus_of_8_to_16(gpu, xo, kind):
    """QuantFast with keep_levels on a partition whose CUs all fit the
    fused kernels: run() must still store the levels - they feed DecodePass and reproduce
    the reconstruction -, run() and kernel_steps() give the same bytes, and the 16x16 grid
    as a partition equals the grid pass, levels included."""
    import oracle_frame
    from xvc_amd import pipeline, synth
    api, ctx = gpu
    w, h, bd, qp = 208, 112, 10, 30
    parts = pipeline.cu_partition(w, h, 16) if kind == "grid16" else mixed_8_16_partition(w, h)
    clip = synth.SyntheticClip(w, h, bd)
    ref_host, orig_host = pad_planes(clip.frame(0)), pad_planes(clip.frame(1))
    O, R, Renc, Rdec, Rsteps = (ctx.picture(w, h, bd) for _ in range(5))
    O.upload(orig_host, BL)
    R.upload(ref_host, BL)
    enc = pipeline.FramePass(ctx, w, h, bd, qp=qp, partition=parts, keep_levels=True)
    assert enc.desc.cu_size == 16 and enc.desc.min_side >= 8 and enc.form == "residual"
    poison = np.full(max(1, enc.n_levels), 0x5a5a, np.int16)
    ctx.h2d(enc.d_levels.ptr, poison)
    enc.run(O, R, Renc)
    ctx.sync()
    res, nnz, cus, ssd = enc.results()
    levels = enc.d_levels.to_array(np.int16, enc.n_levels)
    e_rec, e_res, e_nnz, e_cus, e_ssd = oracle_frame.frame_pass(enc.desc, bd, orig_host, ref_host,
                                                                BL, lib=xo)
    assert np.array_equal(res, e_res) and np.array_equal(nnz, e_nnz)
    assert cus.tobytes() == e_cus.tobytes() and (int(ssd[0]), int(ssd[1])) == e_ssd
    assert int(np.count_nonzero(nnz)) > 0
    # the levels were written: the blocks with nnz hold that many non-zero levels
    off = np.asarray(ctx.level_offsets(enc.desc.tx)[0], np.int64)
    for i in np.nonzero(nnz)[0][:64]:
        t = enc.desc.tx[i]
        blk = levels[off[i]:off[i] + int(t["w"]) * int(t["h"])]
        assert int(np.count_nonzero(blk)) == int(nnz[i]), i
    dec = pipeline.DecodePass(ctx, enc.desc, bd)
    dec.run(R, Rdec, enc.d_res.ptr, enc.d_levels.ptr, enc.d_level_off.ptr, enc.d_nnz.ptr)
    ctx.sync()
    a, b = Renc.download(BL), Rdec.download(BL)
    for c in range(3):
        assert np.array_equal(a[c], e_rec[c]), c
        assert np.array_equal(b[c], e_rec[c]), c
    # launch by launch: the same bytes, levels included
    ctx.h2d(enc.d_levels.ptr, poison)
    for _, fn in enc.kernel_steps(O, R, Rsteps):
        fn()
    ctx.sync()
    for x, y in zip(enc.results(), (res, nnz, cus, ssd)):
        assert x.tobytes() == y.tobytes()
    # (levels of blocks without any are not written by either: compare where nnz says so)
    lv2 = enc.d_levels.to_array(np.int16, enc.n_levels)
    for i in np.nonzero(nnz)[0]:
        t = enc.desc.tx[i]
        n = int(t["w"]) * int(t["h"])
        assert np.array_equal(lv2[off[i]:off[i] + n], levels[off[i]:off[i] + n]), i
    c2 = Rsteps.download(BL)
    for c in range(3):
        assert np.array_equal(c2[c], a[c]), c
    if kind == "grid16":    # partition=cu_partition(...) equals cu=
        g = pipeline.FramePass(ctx, w, h, bd, qp=qp, keep_levels=True)
        g.run(O, R, Rsteps)
        ctx.sync()
        for x, y in zip(g.results(), (res, nnz, cus, ssd)):
            assert x.tobytes() == y.tobytes()
        lg = g.d_levels.to_array(np.int16, g.n_levels)
        for i in np.nonzero(nnz)[0]:
            n = int(enc.desc.tx[i]["w"]) * int(enc.desc.tx[i]["h"])
            assert np.array_equal(lg[off[i]:off[i] + n], levels[off[i]:off[i] + n]), i
        g.destroy()
    enc.destroy()
    dec.destroy()
    for p in (O, R, Renc, Rdec, Rsteps):
        p.destroy()


def test_small_cus_ignore_the_fused_tail_scratch(gpu, xo):
    """xvcgpu_frame_pass_planned given scratch_rec on a plan with 4-wide CUs: the fused tail
    does not cover them, the call ends with the separate launches; against the oracle."""
    import oracle_frame
    from xvc_amd import pipeline, synth
    api, ctx = gpu
    w, h, bd, qp = 208, 112, 10, 30
    parts = small_partition(w, h)
    clip = synth.SyntheticClip(w, h, bd)
    ref_host, orig_host = pad_planes(clip.frame(0)), pad_planes(clip.frame(1))
    O, R, Rec, S = (ctx.picture(w, h, bd) for _ in range(4))
    O.upload(orig_host, BL)
    R.upload(ref_host, BL)
    fp = pipeline.FramePass(ctx, w, h, bd, qp=qp, partition=parts)
    assert not fp.fused_tail
    import ctypes as C
    args = fp._call_args(O, R, Rec)
    args.scratch_rec = S.h_pic
    ctx._check(ctx.lib.xvcgpu_frame_pass_planned(ctx.h, C.byref(args), fp.plan.h, 31))
    ctx.sync()
    res, nnz, cus, ssd = fp.results()
    e_rec, e_res, e_nnz, e_cus, e_ssd = oracle_frame.frame_pass(fp.desc, bd, orig_host, ref_host,
                                                                BL, lib=xo)
    assert np.array_equal(res, e_res) and np.array_equal(nnz, e_nnz)
    got = Rec.download(BL)
    for c in range(3):
        assert np.array_equal(got[c], e_rec[c]), c
    assert (int(ssd[0]), int(ssd[1])) == e_ssd
    fp.destroy()
    for p in (O, R, Rec, S):
        p.destroy()
