"""The P frame pass with merge mode on the GPU (xvcgpu_frame_pass_merge;
pipeline.FramePass(merge_cands=...)): the rank kernel alone over every CU shape at three bit
depths against xvcgpu_mc_metric_batch, the oracle and the model's fold; the choice and the
skip kernel alone on planted records; the pass in all five forms on the grid (10 and 8 bit)
and on the partition against the model composed of the oracle's pieces
(tests/merge_pass_model.py); a pass that lists no CU against the flat pass; the refusals; a
flat pass beside a merge pass on one context; and the C++ class."""
import ctypes as C

import numpy as np
import pytest

import helpers
import merge_pass_model as mm
import oracle_lib as ol

pytestmark = pytest.mark.gpu

BL = mm.BL
ALL = 31    # FP_ENCODE | FP_DEBLOCK_V | FP_DEBLOCK_H | FP_PAD | FP_SSD
POISON = 0xA5


@pytest.fixture(scope="module")
def gpu():
    from xvc_amd import api
    ctx = api.Context(0)
    yield api, ctx
    ctx.close()


@pytest.fixture(scope="module")
def xo():
    return ol.Lib("xo")


def differing(a, b):
    """Indices of the records that differ, byte for byte (any dtype)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype.itemsize == b.dtype.itemsize and len(a) == len(b)
    ra = a.view(np.uint8).reshape(len(a), -1)
    return np.flatnonzero((ra != b.view(np.uint8).reshape(len(b), -1)).any(1))


def poison_like(dtype, n):
    return np.full(n * np.dtype(dtype).itemsize, POISON, np.uint8).view(dtype)


def merge_args(api, n_listed, d_cands=None, d_order=None, d_rank=None, d_choice=None,
               d_chosen=None, lambda_sqrt=mm.LAMBDA_SQRT):
    from xvc_amd import pipeline
    return pipeline.merge_args(n_listed, mm.SIDE_BITS, mm.MERGE_SIDE_BITS, lambda_sqrt,
                               *[b.ptr if b is not None else None
                                 for b in (d_cands, d_order, d_rank, d_choice, d_chosen)])


# ---- the kernels alone -------------------------------------------------------------------
@pytest.mark.parametrize("bd", [8, 10, 12])
def test_rank_kernel_every_shape(gpu, xo, bd):
    """All 25 shapes w, h in {4 .. 64} in the four corners of a 128x128 picture - CUs at
    every picture edge - with candidates that stay inside, candidates that leave the picture
    and far ones ClipMv changes, one candidate that is not valid in every third CU, and a
    12x16 CU: dist against xvcgpu_mc_metric_batch and xo.mc_metric, cost / order / num
    against the model's fold; through a list that leaves every seventh CU out, whose planted
    records stay as they are."""
    api, ctx = gpu
    pw = ph = 128
    rng = np.random.default_rng(6200 + bd)
    orig, ref = helpers.make_pics(rng, bd, pw, ph, BL, (3, -2))
    rects = [(x, y, w, h) for w in mm.SIDES for h in mm.SIDES
             for x in (0, pw - w) for y in (0, ph - h)] + [(16, 32, 12, 16)]
    n = len(rects)
    assert n == 101
    me = np.zeros(n, api.ME_DTYPE)
    for i, r in enumerate(rects):
        me[i]["x"], me[i]["y"], me[i]["w"], me[i]["h"] = r
    cands = mm.cand_array(n)
    mv = rng.integers(-40 * 16, 40 * 16 + 1, (n, mm.CANDS, 2))
    mv[:, 1] = rng.integers(-150 * 16, 150 * 16 + 1, (n, 2))        # leaves the picture
    mv[:, 2] = rng.choice([-mm.FAR, mm.FAR], (n, 2))                # ClipMv acts
    mv[::4, 4] = mv[::4, 3]                                         # equal candidates
    cands["mv"][:, :, 0, :] = mv
    cands["ref_idx"][::3, 3] = (1, -1)
    cands["ref_idx"][1::9, 0] = (0, 0)
    order = np.array([i for i in range(n) if i % 7 != 3], np.int32)
    O, R = ctx.picture(pw, ph, bd), ctx.picture(pw, ph, bd)
    O.upload([orig, None, None], BL)
    R.upload([ref, None, None], BL)
    bufs = [ctx.buffer(a) for a in (me, cands, order, poison_like(api.FP_MERGE_RANK_DTYPE, n + 1))]
    d_me, d_cands, d_order, d_rank = bufs
    try:
        m = merge_args(api, len(order), d_cands, d_order, d_rank)
        ctx._check(ctx.lib.xvcgpu_fp_merge_rank(ctx.h, O.h_pic, R.h_pic, d_me.ptr, n, C.byref(m)))
        ctx.sync()
        got = d_rank.to_array(api.FP_MERGE_RANK_DTYPE, n + 1)
        left = [i for i in range(n + 1) if i not in set(order.tolist())]
        assert (got[left].view(np.uint8) == POISON).all()
        # the device's own per-candidate kernel and the oracle on the valid candidates
        mcm = np.zeros(n * mm.CANDS, api.MCM_DTYPE)
        for k in ("x", "y", "w", "h"):
            mcm[k] = np.repeat(me[k], mm.CANDS)
        mcm["metric"] = mm.SATD
        mcm["mv_x"], mcm["mv_y"] = mv[:, :, 0].reshape(-1), mv[:, :, 1].reshape(-1)
        pow2 = np.repeat(np.isin(me["w"], mm.SIDES) & np.isin(me["h"], mm.SIDES), mm.CANDS)
        ok = pow2 & (cands["ref_idx"][:, :, 0].reshape(-1) == 0) & \
            (cands["ref_idx"][:, :, 1].reshape(-1) == -1)
        batch = np.full(n * mm.CANDS, mm.NONE, np.uint64)
        batch[ok] = ctx.mc_metric_batch(O, R, mcm[ok])
        nums, firsts, clipped = set(), set(), 0
        for i in order:
            x, y, w, h = rects[i]
            exp = batch[mm.CANDS * i:mm.CANDS * (i + 1)]
            assert got[i]["dist"].tolist() == exp.tolist(), (i, rects[i], got[i], exp)
            for k in range(mm.CANDS):
                if ok[mm.CANDS * i + k]:
                    c = xo.clip_mv(x, y, pw, ph, int(mv[i][k][0]), int(mv[i][k][1]))
                    clipped += c != (int(mv[i][k][0]), int(mv[i][k][1]))
                    assert int(exp[k]) == xo.mc_metric(bd, mm.SATD, 0, 0, x, y, w, h, c, pw, ph,
                                                       orig, ref, BL), (i, k)
            cost, rank, num = mm.rank_fold(exp)
            assert got[i]["order"].tolist() == rank and int(got[i]["num"]) == num, (i, got[i])
            assert got[i]["cost"].tolist() == cost and int(got[i]["reserved"]) == 0, (i, got[i])
            nums.add(num)
            firsts.add(rank[0])
        assert (got[n - 1]["dist"] == mm.NONE).all() and got[n - 1]["order"].tolist() == [0, 1, 2, 3, 4]
        assert len(nums) >= 2 and len(firsts) >= 3 and clipped >= 50
        # a NULL list: the CUs 0 .. n_listed - 1
        ctx.h2d(d_rank.ptr, poison_like(api.FP_MERGE_RANK_DTYPE, n + 1))
        m = merge_args(api, 10, d_cands, None, d_rank)
        ctx._check(ctx.lib.xvcgpu_fp_merge_rank(ctx.h, O.h_pic, R.h_pic, d_me.ptr, n, C.byref(m)))
        ctx.sync()
        again = d_rank.to_array(api.FP_MERGE_RANK_DTYPE, n + 1)
        assert (again[10:].view(np.uint8) == POISON).all()
        keep = [i for i in range(10) if i in set(order.tolist())]
        assert not len(differing(again[keep], got[keep]))
        # refusals
        call = ctx.lib.xvcgpu_fp_merge_rank
        for bad in (merge_args(api, n + 1, d_cands, None, d_rank),
                    merge_args(api, -1, d_cands, None, d_rank),
                    merge_args(api, 4, None, None, d_rank), merge_args(api, 4, d_cands, None, None),
                    merge_args(api, 4, d_cands, None, d_rank, lambda_sqrt=float("nan")),
                    merge_args(api, 4, d_cands, None, d_rank, lambda_sqrt=-0.5)):
            assert call(ctx.h, O.h_pic, R.h_pic, d_me.ptr, n, C.byref(bad)) == 10
        ctx.sync()
        assert (d_rank.to_array(api.FP_MERGE_RANK_DTYPE, n + 1)[10:].view(np.uint8) == POISON).all()
    finally:
        for b in bufs:
            b.free()
        O.destroy()
        R.destroy()


def test_choice_kernel_on_planted_records(gpu):
    """A tie, merge one cheaper and one dearer, index 4, a best distortion of UINT32_MAX, a
    LIC job, an unsupported plain result, CUs the list does not name - against the model's
    fold byte for byte; the inputs and the bytes behind the outputs stay as they are."""
    api, ctx = gpu
    lam = mm.LAMBDA16
    n = 10
    me = np.zeros(n, api.ME_DTYPE)
    me["w"], me["h"], me["lambda16"] = 16, 16, lam
    me["mvp_x"], me["mvp_y"] = 8, -4
    me["lambda16"][7] = 0xfff00000          # a product beyond 32 bits
    me["fullpel_mv"][4] = 2                 # XVC_ME_USE_LIC
    me["fullpel_mv"][8] = 1                 # fullpel: the vector difference in whole samples
    res = np.zeros(n, api.MERES_DTYPE)
    res["mv_x"], res["mv_y"] = 16 * np.arange(n), -16 * np.arange(n)
    res["fullpel_x"], res["fullpel_y"], res["fullpel_cost"] = 3, 4, 99
    res["subpel_dist"] = 5000
    res["subpel_dist"][5] = mm.NONE         # XVCGPU_ME_UNSUPPORTED
    import bi_refs_pass_model as rm
    dists = []
    for i in range(n):
        b = me[i]
        bits_p = mm.SIDE_BITS + 1 + rm.mvd_bits(b, (int(res[i]["mv_x"]), int(res[i]["mv_y"])))
        m0 = (0, 1, 2, 4, 0, 0, 3, 0, 0, 1)[i]
        plain = 5000 + ((bits_p * int(b["lambda16"])) >> 16)
        tie = plain - (((mm.MERGE_SIDE_BITS + mm.idx_bits(m0)) * int(b["lambda16"])) >> 16)
        d = [10 ** 8] * 5
        d[m0] = tie + (0, -1, 1, 0, -50, -50, -50, 0, -1, -50)[i]
        if i == 6:
            d = [mm.NONE] * 5
        dists.append(d)
    ranks = np.zeros(n, api.FP_MERGE_RANK_DTYPE)
    for i, d in enumerate(dists):
        cost, order, num = mm.rank_fold(d)
        ranks[i] = (d, order, num, 0, cost)
    cands = mm.cand_array(n)
    cands["mv"][:, :, 0, :] = np.arange(n * 10).reshape(n, 5, 2) * 37 - 2000
    order = np.array([0, 1, 2, 3, 4, 5, 6, 7, 8], np.int32)     # CU 9: not named
    e_choice, e_chosen = mm.choice_fold(me, res, cands, ranks, order)
    assert e_choice["use_merge"].tolist() == [1, 1, 0, 1, 0, -1, 0, 1, 1, 0]
    assert e_choice["merge_idx"].tolist() == [0, 1, -1, 4, -1, -1, -1, 0, 0, -1]
    assert int(e_choice[0]["cost_merge"]) == int(e_choice[0]["cost_plain"])
    bufs = [ctx.buffer(a) for a in (me, res, cands, ranks, order,
                                    poison_like(api.FP_MERGE_RESULT_DTYPE, n + 1),
                                    poison_like(api.MERES_DTYPE, n + 1))]
    d_me, d_res, d_cands, d_rank, d_order, d_choice, d_chosen = bufs
    try:
        call = ctx.lib.xvcgpu_fp_merge_choice
        for d_ord, n_listed, exp in (
                (d_order, len(order), (e_choice, e_chosen)),
                (None, 3, mm.choice_fold(me, res, cands, ranks, [0, 1, 2])),
                (None, 0, mm.choice_fold(me, res, cands, ranks, []))):
            m = merge_args(api, n_listed, d_cands, d_ord, d_rank, d_choice, d_chosen)
            ctx._check(call(ctx.h, d_me.ptr, d_res.ptr, n, C.byref(m)))
            ctx.sync()
            choice = d_choice.to_array(api.FP_MERGE_RESULT_DTYPE, n + 1)
            chosen = d_chosen.to_array(api.MERES_DTYPE, n + 1)
            bad = differing(choice[:n], exp[0])
            assert not len(bad), (n_listed, bad, choice[bad], exp[0][bad])
            bad = differing(chosen[:n], exp[1])
            assert not len(bad), (n_listed, bad, chosen[bad], exp[1][bad])
            assert (choice[n:].view(np.uint8) == POISON).all()
            assert (chosen[n:].view(np.uint8) == POISON).all()
        assert not exp[0]["use_merge"][[0, 1, 2, 3, 4, 6, 7, 8, 9]].any()
        assert not len(differing(exp[1], res))
        for buf, arr in ((d_me, me), (d_res, res), (d_cands, cands.reshape(-1)), (d_rank, ranks)):
            assert not len(differing(buf.to_array(arr.dtype, len(arr)), arr))
        for bad in (merge_args(api, n + 1, d_cands, None, d_rank, d_choice, d_chosen),
                    merge_args(api, 2, d_cands, None, d_rank, None, d_chosen),
                    merge_args(api, 2, d_cands, None, d_rank, d_choice, None),
                    merge_args(api, 2, d_cands, None, None, d_choice, d_chosen)):
            assert call(ctx.h, d_me.ptr, d_res.ptr, n, C.byref(bad)) == 10
        assert call(ctx.h, None, d_res.ptr, n, C.byref(m)) == 10
    finally:
        for b in bufs:
            b.free()


def test_skip_kernel_on_planted_nnz(gpu):
    """Each of Y, U and V alone keeps a merge CU from skip; a plain CU without levels is not
    skip; an all-ones record is left alone; nothing but `skip` is written; both layouts."""
    api, ctx = gpu
    n = 8
    choice = np.zeros(n, api.FP_MERGE_RESULT_DTYPE)
    choice["use_merge"] = [1, 1, 1, 1, 0, 0, 1, 1]
    choice["merge_idx"] = [0, 1, 2, 3, -1, -1, 4, 0]
    choice["skip"] = 7                      # (whatever stood there)
    choice["cost"] = np.arange(n) + 100
    choice[5:6].view(np.uint8)[:] = 0xff    # no search result
    luma = np.array([21, 0, 3, 6, 9, 12, 15, 18], np.int32)       # not 3 i
    nnz = np.zeros(3 * n, np.int32)
    nnz[0], nnz[3 + 1], nnz[6 + 2] = 5, 1, 2    # Y of CU 1, U of CU 2, V of CU 3 (by `luma`)
    nnz[9] = 0                                  # CU 4: plain, no level
    nnz[15 + 1] = 3                             # CU 6
    bufs = [ctx.buffer(a) for a in (choice, luma, nnz)]
    d_choice, d_luma, d_nnz = bufs
    try:
        call = ctx.lib.xvcgpu_fp_merge_skip
        for d_l, idx in ((d_luma, luma), (None, 3 * np.arange(n))):
            ctx.h2d(d_choice.ptr, choice)
            ctx._check(call(ctx.h, d_nnz.ptr, d_l.ptr if d_l is not None else None, n, d_choice.ptr))
            ctx.sync()
            got = d_choice.to_array(api.FP_MERGE_RESULT_DTYPE, n)
            exp = choice.copy()
            for i in range(n):
                if i != 5:
                    exp[i]["skip"] = int(choice[i]["use_merge"] == 1 and
                                         not nnz[idx[i]:idx[i] + 3].any())
            assert not len(differing(got, exp)), (got, exp)
            assert (got[5:6].view(np.uint8) == 0xff).all()
        assert exp["skip"].tolist()[:5] == [0, 0, 0, 1, 0]          # the 3 i layout
        ctx.h2d(d_choice.ptr, choice)
        ctx._check(call(ctx.h, d_nnz.ptr, d_luma.ptr, n, d_choice.ptr))
        ctx.sync()
        assert d_choice.to_array(api.FP_MERGE_RESULT_DTYPE, n)["skip"].tolist() == \
            [1, 0, 0, 0, 0, -1, 0, 1]
        assert call(ctx.h, None, d_luma.ptr, n, d_choice.ptr) == 10
        assert call(ctx.h, d_nnz.ptr, d_luma.ptr, n, None) == 10
    finally:
        for b in bufs:
            b.free()


# ---- the pass ----------------------------------------------------------------------------
_FORMS = {"residual": dict(fused=False, keep_levels=True),
          "residual_rdoq": dict(rdoq=True, fused=False, keep_levels=True),
          "fwd_transform": dict(rdoq=True, keep_levels=True),
          "fwd_from_me": dict(rdoq=True),
          "recon_from_me": dict()}


class Scene:
    """merge_pass_model.scene(name) on the device and a FramePass of the named form over it
    with the model's lambda in its job arrays and the model's candidates."""

    def __init__(self, ctx, xo, name, form, merge=True, listed=None, lambda16=mm.LAMBDA16,
                 qp=mm.QP):
        from xvc_amd import pipeline
        pw, ph, bd, part, orig, ref = mm.scene(name)
        self.ctx, self.name, self.size = ctx, name, (pw, ph, bd)
        self.O, self.R, self.Rec = (ctx.picture(pw, ph, bd) for _ in range(3))
        self.O.upload(orig, BL)
        self.R.upload(ref, BL)
        kw = dict(qp=qp, search_range=mm.SEARCH_RANGE, partition=part, **_FORMS[form])
        if form == "fwd_transform" and part is None:
            kw.update(form="fwd_transform")
        if merge:
            kw.update(merge_cands=mm.search(xo, name)[1], merge_order=listed,
                      merge_side_bits=mm.MERGE_SIDE_BITS,
                      merge_lambda_sqrt=mm.LAMBDA_SQRT if lambda16 is not None else None)
        self.fp = fp = pipeline.FramePass(ctx, pw, ph, bd, **kw)
        assert fp.form == form and (fp.plan is not None) == (part is not None)
        if lambda16 is not None:
            fp.desc.me["lambda16"] = lambda16
            ctx.h2d(fp.d_me.ptr, fp.desc.me)

    def run(self, **kw):
        self.Rec.upload([np.full_like(p, 0x0123) for p in mm.scene(self.name)[4]], BL)
        self.fp.run(self.O, self.R, self.Rec, **kw)
        self.ctx.sync()
        fp = self.fp
        levels = fp.d_levels.to_array(np.int16, max(1, fp.n_levels)) if fp.d_levels else None
        return fp.results(), self.Rec.download(BL), levels

    def destroy(self):
        self.fp.destroy()
        for p in (self.O, self.R, self.Rec):
            p.destroy()


def split_levels(ctx, desc, levels):
    off = np.asarray(ctx.level_offsets(desc.tx)[0], np.int64)
    return [levels[off[t]:off[t] + int(b["w"]) * int(b["h"])] for t, b in enumerate(desc.tx)]


_expected = {}


def expected(xo, name, rdoq):
    """The model's pass, once per (input, quantiser)."""
    if (name, rdoq) not in _expected:
        pw, ph, bd, _, orig, ref = mm.scene(name)
        desc = mm.descriptors(name, rdoq)
        e = _expected[name, rdoq] = mm.frame_pass(xo, desc, bd, orig, ref, mm.search(xo, name))
        # what is compared is there: coded blocks in every component, every state chosen
        coded = [int((e[2][desc.tx["comp"] == c] != 0).sum()) for c in range(3)]
        use, skip = e[5]["use_merge"], e[5]["skip"]
        assert min(coded) >= 4 and int(use.sum()) >= 4 and int((use == 0).sum()) >= 4, coded
        assert int(skip.sum()) >= 1 and int(((use == 1) & (skip == 0)).sum()) >= 1
    return _expected[name, rdoq]


def assert_pass_equal(scene, got, exp, searched, what):
    """got: Scene.run(); exp: mm.frame_pass's answer; searched: mm.search's."""
    (res, nnz, cus, ssd), rec, levels = got
    e_rec, e_res, e_nnz, e_cus, e_ssd, e_choice, e_chosen, e_levels = exp
    fp = scene.fp
    bad = differing(res, e_res)
    assert not len(bad), (what, "search", bad[:4], res[bad[:4]], e_res[bad[:4]])
    ranks = fp.merge_rank()
    bad = differing(ranks, searched[2])
    assert not len(bad), (what, "rank", bad[:4], ranks[bad[:4]], searched[2][bad[:4]])
    chosen = fp.chosen_results()
    bad = differing(chosen, e_chosen)
    assert not len(bad), (what, "chosen", bad[:4], chosen[bad[:4]], e_chosen[bad[:4]])
    assert np.array_equal(nnz, e_nnz), (what, "nnz", np.flatnonzero(nnz != e_nnz)[:8])
    choice = fp.merge_choice()
    bad = differing(choice, e_choice)
    assert not len(bad), (what, "choice", bad[:4], choice[bad[:4]], e_choice[bad[:4]])
    bad = differing(cus, e_cus)
    assert not len(bad), (what, "CU records", bad[:4], cus[bad[:4]], e_cus[bad[:4]])
    for c in range(3):
        assert np.array_equal(rec[c], e_rec[c]), (what, "plane", c,
                                                  np.argwhere(rec[c] != e_rec[c])[:4])
    assert (int(ssd[0]), int(ssd[1])) == e_ssd, (what, "ssd")
    if levels is not None:
        for t, g in enumerate(split_levels(scene.ctx, fp.desc, levels)):
            if e_nnz[t]:    # (a block without levels: its part of the buffer is unspecified)
                assert np.array_equal(g, e_levels[t]), (what, "levels of block", t)


_CASES = [(name, form) for name in ("grid10", "grid8", "part10")
          for form in ("residual", "residual_rdoq", "fwd_transform")] + \
         [(name, form) for name in ("grid10", "grid8") for form in ("fwd_from_me", "recon_from_me")]


@pytest.mark.parametrize("name,form", _CASES)
def test_pass_equals_model(gpu, xo, name, form):
    """Search results (unchanged), rank records, choice records with skip, chosen results,
    levels, nnz, CU records, reconstruction and SSD of the pass against the model; the fused
    and the separate tail (the partition holds sides of 4: the separate one only); a second
    run of the same object."""
    api, ctx = gpu
    rdoq = form not in ("residual", "recon_from_me")
    exp, searched = expected(xo, name, rdoq), mm.search(xo, name)
    s = Scene(ctx, xo, name, form)
    try:
        part = name == "part10"
        assert s.fp.fused_tail == (not part)
        got = s.run()
        assert_pass_equal(s, got, exp, searched, "one call")
        if not part:
            assert_pass_equal(s, s.run(fused_tail=False), exp, searched, "separate tail")
        assert_pass_equal(s, s.run(), exp, searched, "again")
    finally:
        s.destroy()


@pytest.mark.parametrize("name,form", [("grid10", "residual"), ("grid10", "fwd_from_me"),
                                       ("grid8", "recon_from_me"), ("part10", "fwd_transform")])
def test_pass_without_listed_cus_equals_flat_pass(gpu, xo, name, form):
    """merge_cands with no CU listed gives the flat pass's bytes - results, nnz, records, SSD,
    levels, picture - and records that say plain for every CU; the pass that lists every CU
    gives another picture."""
    api, ctx = gpu
    a, f = Scene(ctx, xo, name, form, listed=[]), Scene(ctx, xo, name, form, merge=False)
    m = Scene(ctx, xo, name, form)
    try:
        assert a.fp.merge.n_listed == 0 and m.fp.merge.n_listed == a.fp.desc.n_cus
        (ra, pa, la), (rf, pf, lf) = a.run(), f.run()
        assert all(not len(differing(x, y)) for x, y in zip(ra, rf))
        assert all(np.array_equal(x, y) for x, y in zip(pa, pf))
        if lf is not None:
            for t, (g, e) in enumerate(zip(split_levels(ctx, a.fp.desc, la),
                                           split_levels(ctx, f.fp.desc, lf))):
                if rf[1][t]:
                    assert np.array_equal(g, e), t
        assert rf[1].any() and rf[0]["subpel_dist"].any()
        choice = a.fp.merge_choice()
        assert not choice["use_merge"].any() and (choice["cost_merge"] == mm.NONE).all()
        assert not choice["skip"].any() and (choice["merge_idx"] == -1).all()
        assert np.array_equal(choice["mv"][:, 0], rf[0]["mv_x"])
        assert not len(differing(a.fp.chosen_results(), rf[0]))
        (rm_, pm, _) = m.run()
        assert not len(differing(rm_[0], rf[0]))       # (the search is the flat one)
        assert len(differing(rm_[2], rf[2])) >= 4
        assert any(not np.array_equal(x, y) for x, y in zip(pm, pf))
    finally:
        for s in (a, f, m):
            s.destroy()


# ---- refusals ----------------------------------------------------------------------------
def test_refusals_enqueue_nothing(gpu, xo):
    """Every missing array, n_listed outside [0, n_cus], part of a picture, phases without
    ENCODE, a lambda_sqrt that is not finite or below 0, and the flat pass's own refusals:
    XVCGPU_INVALID_ARGUMENT naming the field, with the job arrays, the work arrays and rec as
    they were."""
    api, ctx = gpu
    s = Scene(ctx, xo, "grid10", "fwd_transform")
    p = Scene(ctx, xo, "part10", "residual")
    try:
        def a_set(**kw):
            return lambda a, m: [setattr(a, k, v) for k, v in kw.items()]

        def m_set(**kw):
            return lambda a, m: [setattr(m, k, v) for k, v in kw.items()]
        n = s.fp.desc.n_cus
        cases = [
            (m_set(d_cands=None), "d_cands", ALL),
            (m_set(d_rank=None), "d_rank", ALL),
            (m_set(d_choice=None), "d_choice", ALL),
            (m_set(d_chosen=None), "d_chosen", ALL),
            (m_set(n_listed=-1), "n_listed", ALL),
            (lambda a, m: setattr(m, "n_listed", a.n_cus + 1), "n_listed", ALL),
            (m_set(lambda_sqrt=float("nan")), "lambda_sqrt", ALL),
            (m_set(lambda_sqrt=float("inf")), "lambda_sqrt", ALL),
            (m_set(lambda_sqrt=-1.0), "lambda_sqrt", ALL),
            (a_set(d_nnz=None), "d_nnz", ALL),
            (a_set(), "phases", ALL & ~api.FP_ENCODE),
            (a_set(db_y_end=64), "whole pictures", ALL),
            (a_set(ssd_y_begin=8), "whole pictures", ALL),
            (a_set(n_cus_total=n + 1), "whole pictures", ALL),
            (a_set(d_tx=None), "d_tx", ALL),
            (a_set(pred=None), "pred", ALL),
            (a_set(form=0), "form", ALL),
            (a_set(d_results=None), "d_results", ALL),
        ]
        for scene, todo in ((s, cases), (p, cases[:11])):
            fp, d = scene.fp, scene.fp.desc
            scene.Rec.upload([np.full_like(q, 0x0123) for q in mm.scene(scene.name)[4]], BL)
            fm = fp.merge
            bufs = [fp.d_res, fp.d_nnz, fp.d_cus, fp.d_ssd, fp.d_levels, fm.d_rank, fm.d_choice,
                    fm.d_chosen]
            for b in bufs:
                ctx._check(ctx.lib.xvcgpu_memset(ctx.h, b.ptr, POISON, b.nbytes))
            plan = fp.plan.h if fp.plan is not None else None
            for change, match, phases in todo:
                a, m = fp._call_args(scene.O, scene.R, scene.Rec), fm.args()
                change(a, m)
                with pytest.raises(api.XvcGpuError, match="status 10: .*" + match):
                    ctx._check(ctx.lib.xvcgpu_frame_pass_merge(ctx.h, C.byref(a), C.byref(m),
                                                               plan, phases))
                ctx.sync()
                for b in bufs:
                    assert (b.to_array(np.uint8, b.nbytes) == POISON).all(), match
                assert all((q == 0x0123).all() for q in scene.Rec.download(BL)), match
                assert not len(differing(fp.d_me.to_array(api.ME_DTYPE, d.n_cus), d.me)), match
                assert not len(differing(fp.d_tx.to_array(api.TX_DTYPE, len(d.tx)), d.tx)), match
                assert not len(differing(fm.d_cands.to_array(api.FP_MERGE_CAND_DTYPE,
                                                             5 * d.n_cus), fm.cands.reshape(-1)))
        # no xvcgpu_frame_pass_merge_args at all; a plan made for other jobs
        a = s.fp._call_args(s.O, s.R, s.Rec)
        assert ctx.lib.xvcgpu_frame_pass_merge(ctx.h, C.byref(a), None, None, ALL) == 10
        m = s.fp.merge.args()
        assert ctx.lib.xvcgpu_frame_pass_merge(ctx.h, C.byref(a), C.byref(m), p.fp.plan.h, ALL) == 10
        ctx.sync()
        assert (s.fp.merge.d_choice.to_array(np.uint8, s.fp.merge.d_choice.nbytes) == POISON).all()
        # ... and the same blocks run when nothing is wrong with them
        for scene in (s, p):
            exp = expected(xo, scene.name, scene is s)
            assert_pass_equal(scene, scene.run(), exp, mm.search(xo, scene.name), "after refusals")
    finally:
        s.destroy()
        p.destroy()


def test_python_refusals(gpu, xo):
    from xvc_amd import pipeline
    api, ctx = gpu
    mv = np.zeros((35, 5, 2), np.int32)
    with pytest.raises(ValueError, match="merge_cands and affine"):
        pipeline.FramePass(ctx, 104, 72, 10, fused=False, affine=True, merge_cands=mv)
    with pytest.raises(ValueError, match="merge_cands and aqp_strength"):
        pipeline.FramePass(ctx, 104, 72, 10, fused=False, aqp_strength=13, merge_cands=mv)
    with pytest.raises(ValueError, match="merge_cands and row_range"):
        pipeline.FramePass(ctx, 104, 72, 10, row_range=(0, 32), merge_cands=mv[:14])
    s = Scene(ctx, xo, "grid10", "residual")
    f = Scene(ctx, xo, "grid10", "residual", merge=False)
    try:
        with pytest.raises(ValueError, match="merge_cands and run_multi"):
            pipeline.run_multi([f.fp, s.fp], [f.O, s.O], [f.R, s.R], [f.Rec, s.Rec])
        with pytest.raises(ValueError, match="merge mode"):
            s.fp.kernel_steps(s.O, s.R, s.Rec)
    finally:
        s.destroy()
        f.destroy()


# ---- state and the C++ class -------------------------------------------------------------
def test_flat_pass_untouched_beside_the_merge_pass(gpu, xo):
    """Flat FramePass objects answer the same before and after a pass with merge mode ran on
    their context - the form whose tail moves to the other stream among them: no scratch or
    context state leaks between them."""
    api, ctx = gpu
    flats = [Scene(ctx, xo, "grid10", "fwd_from_me", merge=False),
             Scene(ctx, xo, "grid10", "residual", merge=False)]
    merges = [Scene(ctx, xo, "grid10", "fwd_from_me"), Scene(ctx, xo, "grid10", "residual")]
    try:
        before = [f.run() for f in flats]
        first = [s.run() for s in merges]
        after = [f.run() for f in flats]
        for (ra, pa, _), (rb, pb, _) in zip(before, after):
            assert all(not len(differing(x, y)) for x, y in zip(ra, rb))
            assert all(np.array_equal(x, y) for x, y in zip(pa, pb))
        assert before[0][0][0]["subpel_dist"].any()
        again = [s.run() for s in merges]
        for (ra, pa, _), (rb, pb, _) in zip(first, again):
            assert all(not len(differing(x, y)) for x, y in zip(ra, rb))
            assert all(np.array_equal(x, y) for x, y in zip(pa, pb))
        assert any(not np.array_equal(x, y) for x, y in zip(first[0][1], before[0][1]))
    finally:
        for f in flats + merges:
            f.destroy()


@pytest.mark.parametrize("name,form", [("grid10", "recon_from_me"), ("part10", "residual")])
def test_host_class_equals_python_pass(gpu, xo, name, form):
    """xvc_gpu::FramePass with SetMerge (through xvc_host_frame_pass_merge) equals
    pipeline.FramePass(merge_cands=...) at the QP's own lambda and lambda_sqrt: search
    results, rank, choice and chosen records, CU records, SSD, picture."""
    from xvc_amd import decoder
    api, ctx = gpu
    L = decoder.load_host_library()
    L.xvc_host_frame_pass_merge.argtypes = [C.c_void_p] + [C.c_int] * 6 + [C.c_void_p, C.c_int] + \
        [C.c_void_p] * 3 + [C.c_int] * 2 + [C.c_void_p] * 7
    qp = 27
    s = Scene(ctx, xo, name, form, lambda16=None, qp=qp)
    pw, ph, bd = s.size
    Rec = ctx.picture(pw, ph, bd)
    try:
        (res, nnz, cus, ssd), rec, _ = s.run(fused_tail=False)
        choice = s.fp.merge_choice()
        assert int(choice["use_merge"].sum()) >= 2 and int((choice["use_merge"] == 0).sum()) >= 2
        n = s.fp.desc.n_cus
        part = mm.scene(name)[3]
        parts = np.ascontiguousarray(part, np.int32) if part is not None else None
        mv = np.ascontiguousarray(s.fp.merge.cands["mv"][:, :, 0, :], np.int32)
        cands = s.fp.merge.cands.copy()     # the class takes vectors: every candidate valid
        cands["ref_idx"] = (0, -1)
        ctx.h2d(s.fp.merge.d_cands.ptr, cands)
        (res, nnz, cus, ssd), rec, _ = s.run(fused_tail=False)
        choice = s.fp.merge_choice()
        h_res, h_chosen = np.zeros(n, api.MERES_DTYPE), np.zeros(n, api.MERES_DTYPE)
        h_cus, h_rank = np.zeros(n, api.CU_DTYPE), np.zeros(n, api.FP_MERGE_RANK_DTYPE)
        h_choice, h_ssd = np.zeros(n, api.FP_MERGE_RESULT_DTYPE), np.zeros(2, np.uint64)
        assert L.xvc_host_frame_pass_merge(
            ctx.h, pw, ph, bd, qp, 16, mm.SEARCH_RANGE, parts.ctypes.data if part is not None else None,
            len(parts) if part is not None else 0, s.O.h_pic, s.R.h_pic, Rec.h_pic, 0, n,
            mv.ctypes.data, h_res.ctypes.data, h_rank.ctypes.data, h_choice.ctypes.data,
            h_chosen.ctypes.data, h_cus.ctypes.data, h_ssd.ctypes.data) == 0
        assert not len(differing(h_res, res)) and not len(differing(h_cus, cus))
        assert not len(differing(h_rank, s.fp.merge_rank()))
        assert not len(differing(h_choice, choice))
        assert not len(differing(h_chosen, s.fp.chosen_results()))
        assert h_ssd.tolist() == ssd.tolist()
        assert all(np.array_equal(x, y) for x, y in zip(Rec.download(BL), rec))
    finally:
        Rec.destroy()
        s.destroy()
