"""The P frame pass with affine motion on the GPU (xvcgpu_frame_pass_affine;
pipeline.FramePass(affine=True)): each small kernel alone against the model's arrays byte for
byte, the listed search against xvcgpu_affine_me_batch, the pass in its three forms on the
grid (10 and 8 bit) and on the partition against the model composed of the oracle's pieces
(tests/affine_pass_model.py), a pass without capable CUs against the flat pass, the refusals,
a flat pass beside an affine one on one context, and the C++ class."""
import ctypes as C

import numpy as np
import pytest

import affine_pass_model as fm
import oracle_lib as ol

pytestmark = pytest.mark.gpu

BL = fm.BL
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


_expected = {}


def expected(xo, name, rdoq):
    """The model's pass, once per (input, quantiser)."""
    if (name, rdoq) not in _expected:
        pw, ph, bd, _, orig, ref = fm.scene(name)
        desc = fm.descriptors(name, rdoq)
        e = _expected[name, rdoq] = fm.frame_pass(xo, desc, bd, orig, ref, fm.search(xo, name))
        # what is compared is there: coded blocks in every component, both states chosen
        coded = [int((e[2][desc.tx["comp"] == c] != 0).sum()) for c in range(3)]
        assert min(coded) >= 8 and int(e[5]["use_affine"].sum()) >= 4, coded
    return _expected[name, rdoq]


# ---- the kernels alone -------------------------------------------------------------------
def test_boot_equals_model(gpu, xo):
    """xvcgpu_fp_affine_boot over the partition's 23 listed CUs with planted plain vectors -
    some of +-3000, where ClipMv acts - and one unsupported result: every job byte for byte
    against the model's, so the fields it does not name and the unlisted jobs stay."""
    api, ctx = gpu
    pw, ph = fm.INPUTS["part10"][:2]
    d = fm.descriptors("part10")
    jobs0, order, _ = d.affine_jobs()
    rng = np.random.default_rng(21)
    n = d.n_cus
    jobs0["reserved"], jobs0["other_mv"] = rng.integers(0, 256, n), rng.integers(-9, 9, (n, 3, 2))
    jobs0["bootstrap"], jobs0["flags"] = rng.integers(-9, 9, (n, 3, 2)), 2
    res = np.zeros(n, api.MERES_DTYPE)
    res["mv_x"], res["mv_y"] = rng.integers(-60, 61, n), rng.integers(-60, 61, n)
    res["mv_x"][order[::3]] = rng.choice([-3000, 3000], len(order[::3]))
    res["mv_y"][order[1::3]] = rng.choice([-3000, 3000], len(order[1::3]))
    res["subpel_dist"][order[7]] = fm.NONE
    exp = fm.boot(xo, res, order, pw, ph, jobs0)
    assert (exp["bootstrap"][order, 0, 0] != res["mv_x"][order]).sum() >= 4
    d_jobs, d_res, d_order = ctx.buffer(jobs0), ctx.buffer(res), ctx.buffer(order)
    try:
        ctx._check(ctx.lib.xvcgpu_fp_affine_boot(ctx.h, d_res.ptr, d_order.ptr, len(order), pw,
                                                 ph, d_jobs.ptr))
        ctx.sync()
        got = d_jobs.to_array(api.AFFINE_ME_DTYPE, n)
        bad = differing(got, exp)
        assert not len(bad), (bad[:4], got[bad[:4]], exp[bad[:4]])
        assert len(differing(got, jobs0)) == len(order)
        assert ctx.lib.xvcgpu_fp_affine_boot(ctx.h, d_res.ptr, None, 3, pw, ph, d_jobs.ptr) == 10
        assert ctx.lib.xvcgpu_fp_affine_boot(ctx.h, d_res.ptr, d_order.ptr, 3, 0, ph,
                                             d_jobs.ptr) == 10
    finally:
        for b in (d_jobs, d_res, d_order):
            b.free()


@pytest.mark.parametrize("name", ["grid8", "part10"])
def test_listed_search_equals_batch(gpu, xo, name):
    """xvcgpu_affine_me_listed against xvcgpu_affine_me_batch over the same jobs (the
    model's, after boot: NW = 2, 4, 8 and w != h on the partition) record for record, and
    against the oracle; records outside the list - and a NO_JOB job's - are untouched."""
    api, ctx = gpu
    pw, ph, bd, _, orig, ref = fm.scene(name)
    _, jobs, ares, _, _, order, n_class = fm.search(xo, name)
    jobs = jobs.copy()
    skipped = int(order[2])
    jobs["flags"][skipped] = fm.NO_JOB
    O, R = ctx.picture(pw, ph, bd), ctx.picture(pw, ph, bd)
    O.upload(orig, BL)
    R.upload(ref, BL)
    n = len(jobs)
    d_jobs, d_order = ctx.buffer(jobs), ctx.buffer(order)
    d_out = ctx.buffer(poison_like(api.AFFINE_ME_RESULT_DTYPE, n))
    try:
        listed = [int(i) for i in order if int(i) != skipped]
        batch = ctx.affine_me_batch(O, R, jobs[listed])     # (it takes capable shapes only)
        cls = (C.c_int32 * 3)(*n_class)
        ctx._check(ctx.lib.xvcgpu_affine_me_listed(ctx.h, O.h_pic, R.h_pic, d_jobs.ptr, n,
                                                   d_order.ptr, cls, d_out.ptr))
        ctx.sync()
        got = d_out.to_array(api.AFFINE_ME_RESULT_DTYPE, n)
        bad = differing(got[listed], batch)
        assert not len(bad), (bad[:4], got[listed][bad[:4]], batch[bad[:4]])
        assert not len(differing(got[listed], ares[listed]))
        rest = [i for i in range(n) if i not in listed]
        assert (got[rest].view(np.uint8) == POISON).all()
        assert got["iterations"][listed].max() >= 2
        # counts that name more jobs than there are, a negative count: refused
        for bad_counts in ((n, 1, 0), (-1, 0, 0)):
            assert ctx.lib.xvcgpu_affine_me_listed(
                ctx.h, O.h_pic, R.h_pic, d_jobs.ptr, n, d_order.ptr, (C.c_int32 * 3)(*bad_counts),
                d_out.ptr) == 10
    finally:
        for b in (d_jobs, d_order, d_out):
            b.free()
        O.destroy()
        R.destroy()


def _affine_args(api, d_aff, d_ares, d_choice, d_inter, side_bits=fm.SIDE_BITS):
    f = api.FramePassAffineArgs()
    f.d_affine, f.d_affine_results = d_aff.ptr, d_ares.ptr
    f.d_choice, f.d_inter, f.side_bits = d_choice.ptr, d_inter.ptr, side_bits
    return f


def test_choice_equals_model(gpu, xo):
    """xvcgpu_fp_affine_choice over the partition's searched arrays with planted extras: a
    tie, an affine state one cheaper, an unsupported plain result, a fullpel job, a job
    without bootstrap: records and prediction jobs byte for byte against the model's."""
    api, ctx = gpu
    d = fm.descriptors("part10")
    res, jobs, ares, _, _, order, _ = fm.search(xo, "part10")
    me, res, jobs, ares = d.me.copy(), res.copy(), jobs.copy(), ares.copy()
    rng = np.random.default_rng(22)
    n = d.n_cus
    me["mvp_x"], me["mvp_y"] = rng.integers(-40, 40, n), rng.integers(-40, 40, n)
    jobs["mvp"] = rng.integers(-40, 40, (n, 3, 2))
    me["fullpel_mv"][order[3]] = 1
    me["fullpel_mv"][n - 1] = 1            # (a 4x8 CU: its price shifts by 4)
    jobs["flags"][order[4]] = 0
    res["subpel_dist"][order[5]] = res["subpel_dist"][n - 2] = fm.NONE
    base, _ = fm.choice_fold(me, res, jobs, ares)
    for i, delta in ((int(order[0]), 0), (int(order[1]), -1), (int(order[2]), 1)):
        # move the affine distortion so that cost_affine = cost_plain + delta
        ares["dist"][i] = int(ares["dist"][i]) + int(base["cost_plain"][i]) - \
            int(base["cost_affine"][i]) + delta
    exp_c, exp_i = fm.choice_fold(me, res, jobs, ares)
    assert [int(exp_c["use_affine"][order[k]]) for k in range(3)] == [0, 1, 0]
    assert int(exp_c["cost_affine"][order[0]]) == int(exp_c["cost_plain"][order[0]])
    bufs = [ctx.buffer(a) for a in (me, res, jobs, ares, poison_like(api.FP_AFFINE_RESULT_DTYPE, n + 1),
                                    poison_like(api.INTER_DTYPE, 3 * n + 1))]
    d_me, d_res, d_jobs, d_ares, d_choice, d_inter = bufs
    try:
        f = _affine_args(api, d_jobs, d_ares, d_choice, d_inter)
        ctx._check(ctx.lib.xvcgpu_fp_affine_choice(ctx.h, d_me.ptr, d_res.ptr, n, C.byref(f)))
        ctx.sync()
        got_c = d_choice.to_array(api.FP_AFFINE_RESULT_DTYPE, n + 1)
        got_i = d_inter.to_array(api.INTER_DTYPE, 3 * n + 1)
        bad = differing(got_c[:n], exp_c)
        assert not len(bad), (bad[:4], got_c[bad[:4]], exp_c[bad[:4]])
        bad = differing(got_i[:3 * n], exp_i)
        assert not len(bad), (bad[:4], got_i[bad[:4]], exp_i[bad[:4]])
        assert (got_c[n:].view(np.uint8) == POISON).all() and (got_i[3 * n:].view(np.uint8) == POISON).all()
        for a, e in ((d_me, me), (d_res, res), (d_jobs, jobs), (d_ares, ares)):
            assert not len(differing(a.to_array(e.dtype, n), e))
        f.d_choice = None
        with pytest.raises(api.XvcGpuError, match="status 10: .*d_choice"):
            ctx._check(ctx.lib.xvcgpu_fp_affine_choice(ctx.h, d_me.ptr, d_res.ptr, n, C.byref(f)))
    finally:
        for b in bufs:
            b.free()


def test_cu_records_equal_model(gpu, xo):
    """xvcgpu_cu_info_from_affine_choice over the partition's choice (affine CUs: the fourth
    corner UR + DL - UL), 111 records, with and without a luma index: byte for byte."""
    api, ctx = gpu
    d = fm.descriptors("part10")
    choice = fm.search(xo, "part10")[3]
    n = d.n_cus
    rng = np.random.default_rng(23)
    nnz = rng.integers(0, 2, 3 * n).astype(np.int32)
    exp = fm.cu_records(d, choice, nnz, ref_poc=5)
    assert any((c["mv"][0][3] != c["mv"][0][0]).any() for c in exp)
    bufs = [ctx.buffer(a) for a in (d.me, choice, nnz, d.luma_idx, poison_like(api.CU_DTYPE, n + 1))]
    d_me, d_choice, d_nnz, d_luma, d_cus = bufs
    try:
        call = ctx.lib.xvcgpu_cu_info_from_affine_choice
        ctx._check(call(ctx.h, d_me.ptr, d_choice.ptr, d_nnz.ptr, d_luma.ptr, n, d.qp, d.qp_c, 5,
                        d_cus.ptr))
        ctx.sync()
        got = d_cus.to_array(api.CU_DTYPE, n + 1)
        bad = differing(got[:n], exp)
        assert not len(bad), (bad[:4], got[bad[:4]], exp[bad[:4]])
        assert (got[n:].view(np.uint8) == POISON).all()
        ctx._check(call(ctx.h, d_me.ptr, d_choice.ptr, d_nnz.ptr, None, n, d.qp, d.qp_c, 5,
                        d_cus.ptr))
        ctx.sync()
        exp["cbf_luma"] = nnz[:n] != 0
        assert not len(differing(d_cus.to_array(api.CU_DTYPE, n), exp))
        assert call(ctx.h, d_me.ptr, None, d_nnz.ptr, None, n, d.qp, d.qp_c, 5, d_cus.ptr) == 10
    finally:
        for b in bufs:
            b.free()


# ---- the pass ----------------------------------------------------------------------------
class Scene:
    """affine_pass_model.scene(name) on the device and a FramePass of the named form over it
    with the model's lambda in its job arrays."""

    def __init__(self, ctx, name, form, affine=True, cu=16, lambda16=fm.LAMBDA16, qp=fm.QP):
        from xvc_amd import pipeline
        pw, ph, bd, part, orig, ref = fm.scene(name)
        self.ctx, self.name, self.size = ctx, name, (pw, ph, bd)
        self.O, self.R, self.Rec = (ctx.picture(pw, ph, bd) for _ in range(3))
        self.O.upload(orig, BL)
        self.R.upload(ref, BL)
        kw = dict(qp=qp, cu=cu, search_range=fm.SEARCH_RANGE, keep_levels=True, partition=part,
                  affine=affine)
        if form == "residual":
            kw.update(fused=False)
        elif form == "residual_rdoq":
            kw.update(rdoq=True, fused=False)
        else:
            kw.update(rdoq=True, form=None if part is not None else "fwd_transform")
        self.fp = fp = pipeline.FramePass(ctx, pw, ph, bd, **kw)
        assert fp.form == form and (fp.plan is not None) == (part is not None)
        if lambda16 is not None:
            fp.desc.me["lambda16"] = lambda16
            ctx.h2d(fp.d_me.ptr, fp.desc.me)
            if fp.affine is not None:
                fp.affine.jobs["lambda16"] = lambda16
                ctx.h2d(fp.affine.d_affine.ptr, fp.affine.jobs)

    def run(self, **kw):
        self.Rec.upload([np.full_like(p, 0x0123) for p in fm.scene(self.name)[4]], BL)
        self.fp.run(self.O, self.R, self.Rec, **kw)
        self.ctx.sync()
        fp = self.fp
        levels = fp.d_levels.to_array(np.int16, max(1, fp.n_levels))
        return fp.results(), self.Rec.download(BL), levels

    def destroy(self):
        self.fp.destroy()
        for p in (self.O, self.R, self.Rec):
            p.destroy()


def split_levels(ctx, desc, levels):
    off = np.asarray(ctx.level_offsets(desc.tx)[0], np.int64)
    return [levels[off[t]:off[t] + int(b["w"]) * int(b["h"])] for t, b in enumerate(desc.tx)]


def assert_pass_equal(api, scene, got, exp, searched, what):
    """got: Scene.run(); exp: fm.frame_pass's answer; searched: fm.search's."""
    (res, nnz, cus, ssd), rec, levels = got
    e_rec, e_res, e_nnz, e_cus, e_ssd, e_choice, _, e_levels = exp
    _, e_jobs, e_ares, _, e_inter, order, _ = searched
    fa = scene.fp.affine
    bad = differing(res, e_res)
    assert not len(bad), (what, "search", bad[:4], res[bad[:4]], e_res[bad[:4]])
    bad = differing(fa.affine_blocks(), e_jobs)
    assert not len(bad), (what, "boot", bad[:4])
    a_got = fa.affine_results()
    bad = differing(a_got[order], e_ares[order])
    assert not len(bad), (what, "affine search", bad[:4], a_got[order][bad[:4]], e_ares[order][bad[:4]])
    choice = scene.fp.affine_choice()
    bad = differing(choice, e_choice)
    assert not len(bad), (what, "choice", bad[:4], choice[bad[:4]], e_choice[bad[:4]])
    assert not len(differing(fa.inter_jobs(), e_inter)), (what, "prediction jobs")
    assert np.array_equal(nnz, e_nnz), (what, "nnz", np.flatnonzero(nnz != e_nnz)[:8])
    bad = differing(cus, e_cus)
    assert not len(bad), (what, "CU records", bad[:4], cus[bad[:4]], e_cus[bad[:4]])
    for c in range(3):
        assert np.array_equal(rec[c], e_rec[c]), (what, "plane", c,
                                                  np.argwhere(rec[c] != e_rec[c])[:4])
    assert (int(ssd[0]), int(ssd[1])) == e_ssd, (what, "ssd")
    for t, g in enumerate(split_levels(scene.ctx, scene.fp.desc, levels)):
        if e_nnz[t]:        # (a block without levels: its part of the buffer is unspecified)
            assert np.array_equal(g, e_levels[t]), (what, "levels of block", t)


_CASES = [("grid10", "residual"), ("grid10", "fwd_transform"), ("grid8", "residual_rdoq"),
          ("part10", "residual"), ("part10", "residual_rdoq"), ("part10", "fwd_transform")]


@pytest.mark.parametrize("name,form", _CASES)
def test_pass_equals_model(gpu, xo, name, form):
    """Search results, bootstrap, affine results, choice records, prediction jobs, levels,
    nnz, CU records, reconstruction and SSD of the pass against the model; the fused and the
    separate tail (the partition holds sides of 4: the separate one only); a second run of
    the same object; and the picture is not the flat pass's."""
    api, ctx = gpu
    exp, searched = expected(xo, name, form != "residual"), fm.search(xo, name)
    s = Scene(ctx, name, form)
    flat = Scene(ctx, name, form, affine=False)
    try:
        part = name == "part10"
        assert s.fp.fused_tail == (not part)
        got = s.run()
        assert_pass_equal(api, s, got, exp, searched, "one call")
        if not part:
            assert_pass_equal(api, s, s.run(fused_tail=False), exp, searched, "separate tail")
        else:
            counts = dict(zip(api.ME_PLAN_BIN_NAMES, s.fp.plan.counts.tolist()))
            assert counts["c32"] and counts["c64_team"] + counts["c64_wave"] == 1, counts
            assert s.fp.affine.n_class == [18, 4, 1]
        assert_pass_equal(api, s, s.run(), exp, searched, "again")
        (f_res, _, f_cus, _), f_rec, _ = flat.run()
        assert not len(differing(f_res, got[0][0]))       # (the first search is the flat one)
        assert len(differing(f_cus, got[0][2])) >= 4
        assert any(not np.array_equal(a, b) for a, b in zip(f_rec, got[1]))
    finally:
        s.destroy()
        flat.destroy()


@pytest.mark.parametrize("form", ["residual", "fwd_transform"])
def test_pass_without_capable_cus_equals_flat_pass(gpu, form):
    """On the 8-sample grid no CU is capable: affine=True gives the flat pass's bytes -
    results, records, levels, picture - and records that say plain for every CU."""
    api, ctx = gpu
    a, f = Scene(ctx, "grid10", form, cu=8), Scene(ctx, "grid10", form, affine=False, cu=8)
    try:
        assert a.fp.affine.n_class == [0, 0, 0]
        (ra, pa, la), (rf, pf, lf) = a.run(), f.run()
        assert all(not len(differing(x, y)) for x, y in zip(ra, rf))
        assert all(np.array_equal(x, y) for x, y in zip(pa, pf))
        for t, (g, e) in enumerate(zip(split_levels(ctx, a.fp.desc, la),
                                       split_levels(ctx, f.fp.desc, lf))):
            if rf[1][t]:
                assert np.array_equal(g, e), t
        assert rf[1].any() and rf[0]["subpel_dist"].any()
        choice = a.fp.affine_choice()
        assert not choice["use_affine"].any() and (choice["cost_affine"] == fm.NONE).all()
        assert np.array_equal(choice["mv"][:, 0, 0], rf[0]["mv_x"])
    finally:
        a.destroy()
        f.destroy()


# ---- refusals ----------------------------------------------------------------------------
def test_refusals_enqueue_nothing(gpu):
    """Both _from_me forms, every missing array, counts above n_cus, part of a picture,
    phases without ENCODE, a plan with LIC jobs: XVCGPU_INVALID_ARGUMENT naming the field,
    with the job arrays, the work arrays and rec as they were."""
    api, ctx = gpu
    s = Scene(ctx, "grid10", "fwd_transform")
    p = Scene(ctx, "part10", "residual")
    try:
        form = api.FP_FORM_NAMES.index

        def a_set(**kw):
            return lambda a, f: [setattr(a, k, v) for k, v in kw.items()]

        def f_set(**kw):
            return lambda a, f: [setattr(f, k, v) for k, v in kw.items()]

        def counts(first):      # first: the 16 class's count, or None for the pass's n_cus
            return lambda a, f: f.n_class.__setitem__(
                slice(0, 3), (a.n_cus if first is None else first, 1, 0))
        n = s.fp.desc.n_cus
        cases = [
            (a_set(form=form("recon_from_me")), "form", ALL),
            (a_set(form=form("fwd_from_me")), "form", ALL),
            (f_set(d_affine=None), "d_affine", ALL),
            (f_set(d_affine_results=None), "d_affine_results", ALL),
            (f_set(d_choice=None), "d_choice", ALL),
            (f_set(d_inter=None), "d_inter", ALL),
            (f_set(d_order=None), "d_order", ALL),
            (counts(None), "n_class", ALL),
            (counts(-1), "n_class", ALL),
            (a_set(db_y_end=64), "whole pictures", ALL),
            (a_set(ssd_y_begin=8), "whole pictures", ALL),
            (a_set(n_cus_total=n + 1), "whole pictures", ALL),
            (a_set(d_tx=None), "d_tx", ALL),
            (a_set(pred=None), "pred", ALL),
            (a_set(), "phases", ALL & ~api.FP_ENCODE),
        ]
        for scene, todo in ((s, cases), (p, cases[2:9])):
            fp, d = scene.fp, scene.fp.desc
            scene.Rec.upload([np.full_like(q, 0x0123) for q in fm.scene(scene.name)[4]], BL)
            fa = fp.affine
            bufs = [fp.d_res, fp.d_nnz, fp.d_cus, fp.d_ssd, fp.d_levels, fa.d_affine_res,
                    fa.d_choice, fa.d_inter]
            for b in bufs:
                ctx._check(ctx.lib.xvcgpu_memset(ctx.h, b.ptr, POISON, b.nbytes))
            plan = fp.plan.h if fp.plan is not None else None
            for change, match, phases in todo:
                a, f = fp._call_args(scene.O, scene.R, scene.Rec), fa.args()
                change(a, f)
                with pytest.raises(api.XvcGpuError, match="status 10: .*" + match):
                    ctx._check(ctx.lib.xvcgpu_frame_pass_affine(ctx.h, C.byref(a), C.byref(f),
                                                                plan, phases))
                ctx.sync()
                for b in bufs:
                    assert (b.to_array(np.uint8, b.nbytes) == POISON).all(), match
                assert all((q == 0x0123).all() for q in scene.Rec.download(BL)), match
                assert not len(differing(fp.d_me.to_array(api.ME_DTYPE, d.n_cus), d.me)), match
                assert not len(differing(fp.d_tx.to_array(api.TX_DTYPE, len(d.tx)), d.tx)), match
                assert not len(differing(fa.affine_blocks(), fa.jobs)), match
        # no xvcgpu_frame_pass_affine_args at all; a plan that holds LIC jobs
        a = s.fp._call_args(s.O, s.R, s.Rec)
        assert ctx.lib.xvcgpu_frame_pass_affine(ctx.h, C.byref(a), None, None, ALL) == 10
        fp, fa = p.fp, p.fp.affine
        lic = fp.desc.me.copy()
        lic["fullpel_mv"][7] = 2      # XVC_ME_USE_LIC on the first 16x16 CU
        ctx.h2d(fp.d_me.ptr, lic)
        plan = ctx.me_plan(fp.d_me.ptr, fp.desc.n_cus, fp.desc.cu_size)
        try:
            a, f = fp._call_args(p.O, p.R, p.Rec), fa.args()
            with pytest.raises(api.XvcGpuError, match="status 10: .*LIC"):
                ctx._check(ctx.lib.xvcgpu_frame_pass_affine(ctx.h, C.byref(a), C.byref(f), plan.h,
                                                            ALL))
            ctx.sync()
            assert (fa.d_choice.to_array(np.uint8, fa.d_choice.nbytes) == POISON).all()
        finally:
            plan.destroy()
            ctx.h2d(fp.d_me.ptr, fp.desc.me)
        # ... and the same blocks run when nothing is wrong with them
        for scene in (s, p):
            scene.run()
            assert int(scene.fp.affine_choice()["use_affine"].sum()) >= 4
    finally:
        s.destroy()
        p.destroy()


def test_python_refusals(gpu):
    from xvc_amd import pipeline
    api, ctx = gpu
    with pytest.raises(ValueError, match="recon_from_me"):
        pipeline.FramePass(ctx, 104, 72, 10, affine=True)
    with pytest.raises(ValueError, match="aqp_strength"):
        pipeline.FramePass(ctx, 104, 72, 10, fused=False, aqp_strength=13, affine=True)
    s = Scene(ctx, "grid10", "residual")
    f = Scene(ctx, "grid10", "residual", affine=False)
    try:
        with pytest.raises(ValueError, match="run_multi"):
            pipeline.run_multi([f.fp, s.fp], [f.O, s.O], [f.R, s.R], [f.Rec, s.Rec])
    finally:
        s.destroy()
        f.destroy()


# ---- state and the C++ class -------------------------------------------------------------
def test_flat_pass_untouched_beside_the_affine_pass(gpu):
    """Flat FramePass objects answer the same before and after a pass with affine motion ran
    on their context: no scratch or context state leaks between them."""
    api, ctx = gpu
    flats = [Scene(ctx, "grid10", "fwd_transform", affine=False),
             Scene(ctx, "grid10", "residual", affine=False)]
    s = Scene(ctx, "grid10", "fwd_transform")
    try:
        before = [f.run() for f in flats]
        first = s.run()
        after = [f.run() for f in flats]
        for (ra, pa, _), (rb, pb, _) in zip(before, after):
            assert all(not len(differing(x, y)) for x, y in zip(ra, rb))
            assert all(np.array_equal(x, y) for x, y in zip(pa, pb))
        assert before[0][0][0]["subpel_dist"].any()
        again = s.run()
        assert all(not len(differing(x, y)) for x, y in zip(first[0], again[0]))
        assert all(np.array_equal(x, y) for x, y in zip(first[1], again[1]))
    finally:
        for f in flats + [s]:
            f.destroy()


@pytest.mark.parametrize("name", ["grid10", "part10"])
def test_host_class_equals_python_pass(gpu, name):
    """xvc_gpu::FramePass with SetAffine (through xvc_host_frame_pass_affine) equals
    pipeline.FramePass(affine=True) at the QP's own lambda: search results, choice records,
    CU records, SSD, picture."""
    from xvc_amd import decoder
    api, ctx = gpu
    L = decoder.load_host_library()
    L.xvc_host_frame_pass_affine.argtypes = [C.c_void_p] + [C.c_int] * 6 + [C.c_void_p, C.c_int] + \
        [C.c_void_p] * 3 + [C.c_int] * 2 + [C.c_void_p] * 4
    qp = 27
    s = Scene(ctx, name, "residual", lambda16=None, qp=qp)
    pw, ph, bd = s.size
    Rec = ctx.picture(pw, ph, bd)
    try:
        (res, nnz, cus, ssd), rec, _ = s.run(fused_tail=False)
        choice = s.fp.affine_choice()
        assert int(choice["use_affine"].sum()) >= 2
        n = s.fp.desc.n_cus
        part = fm.scene(name)[3]
        parts = np.ascontiguousarray(part, np.int32) if part is not None else None
        h_res, h_cus = np.zeros(n, api.MERES_DTYPE), np.zeros(n, api.CU_DTYPE)
        h_choice, h_ssd = np.zeros(n, api.FP_AFFINE_RESULT_DTYPE), np.zeros(2, np.uint64)
        assert L.xvc_host_frame_pass_affine(
            ctx.h, pw, ph, bd, qp, 16, fm.SEARCH_RANGE, parts.ctypes.data if part is not None else None,
            len(parts) if part is not None else 0, s.O.h_pic, s.R.h_pic, Rec.h_pic, 0, n,
            h_res.ctypes.data, h_choice.ctypes.data, h_cus.ctypes.data, h_ssd.ctypes.data) == 0
        assert not len(differing(h_res, res)) and not len(differing(h_cus, cus))
        assert not len(differing(h_choice, choice))
        assert h_ssd.tolist() == ssd.tolist()
        assert all(np.array_equal(x, y) for x, y in zip(Rec.download(BL), rec))
    finally:
        Rec.destroy()
        s.destroy()
