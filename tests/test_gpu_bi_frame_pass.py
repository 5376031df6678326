"""The frame pass of a B picture on the GPU (xvcgpu_frame_pass_bi, pipeline.BiFramePass):
the whole pass bit-exact against the model composed of the oracle's pieces
(tests/bi_pass_model.py, whose SearchMotion half tests/test_bi_pass_model.py pins to the
reference), the one call against its parts issued one by one, the folds on jobs with
predictors against the host control (xvc_gpu::InterSearch::SearchMotionBatch), the
refusals, and the P pass beside it on one context."""
import ctypes as C

import numpy as np
import pytest

import bi_pass_model as bm
import oracle_lib as ol

pytestmark = pytest.mark.gpu

BL = bm.BL
ALL = 31    # FP_ENCODE | FP_DEBLOCK_V | FP_DEBLOCK_H | FP_PAD | FP_SSD


@pytest.fixture(scope="module")
def gpu():
    from xvc_amd import api
    ctx = api.Context(0)
    yield api, ctx
    ctx.close()


@pytest.fixture(scope="module")
def xo():
    return ol.Lib("xo")


_inputs, _searched, _expected = {}, {}, {}


def model_input(name):
    if name not in _inputs:
        _inputs[name] = bm.make_input(name)
    return _inputs[name]


def expected(xo, name, rdoq):
    """The model's pass, computed once per (input, quantiser) and shared."""
    if (name, rdoq) not in _expected:
        pw, ph, bd, _, orig, ref0, ref1 = model_input(name)
        desc = bm.descriptors(name, rdoq)
        if name not in _searched:
            _searched[name] = bm.search_motion(xo, bd, pw, ph, orig[0], (ref0[0], ref1[0]),
                                               (desc.me, desc.me))
        _expected[name, rdoq] = bm.frame_pass(xo, desc, bd, orig, ref0, ref1, _searched[name])
    return _expected[name, rdoq]


class Scene:
    """The input's pictures on the device and a BiFramePass over them."""

    def __init__(self, ctx, name, form="residual"):
        from xvc_amd import pipeline
        pw, ph, bd, part, orig, ref0, ref1 = model_input(name)
        self.ctx, self.size = ctx, (pw, ph, bd)
        self.O, self.R0, self.R1, self.Rec = (ctx.picture(pw, ph, bd) for _ in range(4))
        for pic, planes in ((self.O, orig), (self.R0, ref0), (self.R1, ref1)):
            pic.upload(planes, BL)
        self.fp = pipeline.BiFramePass(
            ctx, pw, ph, bd, bm.QP, rdoq=form != "residual", rdoq_packed=form == "fwd_transform",
            partition=part, ref_pocs=bm.REF_POCS, search_range=bm.SEARCH_RANGE,
            side_bits=bm.SIDE_BITS)
        assert self.fp.form == form
        me = self.fp.desc.me.copy()
        me["lambda16"] = bm.LAMBDA16
        self.fp.set_jobs(me, me)

    def run(self, **kw):
        self.fp.run(self.O, self.R0, self.R1, self.Rec, **kw)
        self.ctx.sync()
        return self.fp.results(), self.Rec.download(BL)

    def destroy(self):
        self.fp.destroy()
        for p in (self.O, self.R0, self.R1, self.Rec):
            p.destroy()


def differing(a, b):
    """Indices of the records that differ, byte for byte (any dtype)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype.itemsize == b.dtype.itemsize and len(a) == len(b)
    ra = a.view(np.uint8).reshape(len(a), -1)
    return np.flatnonzero((ra != b.view(np.uint8).reshape(len(b), -1)).any(1))


def assert_pass_equal(got, exp, what):
    ((res0, res1), nnz, cus, ssd, choice), rec = got
    e_rec, (e_res0, e_res1), e_nnz, e_cus, e_ssd, e_choice = exp
    for l, (r, e) in enumerate(((res0, e_res0), (res1, e_res1))):
        bad = differing(r, e)
        assert not len(bad), (what, "search of list", l, bad[:4], r[bad[:4]], e[bad[:4]])
    bad = differing(choice, e_choice)
    assert not len(bad), (what, "choice", bad[:4], choice[bad[:4]], e_choice[bad[:4]])
    assert np.array_equal(nnz, e_nnz), (what, "nnz", np.flatnonzero(nnz != e_nnz)[:8])
    bad = differing(cus, e_cus)
    assert not len(bad), (what, "CU records", bad[:4], cus[bad[:4]], e_cus[bad[:4]])
    for c in range(3):
        assert np.array_equal(rec[c], e_rec[c]), (what, "plane", c,
                                                  np.argwhere(rec[c] != e_rec[c])[:4])
    assert (int(ssd[0]), int(ssd[1])) == tuple(int(v) for v in e_ssd), (what, "ssd")


def as_expected(results, rec):
    """A run's answer in the model's order, to compare two runs."""
    (res0, res1), nnz, cus, ssd, choice = results
    return rec, (res0, res1), nnz, cus, ssd, choice


@pytest.mark.parametrize("name,form", [
    ("grid10", "residual"), ("grid10", "residual_rdoq"), ("grid10", "fwd_transform"),
    ("grid8", "residual"), ("part10", "residual"), ("part10", "fwd_transform")])
def test_whole_pass_equals_model(gpu, xo, name, form):
    api, ctx = gpu
    exp = expected(xo, name, form != "residual")
    dirs = np.bincount(exp[5]["inter_dir"], minlength=3)
    assert (dirs >= 4).all(), dirs          # every direction, also through MC and the filter
    s = Scene(ctx, name, form)
    try:
        fused = s.fp.p.fused_tail
        # the grid's CUs are all at least 8x8; the partition holds sides of 4
        assert fused == (name != "part10")
        assert (s.fp.p.plan is not None) == (name == "part10")
        if name == "part10":
            counts = dict(zip(api.ME_PLAN_BIN_NAMES, s.fp.plan_l1.counts.tolist()))
            assert all(counts[k] > 0 for k in ("16x16", "8x8", "other16", "c32")) and \
                counts["c64_team"] + counts["c64_wave"] > 0 and not counts["unsupported"], counts
        assert_pass_equal(s.run(), exp, "fused tail" if fused else "separate tail")
        if fused:
            s.Rec.upload([np.zeros_like(p) for p in exp[0]], BL)
            assert_pass_equal(s.run(fused_tail=False), exp, "separate tail")
    finally:
        s.destroy()


def test_one_call_equals_its_parts(gpu):
    """xvcgpu_frame_pass_bi against the entry points it is made of, issued in order from
    Python on a second set of buffers."""
    api, ctx = gpu
    a, b = Scene(ctx, "grid10"), Scene(ctx, "grid10")
    try:
        one = a.run()
        steps = b.fp.kernel_steps(b.O, b.R0, b.R1, b.Rec)
        assert [n for n, _ in steps] == [
            "me_search_l0", "me_search_l1", "uni_fold", "bipred_l0", "bipred_l1", "choice",
            "inter_pred", "residual", "cu_info", "deblock_pad_ssd"]
        for _, fn in steps:
            fn()
        ctx.sync()
        parts = b.fp.results(), b.Rec.download(BL)
        assert_pass_equal(parts, as_expected(*one), "parts")
        # the work arrays between the launches too: jobs, refinement results, prediction jobs
        n = a.fp.desc.n_cus
        for x, y, dt, k in [(a.fp.d_bi_jobs[l], b.fp.d_bi_jobs[l], api.BI_DTYPE, n)
                            for l in range(2)] + [(a.fp.d_inter, b.fp.d_inter, api.INTER_DTYPE,
                                                   3 * n)]:
            assert not len(differing(x.to_array(dt, k), y.to_array(dt, k)))
        choice = one[0][4]
        for l in range(2):      # a width-0 job exactly where the CU refines the other list
            jobs = a.fp.d_bi_jobs[l].to_array(api.BI_DTYPE, n)
            assert np.array_equal(jobs["blk"]["w"] == 0, choice["search_list"] != l)
            took = choice["search_list"] == l
            ra = a.fp.d_bi_res[l].to_array(api.MERES_DTYPE, n)
            rb = b.fp.d_bi_res[l].to_array(api.MERES_DTYPE, n)
            assert not len(differing(ra[took], rb[took]))
            assert np.array_equal(np.stack([ra["mv_x"], ra["mv_y"]], 1)[took],
                                  choice["bi_mv"][took])
    finally:
        a.destroy()
        b.destroy()


def test_folds_with_predictors_equal_host_control(gpu):
    """Random per-list predictors and full-pel CUs: the choice records against
    xvc_host_search_motion_batch (pinned to the reference by test_gpu_host_inter_search.py)
    on the same jobs with AMVP pairs {mvp, mvp}."""
    from xvc_amd import decoder
    api, ctx = gpu
    L = decoder.load_host_library()
    L.xvc_host_search_motion_batch.argtypes = [C.c_void_p] * 5 + [C.c_int] + [C.c_void_p] * 3 + \
        [C.c_int, C.c_void_p]
    s = Scene(ctx, "grid10")
    try:
        n = s.fp.desc.n_cus
        rng = np.random.default_rng(31)
        blocks = np.zeros((2, n), api.ME_DTYPE)
        fullpel = (rng.integers(0, 6, n) == 0).astype(np.uint8)
        for l in range(2):
            blocks[l] = s.fp.desc.me
            blocks[l]["mvp_x"] = rng.integers(-160, 161, n)
            blocks[l]["mvp_y"] = rng.integers(-160, 161, n)
            blocks[l]["fullpel_mv"] = fullpel
        assert fullpel.any() and not fullpel.all()
        s.fp.set_jobs(blocks[0], blocks[1])
        (_, _, _, _, choice), _ = s.run()
        mvp = np.zeros((2, n, 4), np.int32)
        for l in range(2):
            mvp[l, :, 0] = mvp[l, :, 2] = blocks[l]["mvp_x"]
            mvp[l, :, 1] = mvp[l, :, 3] = blocks[l]["mvp_y"]
        side_uni = np.zeros((2, n), np.uint32)
        side_uni[0], side_uni[1] = bm.SIDE_BITS[0], bm.SIDE_BITS[1]
        side_bi = np.full(n, bm.SIDE_BITS[2], np.uint32)
        out = np.zeros((n, 18), np.int64)
        bl = np.ascontiguousarray(blocks)
        assert L.xvc_host_search_motion_batch(
            ctx.h, s.O.h_pic, s.R0.h_pic, s.R1.h_pic, bl.ctypes.data, n, mvp.ctypes.data,
            side_uni.ctypes.data, side_bi.ctypes.data, 1, out.ctypes.data) == 0
        for i in range(n):
            q, c = [int(v) for v in out[i]], choice[i]
            d = q[0]
            want_mv = [[q[1 + 2 * l], q[2 + 2 * l]] if d in (2, l) else [0, 0] for l in range(2)]
            got = (int(c["inter_dir"]), c["mv"].tolist(), int(c["cost"]), c["cost_uni"].tolist(),
                   int(c["cost_bi"]))
            assert got == (d, want_mv, q[7], [q[8], q[12]], q[16]), (i, got, q)
            assert q[5] == q[6] == 0 and q[17] == 1     # predictor index 0, one step
        assert len(set(choice["inter_dir"].tolist())) >= 2
    finally:
        s.destroy()


def _poison(ctx, fp):
    bufs = [fp.d_choice, fp.d_res_l1, fp.p.d_res, fp.p.d_nnz, fp.p.d_cus, fp.d_inter] + \
        fp.d_bi_jobs + fp.d_bi_res
    for b in bufs:
        ctx._check(ctx.lib.xvcgpu_memset(ctx.h, b.ptr, 0xA5, b.nbytes))
    return bufs


def _refused(api, ctx, s, bufs, change, plans=None):
    fp = s.fp
    a = fp._call_args(s.O, s.R0, s.R1, s.Rec)
    change(a)
    if plans is None:
        plans = (fp.p.plan, fp.plan_l1)
    with pytest.raises(api.XvcGpuError, match="status 10: frame_pass_bi: "):
        ctx._check(ctx.lib.xvcgpu_frame_pass_bi(
            ctx.h, C.byref(a), *[p.h if p is not None else None for p in plans], ALL))
    ctx.sync()
    for b in bufs:
        assert (b.to_array(np.uint8, b.nbytes) == 0xA5).all()
    rec = s.Rec.download(BL)
    assert all((p == 0x0123).all() for p in rec)


def test_refusals_enqueue_nothing(gpu):
    api, ctx = gpu
    g, p = Scene(ctx, "grid10"), Scene(ctx, "part10")
    try:
        for s in (g, p):
            s.Rec.upload([np.full_like(q, 0x0123) for q in model_input("grid10" if s is g
                                                                       else "part10")[4]], BL)
        bufs = _poison(ctx, g.fp)

        def form(v):
            def change(a):
                a.p.form = v
            return change

        def no_ref1(a):
            a.ref1 = None
        # the forms that predict from one list inside their kernel (the P pass runs both on
        # this grid), and a missing list-1 picture
        _refused(api, ctx, g, bufs, form(api.FP_FORM_NAMES.index("recon_from_me")))
        _refused(api, ctx, g, bufs, form(api.FP_FORM_NAMES.index("fwd_from_me")))
        _refused(api, ctx, g, bufs, no_ref1)
        bufs = _poison(ctx, p.fp)
        fp = p.fp
        _refused(api, ctx, p, bufs, lambda a: None, (fp.p.plan, None))
        _refused(api, ctx, p, bufs, lambda a: None, (None, fp.plan_l1))
        _refused(api, ctx, p, bufs, lambda a: None, (fp.plan_l1, fp.p.plan))
        # and the same blocks run when nothing is wrong with them
        assert int(p.run()[0][4]["inter_dir"].max()) == 2
    finally:
        g.destroy()
        p.destroy()


def test_p_pass_untouched_beside_the_b_pass(gpu):
    """A FramePass on list 0 of the same input answers the same before and after a
    BiFramePass ran on its context: no scratch or context state leaks between them."""
    from xvc_amd import pipeline
    api, ctx = gpu
    s = Scene(ctx, "grid10", "fwd_transform")
    pw, ph, bd = s.size
    P = ctx.picture(pw, ph, bd)
    passes = [pipeline.FramePass(ctx, pw, ph, bd, bm.QP),
              pipeline.FramePass(ctx, pw, ph, bd, bm.QP, rdoq=True)]
    try:
        def run_p():
            out = []
            for fp in passes:
                fp.run(s.O, s.R0, P)
                ctx.sync()
                out.append((fp.results(), P.download(BL)))
            return out
        before = run_p()
        b1 = s.run()
        after = run_p()
        for (ra, pa), (rb, pb) in zip(before, after):
            assert all(not len(differing(x, y)) for x, y in zip(ra, rb))
            assert all(np.array_equal(x, y) for x, y in zip(pa, pb))
        assert before[0][0][0]["subpel_dist"].any()
        # ... and the B pass the same after the P passes
        assert_pass_equal(s.run(), as_expected(*b1), "B pass again")
    finally:
        for fp in passes:
            fp.destroy()
        P.destroy()
        s.destroy()
