"""The frame passes with adaptive QP on the GPU (xvcgpu_frame_pass_aqp,
xvcgpu_frame_pass_bi_refs_aqp; pipeline.FramePass / BiRefsFramePass with aqp_strength): the
two kernels alone against the model's arrays byte for byte, the P pass in its three forms on
the grid and on a partition against the model composed of the oracle's pieces
(tests/aqp_pass_model.py), strength 0 against the flat pass, the B pass on two reference
sets, the refusals, a flat pass beside an adaptive one on one context, and the C++ class."""
import ctypes as C

import numpy as np
import pytest

import aqp_pass_model as am
import bi_refs_pass_model as rm
import oracle_lib as ol

pytestmark = pytest.mark.gpu

BL = am.BL
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


def poisoned(ctx, nbytes):
    b = ctx.alloc(max(1, nbytes))
    ctx._check(ctx.lib.xvcgpu_memset(ctx.h, b.ptr, POISON, b.nbytes))
    return b


_tables, _expected = {}, {}


def table(bd, strength=am.STRENGTH, width=am.W, qp=am.QP):
    from xvc_amd import pipeline
    if (bd, strength, width, qp) not in _tables:
        _tables[bd, strength, width, qp] = pipeline.aqp_table(qp, bd, strength, width)
    return _tables[bd, strength, width, qp]


def expected_p(xo, bd, rdoq, part):
    """The model's P pass, once per (depth, quantiser, CU list)."""
    if (bd, rdoq, part) not in _expected:
        orig, ref = am.scene(bd)
        desc = am.descriptors(bd, rdoq, part)
        e = _expected[bd, rdoq, part] = am.p_pass(xo, desc, bd, orig, ref, table(bd))
        # what is compared is there: coded blocks in every component, vectors, QPs
        coded = [int((e[2][desc.tx["comp"] == c] != 0).sum()) for c in range(3)]
        assert min(coded) >= 10 and (e[1]["mv_x"] != 0).any(), coded
        assert len(set(e[3]["qp_y"].tolist())) >= 5
    return _expected[bd, rdoq, part]


# ---- the kernels alone -------------------------------------------------------------------
@pytest.mark.parametrize("part", [False, True], ids=["grid", "partition"])
def test_aqp_apply_equals_model(gpu, xo, part):
    """xvcgpu_aqp_apply on the 16x16 grid and on the partition (a 64x64 CU, 4-wide CUs, CUs in
    the cut CTUs), two job arrays: every array byte for byte against the model's - so the
    fields it does not name (planted ctx_index, flags and reserved bytes among them) stay."""
    api, ctx = gpu
    bd = 10
    desc = am.descriptors(bd, rdoq=True, part=part)
    n = desc.n_cus
    t = table(bd)
    ctu_var = am.ctu_variances(xo, am.W, am.H, am.scene(bd)[0][0])
    rng = np.random.default_rng(11)
    me0, me1 = desc.me.copy(), desc.me.copy()
    me1["mvp_x"], me1["prev_y"] = rng.integers(-99, 99, n), rng.integers(-99, 99, n)
    prm = desc.rdoq_params.copy()
    prm["ctx_index"], prm["flags"] = rng.integers(0, 60000, 3 * n), rng.integers(0, 4, 3 * n)
    prm["reserved"] = rng.integers(0, 256, (3 * n, 5))
    tx = desc.tx.copy()
    tx["tx_hor"], tx["dst4x4"] = rng.integers(0, 6, 3 * n), rng.integers(0, 2, 3 * n)
    (e0, e1), e_tx, e_prm, e_cu_qp, e_dqp, written = am.apply(t, ctu_var, [me0, me1], tx, prm,
                                                              desc.luma_idx)
    assert written.all() and len(set(e_cu_qp[:, 0].tolist())) >= 5
    bufs = [ctx.buffer(a) for a in (me0, me1, tx, prm, desc.luma_idx,
                                    np.ascontiguousarray(ctu_var, np.uint64))]
    d_me0, d_me1, d_tx, d_prm, d_luma, d_var = bufs
    d_cu_qp, d_dqp = poisoned(ctx, 2 * n + 16), poisoned(ctx, 12 + 16)
    bufs += [d_cu_qp, d_dqp]
    try:
        arrays = (C.c_void_p * 2)(d_me0.ptr, d_me1.ptr)
        ctx._check(ctx.lib.xvcgpu_aqp_apply(ctx.h, C.byref(t), d_var.ptr, arrays, 2, d_tx.ptr,
                                            d_prm.ptr, d_luma.ptr, n, d_cu_qp.ptr, d_dqp.ptr))
        ctx.sync()
        for name, buf, exp in (("jobs 0", d_me0, e0), ("jobs 1", d_me1, e1),
                               ("transform blocks", d_tx, e_tx), ("parameters", d_prm, e_prm)):
            got = buf.to_array(exp.dtype, len(exp))
            bad = differing(got, exp)
            assert not len(bad), (name, bad[:4], got[bad[:4]], exp[bad[:4]])
        got = d_cu_qp.to_array(np.int8, 2 * n + 16)
        assert np.array_equal(got[:2 * n].reshape(-1, 2), e_cu_qp)
        assert (got[2 * n:].view(np.uint8) == POISON).all()
        got = d_dqp.to_array(np.int8, 12 + 16)
        assert got[:12].tolist() == e_dqp.tolist() and (got[12:].view(np.uint8) == POISON).all()
        # QuantFast (no parameters) and no delta array: one job array, the rest as before
        ctx.h2d(d_me0.ptr, me0)
        ctx.h2d(d_tx.ptr, tx)
        ctx._check(ctx.lib.xvcgpu_memset(ctx.h, d_cu_qp.ptr, POISON, d_cu_qp.nbytes))
        ctx._check(ctx.lib.xvcgpu_memset(ctx.h, d_dqp.ptr, POISON, d_dqp.nbytes))
        one = (C.c_void_p * 1)(d_me0.ptr)
        ctx._check(ctx.lib.xvcgpu_aqp_apply(ctx.h, C.byref(t), d_var.ptr, one, 1, d_tx.ptr, None,
                                            d_luma.ptr, n, d_cu_qp.ptr, None))
        ctx.sync()
        assert not len(differing(d_me0.to_array(api.ME_DTYPE, n), e0))
        assert not len(differing(d_tx.to_array(api.TX_DTYPE, 3 * n), e_tx))
        assert not len(differing(d_me1.to_array(api.ME_DTYPE, n), e1))      # (untouched now)
        assert not len(differing(d_prm.to_array(api.RDOQ_PARAMS_DTYPE, 3 * n), e_prm))
        assert np.array_equal(d_cu_qp.to_array(np.int8, 2 * n).reshape(-1, 2), e_cu_qp)
        assert (d_dqp.to_array(np.uint8, 28) == POISON).all()
        # refused before a launch: no job array, a ctu_size that is none, a missing array
        for call in (
                lambda: ctx.lib.xvcgpu_aqp_apply(ctx.h, C.byref(t), d_var.ptr, one, 0, d_tx.ptr,
                                                 None, d_luma.ptr, n, d_cu_qp.ptr, None),
                lambda: ctx.lib.xvcgpu_aqp_apply(ctx.h, C.byref(t), d_var.ptr, one, 1, d_tx.ptr,
                                                 None, d_luma.ptr, n, None, None)):
            assert call() == 10
    finally:
        for b in bufs:
            b.free()


def test_cu_info_set_qp_alone(gpu):
    """qp_y and qp_c of 300 records (two workgroups) become the pair's; nothing else moves."""
    api, ctx = gpu
    n = 300
    rng = np.random.default_rng(12)
    cus = rng.integers(0, 256, (n + 2) * api.CU_DTYPE.itemsize, dtype=np.uint8).view(api.CU_DTYPE)
    cu_qp = rng.integers(0, 64, (n, 2)).astype(np.int8)
    d_cus, d_qp = ctx.buffer(cus), ctx.buffer(cu_qp)
    try:
        ctx._check(ctx.lib.xvcgpu_cu_info_set_qp(ctx.h, d_cus.ptr, d_qp.ptr, n))
        ctx.sync()
        exp = cus.copy()
        exp["qp_y"][:n], exp["qp_c"][:n] = cu_qp[:, 0], cu_qp[:, 1]
        got = d_cus.to_array(api.CU_DTYPE, n + 2)
        assert not len(differing(got, exp)) and len(differing(got, cus)) > n // 2
        assert ctx.lib.xvcgpu_cu_info_set_qp(ctx.h, None, d_qp.ptr, n) == 10
    finally:
        d_cus.free()
        d_qp.free()


# ---- the P pass --------------------------------------------------------------------------
class PScene:
    """The 200x136 scene on the device and a FramePass of the named form over it."""

    def __init__(self, ctx, bd, form, part=False, strength=am.STRENGTH):
        from xvc_amd import pipeline
        self.ctx, self.bd = ctx, bd
        orig, ref = am.scene(bd)
        self.O, self.R, self.Rec = (ctx.picture(am.W, am.H, bd) for _ in range(3))
        self.O.upload(orig, BL)
        self.R.upload(ref, BL)
        kw = dict(qp=am.QP, search_range=am.SEARCH_RANGE, keep_levels=True,
                  partition=am.partition_200() if part else None, aqp_strength=strength)
        if form == "residual":
            kw.update(fused=False)
        elif form == "residual_rdoq":
            kw.update(rdoq=True, fused=False)
        else:
            kw.update(rdoq=True, form="fwd_transform")
        self.fp = pipeline.FramePass(ctx, am.W, am.H, bd, **kw)
        assert self.fp.form == form and (self.fp.plan is not None) == part

    def run(self, **kw):
        self.Rec.upload([np.full_like(p, 0x0123) for p in am.scene(self.bd)[0]], BL)
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


def assert_p_equal(scene, got, exp, what):
    """got: PScene.run(); exp: am.p_pass's answer."""
    (res, nnz, cus, ssd), rec, levels = got
    e_rec, e_res, e_nnz, e_cus, e_ssd, e_cu_qp, e_dqp, e_levels = exp
    bad = differing(res, e_res)
    assert not len(bad), (what, "search", bad[:4], res[bad[:4]], e_res[bad[:4]])
    assert np.array_equal(nnz, e_nnz), (what, "nnz", np.flatnonzero(nnz != e_nnz)[:8])
    bad = differing(cus, e_cus)
    assert not len(bad), (what, "CU records", bad[:4], cus[bad[:4]], e_cus[bad[:4]])
    for c in range(3):
        assert np.array_equal(rec[c], e_rec[c]), (what, "plane", c,
                                                  np.argwhere(rec[c] != e_rec[c])[:4])
    assert (int(ssd[0]), int(ssd[1])) == e_ssd, (what, "ssd")
    assert np.array_equal(scene.fp.cu_qp(), e_cu_qp), (what, "cu_qp")
    assert np.array_equal(scene.fp.ctu_delta_qp(), e_dqp), (what, "ctu_dqp")
    for t, g in enumerate(split_levels(scene.ctx, scene.fp.desc, levels)):
        if e_nnz[t]:        # (a block without levels: its part of the buffer is unspecified)
            assert np.array_equal(g, e_levels[t]), (what, "levels of block", t)


_P_CASES = [(10, "residual", False), (10, "residual_rdoq", False), (10, "fwd_transform", False),
            (8, "fwd_transform", False), (10, "residual", True), (10, "residual_rdoq", True),
            (10, "fwd_transform", True), (8, "residual_rdoq", True)]


@pytest.mark.parametrize("bd,form,part", _P_CASES)
def test_p_pass_equals_model(gpu, xo, bd, form, part):
    """Search results, levels, nnz, CU records, reconstruction and SSD of the pass with
    adaptive QP against the model; the fused and the separate tail (the partition holds
    sides of 4: the separate one only); the records hold at least five luma QPs and the
    picture is not the flat pass's."""
    api, ctx = gpu
    exp = expected_p(xo, bd, form != "residual", part)
    s = PScene(ctx, bd, form, part)
    flat = PScene(ctx, bd, form, part, strength=None)
    try:
        assert s.fp.fused_tail == (not part)
        got = s.run()
        assert_p_equal(s, got, exp, "one call")
        assert len(set(got[0][2]["qp_y"].tolist())) >= 5
        assert s.fp.ctu_delta_qp().tolist() == [list(r) for r in am.SCENE_DELTAS]
        if not part:
            assert_p_equal(s, s.run(fused_tail=False), exp, "separate tail")
        else:       # the plan: every search class of the partition is in it
            counts = dict(zip(api.ME_PLAN_BIN_NAMES, s.fp.plan.counts.tolist()))
            assert counts["16x16"] and counts["c32"] and counts["other16"] and \
                counts["c64_team"] + counts["c64_wave"] == 1 and not counts["unsupported"], counts
        # a second run of the same object: the arrays it wrote itself change nothing
        assert_p_equal(s, s.run(), exp, "again")
        (_, f_nnz, f_cus, _), f_rec, _ = flat.run()
        assert set(f_cus["qp_y"].tolist()) == {am.QP}
        assert any(not np.array_equal(a, b) for a, b in zip(f_rec, got[1]))
    finally:
        s.destroy()
        flat.destroy()


@pytest.mark.parametrize("form,part", [("residual", False), ("fwd_transform", False),
                                       ("residual_rdoq", True)])
def test_strength_zero_equals_flat_pass(gpu, form, part):
    """A table of strength 0 holds delta 0 for every statistic: the pass with it gives the
    flat pass's bytes - results, records, levels, picture."""
    api, ctx = gpu
    bd = 10
    a, f = PScene(ctx, bd, form, part, strength=0), PScene(ctx, bd, form, part, strength=None)
    try:
        (ra, pa, la), (rf, pf, lf) = a.run(), f.run()
        assert not a.fp.ctu_delta_qp().any()
        assert all(not len(differing(x, y)) for x, y in zip(ra, rf))
        assert all(np.array_equal(x, y) for x, y in zip(pa, pf))
        for t, (g, e) in enumerate(zip(split_levels(ctx, a.fp.desc, la),
                                       split_levels(ctx, f.fp.desc, lf))):
            if rf[1][t]:
                assert np.array_equal(g, e), t
        assert rf[1].any() and rf[0]["subpel_dist"].any()
        # the job arrays hold what they held: the flat pass's values
        d = a.fp.desc
        assert not len(differing(a.fp.d_me.to_array(api.ME_DTYPE, d.n_cus), d.me))
        assert not len(differing(a.fp.d_tx.to_array(api.TX_DTYPE, len(d.tx)), d.tx))
        if a.fp.rdoq:
            assert not len(differing(a.fp.d_rdoq_prm.to_array(api.RDOQ_PARAMS_DTYPE, len(d.tx)),
                                     d.rdoq_params))
    finally:
        a.destroy()
        f.destroy()


# ---- the B pass --------------------------------------------------------------------------
class BScene:
    """aqp_pass_model.b_scene(name) on the device and a BiRefsFramePass with adaptive QP."""

    def __init__(self, ctx, name, which, form, strength=am.STRENGTH):
        from xvc_amd import pipeline
        pw, ph, bd, part, orig, refs = am.b_scene(name)
        self.ctx, self.size, self.name = ctx, (pw, ph, bd), name
        self.lists = lists = rm.SETS[which]
        self.O, self.Rec = ctx.picture(pw, ph, bd), ctx.picture(pw, ph, bd)
        self.O.upload(orig, BL)
        self.by_poc = {}
        for poc in sorted(set(lists[0]) | set(lists[1])):
            self.by_poc[poc] = ctx.picture(pw, ph, bd)
            self.by_poc[poc].upload(refs[poc], BL)
        self.refs = [[self.by_poc[poc] for poc in lists[l]] for l in range(2)]
        self.fp = pipeline.BiRefsFramePass(
            ctx, pw, ph, bd, rm.QP, rdoq=form != "residual", rdoq_packed=form == "fwd_transform",
            partition=part, cur_poc=rm.CUR_POC, ref_pocs=lists, search_range=rm.SEARCH_RANGE,
            side_bits=rm.SIDE_BITS, aqp_strength=strength)
        assert self.fp.form == form
        me = [[self.fp.desc.me.copy() for _ in lists[l]] for l in range(2)]
        for l in range(2):
            for r, poc in enumerate(lists[l]):
                me[l][r]["search_range"] = rm.search_range(poc)
        self.fp.set_jobs(me)

    def run(self, **kw):
        self.Rec.upload([np.full_like(p, 0x0123) for p in am.b_scene(self.name)[4]], BL)
        self.fp.run(self.O, self.refs, self.Rec, **kw)
        self.ctx.sync()
        return self.fp.results(), self.Rec.download(BL)

    def destroy(self):
        self.fp.destroy()
        for p in [self.O, self.Rec] + list(self.by_poc.values()):
            p.destroy()


@pytest.mark.parametrize("name,form,which", [
    ("grid10", "residual_rdoq", "A"), ("grid10", "residual_rdoq", "C"),
    ("part10", "fwd_transform", "A"), ("part10", "fwd_transform", "C")])
def test_b_pass_equals_model(gpu, xo, name, form, which):
    """Sets A and C of bi_refs_pass_model with a contrast per CTU: searches, folds, choice,
    refinement, nnz, levels, prediction, CU records, picture and SSD against the model."""
    import test_gpu_bi_refs_frame_pass as tb
    api, ctx = gpu
    pw, ph, bd = am.b_scene(name)[:3]
    t = table(bd, width=pw, qp=rm.QP)
    exp, e_cu_qp, e_dqp = am.b_pass(xo, name, which, True, t)
    assert len(set(e_dqp.ravel().tolist())) >= 3, e_dqp
    s = BScene(ctx, name, which, form)
    try:
        got = s.run()
        tb.assert_pass_equal(got, exp, "one call", s)
        assert np.array_equal(s.fp.cu_qp(), e_cu_qp)
        assert np.array_equal(s.fp.ctu_delta_qp(), e_dqp)
        assert len(set(got[0][2]["qp_y"].tolist())) >= 3
        # every (list, picture)'s jobs carry the CU's lambda16, re-used entries too
        k = e_cu_qp[:, 0].astype(int) - (rm.QP + am.DELTA_MIN)
        lam = np.array(list(t.lambda16), np.uint32)[k]
        for l in range(2):
            for b in s.fp.d_me[l]:
                assert np.array_equal(b.to_array(api.ME_DTYPE, len(lam))["lambda16"], lam)
        if name == "part10":
            tb.assert_pass_equal(s.run(planned=False), exp, "without plans", s)
        else:
            tb.assert_pass_equal(s.run(fused_tail=False), exp, "separate tail", s)
    finally:
        s.destroy()


# ---- refusals ----------------------------------------------------------------------------
def _p_buffers(fp):
    return [fp.d_res, fp.d_nnz, fp.d_cus, fp.d_ssd, fp.d_levels, fp.aqp.d_var16,
            fp.aqp.d_ctu_var, fp.aqp.d_ctu_dqp, fp.aqp.d_cu_qp]


def test_p_refusals_enqueue_nothing(gpu):
    """Both _from_me forms, a NULL array, a row shard, a ctus_per_row that does not fit the
    width, a ctu_size that is none, phases without ENCODE: XVCGPU_INVALID_ARGUMENT naming the
    field, with every output buffer, the job arrays and rec as they were."""
    api, ctx = gpu
    s = PScene(ctx, 10, "fwd_transform")
    try:
        fp, d = s.fp, s.fp.desc
        s.Rec.upload([np.full_like(p, 0x0123) for p in am.scene(10)[0]], BL)
        bufs = _p_buffers(fp)
        for b in bufs:
            ctx._check(ctx.lib.xvcgpu_memset(ctx.h, b.ptr, POISON, b.nbytes))
        form = api.FP_FORM_NAMES.index

        def a_set(**kw):
            return lambda a, q: [setattr(a, k, v) for k, v in kw.items()]

        def q_set(**kw):
            return lambda a, q: [setattr(q, k, v) for k, v in kw.items()]

        def t_set(**kw):
            return lambda a, q: [setattr(q.table, k, v) for k, v in kw.items()]
        cases = [
            (a_set(form=form("recon_from_me")), "frame_pass_aqp: the form must be", ALL),
            (a_set(form=form("fwd_from_me")), "frame_pass_aqp: the form must be", ALL),
            (q_set(d_cu_qp=None), "d_cu_qp", ALL),
            (q_set(d_var16=None), "d_var16", ALL),
            (q_set(d_ctu_var=None), "d_ctu_var", ALL),
            (a_set(db_y_end=64), "whole pictures", ALL),
            (a_set(ssd_y_begin=8), "whole pictures", ALL),
            (a_set(n_cus_total=d.n_cus + 1), "whole pictures", ALL),
            (t_set(ctus_per_row=3), "ctus_per_row", ALL),
            (t_set(ctus_per_row=5), "ctus_per_row", ALL),
            (t_set(ctu_size=48), "ctu_size", ALL),
            (a_set(d_tx=None), "d_tx", ALL),
            (a_set(), "phases", ALL & ~api.FP_ENCODE),
        ]
        for change, match, phases in cases:
            a, q = fp._call_args(s.O, s.R, s.Rec), fp.aqp.args()
            change(a, q)
            with pytest.raises(api.XvcGpuError, match="status 10: .*" + match):
                ctx._check(ctx.lib.xvcgpu_frame_pass_aqp(ctx.h, C.byref(a), C.byref(q), None,
                                                         phases))
            ctx.sync()
            for b in bufs:
                assert (b.to_array(np.uint8, b.nbytes) == POISON).all(), match
            assert all((p == 0x0123).all() for p in s.Rec.download(BL)), match
            assert not len(differing(fp.d_me.to_array(api.ME_DTYPE, d.n_cus), d.me)), match
            assert not len(differing(fp.d_tx.to_array(api.TX_DTYPE, len(d.tx)), d.tx)), match
        # no xvcgpu_aqp_args at all
        a = fp._call_args(s.O, s.R, s.Rec)
        assert ctx.lib.xvcgpu_frame_pass_aqp(ctx.h, C.byref(a), None, None, ALL) == 10
        # ... and the same blocks run when nothing is wrong with them
        (_, _, cus, _), _, _ = s.run()
        assert len(set(cus["qp_y"].tolist())) >= 5
    finally:
        s.destroy()


def test_python_refusals(gpu):
    """A negative strength and a form the pass refuses raise ValueError before anything is
    allocated; a row shard too."""
    from xvc_amd import pipeline
    api, ctx = gpu
    with pytest.raises(ValueError, match="strength"):
        pipeline.FramePass(ctx, am.W, am.H, 10, fused=False, aqp_strength=-1)
    with pytest.raises(ValueError, match="strength"):
        pipeline.BiRefsFramePass(ctx, 104, 72, 10, aqp_strength=-3)
    with pytest.raises(ValueError, match="recon_from_me"):
        pipeline.FramePass(ctx, am.W, am.H, 10, aqp_strength=13)
    with pytest.raises(ValueError, match="fwd_from_me"):
        pipeline.FramePass(ctx, am.W, am.H, 10, rdoq=True, aqp_strength=13)
    with pytest.raises(ValueError, match="whole pictures"):
        pipeline.FramePass(ctx, am.W, am.H, 10, fused=False, row_range=(0, 64), aqp_strength=13)
    with pytest.raises(ValueError, match="form"):
        pipeline.FramePass(ctx, am.W, am.H, 10, form="residual_rdoq")


def test_b_refusals_enqueue_nothing(gpu):
    api, ctx = gpu
    s = BScene(ctx, "grid10", "C", "residual_rdoq")
    try:
        fp = s.fp
        s.Rec.upload([np.full_like(p, 0x0123) for p in am.b_scene("grid10")[4]], BL)
        bufs = [fp.d_choice, fp.p.d_nnz, fp.p.d_cus, fp.d_inter, fp.d_bi_jobs, fp.d_bi_res,
                fp.d_bi_slots, fp.aqp.d_var16, fp.aqp.d_ctu_var, fp.aqp.d_ctu_dqp,
                fp.aqp.d_cu_qp] + [b for row in fp.d_res for b in row if b is not None]
        for b in bufs:
            ctx._check(ctx.lib.xvcgpu_memset(ctx.h, b.ptr, POISON, b.nbytes))
        form = api.FP_FORM_NAMES.index

        def case(change, match):
            a, q = fp._call_args(s.O, s.refs, s.Rec), fp.aqp.args()
            change(a, q)
            with pytest.raises(api.XvcGpuError, match="status 10: .*" + match):
                ctx._check(ctx.lib.xvcgpu_frame_pass_bi_refs_aqp(
                    ctx.h, C.byref(a), C.byref(q), fp.plan_handles(), ALL))
            ctx.sync()
            for b in bufs:
                assert (b.to_array(np.uint8, b.nbytes) == POISON).all(), match
            assert all((p == 0x0123).all() for p in s.Rec.download(BL)), match
            for l in range(2):
                for r, b in enumerate(fp.d_me[l]):
                    assert not len(differing(b.to_array(api.ME_DTYPE, len(fp.me[l][r])),
                                             fp.me[l][r])), match
        case(lambda a, q: setattr(a.p, "form", form("recon_from_me")), "form")
        case(lambda a, q: setattr(a.p, "form", form("fwd_from_me")), "form")
        case(lambda a, q: setattr(q, "d_ctu_var", None), "d_ctu_var")
        case(lambda a, q: setattr(q, "d_cu_qp", None), "d_cu_qp")
        case(lambda a, q: setattr(a.p, "db_y_end", 16), "whole pictures")
        case(lambda a, q: setattr(q.table, "ctus_per_row", 1), "ctus_per_row")
        case(lambda a, q: setattr(a, "force_l1_mvd_zero", 1), "force_l1_mvd_zero")
        assert int(s.run()[0][4]["inter_dir"].max()) == 2
    finally:
        s.destroy()


# ---- state and the C++ class -------------------------------------------------------------
def test_flat_pass_untouched_beside_the_aqp_pass(gpu):
    """Flat FramePass objects answer the same before and after a pass with adaptive QP ran
    on their context: no scratch or context state leaks between them."""
    api, ctx = gpu
    flats = [PScene(ctx, 10, "fwd_transform", strength=None),
             PScene(ctx, 10, "residual", strength=None)]
    s = PScene(ctx, 10, "fwd_transform")
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


def test_host_class_equals_python_pass(gpu):
    """xvc_gpu::FramePass with SetAdaptiveQp (through xvc_host_frame_pass_aqp) equals
    pipeline.FramePass(aqp_strength=...): search results, CU records, QP map, SSD, picture."""
    from xvc_amd import decoder
    api, ctx = gpu
    L = decoder.load_host_library()
    L.xvc_host_frame_pass_aqp.argtypes = [C.c_void_p] + [C.c_int] * 6 + [C.c_void_p] * 3 + \
        [C.c_int] * 3 + [C.c_void_p] * 5
    bd = 10
    s = PScene(ctx, bd, "residual")
    Rec = ctx.picture(am.W, am.H, bd)
    try:
        (res, nnz, cus, ssd), rec, _ = s.run(fused_tail=False)
        n = s.fp.desc.n_cus
        h_res, h_cus = np.zeros(n, api.MERES_DTYPE), np.zeros(n, api.CU_DTYPE)
        h_ssd, h_dqp, h_qp = np.zeros(2, np.uint64), np.zeros(12, np.int8), np.zeros((n, 2), np.int8)
        assert L.xvc_host_frame_pass_aqp(
            ctx.h, am.W, am.H, bd, am.QP, am.STRENGTH, am.SEARCH_RANGE, s.O.h_pic, s.R.h_pic,
            Rec.h_pic, 0, n, 12, h_res.ctypes.data, h_cus.ctypes.data, h_ssd.ctypes.data,
            h_dqp.ctypes.data, h_qp.ctypes.data) == 0
        assert not len(differing(h_res, res)) and not len(differing(h_cus, cus))
        assert h_ssd.tolist() == ssd.tolist()
        assert np.array_equal(h_dqp.reshape(3, 4), s.fp.ctu_delta_qp())
        assert np.array_equal(h_qp, s.fp.cu_qp())
        assert all(np.array_equal(x, y) for x, y in zip(Rec.download(BL), rec))
        assert len(set(h_cus["qp_y"].tolist())) >= 5
        # a negative strength: refused by the class
        assert L.xvc_host_frame_pass_aqp(
            ctx.h, am.W, am.H, bd, am.QP, -1, am.SEARCH_RANGE, s.O.h_pic, s.R.h_pic, Rec.h_pic,
            0, n, 12, h_res.ctypes.data, h_cus.ctypes.data, h_ssd.ctypes.data,
            h_dqp.ctypes.data, h_qp.ctypes.data) == 10
    finally:
        Rec.destroy()
        s.destroy()
