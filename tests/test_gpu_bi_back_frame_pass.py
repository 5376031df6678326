"""The frame pass of a B picture with only back references on the GPU
(xvcgpu_frame_pass_bi_back, pipeline.BiRefsFramePass(low_delay=True)): the predictor-cost
kernel and the two folds alone, the whole pass bit-exact against the model composed of the
oracle's pieces (tests/bi_back_pass_model.py, which tests/test_bi_back_pass_model.py pins to
the reference), the one call against its parts, adaptive QP, the refusals, the
two-directional pass beside it on one context and the C++ class."""
import ctypes as C

import numpy as np
import pytest

import aqp_pass_model as am
import bi_back_pass_model as bm
import bi_refs_pass_model as rm
import helpers
import oracle_lib as ol

pytestmark = pytest.mark.gpu

BL = bm.BL
ALL = 31    # FP_ENCODE | FP_DEBLOCK_V | FP_DEBLOCK_H | FP_PAD | FP_SSD
NONE = bm.NONE


@pytest.fixture(scope="module")
def gpu():
    from xvc_amd import api
    ctx = api.Context(0)
    yield api, ctx
    ctx.close()


@pytest.fixture(scope="module")
def xo():
    return ol.Lib("xo")


@pytest.fixture(scope="module")
def tb():
    """The B pass's test helpers (Folds, differing, assert_pass_equal, as_expected)."""
    import test_gpu_bi_refs_frame_pass as t
    return t


_inputs, _searched, _expected = {}, {}, {}


def model_input(name):
    if name not in _inputs:
        _inputs[name] = bm.make_refs(name)
    return _inputs[name]


def expected(xo, name, which, rdoq):
    """The model's pass, computed once per (input, set, quantiser) and shared."""
    if (name, which, rdoq) not in _expected:
        pw, ph, bd, _, orig, refs = model_input(name)
        lists = bm.SETS[which]
        desc = bm.descriptors(name, rdoq)
        if (name, which) not in _searched:
            _searched[name, which] = bm.search_motion(xo, bd, pw, ph, orig[0], refs, lists,
                                                      bm.jobs(desc, lists), key=name)
        _expected[name, which, rdoq] = bm.frame_pass(xo, desc, bd, orig, refs, lists,
                                                     _searched[name, which])
    return _expected[name, which, rdoq]


class Scene:
    """The input's pictures on the device and a BiRefsFramePass(low_delay=True) over them.
    pictures: (orig, {poc: planes}) in place of the input's own."""

    def __init__(self, ctx, name, which="E", form="residual", pictures=None, low_delay=True,
                 lists=None, cur_poc=bm.CUR_POC, **kw):
        from xvc_amd import pipeline
        pw, ph, bd, part, orig, refs = model_input(name)
        if pictures is not None:
            orig, refs = pictures
        self.ctx, self.size, self.fill = ctx, (pw, ph, bd), orig
        self.lists = lists = bm.SETS[which] if lists is None else lists
        self.O, self.Rec = ctx.picture(pw, ph, bd), ctx.picture(pw, ph, bd)
        self.O.upload(orig, BL)
        self.by_poc = {}
        for poc in sorted(set(lists[0]) | set(lists[1])):
            self.by_poc[poc] = ctx.picture(pw, ph, bd)
            self.by_poc[poc].upload(refs[poc], BL)
        self.refs = [[self.by_poc[poc] for poc in lists[l]] for l in range(2)]
        self.fp = pipeline.BiRefsFramePass(
            ctx, pw, ph, bd, bm.QP, rdoq=form != "residual", rdoq_packed=form == "fwd_transform",
            partition=part, cur_poc=cur_poc, ref_pocs=lists, search_range=bm.SEARCH_RANGE,
            side_bits=bm.SIDE_BITS, low_delay=low_delay, **kw)
        assert self.fp.form == form
        base = self.fp.desc.me.copy()
        if "aqp_strength" not in kw:
            base["lambda16"] = bm.LAMBDA16
        self.me = [[base.copy() for _ in lists[l]] for l in range(2)]
        for l in range(2):
            for r, poc in enumerate(lists[l]):
                self.me[l][r]["search_range"] = min(256, max(96, (256 * abs(cur_poc - poc) + 8) // 16))
        self.fp.set_jobs(self.me)

    def clear(self, value=0):
        self.Rec.upload([np.full_like(p, value) for p in self.fill], BL)

    def run(self, **kw):
        self.fp.run(self.O, self.refs, self.Rec, **kw)
        self.ctx.sync()
        return self.fp.results(), self.Rec.download(BL)

    def destroy(self):
        self.fp.destroy()
        for p in [self.O, self.Rec] + list(self.by_poc.values()):
            p.destroy()


def assert_back_equal(tb, api, s, got, exp, what):
    """tb.assert_pass_equal and what the low-delay pass adds: the predictor costs, the
    refinement jobs where there is one, the prediction jobs."""
    tb.assert_pass_equal(got, exp, what, s)
    fp, n = s.fp, s.fp.desc.n_cus
    cost = fp.l1_mvp_cost()
    assert np.array_equal(cost, exp[10]), (what, "predictor costs",
                                           np.argwhere(cost != exp[10])[:4])
    e_slots, e_jobs = exp[7], exp[11]
    job = (e_slots[:, :, 0] != bm.NO_JOB).reshape(-1)
    jobs = fp.d_bi_jobs.to_array(api.BI_DTYPE, n * fp.rmax)
    assert not len(tb.differing(jobs[job], e_jobs.reshape(-1)[job])), (what, "refinement jobs")
    choice = got[0][4]
    inter = fp.d_inter.to_array(api.INTER_DTYPE, 3 * n).reshape(n, 3)
    _, _, _, slot = bm.tables(s.lists)
    for i in range(n):
        c = choice[i]
        ref = [slot[l][int(c["ref_idx"][l])] if int(c["ref_idx"][l]) >= 0 else -1 for l in (0, 1)]
        for comp in range(3):
            q = inter[i][comp]
            assert q["ref"].tolist() == ref and int(q["comp"]) == comp and \
                q["mv"][:, 0].tolist() == c["mv"].tolist(), (what, "prediction job", i, comp)


# ---- the three kernels alone -------------------------------------------------------------
def _back_folds(tb, api, ctx, lists, me, res, orig=None, pics=None):
    """tb.Folds with the flag set, the predictor-cost array and, for the predictor-cost
    kernel, the pictures."""
    f = tb.Folds(api, ctx, lists, me, res)
    f.args.force_l1_mvd_zero = 1
    f.l1 = f.poisoned(4 * api.CS_MAX_REFS * f.n)
    if orig is not None:
        f.args.p.orig = orig.h_pic
        for k, p in enumerate(pics):
            f.args.refs[k] = p.h_pic
    return f


def _call_with_cost(f, name):
    f.ctx._check(getattr(f.ctx.lib, name)(f.ctx.h, C.byref(f.args), f.l1.ptr))
    f.ctx.sync()


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_predictor_cost_kernel_alone(gpu, xo, tb, bd):
    """xvcgpu_fp_bi_back_mvp_cost against bm.mvp_cost on every shape of partition_128 (sides
    of 4 included) with planted predictors of up to +-40 and, for every third CU, +-3000
    (ClipMv changes them), two list-1 pictures of three slots, per-CU lambdas; a shape the
    kernel does not take answers UINT32_MAX."""
    api, ctx = gpu
    rng = np.random.default_rng(6100 + bd)
    pw = ph = 128
    orig, ref_a = helpers.make_pics(rng, bd, pw, ph, BL, (3, -2))
    ref_b = np.ascontiguousarray(np.roll(ref_a, (2, -5), (0, 1)))
    lists = ((16,), (12, 16))       # list 1: a unique picture (slot 1) and the re-used one
    planes = {16: ref_a, 12: ref_b}
    rects = np.concatenate([rm.partition_128(), np.array([(0, 0, 12, 8), (16, 0, 8, 2)])])
    n = len(rects)
    base = np.zeros(n, api.ME_DTYPE)
    base["x"], base["y"], base["w"], base["h"] = rects.T
    base["depth_nonzero"], base["search_range"] = 1, 96
    base["lambda16"] = rng.choice([20000, 498000, 1500000], n)
    me = [[base.copy()], [base.copy(), base.copy()]]
    for r in range(2):
        q = me[1][r]
        q["mvp_x"], q["mvp_y"] = rng.integers(-40, 41, (2, n))
        q["mvp_x"][r::3] = rng.choice([-3000, 3000], len(q["mvp_x"][r::3]))
        q["mvp_y"][r::3] = rng.choice([-3000, 0, 3000], len(q["mvp_y"][r::3]))
    res = [[np.zeros(n, api.MERES_DTYPE)], [np.zeros(n, api.MERES_DTYPE), None]]
    exp = np.full((n, 3), NONE, np.uint32)
    for r, poc in enumerate(lists[1]):
        for i in range(n):
            exp[i][r] = bm.mvp_cost(xo, bd, pw, ph, orig, planes[poc], me[1][r][i])
    assert (exp[-2:, :2] == NONE).all() and (exp[:-2, :2] != NONE).all()
    assert len(set(exp[:-2, :2].ravel().tolist())) > n
    O, A, B = (ctx.picture(pw, ph, bd) for _ in range(3))
    O.upload([orig, None, None], BL)
    A.upload([ref_a, None, None], BL)
    B.upload([ref_b, None, None], BL)
    f = _back_folds(tb, api, ctx, lists, me, res, O, [A, B])
    try:
        _call_with_cost(f, "xvcgpu_fp_bi_back_mvp_cost")
        got = f.l1.to_array(np.uint32, 3 * n).reshape(n, 3)
        assert np.array_equal(got, exp), (np.argwhere(got != exp)[:6], got[got != exp][:6],
                                          exp[got != exp][:6])
        # nothing else of the block's arrays is written
        for b in (f.jobs, f.bi, f.slots, f.choice, f.inter):
            assert (b.to_array(np.uint8, b.nbytes) == 0xA5).all()
    finally:
        f.destroy()
        for p in (O, A, B):
            p.destroy()


def _hand_made(api, lists, n, seed):
    num_ref, same, _, _ = bm.tables(lists)
    rng = np.random.default_rng(seed)
    base = np.zeros(n, api.ME_DTYPE)
    base["x"], base["y"] = 8 * (np.arange(n) % 8), 8 * (np.arange(n) // 8)
    base["w"], base["h"] = rng.choice([4, 8], n), rng.choice([4, 8], n)
    base["depth_nonzero"], base["lambda16"] = 1, rng.choice([120000, 498000, 1500000], n)
    base["fullpel_mv"] = rng.integers(0, 5, n) == 0
    me = [[base.copy() for _ in range(num_ref[l])] for l in range(2)]
    res = [[None] * num_ref[l] for l in range(2)]
    for l in range(2):
        for r in range(num_ref[l]):
            me[l][r]["mvp_x"], me[l][r]["mvp_y"] = rng.integers(-160, 161, (2, n))
            if l == 0 or same[r] < 0:
                q = res[l][r] = np.zeros(n, api.MERES_DTYPE)
                q["mv_x"], q["mv_y"] = rng.integers(-300, 301, (2, n))
                q["subpel_dist"] = rng.integers(400, 3000, n)
    bi = np.zeros((n, max(num_ref)), api.MERES_DTYPE)
    bi["mv_x"], bi["mv_y"] = rng.integers(-300, 301, (2,) + bi.shape)
    bi["subpel_dist"] = rng.integers(300, 2500, bi.shape)
    l1 = np.full((n, bm.MAX_REFS), NONE, np.uint32)
    l1[:, :num_ref[1]] = rng.integers(500, 4000, (n, num_ref[1]))
    return me, res, bi, l1


def test_folds_alone_on_hand_made_inputs(gpu, tb):
    """xvcgpu_fp_bi_back_uni_fold and xvcgpu_fp_bi_back_choice byte for byte against the
    model's folds on 48 CUs of set F (list 1: one re-used and two unique pictures, Rmax 3, a
    no-job third slot) with planted ties, unsupported entries, full-pel CUs; what a fold does
    not write stays as it was."""
    api, ctx = gpu
    lists = bm.SETS["F"]
    n = 48
    me, res, bi, l1 = _hand_made(api, lists, n, 91)
    # CUs 4 .. 6: an unsupported list-0 search, unique list-1 search, predictor cost
    res[0][1]["subpel_dist"][4] = NONE
    res[1][2]["subpel_dist"][5] = NONE
    l1[6][0] = NONE
    # CUs 8 .. 15: equal predictor costs below the third: the lower index stays
    l1[8:12, 0] = l1[8:12, 1] = 300
    l1[12:16, 1] = l1[12:16, 2] = 300
    # CUs 16 .. 23: list 0's pictures tie (the same predictor and result, one index bit each)
    for i in range(16, 24):
        for a in (me, res):
            a[0][1][i] = a[0][0][i]
    choice0, jobs, slots = bm.uni_fold(lists, me, res, l1)
    # CUs 24 .. 31: cost_bi == cost_l0 <= cost_l1_unique gives bi
    trial, _ = bm.choice_fold(lists, me, res, bi, choice0)
    planted = 0
    for i in range(24, 32):
        c = trial[i]
        bits_cost = int(c["bi_cost"][0]) - int(bi[i][0]["subpel_dist"])
        if int(c["cost_list"][0]) > int(c["cost_l1_unique"]) or int(c["cost_list"][0]) < bits_cost:
            continue
        bi["subpel_dist"][i] = 100000
        bi[i][0]["subpel_dist"] = int(c["cost_list"][0]) - bits_cost
        planted += 1
    assert planted >= 2
    # CUs 32 .. 39: cost_l0 == cost_l1_unique below cost_bi gives list 0
    for i in range(32, 40):
        bi["subpel_dist"][i] = 100000
        res[0][0]["subpel_dist"][i], res[0][1]["subpel_dist"][i] = 100, 50000
        res[1][1]["subpel_dist"][i] = 60000
        res[1][2]["subpel_dist"][i] += 2000
    choice0, jobs, slots = bm.uni_fold(lists, me, res, l1)
    for i in range(32, 40):     # (cost = dist + a constant of the CU: move list 0's to the tie)
        d = int(choice0[i]["cost_l1_unique"]) - int(choice0[i]["cost_list"][0])
        assert d > 0 and int(choice0[i]["best_ref"][0]) == 0
        res[0][0]["subpel_dist"][i] += d
    choice0, jobs, slots = bm.uni_fold(lists, me, res, l1)
    e_choice, e_inter = bm.choice_fold(lists, me, res, bi, choice0)
    # what was planted is what the model sees
    assert (e_choice[4:7].view(np.uint8) == 0xff).all() and (slots[4:7] == bm.NO_JOB).all()
    assert (e_choice["best_ref"][8:12, 1] == 0).all() and (e_choice["best_ref"][12:16, 1] == 1).all()
    c = e_choice[16:24]
    assert (c["cost_uni"][:, 0, 0] == c["cost_uni"][:, 0, 1]).all() and (c["best_ref"][:, 0] == 0).all()
    c = e_choice[24:32]
    assert ((c["cost_bi"] == c["cost_list"][:, 0]) & (c["inter_dir"] == 2)).sum() == planted
    c = e_choice[32:40]
    assert (c["cost_list"][:, 0] == c["cost_l1_unique"]).all() and (c["inter_dir"] == 0).all()
    ok = np.ones(n, bool)
    ok[4:7] = False
    assert len(set(e_choice["inter_dir"][ok].tolist())) == 3
    assert (e_choice["search_list"][ok] == 0).all()
    assert (slots[ok, 2, 0] == bm.NO_JOB).all() and (slots[ok, :2, 0] != bm.NO_JOB).all()

    f = _back_folds(tb, api, ctx, lists, me, res)
    try:
        ctx.h2d(f.l1.ptr, l1)
        ctx.h2d(f.bi.ptr, bi)
        _call_with_cost(f, "xvcgpu_fp_bi_back_uni_fold")
        got = f.choice.to_array(api.FP_BI_REFS_RESULT_DTYPE, n)
        bad = tb.differing(got, choice0)
        assert not len(bad), ("uni fold", bad[:4], got[bad[:4]], choice0[bad[:4]])
        g_slots = f.slots.to_array(np.uint8, 2 * n * 3).reshape(n, 3, 2)
        assert np.array_equal(g_slots, slots)
        g_jobs = f.jobs.to_array(api.BI_DTYPE, n * 3).reshape(n, 3)
        job = slots[:, :, 0] != bm.NO_JOB
        assert not len(tb.differing(g_jobs[job], jobs[job]))
        assert (g_jobs[~job].view(np.uint8) == 0xA5).all()      # no job: not written
        assert np.array_equal(f.l1.to_array(np.uint32, 3 * n).reshape(n, 3), l1)
        assert not len(tb.differing(f.bi.to_array(api.MERES_DTYPE, 3 * n), bi.reshape(-1)))
        assert (f.inter.to_array(np.uint8, f.inter.nbytes) == 0xA5).all()
        f.call("xvcgpu_fp_bi_back_choice")
        got = f.choice.to_array(api.FP_BI_REFS_RESULT_DTYPE, n)
        bad = tb.differing(got, e_choice)
        assert not len(bad), ("choice", bad[:4], got[bad[:4]], e_choice[bad[:4]])
        g_inter = f.inter.to_array(api.INTER_DTYPE, 3 * n)
        e = np.zeros(3 * n, api.INTER_DTYPE)
        for i, (x, y, w, h, ref, mv) in enumerate(e_inter):
            for comp in range(3):
                q = e[3 * i + comp]
                q["x"], q["y"], q["w"], q["h"], q["comp"] = x, y, w, h, comp
                q["ref"] = ref
                q["mv"][0][0], q["mv"][1][0] = mv[0], mv[1]
        assert not len(tb.differing(g_inter, e))
        # the choice wrote the records and the prediction jobs only
        assert np.array_equal(f.slots.to_array(np.uint8, 2 * n * 3).reshape(n, 3, 2), slots)
        assert not len(tb.differing(f.jobs.to_array(api.BI_DTYPE, n * 3), g_jobs.reshape(-1)))
        assert (f.cus.to_array(np.uint8, f.cus.nbytes) == 0xA5).all()
    finally:
        f.destroy()


# ---- the whole pass ----------------------------------------------------------------------
@pytest.mark.parametrize("name,form,which", [
    ("grid10", "residual", "E"), ("grid8", "fwd_transform", "F"),
    ("part10", "residual_rdoq", "G"), ("part10", "fwd_transform", "E"),
    ("grid10", "residual_rdoq", "F"), ("grid8", "residual", "H")])
def test_whole_pass_equals_model(gpu, xo, tb, name, form, which):
    api, ctx = gpu
    exp = expected(xo, name, which, form != "residual")
    s = Scene(ctx, name, which, form)
    try:
        assert s.fp.p.fused_tail == (name != "part10")      # the partition holds sides of 4
        planned = name == "part10"
        assert all((p is not None) == (planned and s.fp.searched[l][r])
                   for l in range(2) for r, p in enumerate(s.fp.plans[l]))
        assert_back_equal(tb, api, s, s.run(), exp, "one call")
        s.clear()
        if planned:     # sized searches, whole-list class launches
            assert_back_equal(tb, api, s, s.run(planned=False), exp, "without plans")
        else:
            assert_back_equal(tb, api, s, s.run(fused_tail=False), exp, "separate tail")
    finally:
        s.destroy()


def test_planted_predictors_equal_model(gpu, xo, tb):
    """Set F on the grid with a non-zero predictor per (list, picture) and CU, some of list
    1's far outside the picture: the predictor is list 1's candidate, the refinement's other
    vector and the bi-directional CU's list-1 vector."""
    api, ctx = gpu
    name, which = "grid10", "F"
    pw, ph, bd, _, orig, refs = model_input(name)
    lists = bm.SETS[which]
    desc = bm.descriptors(name)
    me = bm.jobs(desc, lists)
    rng = np.random.default_rng(77)
    for l in range(2):
        for r in range(len(lists[l])):
            me[l][r]["mvp_x"], me[l][r]["mvp_y"] = rng.integers(-40, 41, (2, desc.n_cus))
    me[1][0]["mvp_x"][::7], me[1][1]["mvp_y"][::5] = 3000, -3000
    searched = bm.search_motion(xo, bd, pw, ph, orig[0], refs, lists, me)
    exp = bm.frame_pass(xo, desc, bd, orig, refs, lists, searched)
    choice = exp[5]
    is_bi = choice["inter_dir"] == 2
    assert is_bi.sum() >= 3 and choice["mv"][is_bi, 1].any()
    s = Scene(ctx, name, which)
    try:
        s.fp.set_jobs(me)
        assert_back_equal(tb, api, s, s.run(), exp, "planted predictors")
    finally:
        s.destroy()


def test_one_call_equals_its_parts(gpu, tb):
    """xvcgpu_frame_pass_bi_back against the entry points it is made of, issued in order from
    Python on a second set of buffers (set F: two searches of list 0, two of list 1)."""
    api, ctx = gpu
    head = ["me_search_l0_r0", "me_search_l0_r1", "me_search_l1_r1", "me_search_l1_r2",
            "l1_mvp_cost", "uni_fold"]
    for name, names in (
            ("grid10", head + ["bipred_c16", "choice", "inter_pred", "residual", "cu_info",
                               "deblock_pad_ssd"]),
            ("part10", head + ["bipred_planned", "choice", "inter_pred", "residual", "cu_info",
                               "deblock", "pad_border", "picture_ssd"])):
        a, b = Scene(ctx, name, "F"), Scene(ctx, name, "F")
        try:
            one = a.run()
            steps = b.fp.kernel_steps(b.O, b.refs, b.Rec)
            assert [k for k, _ in steps] == names
            for _, fn in steps:
                fn()
            ctx.sync()
            parts = b.fp.results(), b.Rec.download(BL)
            tb.assert_pass_equal(parts, tb.as_expected(*one), "parts")
            n, rmax = a.fp.desc.n_cus, a.fp.rmax
            assert np.array_equal(a.fp.l1_mvp_cost(), b.fp.l1_mvp_cost())
            job = one[0][6][:, :, 0].reshape(-1) != bm.NO_JOB
            ja = a.fp.d_bi_jobs.to_array(api.BI_DTYPE, n * rmax)
            jb = b.fp.d_bi_jobs.to_array(api.BI_DTYPE, n * rmax)
            assert job.any() and not job.all() and not len(tb.differing(ja[job], jb[job]))
            ia = a.fp.d_inter.to_array(api.INTER_DTYPE, 3 * n)
            assert not len(tb.differing(ia, b.fp.d_inter.to_array(api.INTER_DTYPE, 3 * n)))
            assert len(set(one[0][4]["inter_dir"].tolist())) == 3
        finally:
            a.destroy()
            b.destroy()


# ---- adaptive QP -------------------------------------------------------------------------
_aqp_scene = {}


def aqp_scene(name):
    """model_input(name) with aqp_pass_model's contrast per CTU (B_GAIN) around mid grey, the
    original and every reference alike."""
    if name not in _aqp_scene:
        pw, ph, bd, part, orig, refs = model_input(name)
        mid = 1 << (bd - 1)

        def scaled(planes):
            out = []
            for c, p in enumerate(planes):
                cs, b = (1 if c else 0), am.BORDERS[c]
                yy, xx = np.mgrid[0:p.shape[0], 0:p.shape[1]]
                r = np.clip(((yy - b) << cs) // am.CTU, 0, 1)
                q = np.clip(((xx - b) << cs) // am.CTU, 0, 1)
                v = np.rint(mid + (p.astype(np.float64) - mid) * np.array(am.B_GAIN)[r, q])
                out.append(np.ascontiguousarray(v.astype(np.uint16)))
            return out
        _aqp_scene[name] = (scaled(orig), {poc: scaled(p) for poc, p in refs.items()})
    return _aqp_scene[name]


def test_adaptive_qp_equals_model(gpu, xo, tb):
    """Set E with aqp_strength = 13 on a contrast per CTU: the apply launch in front reaches
    lambda16 of every (list, picture)'s jobs, which the predictor cost reads too."""
    from xvc_amd import pipeline
    api, ctx = gpu
    name, which = "grid10", "E"
    pw, ph, bd = model_input(name)[:3]
    orig, refs = aqp_scene(name)
    lists = bm.SETS[which]
    table = pipeline.aqp_table(bm.QP, bd, am.STRENGTH, pw)
    desc = bm.descriptors(name, True)
    ctu_var = am.ctu_variances(xo, pw, ph, orig[0], int(table.ctu_size))
    d, cu_qp, ctu_dqp = am.applied_descriptors(desc, table, ctu_var)
    assert len(set(ctu_dqp.ravel().tolist())) >= 3, ctu_dqp
    searched = bm.search_motion(xo, bd, pw, ph, orig[0], refs, lists, bm.jobs(d, lists))
    exp = bm.frame_pass(am._SetQpThenDeblock(xo, cu_qp), d, bd, orig, refs, lists, searched)
    assert len(set(exp[10][:, :2].ravel().tolist())) > 8
    s = Scene(ctx, name, which, "residual_rdoq", pictures=(orig, refs), aqp_strength=am.STRENGTH)
    try:
        got = s.run()
        assert_back_equal(tb, api, s, got, exp, "adaptive QP")
        assert np.array_equal(s.fp.cu_qp(), cu_qp)
        assert np.array_equal(s.fp.ctu_delta_qp(), ctu_dqp.reshape(ctu_var.shape))
        assert len(set(got[0][2]["qp_y"].tolist())) >= 3
        s.clear()
        assert_back_equal(tb, api, s, s.run(fused_tail=False), exp, "separate tail")
    finally:
        s.destroy()


# ---- refusals ----------------------------------------------------------------------------
def _poison(ctx, fp):
    bufs = [fp.d_choice, fp.p.d_nnz, fp.p.d_cus, fp.d_inter, fp.d_bi_jobs, fp.d_bi_res,
            fp.d_bi_slots, fp.d_l1_mvp_cost] + [b for row in fp.d_res for b in row if b is not None]
    for b in bufs:
        ctx._check(ctx.lib.xvcgpu_memset(ctx.h, b.ptr, 0xA5, b.nbytes))
    return bufs


def test_refusals_enqueue_nothing(gpu):
    """Every refusal of xvcgpu_frame_pass_bi_back - the B pass's checks, flag 0, a missing
    d_l1_mvp_cost - names its field and leaves the job arrays, the work arrays and rec as
    they were; xvcgpu_frame_pass_bi_refs still refuses the flag."""
    api, ctx = gpu
    s = Scene(ctx, "grid10", "F")
    other = ctx.picture(64, 64, 10)
    try:
        fp = s.fp
        s.clear(0x0123)
        bufs = _poison(ctx, fp)
        jobs_before = [[b.to_array(api.ME_DTYPE, fp.desc.n_cus) for b in row] for row in fp.d_me]
        form = api.FP_FORM_NAMES.index

        def setter(path, value):
            def change(a):
                obj = a
                for k in path[:-1]:
                    obj = getattr(obj, k) if isinstance(k, str) else obj[k]
                if isinstance(path[-1], str):
                    setattr(obj, path[-1], value)
                else:
                    obj[path[-1]] = value
            return change

        def refused(change, match, cost=True, entry="frame_pass_bi_back"):
            a = fp._call_args(s.O, s.refs, s.Rec)
            change(a)
            with pytest.raises(api.XvcGpuError, match="status 10: %s: .*%s" % (entry, match)):
                if entry == "frame_pass_bi_back":
                    ctx._check(ctx.lib.xvcgpu_frame_pass_bi_back(
                        ctx.h, C.byref(a), fp.d_l1_mvp_cost.ptr if cost else None, None,
                        fp.plan_handles(), ALL))
                else:
                    ctx._check(ctx.lib.xvcgpu_frame_pass_bi_refs(ctx.h, C.byref(a),
                                                                 fp.plan_handles(), ALL))
            ctx.sync()
            for b in bufs:
                assert (b.to_array(np.uint8, b.nbytes) == 0xA5).all(), match
            assert all((p == 0x0123).all() for p in s.Rec.download(BL)), match
            for row, before in zip(fp.d_me, jobs_before):
                for b, e in zip(row, before):
                    assert np.array_equal(b.to_array(api.ME_DTYPE, len(e)), e), match
        same = lambda a: None       # noqa: E731
        refused(setter(("force_l1_mvd_zero",), 0), "force_l1_mvd_zero must be 1")
        refused(same, "d_l1_mvp_cost", cost=False)
        refused(same, "force_l1_mvd_zero", entry="frame_pass_bi_refs")
        for change, match in [
                (setter(("num_ref", 0), 0), "num_ref"),
                (setter(("num_ref", 1), 4), "num_ref"),
                (setter(("same_poc_in_l0", 1), 3), "same_poc_in_l0"),
                (setter(("slot", 1, 0), 0), "slot of a re-used picture"),
                (setter(("ref_poc", 1, 0), 4), "ref_poc of a re-used picture"),
                (setter(("slot", 0, 0), 5), "slot is not below n_refs"),
                (setter(("d_choice",), None), "d_choice"),
                (setter(("d_me", 1, 0), None), "d_me"),
                (setter(("d_results", 1, 2), None), "d_results"),
                (setter(("p", "form"), form("recon_from_me")), "form"),
                (setter(("p", "db_y_end"), 16), "whole pictures"),
                (setter(("refs", 2), other.h_pic), "refs"),
                (setter(("refs", 3), None), "refs"),
                (setter(("p", "orig"), None), "orig")]:
            refused(change, match)
        # the step entries refuse a block without the flag too
        a = fp._call_args(s.O, s.refs, s.Rec)
        a.force_l1_mvd_zero = 0
        for call in (lambda: ctx.lib.xvcgpu_fp_bi_back_mvp_cost(ctx.h, C.byref(a),
                                                                fp.d_l1_mvp_cost.ptr),
                     lambda: ctx.lib.xvcgpu_fp_bi_back_uni_fold(ctx.h, C.byref(a),
                                                                fp.d_l1_mvp_cost.ptr),
                     lambda: ctx.lib.xvcgpu_fp_bi_back_choice(ctx.h, C.byref(a))):
            with pytest.raises(api.XvcGpuError, match="force_l1_mvd_zero must be 1"):
                ctx._check(call())
        # and the same block runs when nothing is wrong with it
        assert int(s.run()[0][4]["inter_dir"].max()) == 2
    finally:
        other.destroy()
        s.destroy()


def test_two_directional_pass_untouched_beside_the_low_delay_pass(gpu, tb):
    """A two-directional BiRefsFramePass answers the same bytes before and after a low-delay
    one ran on its context, and the low-delay one the same after it."""
    api, ctx = gpu
    two = tb.Scene(ctx, "grid10", "A", "fwd_transform")
    low = Scene(ctx, "grid10", "E", "fwd_transform")
    try:
        before = two.run()
        l1 = low.run()
        after = two.run()
        tb.assert_pass_equal(after, tb.as_expected(*before), "two-directional pass again")
        assert len(set(before[0][4]["inter_dir"].tolist())) == 3
        tb.assert_pass_equal(low.run(), tb.as_expected(*l1), "low-delay pass again")
    finally:
        two.destroy()
        low.destroy()


# ---- the host class ----------------------------------------------------------------------
@pytest.mark.parametrize("strength", [-1, 13], ids=["flat", "aqp"])
def test_host_class_equals_python_pass(gpu, tb, strength):
    """xvc_gpu::FramePassBiRefs with RefLists::low_delay (through
    xvc_host_frame_pass_bi_back) on set F equals pipeline.BiRefsFramePass(low_delay=True):
    choice records, CU records, predictor costs, SSD and the picture."""
    from xvc_amd import decoder
    api, ctx = gpu
    L = decoder.load_host_library()
    L.xvc_host_frame_pass_bi_back.argtypes = [C.c_void_p] + [C.c_int] * 6 + [C.c_void_p] * 6 + \
        [C.c_int] + [C.c_void_p] * 4
    kw = {"aqp_strength": strength} if strength >= 0 else {}
    s = Scene(ctx, "grid10", "F", pictures=aqp_scene("grid10") if kw else None, **kw)
    pw, ph, bd = s.size
    Rec = ctx.picture(pw, ph, bd)
    try:
        (res, nnz, cus, ssd, choice, bi, slots), rec = s.run()
        n = s.fp.desc.n_cus
        num_ref = np.array([len(l) for l in s.lists], np.int32)
        pocs = np.zeros((2, 3), np.int32)
        blocks = np.zeros((2, 3, n), api.ME_DTYPE)
        pics = (C.c_void_p * 6)()
        for l in range(2):
            for r, poc in enumerate(s.lists[l]):
                pocs[l][r], blocks[l][r] = poc, s.me[l][r]
                pics[3 * l + r] = s.refs[l][r].h_pic
        h_choice = np.zeros(n, api.FP_BI_REFS_RESULT_DTYPE)
        h_cus = np.zeros(n, api.CU_DTYPE)
        h_ssd = np.zeros(2, np.uint64)
        h_cost = np.zeros((n, 3), np.uint32)
        assert L.xvc_host_frame_pass_bi_back(
            ctx.h, pw, ph, bd, bm.QP, bm.CUR_POC, strength, num_ref.ctypes.data,
            pocs.ctypes.data, s.O.h_pic, pics, Rec.h_pic, blocks.ctypes.data, n,
            h_choice.ctypes.data, h_cus.ctypes.data, h_ssd.ctypes.data, h_cost.ctypes.data) == 0
        assert not len(tb.differing(h_choice, choice)) and not len(tb.differing(h_cus, cus))
        assert np.array_equal(h_cost, s.fp.l1_mvp_cost())
        assert h_ssd.tolist() == ssd.tolist()
        assert all(np.array_equal(x, y) for x, y in zip(Rec.download(BL), rec))
        assert len(set(choice["inter_dir"].tolist())) >= 2
        if kw:
            assert len(set(cus["qp_y"].tolist())) >= 3
        # a forward reference is no low-delay picture: the class refuses the lists
        assert L.xvc_host_frame_pass_bi_back(
            ctx.h, pw, ph, bd, bm.QP, 8, strength, num_ref.ctypes.data, pocs.ctypes.data,
            s.O.h_pic, pics, Rec.h_pic, blocks.ctypes.data, n, h_choice.ctypes.data,
            h_cus.ctypes.data, h_ssd.ctypes.data, h_cost.ctypes.data) == 10
    finally:
        Rec.destroy()
        s.destroy()
