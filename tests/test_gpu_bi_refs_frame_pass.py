"""The frame pass of a B picture on the GPU (xvcgpu_frame_pass_bi_refs,
pipeline.BiRefsFramePass): the three decision kernels alone on hand-made inputs, the whole
pass bit-exact against the model composed of the oracle's pieces
(tests/bi_refs_pass_model.py, whose SearchMotion half tests/test_bi_refs_pass_model.py pins
to the reference) from one to three pictures per list, the one call against its parts, the
planned refinement against the whole-list class launches, the refusals, the P pass beside it
on one context, the C++ class and the host controls."""
import ctypes as C

import numpy as np
import pytest

import bi_refs_pass_model as rm
import oracle_lib as ol

pytestmark = pytest.mark.gpu

BL = rm.BL
ALL = 31    # FP_ENCODE | FP_DEBLOCK_V | FP_DEBLOCK_H | FP_PAD | FP_SSD
NONE = rm.NONE


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
        _inputs[name] = rm.make_refs(name)
    return _inputs[name]


def expected(xo, name, which, rdoq):
    """The model's pass, computed once per (input, set, quantiser) and shared; the searches
    per (input, picture) are shared among the sets (rm.uni_search)."""
    if (name, which, rdoq) not in _expected:
        pw, ph, bd, _, orig, refs = model_input(name)
        lists = rm.SETS[which]
        desc = rm.descriptors(name, rdoq)
        if (name, which) not in _searched:
            _searched[name, which] = rm.search_motion(xo, bd, pw, ph, orig[0], refs, lists,
                                                      rm.jobs(desc, lists), key=name)
        _expected[name, which, rdoq] = rm.frame_pass(xo, desc, bd, orig, refs, lists,
                                                     _searched[name, which])
    return _expected[name, which, rdoq]


class Scene:
    """The input's pictures on the device and a BiRefsFramePass over them."""

    def __init__(self, ctx, name, which="A", form="residual", lists=None):
        from xvc_amd import pipeline
        pw, ph, bd, part, orig, refs = model_input(name)
        self.ctx, self.size = ctx, (pw, ph, bd)
        self.lists = lists = rm.SETS[which] if lists is None else lists
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
            side_bits=rm.SIDE_BITS)
        assert self.fp.form == form
        base = self.fp.desc.me.copy()
        base["lambda16"] = rm.LAMBDA16
        self.me = [[base.copy() for _ in lists[l]] for l in range(2)]
        for l in range(2):
            for r, poc in enumerate(lists[l]):
                self.me[l][r]["search_range"] = rm.search_range(poc)
        self.fp.set_jobs(self.me)

    def run(self, **kw):
        self.fp.run(self.O, self.refs, self.Rec, **kw)
        self.ctx.sync()
        return self.fp.results(), self.Rec.download(BL)

    def destroy(self):
        self.fp.destroy()
        for p in [self.O, self.Rec] + list(self.by_poc.values()):
            p.destroy()


def differing(a, b):
    """Indices of the records that differ, byte for byte (any dtype)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype.itemsize == b.dtype.itemsize and len(a) == len(b)
    ra = a.view(np.uint8).reshape(len(a), -1)
    return np.flatnonzero((ra != b.view(np.uint8).reshape(len(b), -1)).any(1))


def assert_pass_equal(got, exp, what, scene=None):
    """got: (BiRefsFramePass.results(), rec planes); exp: rm.frame_pass's answer."""
    (res, nnz, cus, ssd, choice, bi, slots), rec = got
    e_rec, e_res, e_nnz, e_cus, e_ssd, e_choice, e_bi, e_slots = exp[:8]
    for l in range(2):
        for r in range(len(res[l])):
            assert (res[l][r] is None) == (e_res[l][r] is None), (what, "re-use", l, r)
            if res[l][r] is not None:
                bad = differing(res[l][r], e_res[l][r])
                assert not len(bad), (what, "search", l, r, bad[:4], res[l][r][bad[:4]],
                                      e_res[l][r][bad[:4]])
    bad = differing(choice, e_choice)
    assert not len(bad), (what, "choice", bad[:4], choice[bad[:4]], e_choice[bad[:4]])
    assert np.array_equal(slots, e_slots), (what, "slot bytes", np.argwhere(slots != e_slots)[:4])
    job = e_slots[:, :, 0] != rm.NO_JOB
    for f in ("mv_x", "mv_y", "subpel_dist"):       # the refinement where there is a job
        assert np.array_equal(bi[f][job], e_bi[f][job]), (what, "refinement", f)
    assert np.array_equal(nnz, e_nnz), (what, "nnz", np.flatnonzero(nnz != e_nnz)[:8])
    bad = differing(cus, e_cus)
    assert not len(bad), (what, "CU records", bad[:4], cus[bad[:4]], e_cus[bad[:4]])
    for c in range(3):
        assert np.array_equal(rec[c], e_rec[c]), (what, "plane", c,
                                                  np.argwhere(rec[c] != e_rec[c])[:4])
    assert (int(ssd[0]), int(ssd[1])) == tuple(int(v) for v in e_ssd), (what, "ssd")
    if scene is not None and len(exp) > 8:
        pred = scene.fp.p.pred.download(0)
        for c in range(3):
            assert np.array_equal(pred[c], exp[8][c]), (what, "prediction plane", c)
        p = scene.fp.p
        if p.d_levels is not None:
            levels = p.d_levels.to_array(np.int16, max(1, p.n_levels))
            off = np.asarray(scene.ctx.level_offsets(p.desc.tx)[0], np.int64)
            for t, lv in enumerate(exp[9]):
                g = levels[off[t]:off[t] + len(lv)]
                if e_nnz[t]:
                    assert np.array_equal(g, lv), (what, "levels of block", t)
                else:       # cbf = 0: the level buffer is unspecified in the model, zeros here
                    assert not g.any(), (what, "levels of block", t)


def as_expected(results, rec):
    """A run's answer in the model's order, to compare two runs."""
    res, nnz, cus, ssd, choice, bi, slots = results
    return rec, res, nnz, cus, ssd, choice, bi, slots


# ---- the three kernels alone -------------------------------------------------------------
class Folds:
    """Device arrays and the args block for the decision kernels on given jobs / results."""

    def __init__(self, api, ctx, lists, me, res):
        self.api, self.ctx, self.lists = api, ctx, lists
        num_ref, same, distinct, slot = rm.tables(lists)
        self.n, self.rmax = len(me[0][0]), max(num_ref)
        n, rmax = self.n, self.rmax
        self.bufs = []
        a = self.args = api.FramePassBiRefsArgs()
        a.p.n_cus = a.p.n_cus_total = n
        a.p.qp_y, a.p.qp_c = 31, 29
        a.n_refs = len(distinct)
        for r in range(api.CS_MAX_REFS):
            a.same_poc_in_l0[r] = same[r] if r < num_ref[1] else -1
        for l in range(2):
            a.num_ref[l] = num_ref[l]
            for r in range(num_ref[l]):
                a.slot[l][r], a.ref_poc[l][r] = slot[l][r], lists[l][r]
                a.d_me[l][r] = self.buf(me[l][r]).ptr
                if res[l][r] is not None:
                    a.d_results[l][r] = self.buf(res[l][r]).ptr
        a.side_bits_uni[0], a.side_bits_uni[1], a.side_bits_bi = rm.SIDE_BITS
        self.jobs = self.poisoned(api.BI_DTYPE.itemsize * n * rmax)
        self.bi = self.poisoned(api.MERES_DTYPE.itemsize * n * rmax)
        self.slots = self.poisoned(2 * n * rmax)
        self.choice = self.poisoned(api.FP_BI_REFS_RESULT_DTYPE.itemsize * n)
        self.inter = self.poisoned(api.INTER_DTYPE.itemsize * 3 * n)
        self.cus = self.poisoned(api.CU_DTYPE.itemsize * n)
        a.d_bi_jobs, a.d_bi_results, a.d_bi_slots = self.jobs.ptr, self.bi.ptr, self.slots.ptr
        a.d_choice, a.d_inter, a.p.d_cus_own = self.choice.ptr, self.inter.ptr, self.cus.ptr

    def buf(self, arr):
        self.bufs.append(self.ctx.buffer(arr))
        return self.bufs[-1]

    def poisoned(self, nbytes):
        b = self.ctx.alloc(nbytes)
        self.ctx._check(self.ctx.lib.xvcgpu_memset(self.ctx.h, b.ptr, 0xA5, b.nbytes))
        self.bufs.append(b)
        return b

    def call(self, name):
        self.ctx._check(getattr(self.ctx.lib, name)(self.ctx.h, C.byref(self.args)))
        self.ctx.sync()

    def destroy(self):
        for b in self.bufs:
            b.free()


def hand_made(api, lists, n, seed):
    """Random jobs and search results per (list, picture): the same CUs, per-picture
    predictors (a re-used list-1 entry has its own), some full-pel CUs."""
    num_ref, same, _, _ = rm.tables(lists)
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
    return me, res, bi


def test_decision_kernels_on_hand_made_inputs(gpu):
    """uni fold, choice and CU records against the model's folds on 48 CUs with planted
    ties, an unsupported search result, a re-used picture with its own predictor and
    no-job slots (set C: list 1 has two pictures, Rmax is 3)."""
    api, ctx = gpu
    lists = rm.SETS["C"]
    num_ref, same, distinct, slot = rm.tables(lists)
    n = 48
    me, res, bi = hand_made(api, lists, n, 77)
    # CUs 4, 5: a searched picture without a kernel instance (in list 0; in list 1)
    res[0][1]["subpel_dist"][4] = NONE
    res[1][1]["subpel_dist"][5] = NONE
    # CUs 8 .. 15: list 0's pictures 1 and 2 (two index bits each, the same predictor) tie:
    # 8 .. 11 as uni-directional results below picture 0; 12 .. 15, where list 0 loses and is
    # refined, as refined vectors below everything.  The lower index stays.
    for i in range(8, 16):
        for a in (me, res):
            a[0][2][i] = a[0][1][i]
        if i < 12:
            res[0][1]["subpel_dist"][i] = res[0][2]["subpel_dist"][i] = 50
            continue
        for r in range(3):
            res[0][r]["subpel_dist"][i] += 30000
        res[1][1]["subpel_dist"][i] += 20000
        bi[i][2] = bi[i][1]
        bi[i][1]["subpel_dist"] = bi[i][2]["subpel_dist"] = 20
    # CUs 16 .. 23: list 0's picture 0 and list 1's unique picture (index 1: one bit each,
    # side bits 3 and 3) tie below everything, no refinement comes near: list 0 stays
    for i in range(16, 24):
        me[1][1][i], res[1][1][i] = me[0][0][i], res[0][0][i]
        res[0][0]["subpel_dist"][i] = res[1][1]["subpel_dist"][i] = 60
        bi["subpel_dist"][i] = 100000
    choice0, jobs, slots = rm.uni_fold(lists, me, res)
    # CUs 24 .. 31: cost_bi == cost_l0 <= cost_l1_unique gives bi.  The refined picture 0
    # gets the distortion that makes its cost list 0's exactly (the model says its bits).
    trial, _ = rm.choice_fold(lists, me, res, bi, choice0)
    planted = 0
    for i in range(24, 32):
        c = trial[i]
        bits_cost = int(c["bi_cost"][0]) - int(bi[i][0]["subpel_dist"])
        if int(c["cost_list"][0]) > int(c["cost_l1_unique"]) or \
                int(c["cost_list"][0]) < bits_cost:
            continue
        bi["subpel_dist"][i] = 100000
        bi[i][0]["subpel_dist"] = int(c["cost_list"][0]) - bits_cost
        planted += 1
    assert planted >= 2
    e_choice, e_inter = rm.choice_fold(lists, me, res, bi, choice0)
    # what was planted is what the model sees
    assert (e_choice[4:6].view(np.uint8) == 0xff).all() and (slots[4:6] == rm.NO_JOB).all()
    c = e_choice[8:12]
    assert (c["cost_uni"][:, 0, 1] == c["cost_uni"][:, 0, 2]).all() and \
        (c["best_ref"][:, 0] == 1).all()
    c = e_choice[12:16]
    assert (c["search_list"] == 0).all() and (c["inter_dir"] == 2).all() and \
        (c["bi_cost"][:, 1] == c["bi_cost"][:, 2]).all() and (c["ref_idx"][:, 0] == 1).all()
    c = e_choice[16:24]
    assert (c["cost_list"][:, 0] == c["cost_l1_unique"]).all() and (c["inter_dir"] == 0).all()
    c = e_choice[24:32]
    assert ((c["cost_bi"] == c["cost_list"][:, 0]) & (c["inter_dir"] == 2)).sum() == planted
    # the re-used picture (list 1's index 0 = list 0's index 2) is priced with its own mvp
    ok = np.ones(n, bool)
    ok[4:6] = False
    assert (e_choice["cost_uni"][ok, 1, 0] != e_choice["cost_uni"][ok, 0, 2]).any()
    s1 = ok & (e_choice["search_list"] == 1)
    assert s1.any() and (slots[s1, 2, 0] == rm.NO_JOB).all() and (~s1 & ok).any()
    assert len(set(e_choice["inter_dir"][ok].tolist())) == 3

    f = Folds(api, ctx, lists, me, res)
    try:
        f.call("xvcgpu_fp_bi_refs_uni_fold")
        got = f.choice.to_array(api.FP_BI_REFS_RESULT_DTYPE, n)
        bad = differing(got, choice0)
        assert not len(bad), ("uni fold", bad[:4], got[bad[:4]], choice0[bad[:4]])
        g_slots = f.slots.to_array(np.uint8, 2 * n * 3).reshape(n, 3, 2)
        assert np.array_equal(g_slots, slots)
        g_jobs = f.jobs.to_array(api.BI_DTYPE, n * 3).reshape(n, 3)
        job = slots[:, :, 0] != rm.NO_JOB
        assert not len(differing(g_jobs[job], jobs[job]))
        # a slot without a job: the job's bytes are not written
        assert (g_jobs[~job].view(np.uint8) == 0xA5).all()
        ctx.h2d(f.bi.ptr, bi)
        f.call("xvcgpu_fp_bi_refs_choice")
        got = f.choice.to_array(api.FP_BI_REFS_RESULT_DTYPE, n)
        bad = differing(got, e_choice)
        assert not len(bad), ("choice", bad[:4], got[bad[:4]], e_choice[bad[:4]])
        g_inter = f.inter.to_array(api.INTER_DTYPE, 3 * n)
        e = np.zeros(3 * n, api.INTER_DTYPE)
        for i, (x, y, w, h, ref, mv) in enumerate(e_inter):
            for comp in range(3):
                q = e[3 * i + comp]
                q["x"], q["y"], q["w"], q["h"], q["comp"] = x, y, w, h, comp
                q["ref"] = ref
                q["mv"][0][0], q["mv"][1][0] = mv[0], mv[1]
        assert not len(differing(g_inter, e))
        nnz = (np.arange(n) % 3 == 0).astype(np.int32)
        f.args.p.d_nnz = f.buf(nnz).ptr
        f.call("xvcgpu_cu_info_from_choice_refs")
        g_cus = f.cus.to_array(api.CU_DTYPE, n)
        e_cus = np.zeros(n, api.CU_DTYPE)
        for i in range(n):
            q, ch, b = e_cus[i], e_choice[i], me[0][0][i]
            q["x"], q["y"], q["w"], q["h"] = b["x"], b["y"], b["w"], b["h"]
            q["cbf_luma"], q["qp_y"], q["qp_c"] = nnz[i] != 0, 31, 29
            used = [int(ch["inter_dir"]) in (2, l) for l in range(2)]
            q["ref_idx0"] = ch["ref_idx"][0] if used[0] else -1
            for l in range(2):
                q["ref_poc"][l] = lists[l][int(ch["ref_idx"][l])] if used[l] else -1
                q["mv"][l][:] = ch["mv"][l] if used[l] else 0
        bad = differing(g_cus, e_cus)
        assert not len(bad), ("CU records", bad[:4], g_cus[bad[:4]], e_cus[bad[:4]])
    finally:
        f.destroy()


# ---- the whole pass ----------------------------------------------------------------------
_FORMS = [("grid10", "residual"), ("grid10", "fwd_transform"), ("grid8", "residual"),
          ("grid8", "fwd_transform"), ("part10", "residual"), ("part10", "fwd_transform")]


@pytest.mark.parametrize("name,form,which", [
    (name, form, which) for which in "ABCD" for name, form in _FORMS] + [
    ("grid10", "residual_rdoq", "D")])
def test_whole_pass_equals_model(gpu, xo, name, form, which):
    api, ctx = gpu
    exp = expected(xo, name, which, form != "residual")
    if which == "D":        # every direction, also through MC and the filter
        dirs = np.bincount(exp[5]["inter_dir"], minlength=3)
        assert (dirs >= 4).all(), dirs
    s = Scene(ctx, name, which, form)
    try:
        fused = s.fp.p.fused_tail
        assert fused == (name != "part10")      # the partition holds sides of 4
        planned = name == "part10"
        assert all((p is not None) == (planned and s.fp.searched[l][r])
                   for l in range(2) for r, p in enumerate(s.fp.plans[l]))
        if planned and which == "D":    # every search and refinement class is in the plan
            counts = dict(zip(api.ME_PLAN_BIN_NAMES, s.fp.plans[1][0].counts.tolist()))
            assert all(counts[k] > 0 for k in ("16x16", "8x8", "other16", "c32")) and \
                counts["c64_team"] + counts["c64_wave"] > 0 and not counts["unsupported"], counts
        got = s.run()
        assert_pass_equal(got, exp, "one call", s)
        if which == "D":        # one job per CU: its answer is the record's refined vector
            choice, bi = got[0][4], got[0][5]
            assert np.array_equal(np.stack([bi[:, 0]["mv_x"], bi[:, 0]["mv_y"]], 1),
                                  choice["bi_mv"][:, 0])
        if planned:
            # the same blocks without plans: sized searches, whole-list class launches (the
            # 16 launch answers the larger classes with the unsupported record first)
            s.Rec.upload([np.zeros_like(p) for p in exp[0]], BL)
            assert_pass_equal(s.run(planned=False), exp, "without plans", s)
        else:
            s.Rec.upload([np.zeros_like(p) for p in exp[0]], BL)
            assert_pass_equal(s.run(fused_tail=False), exp, "separate tail", s)
    finally:
        s.destroy()


def test_one_call_equals_its_parts(gpu):
    """xvcgpu_frame_pass_bi_refs against the entry points it is made of, issued in order
    from Python on a second set of buffers (set C: three searches of list 0, one of list 1)."""
    api, ctx = gpu
    for name, names in (
            ("grid10", ["me_search_l0_r0", "me_search_l0_r1", "me_search_l0_r2",
                        "me_search_l1_r1", "uni_fold", "bipred_c16", "choice", "inter_pred",
                        "residual", "cu_info", "deblock_pad_ssd"]),
            ("part10", ["me_search_l0_r0", "me_search_l0_r1", "me_search_l0_r2",
                        "me_search_l1_r1", "uni_fold", "bipred_planned", "choice", "inter_pred",
                        "residual", "cu_info", "deblock", "pad_border", "picture_ssd"])):
        a, b = Scene(ctx, name, "C"), Scene(ctx, name, "C")
        try:
            one = a.run()
            steps = b.fp.kernel_steps(b.O, b.refs, b.Rec)
            assert [k for k, _ in steps] == names
            for _, fn in steps:
                fn()
            ctx.sync()
            parts = b.fp.results(), b.Rec.download(BL)
            assert_pass_equal(parts, as_expected(*one), "parts")
            n, rmax = a.fp.desc.n_cus, a.fp.rmax
            job = one[0][6][:, :, 0].reshape(-1) != rm.NO_JOB
            ja = a.fp.d_bi_jobs.to_array(api.BI_DTYPE, n * rmax)
            jb = b.fp.d_bi_jobs.to_array(api.BI_DTYPE, n * rmax)
            assert job.any() and not job.all() and not len(differing(ja[job], jb[job]))
            ia = a.fp.d_inter.to_array(api.INTER_DTYPE, 3 * n)
            assert not len(differing(ia, b.fp.d_inter.to_array(api.INTER_DTYPE, 3 * n)))
        finally:
            a.destroy()
            b.destroy()


@pytest.mark.parametrize("lists", [((4, 0), (12,)), rm.SETS["C"]], ids=["rmax2", "rmax3"])
def test_planned_refinement_equals_class_launches(gpu, lists):
    """xvcgpu_bipred_search_refs_planned against the whole-list launches of
    xvcgpu_bipred_search_refs per class, record for record (untouched ones included), on the
    partition's job list as the pass leaves it: every class, no-job slots; and through a plan
    of class 32, whose unsupported bin holds the 64x64 CU."""
    api, ctx = gpu
    s = Scene(ctx, "part10", lists=lists)
    bufs, plan32 = [], None
    try:
        (_, _, _, _, choice, _, slots), _ = s.run()
        fp, n, rmax = s.fp, s.fp.desc.n_cus, s.fp.rmax
        assert rmax == max(len(l) for l in lists)
        assert (slots[:, :, 0] == rm.NO_JOB).any() and (slots[:, -1, 0] != rm.NO_JOB).any()
        pics = fp._distinct_pictures(s.refs)
        handles = (C.c_void_p * len(pics))(*[q.h_pic for q in pics])
        plan64 = fp.plans[0][0]
        plan32 = ctx.me_plan(fp.d_me[0][0].ptr, n, 32)
        assert plan32.counts[api.ME_PLAN_BIN_NAMES.index("unsupported")] == 1

        def poisoned():
            b = ctx.alloc(api.MERES_DTYPE.itemsize * n * rmax)
            ctx._check(ctx.lib.xvcgpu_memset(ctx.h, b.ptr, 0xA5, b.nbytes))
            bufs.append(b)
            return b
        for plan, classes in ((plan64, (16, 32, 64)), (plan32, (16, 32))):
            whole, planned = poisoned(), poisoned()
            for cls in classes:
                ctx._check(ctx.lib.xvcgpu_bipred_search_refs(
                    ctx.h, s.O.h_pic, handles, len(pics), fp.d_bi_jobs.ptr, fp.d_bi_slots.ptr,
                    n * rmax, whole.ptr, cls))
            ctx._check(ctx.lib.xvcgpu_bipred_search_refs_planned(
                ctx.h, s.O.h_pic, handles, len(pics), plan.h, rmax, fp.d_bi_jobs.ptr,
                fp.d_bi_slots.ptr, planned.ptr))
            ctx.sync()
            w = whole.to_array(api.MERES_DTYPE, n * rmax)
            p = planned.to_array(api.MERES_DTYPE, n * rmax)
            bad = differing(w, p)
            assert not len(bad), (classes, bad[:6], w[bad[:6]], p[bad[:6]])
            job = slots[:, :, 0].reshape(-1) != rm.NO_JOB
            assert (w[~job].view(np.uint8) == 0xA5).all()
            assert ((w["subpel_dist"][job] == NONE).sum() > 0) == (plan is plan32)
            if plan is plan64:      # ... and they are the pass's own results
                assert not len(differing(w[job], fp.d_bi_res.to_array(
                    api.MERES_DTYPE, n * rmax)[job]))
    finally:
        if plan32 is not None:
            plan32.destroy()
        for b in bufs:
            b.free()
        s.destroy()


# ---- refusals ----------------------------------------------------------------------------
def _poison(ctx, fp):
    bufs = [fp.d_choice, fp.p.d_nnz, fp.p.d_cus, fp.d_inter, fp.d_bi_jobs, fp.d_bi_res,
            fp.d_bi_slots] + [b for row in fp.d_res for b in row if b is not None]
    for b in bufs:
        ctx._check(ctx.lib.xvcgpu_memset(ctx.h, b.ptr, 0xA5, b.nbytes))
    return bufs


def _refused(api, ctx, s, bufs, change, match, plans=None):
    fp = s.fp
    a = fp._call_args(s.O, s.refs, s.Rec)
    keep = change(a)        # (what the change allocated lives until the call returned)
    with pytest.raises(api.XvcGpuError, match="status 10: frame_pass_bi_refs: .*" + match):
        ctx._check(ctx.lib.xvcgpu_frame_pass_bi_refs(
            ctx.h, C.byref(a), fp.plan_handles() if plans is None else plans, ALL))
    del keep
    ctx.sync()
    for b in bufs:
        assert (b.to_array(np.uint8, b.nbytes) == 0xA5).all(), match
    assert all((p == 0x0123).all() for p in s.Rec.download(BL)), match


def test_refusals_enqueue_nothing(gpu):
    api, ctx = gpu
    g, p = Scene(ctx, "grid10", "C"), Scene(ctx, "part10", "C")
    other = ctx.picture(64, 64, 10)
    deeper = ctx.picture(g.size[0], g.size[1], 12)
    small_plan = None
    try:
        for s, name in ((g, "grid10"), (p, "part10")):
            s.Rec.upload([np.full_like(q, 0x0123) for q in model_input(name)[4]], BL)
        bufs = _poison(ctx, g.fp)

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
        form = api.FP_FORM_NAMES.index
        cases = [
            (setter(("num_ref", 0), 0), "num_ref"),
            (setter(("num_ref", 1), 4), "num_ref"),
            (setter(("same_poc_in_l0", 1), 3), "same_poc_in_l0"),
            (setter(("slot", 1, 0), 0), "slot of a re-used picture"),
            (setter(("ref_poc", 1, 0), 4), "ref_poc of a re-used picture"),
            (setter(("slot", 0, 1), 4), "slot is not below n_refs"),
            (setter(("force_l1_mvd_zero",), 1), "force_l1_mvd_zero"),
            (setter(("d_choice",), None), "d_choice"),
            (setter(("d_bi_slots",), None), "d_bi_slots"),
            (setter(("d_me", 1, 0), None), "d_me"),
            (setter(("d_results", 0, 2), None), "d_results"),
            (setter(("p", "form"), form("recon_from_me")), "form"),
            (setter(("p", "form"), form("fwd_from_me")), "form"),
            (setter(("p", "n_cus_total"), g.fp.desc.n_cus + 1), "whole pictures"),
            (setter(("p", "db_y_end"), 16), "whole pictures"),
            (setter(("refs", 2), other.h_pic), "refs"),
            (setter(("refs", 1), deeper.h_pic), "refs"),
            (setter(("refs", 3), None), "refs"),
            (setter(("p", "orig"), None), "orig"),
        ]
        for change, match in cases:
            _refused(api, ctx, g, bufs, change, match)
        # (a re-used entry's d_results is ignored: NULL there is no refusal - it is NULL)
        assert g.fp._call_args(g.O, g.refs, g.Rec).d_results[1][0] is None

        bufs = _poison(ctx, p.fp)
        fp = p.fp

        def handles(edit):
            h = fp.plan_handles()
            edit(h)
            return h

        def drop(h):
            h[0][1] = None

        def swap(h):
            h[0][0], h[0][1] = h[0][1], h[0][0]
        small_plan = ctx.me_plan(fp.d_me[1][1].ptr, fp.desc.n_cus, 16)

        def other_class(h):
            h[1][1] = small_plan.h
        same = lambda a: None       # noqa: E731
        _refused(api, ctx, p, bufs, same, "plans for every searched picture", handles(drop))
        _refused(api, ctx, p, bufs, same, "not made from its d_me", handles(swap))
        _refused(api, ctx, p, bufs, same, "another max_block_size class", handles(other_class))
        _refused(api, ctx, p, bufs, setter(("p", "n_cus"), fp.desc.n_cus - 1), "whole pictures")
        # and the same blocks run when nothing is wrong with them
        assert int(p.run()[0][4]["inter_dir"].max()) == 2
        assert int(g.run()[0][4]["inter_dir"].max()) == 2
    finally:
        if small_plan is not None:
            small_plan.destroy()
        other.destroy()
        deeper.destroy()
        g.destroy()
        p.destroy()


def test_refusals_enqueue_nothing_one_picture_per_list(gpu):
    """Set D, one plan per list: the forms that predict from one list inside their kernel
    (the P pass runs both on this grid), a missing list-1 picture, a plan for one list only
    and the lists' plans swapped are refused before anything is written."""
    api, ctx = gpu
    g, p = Scene(ctx, "grid10", "D"), Scene(ctx, "part10", "D")
    try:
        for s, name in ((g, "grid10"), (p, "part10")):
            s.Rec.upload([np.full_like(q, 0x0123) for q in model_input(name)[4]], BL)
        bufs = _poison(ctx, g.fp)

        def form(v):
            def change(a):
                a.p.form = v
            return change

        def no_ref1(a):
            a.refs[1] = None
        _refused(api, ctx, g, bufs, form(api.FP_FORM_NAMES.index("recon_from_me")), "form")
        _refused(api, ctx, g, bufs, form(api.FP_FORM_NAMES.index("fwd_from_me")), "form")
        _refused(api, ctx, g, bufs, no_ref1, "refs")
        bufs = _poison(ctx, p.fp)
        fp = p.fp

        def handles(l0, l1):
            h = fp.plan_handles(False)
            h[0][0] = l0.h if l0 is not None else None
            h[1][0] = l1.h if l1 is not None else None
            return h
        p0, p1 = fp.plans[0][0], fp.plans[1][0]
        same = lambda a: None       # noqa: E731
        _refused(api, ctx, p, bufs, same, "plans for every searched picture", handles(p0, None))
        _refused(api, ctx, p, bufs, same, "plans for every searched picture", handles(None, p1))
        _refused(api, ctx, p, bufs, same, "not made from its d_me", handles(p1, p0))
        # and the same blocks run when nothing is wrong with them
        assert int(p.run()[0][4]["inter_dir"].max()) == 2
    finally:
        g.destroy()
        p.destroy()


def test_p_pass_untouched_beside_the_b_pass(gpu):
    """A FramePass on list 0 of the same input answers the same before and after a
    BiRefsFramePass ran on its context: no scratch or context state leaks between them."""
    from xvc_amd import pipeline
    api, ctx = gpu
    s = Scene(ctx, "grid10", "D", "fwd_transform")
    pw, ph, bd = s.size
    P = ctx.picture(pw, ph, bd)
    passes = [pipeline.FramePass(ctx, pw, ph, bd, rm.QP),
              pipeline.FramePass(ctx, pw, ph, bd, rm.QP, rdoq=True)]
    try:
        def run_p():
            out = []
            for fp in passes:
                fp.run(s.O, s.refs[0][0], P)
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


# ---- the host layers ---------------------------------------------------------------------
def test_host_class_equals_python_pass(gpu):
    """xvc_gpu::FramePassBiRefs (through xvc_host_frame_pass_bi_refs) on set A equals
    pipeline.BiRefsFramePass: choice records, CU records, SSD and the picture."""
    from xvc_amd import decoder
    api, ctx = gpu
    L = decoder.load_host_library()
    L.xvc_host_frame_pass_bi_refs.argtypes = [C.c_void_p] + [C.c_int] * 5 + [C.c_void_p] * 6 + \
        [C.c_int] + [C.c_void_p] * 3
    s = Scene(ctx, "grid10", "A")
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
        assert L.xvc_host_frame_pass_bi_refs(
            ctx.h, pw, ph, bd, rm.QP, rm.CUR_POC, num_ref.ctypes.data, pocs.ctypes.data,
            s.O.h_pic, pics, Rec.h_pic, blocks.ctypes.data, n, h_choice.ctypes.data,
            h_cus.ctypes.data, h_ssd.ctypes.data) == 0
        assert not len(differing(h_choice, choice)) and not len(differing(h_cus, cus))
        assert h_ssd.tolist() == ssd.tolist()
        assert all(np.array_equal(x, y) for x, y in zip(Rec.download(BL), rec))
        assert len(set(choice["inter_dir"].tolist())) == 3
    finally:
        Rec.destroy()
        s.destroy()


def test_search_motion_half_equals_host_control(gpu):
    """The choice records on set A against xvc_gpu::InterSearch::SearchMotionMultiBatch
    (xvc_host_search_motion_multi_batch, pinned to the reference by
    test_gpu_host_inter_search.py) on the same jobs with AMVP pairs {mvp, mvp}: random
    per-picture predictors and full-pel CUs."""
    from xvc_amd import decoder
    api, ctx = gpu
    L = decoder.load_host_library()
    L.xvc_host_search_motion_multi_batch.argtypes = [C.c_void_p] * 5 + [
        C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
    s = Scene(ctx, "grid10", "A")
    try:
        n = s.fp.desc.n_cus
        rng = np.random.default_rng(41)
        fullpel = (rng.integers(0, 6, n) == 0).astype(np.uint8)
        assert fullpel.any() and not fullpel.all()
        blocks = np.zeros((2, 3, n), api.ME_DTYPE)
        mvp = np.zeros((2, 3, n, 4), np.int32)
        handles = (C.c_void_p * 6)()
        for l in range(2):
            for r in range(len(s.lists[l])):
                b = s.me[l][r]
                b["mvp_x"], b["mvp_y"] = rng.integers(-160, 161, (2, n))
                b["fullpel_mv"] = fullpel
                blocks[l][r] = b
                mvp[l, r, :, 0] = mvp[l, r, :, 2] = b["mvp_x"]
                mvp[l, r, :, 1] = mvp[l, r, :, 3] = b["mvp_y"]
                handles[3 * l + r] = s.refs[l][r].h_pic
        s.fp.set_jobs(s.me)
        (_, _, _, _, choice, _, _), _ = s.run()
        num_ref = np.array([len(l) for l in s.lists], np.int32)
        same = np.array(s.fp.same + [-1] * (3 - len(s.fp.same)), np.int32)
        out = np.zeros((n, 32), np.int64)
        bl, mv = np.ascontiguousarray(blocks), np.ascontiguousarray(mvp)
        assert L.xvc_host_search_motion_multi_batch(
            ctx.h, s.O.h_pic, handles, num_ref.ctypes.data, same.ctypes.data, 0, 0,
            bl.ctypes.data, n, mv.ctypes.data, 1, out.ctypes.data) == 0
        for i in range(n):
            q, c = [int(v) for v in out[i]], choice[i]
            d = q[0]
            want = [d, q[1], q[10], q[11], q[12], q[13], q[14], q[18]]
            got = [int(c["inter_dir"]), int(c["cost"]), int(c["cost_list"][0]),
                   int(c["cost_list"][1]), int(c["cost_l1_unique"]), int(c["cost_bi"]),
                   int(c["best_ref"][0]), int(c["best_ref"][1])]
            for l in range(2):
                if d in (2, l):     # ref_idx, predictor index 0, vector
                    want += q[2 + 4 * l:6 + 4 * l]
                    got += [int(c["ref_idx"][l]), 0, int(c["mv"][l][0]), int(c["mv"][l][1])]
                else:
                    assert int(c["ref_idx"][l]) == -1 and not c["mv"][l].any()
            assert got == want, (i, got, want)
        assert len(set(choice["inter_dir"].tolist())) >= 2
    finally:
        s.destroy()


def test_folds_with_predictors_equal_host_control(gpu):
    """One picture per list (set D), random per-list predictors and full-pel CUs: the choice
    records against xvc_host_search_motion_batch (pinned to the reference by
    test_gpu_host_inter_search.py) on the same jobs with AMVP pairs {mvp, mvp}."""
    from xvc_amd import decoder
    api, ctx = gpu
    L = decoder.load_host_library()
    L.xvc_host_search_motion_batch.argtypes = [C.c_void_p] * 5 + [C.c_int] + [C.c_void_p] * 3 + \
        [C.c_int, C.c_void_p]
    s = Scene(ctx, "grid10", "D")
    try:
        n = s.fp.desc.n_cus
        rng = np.random.default_rng(31)
        blocks = np.zeros((2, n), api.ME_DTYPE)
        fullpel = (rng.integers(0, 6, n) == 0).astype(np.uint8)
        for l in range(2):
            blocks[l] = s.me[l][0]
            blocks[l]["mvp_x"] = rng.integers(-160, 161, n)
            blocks[l]["mvp_y"] = rng.integers(-160, 161, n)
            blocks[l]["fullpel_mv"] = fullpel
        assert fullpel.any() and not fullpel.all()
        s.fp.set_jobs([[blocks[0]], [blocks[1]]])
        (_, _, _, _, choice, _, _), _ = s.run()
        mvp = np.zeros((2, n, 4), np.int32)
        for l in range(2):
            mvp[l, :, 0] = mvp[l, :, 2] = blocks[l]["mvp_x"]
            mvp[l, :, 1] = mvp[l, :, 3] = blocks[l]["mvp_y"]
        side_uni = np.zeros((2, n), np.uint32)
        side_uni[0], side_uni[1] = rm.SIDE_BITS[0], rm.SIDE_BITS[1]
        side_bi = np.full(n, rm.SIDE_BITS[2], np.uint32)
        out = np.zeros((n, 18), np.int64)
        bl = np.ascontiguousarray(blocks)
        assert L.xvc_host_search_motion_batch(
            ctx.h, s.O.h_pic, s.refs[0][0].h_pic, s.refs[1][0].h_pic, bl.ctypes.data, n,
            mvp.ctypes.data, side_uni.ctypes.data, side_bi.ctypes.data, 1, out.ctypes.data) == 0
        for i in range(n):
            q, c = [int(v) for v in out[i]], choice[i]
            d = q[0]
            want_mv = [[q[1 + 2 * l], q[2 + 2 * l]] if d in (2, l) else [0, 0] for l in range(2)]
            got = (int(c["inter_dir"]), c["mv"].tolist(), int(c["cost"]), c["cost_list"].tolist(),
                   int(c["cost_bi"]))
            assert got == (d, want_mv, q[7], [q[8], q[12]], q[16]), (i, got, q)
            assert q[5] == q[6] == 0 and q[17] == 1     # predictor index 0, one step
        assert len(set(choice["inter_dir"].tolist())) >= 2
    finally:
        s.destroy()
