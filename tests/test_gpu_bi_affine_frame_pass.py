"""The B frame pass with affine motion on the GPU (xvcgpu_frame_pass_bi_refs_affine;
pipeline.BiRefsFramePass(affine=True)): each small kernel alone against the model's arrays
byte for byte with everything else planted and untouched, the listed search against
xvcgpu_affine_me_batch_refs and the oracle, the pass against the model composed of the
oracle's pieces (tests/bi_affine_pass_model.py), the one call against its parts, a pass
without capable CUs against the plain B pass, the refusals, a plain B pass and a P affine
pass beside a B affine one on one context."""
import ctypes as C

import numpy as np
import pytest

import bi_affine_pass_model as am
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
    """Indices of the records that differ, byte for byte (any dtype, any shape)."""
    a, b = np.ascontiguousarray(a).reshape(-1), np.ascontiguousarray(b).reshape(-1)
    assert a.dtype.itemsize == b.dtype.itemsize and len(a) == len(b)
    ra = a.view(np.uint8).reshape(len(a), -1)
    return np.flatnonzero((ra != b.view(np.uint8).reshape(len(b), -1)).any(1))


def poison_like(dtype, n):
    return np.full(n * np.dtype(dtype).itemsize, POISON, np.uint8).view(dtype)


_expected = {}


def expected(xo, name, which, rdoq):
    """The model's pass, once per (input, set, quantiser): (search(), frame_pass())."""
    if (name, which, rdoq) not in _expected:
        pw, ph, bd, _, orig, refs = am.scene(name)
        desc = am.descriptors(name, rdoq)
        found = am.search(xo, name, which)
        e = am.frame_pass(xo, desc, bd, orig, refs, am.SETS[which], found)
        # what is compared is there: coded blocks in every component, both states chosen
        coded = [int((e[1][desc.tx["comp"] == c] != 0).sum()) for c in range(3)]
        assert min(coded) >= 4 and int(found["choice"]["use_affine"].sum()) >= 4, coded
        _expected[name, which, rdoq] = found, e
    return _expected[name, which, rdoq]


class Scene:
    """The input's pictures on the device and a BiRefsFramePass over them."""

    def __init__(self, ctx, name, which="A", form="residual", affine=True, cu=16):
        from xvc_amd import pipeline
        pw, ph, bd, part, orig, refs = am.scene(name)
        self.ctx, self.size, self.name = ctx, (pw, ph, bd), name
        self.lists = lists = am.SETS[which]
        self.O, self.Rec = ctx.picture(pw, ph, bd), ctx.picture(pw, ph, bd)
        self.O.upload(orig, BL)
        self.by_poc = {}
        for poc in sorted(set(lists[0]) | set(lists[1])):
            self.by_poc[poc] = ctx.picture(pw, ph, bd)
            self.by_poc[poc].upload(refs[poc], BL)
        self.refs = [[self.by_poc[poc] for poc in lists[l]] for l in range(2)]
        self.fp = pipeline.BiRefsFramePass(
            ctx, pw, ph, bd, am.QP, cu=cu, rdoq=form != "residual",
            rdoq_packed=form == "fwd_transform", partition=part, cur_poc=am.CUR_POC,
            ref_pocs=lists, search_range=am.rm.SEARCH_RANGE, side_bits=am.SIDE_BITS,
            affine=affine)
        assert self.fp.form == form
        base = self.fp.desc.me.copy()
        base["lambda16"] = am.LAMBDA16
        self.me = [[base.copy() for _ in lists[l]] for l in range(2)]
        for l in range(2):
            for r, poc in enumerate(lists[l]):
                self.me[l][r]["search_range"] = am.rm.search_range(poc)
        self.fp.set_jobs(self.me)

    def run(self, **kw):
        self.fp.run(self.O, self.refs, self.Rec, **kw)
        self.ctx.sync()
        return self.answer()

    def answer(self):
        fp = self.fp
        out = dict(results=fp.results(), rec=self.Rec.download(BL), inter=fp.inter_jobs(),
                   pred=fp.p.pred.download(0))
        if fp.affine is not None:
            bj, bs = fp.affine_bi_jobs()
            out.update(jobs=fp.affine_jobs(), ures=fp.affine_uni_results(), bjobs=bj, bslots=bs,
                       bres=fp.affine_bi_results(), choice=fp.affine_choice())
        return out

    def destroy(self):
        self.fp.destroy()
        for p in [self.O, self.Rec] + list(self.by_poc.values()):
            p.destroy()


def assert_equal_records(got, exp, what):
    bad = differing(got, exp)
    g, e = np.ascontiguousarray(got).reshape(-1), np.ascontiguousarray(exp).reshape(-1)
    assert not len(bad), (what, bad[:4], g[bad[:4]], e[bad[:4]])


def assert_pass_equal(got, found, exp, what, scene):
    """got: Scene.answer(); found, exp: expected()."""
    res, nnz, cus, ssd, choice, bi, slots = got["results"]
    e_res, e_bi, e_slots, e_choice, _ = found["plain"]
    e_rec, e_nnz, e_cus, e_ssd, e_pred, e_levels = exp
    for l in range(2):      # the plain run
        for r in range(len(res[l])):
            assert (res[l][r] is None) == (e_res[l][r] is None), (what, "re-use", l, r)
            if res[l][r] is not None:
                assert_equal_records(res[l][r], e_res[l][r], (what, "search", l, r))
    assert_equal_records(choice, e_choice, (what, "plain choice"))
    assert np.array_equal(slots, e_slots), (what, "plain slot bytes")
    job = e_slots[:, :, 0] != am.NO_SLOT
    for f in ("mv_x", "mv_y", "subpel_dist"):
        assert np.array_equal(bi[f][job], e_bi[f][job]), (what, "plain refinement", f)
    # the affine run (arrays nobody writes are zero on both sides)
    assert_equal_records(got["jobs"], found["jobs"], (what, "bootstrap"))
    assert_equal_records(got["ures"], found["ures"], (what, "affine uni results"))
    assert np.array_equal(got["bslots"], found["bslots"]), (what, "refinement slot bytes")
    assert_equal_records(got["bjobs"], found["bjobs"], (what, "refinement jobs"))
    assert_equal_records(got["bres"], found["bres"], (what, "affine bi results"))
    assert_equal_records(got["choice"], found["choice"], (what, "records"))
    assert_equal_records(got["inter"], found["inter"], (what, "prediction jobs"))
    for c in range(3):
        assert np.array_equal(got["pred"][c], e_pred[c]), (what, "prediction plane", c)
    assert np.array_equal(nnz, e_nnz), (what, "nnz", np.flatnonzero(nnz != e_nnz)[:8])
    p = scene.fp.p
    if p.d_levels is not None:
        levels = p.d_levels.to_array(np.int16, max(1, p.n_levels))
        off = np.asarray(scene.ctx.level_offsets(p.desc.tx)[0], np.int64)
        for t, lv in enumerate(e_levels):
            g = levels[off[t]:off[t] + len(lv)]
            if e_nnz[t]:
                assert np.array_equal(g, lv), (what, "levels of block", t)
            else:
                assert not g.any(), (what, "levels of block", t)
    assert_equal_records(cus, e_cus, (what, "CU records"))
    for c in range(3):
        assert np.array_equal(got["rec"][c], e_rec[c]), (what, "plane", c,
                                                         np.argwhere(got["rec"][c] != e_rec[c])[:4])
    assert (int(ssd[0]), int(ssd[1])) == tuple(int(v) for v in e_ssd), (what, "ssd")


# ---- the kernels alone -------------------------------------------------------------------
class Folds:
    """Device arrays and the two args blocks for the small kernels on given arrays; what a
    kernel is to write starts poisoned."""

    def __init__(self, api, ctx, lists, me, res, jobs, slots, order, n_class, ures=None,
                 bjobs=None, bslots=None, bres=None, fold=None, plain=None, inter=None):
        self.api, self.ctx = api, ctx
        num_ref, same, distinct, slot = am.tables(lists)
        self.n, self.rmax = n, rmax = len(me[0][0]), max(num_ref)
        self.bufs = []
        a = self.a = api.FramePassBiRefsArgs()
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
        a.side_bits_uni[0], a.side_bits_uni[1], a.side_bits_bi = am.SIDE_BITS
        e = 2 * rmax

        def given(arr, dtype, count):
            return self.buf(poison_like(dtype, count) if arr is None else arr)
        self.plain = given(plain, api.FP_BI_REFS_RESULT_DTYPE, n)
        self.inter = given(inter, api.INTER_DTYPE, 3 * n)
        self.cus = given(None, api.CU_DTYPE, n)
        # (the plain pass's own work arrays: the entries check that they are there)
        work = [self.buf(poison_like(np.uint8, 16)) for _ in range(3)]
        a.d_bi_jobs, a.d_bi_results, a.d_bi_slots = (w.ptr for w in work)
        a.d_choice, a.d_inter, a.p.d_cus_own = self.plain.ptr, self.inter.ptr, self.cus.ptr
        f = self.f = api.FramePassBiAffineArgs()
        self.jobs, self.slots = self.buf(jobs), self.buf(slots)
        self.ures = given(ures, api.AFFINE_ME_RESULT_DTYPE, n * e)
        self.bjobs = given(bjobs, api.AFFINE_ME_DTYPE, n * rmax)
        self.bslots = given(bslots, np.uint8, 2 * n * rmax)
        self.bres = given(bres, api.AFFINE_ME_RESULT_DTYPE, n * rmax)
        self.choice = given(fold, api.FP_BI_AFFINE_RESULT_DTYPE, n)
        self.order = self.buf(order)
        f.d_uni, f.d_uni_results, f.d_uni_slots = self.jobs.ptr, self.ures.ptr, self.slots.ptr
        f.d_bi, f.d_bi_results, f.d_bi_slots = self.bjobs.ptr, self.bres.ptr, self.bslots.ptr
        f.d_order, f.d_choice = self.order.ptr, self.choice.ptr
        f.n_class[:] = n_class

    def buf(self, arr):
        self.bufs.append(self.ctx.buffer(np.ascontiguousarray(arr)))
        return self.bufs[-1]

    def call(self, name):
        self.ctx._check(getattr(self.ctx.lib, name)(self.ctx.h, C.byref(self.a), C.byref(self.f)))
        self.ctx.sync()

    def destroy(self):
        for b in self.bufs:
            b.free()


def _planted_me(found, seed):
    """The model's plain jobs with planted predictors (prices that differ per list)"""
    rng = np.random.default_rng(seed)
    me = [[m.copy() for m in row] for row in found["me"]]
    for row in me:
        for m in row:
            m["mvp_x"], m["mvp_y"] = rng.integers(-40, 40, len(m)), rng.integers(-40, 40, len(m))
    return me


def test_boot_equals_model(gpu, xo):
    """xvcgpu_fp_bi_affine_boot over the partition's listed CUs, set C (Rmax 3: a no-job
    slot and a re-used entry per CU), planted plain vectors - some of +-3000, where ClipMv
    acts - and unsupported plain results: every job byte for byte, so the fields the kernel
    does not name, the unlisted CUs' jobs and the jobs without a picture stay."""
    api, ctx = gpu
    lists = am.SETS["C"]
    pw, ph = am.INPUTS["part10"][:2]
    d = am.descriptors("part10")
    me = am.rm.jobs(d, lists)
    order, n_class = am.order_list(me[0][0])
    jobs0, slots = am.uni_jobs(lists, me)
    rng = np.random.default_rng(31)
    n, e = jobs0.shape
    jobs0["reserved"], jobs0["other_mv"] = rng.integers(0, 256, (n, e)), rng.integers(-9, 9, (n, e, 3, 2))
    jobs0["bootstrap"], jobs0["flags"] = rng.integers(-9, 9, (n, e, 3, 2)), 2
    num_ref, same, _, _ = am.tables(lists)
    res = [[None] * num_ref[l] for l in range(2)]
    for l in range(2):
        for r in range(num_ref[l]):
            if l == 1 and same[r] >= 0:
                continue
            q = res[l][r] = np.zeros(n, api.MERES_DTYPE)
            q["mv_x"], q["mv_y"] = rng.integers(-60, 61, n), rng.integers(-60, 61, n)
            q["mv_x"][order[l::3]] = rng.choice([-3000, 3000], len(order[l::3]))
            q["mv_y"][order[r::4]] = rng.choice([-3000, 3000], len(order[r::4]))
    res[0][1]["subpel_dist"][order[7]] = res[1][1]["subpel_dist"][order[2]] = am.NONE
    exp = am.boot(xo, lists, res, jobs0, slots, order, pw, ph)
    assert (exp["flags"] == am.NO_JOB).sum() == 2
    f = Folds(api, ctx, lists, me, res, jobs0, slots, order, n_class)
    f.a.p.orig = None
    try:
        with pytest.raises(api.XvcGpuError, match="status 10: .*orig"):
            f.call("xvcgpu_fp_bi_affine_boot")
        O = ctx.picture(pw, ph, 10)
        f.a.p.orig = O.h_pic
        f.call("xvcgpu_fp_bi_affine_boot")
        got = f.jobs.to_array(api.AFFINE_ME_DTYPE, n * e)
        assert_equal_records(got, exp, "boot")
        searched = sum(sum(1 for r in range(num_ref[l]) if l == 0 or same[r] < 0)
                       for l in range(2))
        assert len(differing(got, jobs0)) == len(order) * searched
        for b, dt in ((f.ures, api.AFFINE_ME_RESULT_DTYPE), (f.bjobs, api.AFFINE_ME_DTYPE),
                      (f.choice, api.FP_BI_AFFINE_RESULT_DTYPE)):
            assert (b.to_array(np.uint8, b.nbytes) == POISON).all()
        O.destroy()
    finally:
        f.destroy()


@pytest.mark.parametrize("name,which", [("grid8", "C"), ("part10", "A")])
def test_listed_search_equals_batch_refs(gpu, xo, name, which):
    """xvcgpu_affine_me_listed_refs over the model's uni-directional jobs (after boot) and
    over its BIPRED refinement jobs against xvcgpu_affine_me_batch_refs on the same jobs per
    height class (NW = 2, 4, 8 on the partition) record for record, and against the oracle;
    the records of unlisted CUs, of no-job slots and of a NO_JOB job: poisoned and untouched."""
    api, ctx = gpu
    pw, ph, bd, _, orig, refs = am.scene(name)
    lists = am.SETS[which]
    found = am.search(xo, name, which)
    _, _, distinct, _ = am.tables(lists)
    order, n_class = found["order"], found["n_class"]
    O = ctx.picture(pw, ph, bd)
    O.upload(orig, BL)
    pics = []
    for poc in distinct:
        pics.append(ctx.picture(pw, ph, bd))
        pics[-1].upload(refs[poc], BL)
    handles = (C.c_void_p * len(pics))(*[p.h_pic for p in pics])
    bufs = []
    try:
        for jobs, slots, want in ((found["jobs"], found["slots"], found["ures"]),
                                  (found["bjobs"], found["bslots"], found["bres"])):
            jobs = jobs.copy()
            n, per_cu = jobs.shape
            skipped = (int(order[2]), 0)
            jobs["flags"][skipped] |= am.NO_JOB
            d_jobs, d_slots, d_order = ctx.buffer(jobs), ctx.buffer(slots), ctx.buffer(order)
            d_out = ctx.buffer(poison_like(api.AFFINE_ME_RESULT_DTYPE, n * per_cu))
            bufs += [d_jobs, d_slots, d_order, d_out]
            ctx._check(ctx.lib.xvcgpu_affine_me_listed_refs(
                ctx.h, O.h_pic, handles, len(pics), d_jobs.ptr, d_slots.ptr, n, per_cu,
                d_order.ptr, (C.c_int32 * 3)(*n_class), d_out.ptr))
            ctx.sync()
            got = d_out.to_array(api.AFFINE_ME_RESULT_DTYPE, n * per_cu).reshape(n, per_cu)
            ran = np.zeros((n, per_cu), bool)
            ran[order] = slots[order][:, :, 0] != am.NO_SLOT
            ran[skipped] = False
            assert ran.any() and not ran.all()
            assert_equal_records(got[ran], want[ran], "oracle")
            assert (got[~ran].view(np.uint8) == POISON).all()
            first = 0
            for k, h in enumerate(am.SIDES):
                cus = order[first:first + n_class[k]]
                first += n_class[k]
                if not len(cus):
                    continue
                sel = [(int(i), e) for i in cus for e in range(per_cu) if ran[i, e]]
                ii, ee = [s[0] for s in sel], [s[1] for s in sel]
                batch = ctx.affine_me_batch_refs(O, pics, jobs[ii, ee], slots[ii, ee], h)
                assert_equal_records(got[ii, ee], batch, ("batch_refs", h))
            assert got["iterations"][ran].max() >= 2
            for bad_counts in ((n, 1, 0), (-1, 0, 0)):
                assert ctx.lib.xvcgpu_affine_me_listed_refs(
                    ctx.h, O.h_pic, handles, len(pics), d_jobs.ptr, d_slots.ptr, n, per_cu,
                    d_order.ptr, (C.c_int32 * 3)(*bad_counts), d_out.ptr) == 10
    finally:
        for b in bufs:
            b.free()
        O.destroy()
        for p in pics:
            p.destroy()


def test_uni_fold_equals_model(gpu, xo):
    """xvcgpu_fp_bi_affine_uni_fold on the 8-bit grid, set C (a re-used list-1 entry and a
    no-job slot per CU) with planted corner predictors and one CU without bootstrap: the
    fold's records, the refinement jobs and every slot byte against the model's; what the
    fold does not write stays poisoned."""
    api, ctx = gpu
    lists = am.SETS["C"]
    found = am.search(xo, "grid8", "C")
    rng = np.random.default_rng(32)
    jobs, slots, ures = found["jobs"].copy(), found["slots"], found["ures"]
    jobs["mvp"] = rng.integers(-40, 40, jobs["mvp"].shape)
    lost = int(found["order"][5])
    jobs["flags"][lost, 1] = 0
    fold, bjobs, bslots = am.uni_fold(lists, found["me"][0][0], jobs, slots, ures)
    ran = np.zeros(len(jobs), bool)
    ran[found["order"]] = True
    ran[lost] = False
    assert set(fold["search_list"][ran].tolist()) == {0, 1}
    f = Folds(api, ctx, lists, found["me"], found["plain"][0], jobs, slots, found["order"],
              found["n_class"], ures=ures)
    try:
        f.call("xvcgpu_fp_bi_affine_uni_fold")
        n, rmax = bjobs.shape
        got_c = f.choice.to_array(api.FP_BI_AFFINE_RESULT_DTYPE, n)
        got_j = f.bjobs.to_array(api.AFFINE_ME_DTYPE, n * rmax).reshape(n, rmax)
        got_s = f.bslots.to_array(np.uint8, 2 * n * rmax).reshape(n, rmax, 2)
        assert_equal_records(got_c[ran], fold[ran], "fold records")
        assert (got_c[~ran].view(np.uint8) == POISON).all()
        assert np.array_equal(got_s, bslots)
        job = bslots[:, :, 0] != am.NO_SLOT
        assert job.any() and not job[ran].all() and not job[~ran].any()
        assert_equal_records(got_j[job], bjobs[job], "refinement jobs")
        assert (got_j[~job].view(np.uint8) == POISON).all()
        assert not len(differing(f.jobs.to_array(api.AFFINE_ME_DTYPE, jobs.size), jobs))
        f.f.d_bi_slots = None
        with pytest.raises(api.XvcGpuError, match="status 10: .*d_bi_slots"):
            f.call("xvcgpu_fp_bi_affine_uni_fold")
    finally:
        f.destroy()


def test_choice_equals_model(gpu, xo):
    """xvcgpu_fp_bi_affine_choice on the 10-bit grid, set C, with planted plain costs: a tie
    (plain stays), an affine state one cheaper and one dearer, every other capable CU's plain
    cost high, so that affine L0, L1 and bi states are all written; an unsupported plain
    record; a capable CU without bootstrap.  Records and prediction jobs byte for byte."""
    api, ctx = gpu
    lists = am.SETS["C"]
    found = am.search(xo, "grid10", "C")
    me00, order = found["me"][0][0], found["order"]
    plain, inter = found["plain"][3].copy(), am.plain_inter(found["plain"][4])
    jobs = found["jobs"].copy()
    base = found["choice"]
    tie, cheaper, dearer, dead, lost = (int(order[k]) for k in (0, 1, 2, 3, 4))
    plain["cost"][order] = am.NONE - 1
    plain["cost"][tie] = base["cost_affine"][tie]
    plain["cost"][cheaper] = int(base["cost_affine"][cheaper]) + 1
    plain["cost"][dearer] = int(base["cost_affine"][dearer]) - 1
    plain[dead:dead + 1].view(np.uint8)[:] = 0xff
    inter["ref"][3 * dead:3 * dead + 3] = -1
    jobs["flags"][lost, 0] = 0
    args = (lists, me00, jobs, found["slots"], found["ures"], found["bres"], found["fold"])
    exp_c, exp_i = am.choice_fold(*args, plain, inter)
    assert [int(exp_c["use_affine"][i]) for i in (tie, cheaper, dearer, lost)] == [0, 1, 0, 0]
    assert int(exp_c["cost_affine"][tie]) == int(exp_c["cost_plain"][tie])
    assert int(exp_c["cost_affine"][lost]) == am.NONE and int(exp_c["inter_dir"][dead]) == -1
    won = exp_c[exp_c["use_affine"] == 1]
    assert set(won["inter_dir"].tolist()) == {0, 1, 2}
    n = len(me00)
    f = Folds(api, ctx, lists, found["me"], found["plain"][0], jobs, found["slots"], order,
              found["n_class"], ures=found["ures"], bjobs=found["bjobs"],
              bslots=found["bslots"], bres=found["bres"], fold=found["fold"], plain=plain,
              inter=inter)
    try:
        f.call("xvcgpu_fp_bi_affine_choice")
        assert_equal_records(f.choice.to_array(api.FP_BI_AFFINE_RESULT_DTYPE, n), exp_c, "records")
        assert_equal_records(f.inter.to_array(api.INTER_DTYPE, 3 * n), exp_i, "prediction jobs")
        for b, arr in ((f.plain, plain), (f.jobs, jobs), (f.ures, found["ures"]),
                       (f.bres, found["bres"]), (f.bjobs, found["bjobs"])):
            assert not len(differing(b.to_array(arr.dtype, arr.size), arr))
        # the CU records of that choice, with and without a luma index
        nnz = np.arange(3 * n, dtype=np.int32) % 3
        index = np.arange(n, dtype=np.int32)[::-1].copy()
        d_nnz, d_index = f.buf(nnz), f.buf(index)
        f.a.p.d_nnz = d_nnz.ptr
        for use_index in (False, True):
            f.a.p.d_luma_tx_index = d_index.ptr if use_index else None
            f.call("xvcgpu_cu_info_from_bi_affine_choice")
            got = f.cus.to_array(api.CU_DTYPE, n)
            for i in range(n):
                c, ch = got[i], exp_c[i]
                d = int(ch["inter_dir"])
                used = (d in (0, 2), d in (1, 2))
                assert int(c["cbf_luma"]) == int(nnz[index[i] if use_index else i] != 0)
                assert (int(c["qp_y"]), int(c["qp_c"]), int(c["intra"])) == (31, 29, 0)
                assert int(c["ref_idx0"]) == (int(ch["ref_idx"][0]) if used[0] else -1)
                for l in range(2):
                    if not used[l]:
                        assert int(c["ref_poc"][l]) == -1 and not c["mv"][l].any()
                        continue
                    assert int(c["ref_poc"][l]) == lists[l][int(ch["ref_idx"][l])]
                    m = ch["mv"][l]
                    want = [m[0], m[1], m[2], m[1] + m[2] - m[0]] if int(ch["use_affine"]) == 1 \
                        else [m[0]] * 4
                    assert np.array_equal(c["mv"][l], np.array(want)), (i, l)
        f.f.d_choice = None
        with pytest.raises(api.XvcGpuError, match="status 10: .*d_choice"):
            f.call("xvcgpu_fp_bi_affine_choice")
    finally:
        f.destroy()


# ---- the pass ----------------------------------------------------------------------------
@pytest.mark.parametrize("name,form,which", [
    ("grid10", "residual", "A"), ("grid10", "residual_rdoq", "A"),
    ("grid10", "fwd_transform", "A"), ("grid8", "residual", "C"), ("part10", "residual", "A"),
    ("grid10", "residual", "D")])
def test_whole_pass_equals_model(gpu, xo, name, form, which):
    api, ctx = gpu
    found, exp = expected(xo, name, which, form != "residual")
    s = Scene(ctx, name, which, form)
    try:
        assert s.fp.p.fused_tail == (name != "part10")      # the partition holds sides of 4
        planned = name == "part10"
        assert all((p is not None) == (planned and s.fp.searched[l][r])
                   for l in range(2) for r, p in enumerate(s.fp.plans[l]))
        assert_pass_equal(s.run(), found, exp, "one call", s)
        s.Rec.upload([np.zeros_like(p) for p in exp[0]], BL)
        if planned:
            assert_pass_equal(s.run(planned=False), found, exp, "without plans", s)
        else:
            assert_pass_equal(s.run(fused_tail=False), found, exp, "separate tail", s)
    finally:
        s.destroy()


def test_one_call_equals_its_parts(gpu):
    """xvcgpu_frame_pass_bi_refs_affine against the entry points it is made of, issued in
    order from Python on a second set of buffers (set C on the grid, set A on the partition)."""
    api, ctx = gpu
    tail = {"grid10": ["deblock_pad_ssd"], "part10": ["deblock", "pad_border", "picture_ssd"]}
    for name, which in (("grid10", "C"), ("part10", "A")):
        a, b = Scene(ctx, name, which), Scene(ctx, name, which)
        try:
            one = a.run()
            steps = b.fp.kernel_steps(b.O, b.refs, b.Rec)
            names = [k for k, _ in steps]
            at = names.index("choice")
            assert names[at:] == ["choice", "affine_boot", "affine_uni", "affine_uni_fold",
                                  "affine_bi", "affine_choice", "inter_pred", "residual",
                                  "cu_info"] + tail[name]
            for _, fn in steps:
                fn()
            ctx.sync()
            parts = b.answer()
            for k in ("jobs", "ures", "bjobs", "bslots", "bres", "choice", "inter"):
                assert_equal_records(parts[k], one[k], ("parts", k))
            for x, y in zip(parts["results"][1:5], one["results"][1:5]):
                assert_equal_records(x, y, "parts: nnz, cus, ssd, plain choice")
            for k in ("rec", "pred"):
                assert all(np.array_equal(x, y) for x, y in zip(parts[k], one[k])), k
            assert int(one["choice"]["use_affine"].sum()) >= 4
        finally:
            a.destroy()
            b.destroy()


def test_no_capable_cu_equals_plain_pass(gpu):
    """affine=True on the 8-sample grid (no CU is capable: nothing is listed) against the
    plain B pass: the same records, pictures and SSD byte for byte, every record plain."""
    api, ctx = gpu
    a, b = Scene(ctx, "grid10", "A", cu=8), Scene(ctx, "grid10", "A", affine=False, cu=8)
    try:
        assert a.fp.affine.n_class == [0, 0, 0] and a.fp.affine.d_order is None
        x, y = a.run(), b.run()
        for k in range(7):
            if k == 0:
                for l in range(2):
                    for p, q in zip(x["results"][0][l], y["results"][0][l]):
                        assert_equal_records(p, q, "search")
            else:
                assert_equal_records(x["results"][k], y["results"][k], ("results", k))
        assert_equal_records(x["inter"], y["inter"], "prediction jobs")
        for k in ("rec", "pred"):
            assert all(np.array_equal(p, q) for p, q in zip(x[k], y[k])), k
        ch, pl = x["choice"], x["results"][4]
        assert not ch["use_affine"].any() and (ch["cost_affine"] == am.NONE).all()
        assert np.array_equal(ch["cost"], pl["cost"]) and np.array_equal(ch["inter_dir"], pl["inter_dir"])
        assert np.array_equal(ch["mv"][:, :, 0], pl["mv"]) and np.array_equal(ch["mv"][:, :, 2], pl["mv"])
        assert len(set(pl["inter_dir"].tolist())) >= 2
    finally:
        a.destroy()
        b.destroy()


def _poison(ctx, fp):
    f = fp.affine
    bufs = [fp.d_choice, fp.p.d_nnz, fp.p.d_cus, fp.d_inter, fp.d_bi_jobs, fp.d_bi_res,
            fp.d_bi_slots, f.d_uni_res, f.d_bi, f.d_bi_res, f.d_bi_slots, f.d_choice] + \
        [b for row in fp.d_res for b in row if b is not None]
    for b in bufs:
        ctx._check(ctx.lib.xvcgpu_memset(ctx.h, b.ptr, POISON, b.nbytes))
    return bufs


def test_refusals_enqueue_nothing(gpu):
    """Every refusal of the entry point happens before the first launch: the job arrays, the
    work arrays and rec are untouched.  And the Python class's own refusals."""
    from xvc_amd import pipeline
    api, ctx = gpu
    g, p = Scene(ctx, "grid10", "C"), Scene(ctx, "part10", "A")
    lic_plan = None
    try:
        for s in (g, p):
            s.Rec.upload([np.full_like(q, 0x0123) for q in am.scene(s.name)[4]], BL)

        def refused(s, bufs, change_a, change_f, match, plans=None, phases=ALL):
            fp = s.fp
            a, f = fp._call_args(s.O, s.refs, s.Rec), fp.affine.args()
            jobs = fp.affine_jobs()
            change_a(a)
            change_f(f)
            with pytest.raises(api.XvcGpuError,
                               match="status 10: frame_pass_bi_refs_affine: .*" + match):
                ctx._check(ctx.lib.xvcgpu_frame_pass_bi_refs_affine(
                    ctx.h, C.byref(a), C.byref(f), fp.plan_handles() if plans is None else plans,
                    phases))
            ctx.sync()
            for b in bufs:
                assert (b.to_array(np.uint8, b.nbytes) == POISON).all(), match
            assert not len(differing(fp.affine_jobs(), jobs)), match
            assert all((q == 0x0123).all() for q in s.Rec.download(BL)), match

        def on(field, value, index=None):
            def change(x):
                if index is None:
                    setattr(x, field, value)
                else:
                    getattr(x, field)[index] = value
            return change

        def on_p(field, value):
            def change(a):
                setattr(a.p, field, value)
            return change
        same = lambda x: None       # noqa: E731
        form = api.FP_FORM_NAMES.index
        bufs = _poison(ctx, g.fp)
        n = g.fp.desc.n_cus
        for change_a, change_f, match in [
                (on("force_l1_mvd_zero", 1), same, "force_l1_mvd_zero"),
                (on_p("form", form("recon_from_me")), same, "form"),
                (on_p("form", form("fwd_from_me")), same, "form"),
                (on_p("n_cus_total", n + 1), same, "whole pictures"),
                (on_p("db_y_end", 16), same, "whole pictures"),
                (on("d_choice", None), same, "d_choice"),
                (same, on("d_uni", None), "d_uni"),
                (same, on("d_uni_results", None), "d_uni"),
                (same, on("d_uni_slots", None), "d_uni"),
                (same, on("d_bi", None), "d_bi"),
                (same, on("d_bi_slots", None), "d_bi"),
                (same, on("d_choice", None), "affine: d_choice"),
                (same, on("d_order", None), "d_order"),
                (same, on("n_class", -1, 0), "n_class"),
                (same, on("n_class", n, 1), "n_class")]:
            refused(g, bufs, change_a, change_f, match)
        refused(g, bufs, same, same, "phases", phases=ALL & ~1)
        a = g.fp._call_args(g.O, g.refs, g.Rec)
        assert ctx.lib.xvcgpu_frame_pass_bi_refs_affine(ctx.h, C.byref(a), None,
                                                        g.fp.plan_handles(), ALL) == 10
        # a plan that holds LIC jobs
        bufs = _poison(ctx, p.fp)
        fp = p.fp
        lic = fp.me[0][0].copy()
        lic["fullpel_mv"][0] |= 2
        d_lic = ctx.buffer(lic)
        lic_plan = ctx.me_plan(d_lic.ptr, fp.desc.n_cus, fp.desc.cu_size)
        h = fp.plan_handles()
        for l in range(2):
            for r in range(len(fp.plans[l])):
                if fp.plans[l][r] is not None:
                    h[l][r] = lic_plan.h

        def lic_jobs(a):
            for l in range(2):
                for r in range(fp.num_ref[l]):
                    a.d_me[l][r] = d_lic.ptr
        refused(p, bufs, lic_jobs, same, "LIC", plans=h)
        d_lic.free()
        # and the same blocks run when nothing is wrong with them
        assert int(p.run()["choice"]["use_affine"].sum()) >= 4
        assert int(g.run()["choice"]["use_affine"].sum()) >= 4
        pw, ph, bd = g.size
        for kw, match in ((dict(ref_pocs=((4,), (0,)), low_delay=True), "low_delay"),
                          (dict(aqp_strength=13), "aqp_strength")):
            with pytest.raises(ValueError, match="affine: .*" + match):
                pipeline.BiRefsFramePass(ctx, pw, ph, bd, am.QP, affine=True, **kw)
    finally:
        if lic_plan is not None:
            lic_plan.destroy()
        g.destroy()
        p.destroy()


def test_other_passes_untouched_beside_the_b_affine_pass(gpu):
    """A plain B pass and a P pass with affine motion answer the same before and after a B
    pass with affine motion ran on their context, and that pass the same after them."""
    from xvc_amd import pipeline
    api, ctx = gpu
    s, plain = Scene(ctx, "grid10", "A"), Scene(ctx, "grid10", "A", affine=False)
    pw, ph, bd = s.size
    P = ctx.picture(pw, ph, bd)
    fp = pipeline.FramePass(ctx, pw, ph, bd, am.QP, fused=False, keep_levels=True, affine=True)
    try:
        def others():
            fp.run(s.O, s.refs[0][0], P)
            ctx.sync()
            return plain.run(), fp.results(), fp.affine_choice(), P.download(BL)

        def same(x, y):
            for k in ("inter", "rec", "pred"):
                assert all(np.array_equal(p, q) for p, q in zip(x[0][k], y[0][k])), k
            for k in range(1, 7):
                assert_equal_records(x[0]["results"][k], y[0]["results"][k], ("plain B", k))
            assert all(not len(differing(p, q)) for p, q in zip(x[1], y[1]))
            assert not len(differing(x[2], y[2]))
            assert all(np.array_equal(p, q) for p, q in zip(x[3], y[3]))
        before = others()
        b1 = s.run()
        same(before, others())
        assert before[2]["use_affine"].any() and before[0]["results"][4]["cost"].any()
        b2 = s.run()
        for k in ("jobs", "ures", "bjobs", "bslots", "bres", "choice", "inter"):
            assert_equal_records(b1[k], b2[k], ("B affine again", k))
        assert all(np.array_equal(p, q) for p, q in zip(b1["rec"], b2["rec"]))
    finally:
        fp.destroy()
        P.destroy()
        s.destroy()
        plain.destroy()


# ---- the host layer ----------------------------------------------------------------------
def test_host_class_equals_python_pass(gpu):
    """xvc_gpu::FramePassBiRefs with SetAffine (through xvc_host_frame_pass_bi_refs_affine)
    on set C equals pipeline.BiRefsFramePass(affine=True): both choice records, the CU
    records, SSD and the picture."""
    from xvc_amd import decoder
    api, ctx = gpu
    L = decoder.load_host_library()
    L.xvc_host_frame_pass_bi_refs_affine.argtypes = [C.c_void_p] + [C.c_int] * 5 + \
        [C.c_void_p] * 6 + [C.c_int] + [C.c_void_p] * 4
    s = Scene(ctx, "grid10", "C")
    pw, ph, bd = s.size
    Rec = ctx.picture(pw, ph, bd)
    try:
        got = s.run()
        _, _, cus, ssd, choice, _, _ = got["results"]
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
        h_affine = np.zeros(n, api.FP_BI_AFFINE_RESULT_DTYPE)
        h_cus = np.zeros(n, api.CU_DTYPE)
        h_ssd = np.zeros(2, np.uint64)
        assert L.xvc_host_frame_pass_bi_refs_affine(
            ctx.h, pw, ph, bd, am.QP, am.CUR_POC, num_ref.ctypes.data, pocs.ctypes.data,
            s.O.h_pic, pics, Rec.h_pic, blocks.ctypes.data, n, h_choice.ctypes.data,
            h_cus.ctypes.data, h_ssd.ctypes.data, h_affine.ctypes.data) == 0
        assert_equal_records(h_choice, choice, "plain choice")
        assert_equal_records(h_affine, got["choice"], "records")
        assert_equal_records(h_cus, cus, "CU records")
        assert h_ssd.tolist() == ssd.tolist()
        assert all(np.array_equal(x, y) for x, y in zip(Rec.download(BL), got["rec"]))
        assert int(h_affine["use_affine"].sum()) >= 4
    finally:
        Rec.destroy()
        s.destroy()
