"""The B frame pass with merge mode on the GPU (xvcgpu_frame_pass_bi_refs_merge;
pipeline.BiRefsFramePass(merge_cands=...)): the rank kernel alone over every CU shape at
five bit depths with candidates of list 0, of list 1 and of both into 2 + 2 pictures against
the model's pieces and xvcgpu_mc_metric_batch_refs; the choice and the skip kernel alone on
planted records; the pass on three picture sets, three inputs and three forms against the
model composed of the oracle's pieces (tests/bi_merge_pass_model.py); a pass that lists no CU
against the plain B pass; the refusals; other passes beside it on one context; and the C++
class."""
import ctypes as C

import numpy as np
import pytest

import bi_merge_pass_model as bm
import bi_refs_pass_model as rm
import helpers
import merge_pass_model as mm
import oracle_lib as ol

pytestmark = pytest.mark.gpu

BL = bm.BL
ALL = 31    # FP_ENCODE | FP_DEBLOCK_V | FP_DEBLOCK_H | FP_PAD | FP_SSD
POISON = 0xA5
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


def differing(a, b):
    """Indices of the records that differ, byte for byte (any dtype)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype.itemsize == b.dtype.itemsize and len(a) == len(b)
    ra = a.view(np.uint8).reshape(len(a), -1)
    return np.flatnonzero((ra != b.view(np.uint8).reshape(len(b), -1)).any(1))


def poison_like(dtype, n):
    return np.full(n * np.dtype(dtype).itemsize, POISON, np.uint8).view(dtype)


class Blocks:
    """The two args blocks for the stage's kernels alone: the tables of `lists`, the same
    jobs `me` for every (list, picture), poisoned work arrays."""

    def __init__(self, api, ctx, lists, me):
        from xvc_amd import pipeline
        self.api, self.ctx, self.bufs = api, ctx, []
        num_ref, same, distinct, slot = rm.tables(lists)
        n, rmax = len(me), max(num_ref)
        self.n = n
        a = self.a = api.FramePassBiRefsArgs()
        a.p.n_cus = a.p.n_cus_total = n
        a.n_refs = len(distinct)
        d_me = self.buf(me)
        for r in range(api.CS_MAX_REFS):
            a.same_poc_in_l0[r] = same[r] if r < num_ref[1] else -1
        for l in range(2):
            a.num_ref[l] = num_ref[l]
            for r in range(num_ref[l]):
                a.slot[l][r], a.ref_poc[l][r] = slot[l][r], lists[l][r]
                a.d_me[l][r] = d_me.ptr
                a.d_results[l][r] = self.poisoned(api.MERES_DTYPE, n).ptr
        self.d_me = d_me
        self.choice = self.poisoned(api.FP_BI_REFS_RESULT_DTYPE, n + 1)
        self.inter = self.poisoned(api.INTER_DTYPE, 3 * n + 3)
        a.d_bi_jobs = self.poisoned(api.BI_DTYPE, n * rmax).ptr
        a.d_bi_results = self.poisoned(api.MERES_DTYPE, n * rmax).ptr
        a.d_bi_slots = self.poisoned(np.uint8, 2 * n * rmax).ptr
        a.d_choice, a.d_inter = self.choice.ptr, self.inter.ptr
        self.rank = self.poisoned(api.FP_MERGE_RANK_DTYPE, n + 1)
        self.won = self.poisoned(api.FP_BI_MERGE_RESULT_DTYPE, n + 1)
        self.chosen = self.poisoned(api.FP_BI_REFS_RESULT_DTYPE, n + 1)
        self.merge_args = pipeline.bi_merge_args

    def buf(self, arr):
        self.bufs.append(self.ctx.buffer(arr))
        return self.bufs[-1]

    def poisoned(self, dtype, n):
        return self.buf(poison_like(dtype, max(1, n)))

    def m(self, n_listed, cands, order=None, lambda_sqrt=bm.LAMBDA_SQRT, **drop):
        """The merge block; drop: the names of pointers to leave NULL"""
        ptrs = dict(d_cands=cands.ptr, d_order=order.ptr if order is not None else None,
                    d_rank=self.rank.ptr, d_choice=self.won.ptr, d_chosen=self.chosen.ptr)
        for k in drop:
            ptrs[k] = None
        return self.merge_args(n_listed, bm.MERGE_SIDE_BITS, lambda_sqrt, **ptrs)

    def destroy(self):
        for b in self.bufs:
            b.free()


# ---- the kernels alone -------------------------------------------------------------------
LISTS_A = bm.SETS["A"]      # 2 + 2 pictures: slots [[0, 1], [2, 3]]


@pytest.mark.parametrize("bd", [8, 9, 10, 11, 12])
def test_rank_kernel_every_shape(gpu, xo, bd):
    """All 25 shapes w, h in {4 .. 64} in the four corners of a 128x128 picture (at 9 and 11
    bit every fourth rectangle: AddAvgBi's shift depends on the depth) and a 12x16 CU, with
    candidates of list 0, of list 1 and of both lists into 2 + 2 pictures: vectors inside,
    vectors that leave the picture and far ones ClipMv changes, the same candidate at indices
    3 and 4, candidates that are not valid.  dist against the model's pieces (xo.mc_block /
    xo.mc_bipred_block + SATD), for one-list candidates also against
    xvcgpu_mc_metric_batch_refs; cost / order / num against the model's fold; through a list
    that leaves every seventh CU out, whose planted records stay as they are."""
    api, ctx = gpu
    pw = ph = 128
    rng = np.random.default_rng(7300 + bd)
    orig, ref = helpers.make_pics(rng, bd, pw, ph, BL, (3, -2))
    smax = (1 << bd) - 1
    planes = [ref]
    for k, shift in enumerate(((2, 1), (-3, 2), (1, -4))):
        noisy = np.roll(ref, shift, (0, 1)).astype(np.int32) + rng.integers(-3 - k, 4 + k, ref.shape)
        planes.append(np.ascontiguousarray(np.clip(noisy, 0, smax).astype(np.uint16)))
    rects = [(x, y, w, h) for w in mm.SIDES for h in mm.SIDES
             for x in (0, pw - w) for y in (0, ph - h)]
    if bd in (9, 11):
        rects = rects[::4]
    rects.append((16, 32, 12, 16))
    n = len(rects)
    me = np.zeros(n, api.ME_DTYPE)
    for i, r in enumerate(rects):
        me[i]["x"], me[i]["y"], me[i]["w"], me[i]["h"] = r
    cands = np.zeros((n, bm.CANDS), api.FP_MERGE_CAND_DTYPE)
    cands["mv"] = rng.integers(-40 * 16, 40 * 16 + 1, (n, bm.CANDS, 2, 2))
    cands["mv"][:, 1] = rng.integers(-150 * 16, 150 * 16 + 1, (n, 2, 2))      # leaves the picture
    cands["mv"][:, 2, 0] = rng.choice([-bm.FAR, bm.FAR], (n, 2))              # ClipMv acts
    cands["mv"][1::2, 2] = cands["mv"][1::2, 2, ::-1].copy()                      # ... in either list
    r0, r1 = rng.integers(0, 2, (n, bm.CANDS)), rng.integers(0, 2, (n, bm.CANDS))
    cands["ref_idx"][:, :, 0], cands["ref_idx"][:, :, 1] = r0, r1
    cands["ref_idx"][:, 0, 1] = -1                                            # list 0 alone
    cands["ref_idx"][:, 1, 0] = -1                                            # list 1 alone
    cands["ref_idx"][::2, 4, int(bd & 1)] = -1
    cands[::4, 4] = cands[::4, 3]                                             # equal candidates
    cands["ref_idx"][::3, 3] = [(-1, -1), (2, -1), (0, 2), (-2, 1)][bd % 4]   # not valid
    order = np.array([i for i in range(n) if i % 7 != 3], np.int32)
    O = ctx.picture(pw, ph, bd)
    O.upload([orig, None, None], BL)
    pics = []
    for p in planes:
        pics.append(ctx.picture(pw, ph, bd))
        pics[-1].upload([p, None, None], BL)
    k = Blocks(api, ctx, LISTS_A, me)
    d_cands, d_order = k.buf(cands), k.buf(order)
    k.a.p.orig = O.h_pic
    for s, p in enumerate(pics):
        k.a.refs[s] = p.h_pic
    try:
        call = ctx.lib.xvcgpu_fp_bi_merge_rank
        m = k.m(len(order), d_cands, d_order)
        ctx._check(call(ctx.h, C.byref(k.a), C.byref(m)))
        ctx.sync()
        got = k.rank.to_array(api.FP_MERGE_RANK_DTYPE, n + 1)
        left = [i for i in range(n + 1) if i not in set(order.tolist())]
        assert (got[left].view(np.uint8) == POISON).all()
        num_ref = [2, 2]
        shape_ok = np.isin(me["w"], mm.SIDES) & np.isin(me["h"], mm.SIDES)
        exp = np.full((n, bm.CANDS), NONE, np.uint64)
        uni, uni_at, clipped, kinds = [], [], 0, [0, 0, 0]
        for i in range(n):
            for c in range(bm.CANDS):
                cd = cands[i][c]
                if not (shape_ok[i] and bm.valid(cd, num_ref)):
                    continue
                r = [int(v) for v in cd["ref_idx"]]
                # list l's picture: slot[l][r] = 2 l + r
                use = [planes[2 * l + r[l]] if r[l] >= 0 else None for l in range(2)]
                exp[i][c] = bm.cand_dist_planes(xo, bd, pw, ph, orig, use, me[i], cd)
                kinds[2 if min(r) >= 0 else (0 if r[0] >= 0 else 1)] += 1
                for l in range(2):
                    if r[l] >= 0:
                        mv = tuple(int(v) for v in cd["mv"][l])
                        clipped += xo.clip_mv(*rects[i][:2], pw, ph, *mv) != mv
                if min(r) < 0:
                    l = 0 if r[0] >= 0 else 1
                    uni.append((rects[i], tuple(int(v) for v in cd["mv"][l]), 2 * l + r[l]))
                    uni_at.append((i, c))
        assert min(kinds) >= n // 2 and clipped >= n // 2
        mcm = np.zeros(len(uni), api.MCM_DTYPE)
        for j, (rect, mv, _) in enumerate(uni):
            mcm[j]["x"], mcm[j]["y"], mcm[j]["w"], mcm[j]["h"] = rect
            mcm[j]["mv_x"], mcm[j]["mv_y"], mcm[j]["metric"] = mv[0], mv[1], bm.SATD
        batch = ctx.mc_metric_batch_refs(O, pics, mcm, [s for _, _, s in uni])
        for (i, c), d in zip(uni_at, batch):
            assert int(exp[i][c]) == int(d), (i, c, rects[i], cands[i][c])
        nums, firsts = set(), set()
        for i in order:
            assert got[i]["dist"].tolist() == exp[i].tolist(), (i, rects[i], got[i], exp[i], cands[i])
            cost, rank, num = mm.rank_fold(exp[i])
            assert got[i]["order"].tolist() == rank and int(got[i]["num"]) == num, (i, got[i])
            assert got[i]["cost"].tolist() == cost and int(got[i]["reserved"]) == 0, (i, got[i])
            nums.add(num)
            firsts.add(rank[0])
        assert (got[n - 1]["dist"] == NONE).all() and got[n - 1]["order"].tolist() == [0, 1, 2, 3, 4]
        assert len(nums) >= 2 and len(firsts) >= 3
        # a NULL list: the CUs 0 .. n_listed - 1
        ctx.h2d(k.rank.ptr, poison_like(api.FP_MERGE_RANK_DTYPE, n + 1))
        m = k.m(10, d_cands)
        ctx._check(call(ctx.h, C.byref(k.a), C.byref(m)))
        ctx.sync()
        again = k.rank.to_array(api.FP_MERGE_RANK_DTYPE, n + 1)
        assert (again[10:].view(np.uint8) == POISON).all()
        keep = [i for i in range(10) if i in set(order.tolist())]
        assert not len(differing(again[keep], got[keep]))
        # refusals
        for bad in (k.m(n + 1, d_cands), k.m(-1, d_cands), k.m(4, d_cands, d_rank=None),
                    k.m(4, d_cands, d_cands=None), k.m(4, d_cands, lambda_sqrt=float("nan")),
                    k.m(4, d_cands, lambda_sqrt=-0.5)):
            assert call(ctx.h, C.byref(k.a), C.byref(bad)) == 10
        ctx.sync()
        assert (k.rank.to_array(api.FP_MERGE_RANK_DTYPE, n + 1)[10:].view(np.uint8) == POISON).all()
    finally:
        k.destroy()
        for p in [O] + pics:
            p.destroy()


def test_choice_kernel_on_planted_records(gpu):
    """A tie, merge one cheaper and one dearer, index 4, a best distortion of UINT32_MAX, a
    LIC job, an all-ones plain record, a candidate that is not valid, CUs the list does not
    name, winners of each direction and of ref_idx > 0 - against the model's fold byte for
    byte; the plain records stay as they are and the jobs are rewritten only for winners."""
    api, ctx = gpu
    lists = bm.SETS["C"]        # (4, 0, 16), (16, 12): slots [[0, 1, 2], [2, 3]]
    n = 12
    me = np.zeros(n, api.ME_DTYPE)
    me["x"], me["y"] = 16 * (np.arange(n) % 4), 16 * (np.arange(n) // 4)
    me["w"], me["h"], me["lambda16"] = 16, 8, bm.LAMBDA16
    me["lambda16"][7] = 0xfff00000          # a product beyond 32 bits
    me["fullpel_mv"][4] = 2                 # XVC_ME_USE_LIC
    rng = np.random.default_rng(41)
    plain = np.zeros(n, api.FP_BI_REFS_RESULT_DTYPE)
    plain["inter_dir"], plain["search_list"] = 2, rng.integers(0, 2, n)
    plain["ref_idx"], plain["mv"] = (1, 0), rng.integers(-300, 301, (n, 2, 2))
    plain["cost"] = 5000 + np.arange(n)
    plain["cost"][7] = 400000               # (above that CU's bits at its lambda)
    for f in ("cost_list", "cost_l1_unique", "cost_bi", "cost_uni", "bi_cost", "bi_mv", "best_ref"):
        plain[f] = rng.integers(0, 4000, plain[f].shape)
    plain[5:6].view(np.uint8)[:] = 0xff     # no search result
    inter_plain = [tuple(int(me[i][f]) for f in ("x", "y", "w", "h")) +
                   ((1, 2), tuple(tuple(int(v) for v in mv) for mv in plain[i]["mv"]))
                   for i in range(n)]
    m0s = (0, 1, 2, 4, 0, 0, 3, 0, 1, 2, 3, 0)
    refs = ((0, -1), (-1, 1), (2, 0), (1, 1), (0, 0), (0, 0), (0, 0), (2, -1), (-1, 0), (0, 1),
            (3, 0), (0, 0))                 # CU 10: an index >= num_ref
    delta = (0, -1, 1, 0, -50, -50, -50, 0, -1, -50, -50, -50)
    cands = np.zeros((n, bm.CANDS), api.FP_MERGE_CAND_DTYPE)
    cands["ref_idx"] = (0, 1)
    cands["mv"] = np.arange(n * 20).reshape(n, 5, 2, 2) * 37 - 4000
    ranks = np.zeros(n, api.FP_MERGE_RANK_DTYPE)
    for i in range(n):
        cands[i][m0s[i]]["ref_idx"] = refs[i]
        lam = int(me[i]["lambda16"])
        tie = (int(plain[i]["cost"]) -
               (((bm.MERGE_SIDE_BITS + mm.idx_bits(m0s[i])) * lam) >> 16)) & NONE
        d = [10 ** 8] * 5
        d[m0s[i]] = tie + delta[i]
        if i == 6:
            d = [NONE] * 5
        cost, order, num = mm.rank_fold(d)
        ranks[i] = (d, order, num, 0, cost)
    order = np.arange(n - 1, dtype=np.int32)        # CU 11: not named
    e_choice, e_chosen, e_inter = bm.choice_fold(lists, me, plain, inter_plain, cands, ranks, order)
    assert e_choice["use_merge"].tolist() == [1, 1, 0, 1, 0, -1, 0, 1, 1, 1, 0, 0]
    assert e_choice["merge_idx"].tolist() == [0, 1, -1, 4, -1, -1, -1, 0, 1, 2, -1, -1]
    assert e_chosen["inter_dir"][[0, 1, 3, 7, 8, 9]].tolist() == [0, 1, 2, 0, 1, 2]
    assert int(e_choice[0]["cost_merge"]) == int(e_choice[0]["cost_plain"])
    k = Blocks(api, ctx, lists, me)
    d_cands, d_order, d_ranks = k.buf(cands), k.buf(order), k.buf(ranks)
    jobs = np.zeros(3 * n + 3, api.INTER_DTYPE)     # the plain run's jobs, as its choice writes them
    for i, (x, y, w, h, ref, mv) in enumerate(inter_plain):
        for comp in range(3):
            j = jobs[3 * i + comp]
            j["x"], j["y"], j["w"], j["h"], j["comp"], j["ref"] = x, y, w, h, comp, ref
            j["mv"][:, 0, :] = mv
    jobs[3 * n:].view(np.uint8)[:] = POISON
    try:
        call = ctx.lib.xvcgpu_fp_bi_merge_choice
        for d_ord, n_listed, listed in ((d_order, len(order), order), (None, 3, [0, 1, 2]),
                                        (None, 0, [])):
            ctx.h2d(k.choice.ptr, np.concatenate([plain, poison_like(plain.dtype, 1)]))
            ctx.h2d(k.inter.ptr, jobs)
            ctx.h2d(k.won.ptr, poison_like(api.FP_BI_MERGE_RESULT_DTYPE, n + 1))
            ctx.h2d(k.chosen.ptr, poison_like(plain.dtype, n + 1))
            m = k.m(n_listed, d_cands, d_ord)
            m.d_rank = d_ranks.ptr
            ctx._check(call(ctx.h, C.byref(k.a), C.byref(m)))
            ctx.sync()
            exp = bm.choice_fold(lists, me, plain, inter_plain, cands, ranks, listed)
            won = k.won.to_array(api.FP_BI_MERGE_RESULT_DTYPE, n + 1)
            chosen = k.chosen.to_array(plain.dtype, n + 1)
            bad = differing(won[:n], exp[0])
            assert not len(bad), (n_listed, bad, won[bad], exp[0][bad])
            bad = differing(chosen[:n], exp[1])
            assert not len(bad), (n_listed, bad, chosen[bad], exp[1][bad])
            assert (won[n:].view(np.uint8) == POISON).all()
            assert (chosen[n:].view(np.uint8) == POISON).all()
            # d_choice keeps the plain answer; the jobs change for winners only
            assert not len(differing(k.choice.to_array(plain.dtype, n), plain))
            after = k.inter.to_array(api.INTER_DTYPE, 3 * n + 3)
            e_jobs = jobs.copy()
            for i in np.flatnonzero(exp[0]["use_merge"] == 1):
                x, y, w, h, ref, mv = exp[2][i]
                for comp in range(3):
                    e_jobs[3 * i + comp] = np.zeros(1, api.INTER_DTYPE)[0]
                    j = e_jobs[3 * i + comp]
                    j["x"], j["y"], j["w"], j["h"], j["comp"], j["ref"] = x, y, w, h, comp, ref
                    j["mv"][:, 0, :] = mv
            bad = differing(after, e_jobs)
            assert not len(bad), (n_listed, bad, after[bad], e_jobs[bad])
        assert not exp[0]["use_merge"][[0, 1, 2, 3, 4, 6, 7, 8, 9, 10, 11]].any()
        assert not len(differing(chosen[:n], plain))
        for buf, arr in ((k.d_me, me), (d_cands, cands.reshape(-1)), (d_ranks, ranks)):
            assert not len(differing(buf.to_array(arr.dtype, len(arr)), arr))
        for bad in (k.m(n + 1, d_cands), k.m(2, d_cands, d_choice=None),
                    k.m(2, d_cands, d_chosen=None), k.m(2, d_cands, d_rank=None)):
            assert call(ctx.h, C.byref(k.a), C.byref(bad)) == 10
        assert call(ctx.h, C.byref(k.a), None) == 10
    finally:
        k.destroy()


def test_skip_kernel_on_planted_nnz(gpu):
    """Each of Y, U and V alone keeps a merge CU from skip; a plain CU without levels is not
    skip; an all-ones record is left alone; nothing but `skip` is written; both layouts."""
    api, ctx = gpu
    n = 8
    choice = np.zeros(n, api.FP_BI_MERGE_RESULT_DTYPE)
    choice["use_merge"] = [1, 1, 1, 1, 0, 0, 1, 1]
    choice["merge_idx"] = [0, 1, 2, 3, -1, -1, 4, 0]
    choice["skip"] = 7                      # (whatever stood there)
    choice["inter_dir"], choice["ref_idx"] = np.arange(n) % 3, (1, -1)
    choice["cost"] = np.arange(n) + 100
    choice[5:6].view(np.uint8)[:] = 0xff    # no search result
    luma = np.array([21, 0, 3, 6, 9, 12, 15, 18], np.int32)       # not 3 i
    nnz = np.zeros(3 * n, np.int32)
    nnz[0], nnz[3 + 1], nnz[6 + 2] = 5, 1, 2    # Y of CU 1, U of CU 2, V of CU 3 (by `luma`)
    nnz[15 + 1] = 3                             # CU 6
    bufs = [ctx.buffer(a) for a in (choice, luma, nnz)]
    d_choice, d_luma, d_nnz = bufs
    try:
        call = ctx.lib.xvcgpu_fp_bi_merge_skip
        for d_l, idx in ((d_luma, luma), (None, 3 * np.arange(n))):
            ctx.h2d(d_choice.ptr, choice)
            ctx._check(call(ctx.h, d_nnz.ptr, d_l.ptr if d_l is not None else None, n, d_choice.ptr))
            ctx.sync()
            got = d_choice.to_array(api.FP_BI_MERGE_RESULT_DTYPE, n)
            exp = choice.copy()
            for i in range(n):
                if i != 5:
                    exp[i]["skip"] = int(choice[i]["use_merge"] == 1 and
                                         not nnz[idx[i]:idx[i] + 3].any())
            assert not len(differing(got, exp)), (got, exp)
        assert exp["skip"].tolist()[:5] == [0, 0, 0, 1, 0]          # the 3 i layout
        ctx.h2d(d_choice.ptr, choice)
        ctx._check(call(ctx.h, d_nnz.ptr, d_luma.ptr, n, d_choice.ptr))
        ctx.sync()
        assert d_choice.to_array(api.FP_BI_MERGE_RESULT_DTYPE, n)["skip"].tolist() == \
            [1, 0, 0, 0, 0, -1, 0, 1]
        assert call(ctx.h, None, d_luma.ptr, n, d_choice.ptr) == 10
        assert call(ctx.h, d_nnz.ptr, d_luma.ptr, n, None) == 10
    finally:
        for b in bufs:
            b.free()


# ---- the pass ----------------------------------------------------------------------------
class Scene:
    """bi_merge_pass_model.scene(name) on the device and a BiRefsFramePass of the named form
    over it with the model's lambda in its jobs and the model's candidates."""

    def __init__(self, ctx, xo, name, which="A", form="residual", merge=True, listed=None,
                 lambda16=bm.LAMBDA16, qp=bm.QP):
        from xvc_amd import pipeline
        pw, ph, bd, part, orig, refs = bm.scene(name)
        self.ctx, self.name, self.which, self.size = ctx, name, which, (pw, ph, bd)
        self.lists = lists = bm.SETS[which]
        self.O, self.Rec = ctx.picture(pw, ph, bd), ctx.picture(pw, ph, bd)
        self.O.upload(orig, BL)
        self.by_poc = {}
        for poc in sorted(set(lists[0]) | set(lists[1])):
            self.by_poc[poc] = ctx.picture(pw, ph, bd)
            self.by_poc[poc].upload(refs[poc], BL)
        self.refs = [[self.by_poc[poc] for poc in lists[l]] for l in range(2)]
        kw = {}
        if merge:
            kw = dict(merge_cands=bm.search(xo, name, which)[1], merge_order=listed,
                      merge_side_bits=bm.MERGE_SIDE_BITS,
                      merge_lambda_sqrt=bm.LAMBDA_SQRT if lambda16 is not None else None)
        self.fp = pipeline.BiRefsFramePass(
            ctx, pw, ph, bd, qp, rdoq=form != "residual", rdoq_packed=form == "fwd_transform",
            keep_levels=True, partition=part, cur_poc=rm.CUR_POC, ref_pocs=lists,
            search_range=rm.SEARCH_RANGE, side_bits=rm.SIDE_BITS, **kw)
        assert self.fp.form == form and (self.fp.p.plan is not None) == (part is not None)
        base = self.fp.desc.me.copy()
        if lambda16 is not None:
            base["lambda16"] = lambda16
        self.me = [[base.copy() for _ in lists[l]] for l in range(2)]
        for l in range(2):
            for r, poc in enumerate(lists[l]):
                self.me[l][r]["search_range"] = rm.search_range(poc)
        self.fp.set_jobs(self.me)

    def run(self, **kw):
        self.Rec.upload([np.full_like(p, 0x0123) for p in bm.scene(self.name)[4]], BL)
        self.fp.run(self.O, self.refs, self.Rec, **kw)
        self.ctx.sync()
        return self.fp.results(), self.Rec.download(BL)

    def destroy(self):
        self.fp.destroy()
        for p in [self.O, self.Rec] + list(self.by_poc.values()):
            p.destroy()


_expected = {}


def expected(xo, name, which, rdoq):
    """The model's pass, once per (input, set, quantiser)."""
    if (name, which, rdoq) not in _expected:
        desc = bm.descriptors(name, rdoq)
        e = _expected[name, which, rdoq] = bm.frame_pass(xo, name, which, desc,
                                                         bm.search(xo, name, which))
        coded = [int((e[2][desc.tx["comp"] == c] != 0).sum()) for c in range(3)]
        use = e[10]["use_merge"]
        assert min(coded) >= 1 and int(use.sum()) >= 12 and int((use == 0).sum()) >= 4, coded
    return _expected[name, which, rdoq]


def assert_pass_equal(scene, got, exp, searched, what):
    """got: Scene.run(); exp: bm.frame_pass's answer; searched: bm.search's."""
    (res, nnz, cus, ssd, choice, bi, slots), rec = got
    e_rec, e_res, e_nnz, e_cus, e_ssd, e_chosen, e_bi, e_slots, e_pred, e_levels, e_won, e_plain = exp
    fp = scene.fp
    for l in range(2):
        for r in range(len(res[l])):
            assert (res[l][r] is None) == (e_res[l][r] is None), (what, "re-use", l, r)
            if res[l][r] is not None:
                bad = differing(res[l][r], e_res[l][r])
                assert not len(bad), (what, "search", l, r, bad[:4])
    bad = differing(choice, e_plain)
    assert not len(bad), (what, "plain choice", bad[:4], choice[bad[:4]], e_plain[bad[:4]])
    ranks = fp.merge_rank()
    bad = differing(ranks, searched[2])
    assert not len(bad), (what, "rank", bad[:4], ranks[bad[:4]], searched[2][bad[:4]],
                          searched[1][bad[:4]])
    chosen = fp.chosen_results()
    bad = differing(chosen, e_chosen)
    assert not len(bad), (what, "chosen", bad[:4], chosen[bad[:4]], e_chosen[bad[:4]])
    pred = fp.p.pred.download(0)
    for c in range(3):
        assert np.array_equal(pred[c], e_pred[c]), (what, "prediction plane", c,
                                                    np.argwhere(pred[c] != e_pred[c])[:4])
    assert np.array_equal(nnz, e_nnz), (what, "nnz", np.flatnonzero(nnz != e_nnz)[:8])
    won = fp.merge_choice()
    bad = differing(won, e_won)
    assert not len(bad), (what, "merge records", bad[:4], won[bad[:4]], e_won[bad[:4]])
    bad = differing(cus, e_cus)
    assert not len(bad), (what, "CU records", bad[:4], cus[bad[:4]], e_cus[bad[:4]])
    for c in range(3):
        assert np.array_equal(rec[c], e_rec[c]), (what, "plane", c,
                                                  np.argwhere(rec[c] != e_rec[c])[:4])
    assert (int(ssd[0]), int(ssd[1])) == tuple(int(v) for v in e_ssd), (what, "ssd")
    p = fp.p
    if p.d_levels is not None:
        levels = p.d_levels.to_array(np.int16, max(1, p.n_levels))
        off = np.asarray(scene.ctx.level_offsets(p.desc.tx)[0], np.int64)
        for t, lv in enumerate(e_levels):
            if e_nnz[t]:    # (a block without levels: its part of the buffer is unspecified)
                assert np.array_equal(levels[off[t]:off[t] + len(lv)], lv), (what, "levels", t)


@pytest.mark.parametrize("form", ["residual", "residual_rdoq", "fwd_transform"])
@pytest.mark.parametrize("name", ["grid10", "grid8", "part10"])
@pytest.mark.parametrize("which", ["A", "C", "D"])
def test_pass_equals_model(gpu, xo, which, name, form):
    """Search results and plain choice records (unchanged), rank, merge and chosen records,
    the prediction picture, levels, nnz, CU records, reconstruction and SSD of the pass
    against the model; the fused and the separate tail; on the partition with and without
    plans."""
    api, ctx = gpu
    exp, searched = expected(xo, name, which, form != "residual"), bm.search(xo, name, which)
    s = Scene(ctx, xo, name, which, form)
    try:
        part = name == "part10"
        assert_pass_equal(s, s.run(), exp, searched, "one call")
        if part:
            assert_pass_equal(s, s.run(planned=False), exp, searched, "without plans")
        else:
            assert_pass_equal(s, s.run(fused_tail=False), exp, searched, "separate tail")
    finally:
        s.destroy()


def test_kernel_steps_equal_the_one_call(gpu, xo):
    """kernel_steps lists the new launches; run in order they are the pass."""
    api, ctx = gpu
    s = Scene(ctx, xo, "grid10", "C", "residual_rdoq")
    try:
        one = s.run()
        records = [s.fp.merge_rank(), s.fp.merge_choice(), s.fp.chosen_results()]
        s.Rec.upload([np.full_like(p, 0x0123) for p in bm.scene(s.name)[4]], BL)
        steps = s.fp.kernel_steps(s.O, s.refs, s.Rec)
        names = [k for k, _ in steps]
        at = [names.index(k) for k in ("choice", "merge_rank", "merge_choice", "inter_pred",
                                       "cu_info", "merge_skip")]
        assert at == sorted(at) and at[1] == at[0] + 1 and at[3] == at[2] + 1
        for _, f in steps:
            f()
        ctx.sync()
        two = s.fp.results(), s.Rec.download(BL)
        assert all(np.array_equal(x, y) for x, y in zip(one[1], two[1]))
        assert not len(differing(one[0][2], two[0][2])) and np.array_equal(one[0][1], two[0][1])
        for a, b in zip(records, [s.fp.merge_rank(), s.fp.merge_choice(), s.fp.chosen_results()]):
            assert not len(differing(a, b))
    finally:
        s.destroy()


@pytest.mark.parametrize("name,which,form", [("grid10", "A", "residual"),
                                             ("part10", "C", "fwd_transform")])
def test_pass_without_listed_cus_equals_plain_pass(gpu, xo, name, which, form):
    """merge_cands with no CU listed gives xvcgpu_frame_pass_bi_refs' bytes - results, nnz,
    records, SSD, jobs, prediction, picture - and records that say plain for every CU; the
    pass that lists every CU gives another picture."""
    api, ctx = gpu
    a, f = Scene(ctx, xo, name, which, form, listed=[]), Scene(ctx, xo, name, which, form, merge=False)
    m = Scene(ctx, xo, name, which, form)
    try:
        assert a.fp.merge.n_listed == 0 and m.fp.merge.n_listed == a.fp.desc.n_cus
        (ra, pa), (rf, pf) = a.run(), f.run()
        for x, y in zip(ra[1:5] + ra[6:], rf[1:5] + rf[6:]):
            assert np.ascontiguousarray(x).tobytes() == np.ascontiguousarray(y).tobytes()
        job = rf[6][:, :, 0] != rm.NO_JOB       # (no job: nobody writes the refinement's record)
        assert ra[5][job].tobytes() == rf[5][job].tobytes() and job.any()
        for l in range(2):
            for x, y in zip(ra[0][l], rf[0][l]):
                assert (x is None and y is None) or x.tobytes() == y.tobytes()
        assert all(np.array_equal(x, y) for x, y in zip(pa, pf))
        assert a.fp.inter_jobs().tobytes() == f.fp.inter_jobs().tobytes()
        assert all(np.array_equal(x, y) for x, y in zip(a.fp.p.pred.download(0),
                                                        f.fp.p.pred.download(0)))
        assert rf[1].any()
        won = a.fp.merge_choice()
        assert not won["use_merge"].any() and (won["cost_merge"] == NONE).all()
        assert not won["skip"].any() and (won["merge_idx"] == -1).all()
        assert np.array_equal(won["mv"], rf[4]["mv"]) and np.array_equal(won["cost"], rf[4]["cost"])
        assert a.fp.chosen_results().tobytes() == rf[4].tobytes()
        rm_, pm = m.run()
        assert rm_[4].tobytes() == rf[4].tobytes()       # (the plain run is the plain pass's)
        assert len(differing(rm_[2], rf[2])) >= 4
        assert any(not np.array_equal(x, y) for x, y in zip(pm, pf))
    finally:
        for s in (a, f, m):
            s.destroy()


# ---- refusals ----------------------------------------------------------------------------
def test_refusals_enqueue_nothing(gpu, xo):
    """Every missing array, n_listed outside [0, n_cus], phases without ENCODE, a lambda_sqrt
    that is not finite or below 0, force_l1_mvd_zero, and refusals of the plain pass:
    XVCGPU_INVALID_ARGUMENT naming the field, with the work arrays and rec as they were."""
    api, ctx = gpu
    s = Scene(ctx, xo, "grid10", "A", "fwd_transform")
    try:
        def a_set(**kw):
            return lambda a, m: [setattr(a.p, k, v) for k, v in kw.items()]

        def m_set(**kw):
            return lambda a, m: [setattr(m, k, v) for k, v in kw.items()]
        cases = [
            (m_set(d_cands=None), "d_cands", ALL),
            (m_set(d_rank=None), "d_rank", ALL),
            (m_set(d_choice=None), "d_choice", ALL),
            (m_set(d_chosen=None), "d_chosen", ALL),
            (lambda a, m: setattr(m, "d_chosen", a.d_choice), "plain pass's d_choice", ALL),
            (lambda a, m: setattr(m, "d_choice", a.d_choice), "plain pass's d_choice", ALL),
            (lambda a, m: setattr(m, "d_choice", m.d_chosen), "two arrays", ALL),
            (m_set(n_listed=-1), "n_listed", ALL),
            (lambda a, m: setattr(m, "n_listed", a.p.n_cus + 1), "n_listed", ALL),
            (m_set(lambda_sqrt=float("nan")), "lambda_sqrt", ALL),
            (m_set(lambda_sqrt=float("inf")), "lambda_sqrt", ALL),
            (m_set(lambda_sqrt=-1.0), "lambda_sqrt", ALL),
            (a_set(d_nnz=None), "d_nnz", ALL),
            (a_set(), "phases", ALL & ~api.FP_ENCODE),
            (lambda a, m: setattr(a, "force_l1_mvd_zero", 1), "force_l1_mvd_zero", ALL),
            (a_set(db_y_end=64), "whole pictures", ALL),
            (a_set(form=2), "form", ALL),
            (lambda a, m: setattr(a, "d_inter", None), "d_inter", ALL),
        ]
        fp, fm = s.fp, s.fp.merge
        s.Rec.upload([np.full_like(q, 0x0123) for q in bm.scene(s.name)[4]], BL)
        bufs = [fp.d_choice, fp.d_inter, fp.d_bi_res, fp.p.d_nnz, fp.p.d_cus, fp.p.d_ssd,
                fm.d_rank, fm.d_choice, fm.d_chosen] + [b for row in fp.d_res for b in row if b]
        for b in bufs:
            ctx._check(ctx.lib.xvcgpu_memset(ctx.h, b.ptr, POISON, b.nbytes))
        call = ctx.lib.xvcgpu_frame_pass_bi_refs_merge
        for change, match, phases in cases:
            a, m = fp._call_args(s.O, s.refs, s.Rec), fm.args()
            change(a, m)
            with pytest.raises(api.XvcGpuError, match="status 10: .*" + match):
                ctx._check(call(ctx.h, C.byref(a), C.byref(m), fp.plan_handles(), phases))
            ctx.sync()
            for b in bufs:
                assert (b.to_array(np.uint8, b.nbytes) == POISON).all(), match
            assert all((q == 0x0123).all() for q in s.Rec.download(BL)), match
        a = fp._call_args(s.O, s.refs, s.Rec)
        assert call(ctx.h, C.byref(a), None, fp.plan_handles(), ALL) == 10
        ctx.sync()
        assert (fm.d_choice.to_array(np.uint8, fm.d_choice.nbytes) == POISON).all()
        # ... and the same blocks run when nothing is wrong with them
        exp = expected(xo, s.name, s.which, True)
        assert_pass_equal(s, s.run(), exp, bm.search(xo, s.name, s.which), "after refusals")
    finally:
        s.destroy()


# ---- state and the C++ class -------------------------------------------------------------
def test_other_passes_untouched_beside_the_b_merge_pass(gpu, xo):
    """A plain B pass and a P pass with merge mode answer the same before and after a B pass
    with merge mode ran on their context."""
    import test_gpu_merge_frame_pass as tp
    api, ctx = gpu
    plain = Scene(ctx, xo, "grid10", "A", "residual_rdoq", merge=False)
    p_merge = tp.Scene(ctx, xo, "grid10", "residual")
    b_merge = Scene(ctx, xo, "grid10", "A", "residual_rdoq")
    try:
        before = plain.run(), p_merge.run()
        p_records = [p_merge.fp.merge_rank(), p_merge.fp.merge_choice()]
        first = b_merge.run()
        after = plain.run(), p_merge.run()
        for (ra, pa), (rb, pb) in ((before[0], after[0]),):
            assert all(np.ascontiguousarray(x).tobytes() == np.ascontiguousarray(y).tobytes()
                       for x, y in zip(ra[1:5], rb[1:5]))
            assert all(np.array_equal(x, y) for x, y in zip(pa, pb))
        (ra, pa, _), (rb, pb, _) = before[1], after[1]
        assert all(not len(differing(x, y)) for x, y in zip(ra, rb))
        assert all(np.array_equal(x, y) for x, y in zip(pa, pb))
        for x, y in zip(p_records, [p_merge.fp.merge_rank(), p_merge.fp.merge_choice()]):
            assert not len(differing(x, y))
        again = b_merge.run()
        assert all(np.array_equal(x, y) for x, y in zip(first[1], again[1]))
        assert any(not np.array_equal(x, y) for x, y in zip(first[1], before[0][1]))
        exp = expected(xo, "grid10", "A", True)
        assert_pass_equal(b_merge, again, exp, bm.search(xo, "grid10", "A"), "beside others")
    finally:
        for s in (plain, p_merge, b_merge):
            s.destroy()


@pytest.mark.parametrize("name,which", [("grid10", "C"), ("grid8", "D")])
def test_host_class_equals_python_pass(gpu, xo, name, which):
    """xvc_gpu::FramePassBiRefs with SetMerge (through xvc_host_frame_pass_bi_refs_merge)
    equals pipeline.BiRefsFramePass(merge_cands=...) at the QP's own lambda_sqrt: plain choice,
    rank, merge and chosen records, CU records, SSD, picture."""
    from xvc_amd import decoder
    api, ctx = gpu
    L = decoder.load_host_library()
    f = L.xvc_host_frame_pass_bi_refs_merge
    f.restype = C.c_int
    f.argtypes = [C.c_void_p] + [C.c_int] * 5 + [C.c_void_p] * 6 + [C.c_int] + [C.c_void_p] * 2 + \
        [C.c_double] + [C.c_void_p] * 6
    qp = 27
    s = Scene(ctx, xo, name, which, "residual", lambda16=None, qp=qp)
    pw, ph, bd = s.size
    Rec = ctx.picture(pw, ph, bd)
    try:
        (res, nnz, cus, ssd, choice, _, _), rec = s.run()
        won = s.fp.merge_choice()
        assert int(won["use_merge"].sum()) >= 4 and int((won["use_merge"] == 0).sum()) >= 2
        n = s.fp.desc.n_cus
        lists = s.lists
        num_ref = np.array([len(lists[0]), len(lists[1])], np.int32)
        pocs = np.zeros((2, api.CS_MAX_REFS), np.int32)
        handles = (C.c_void_p * (2 * api.CS_MAX_REFS))()
        blocks = np.zeros((2, api.CS_MAX_REFS, n), api.ME_DTYPE)
        for l in range(2):
            for r, poc in enumerate(lists[l]):
                pocs[l][r], handles[api.CS_MAX_REFS * l + r] = poc, s.by_poc[poc].h_pic
                blocks[l][r] = s.me[l][r]
        cands = s.fp.merge.cands
        ri = np.ascontiguousarray(cands["ref_idx"], np.int32)
        mv = np.ascontiguousarray(cands["mv"], np.int32)
        h_choice, h_chosen = np.zeros(n, choice.dtype), np.zeros(n, choice.dtype)
        h_cus, h_rank = np.zeros(n, api.CU_DTYPE), np.zeros(n, api.FP_MERGE_RANK_DTYPE)
        h_won, h_ssd = np.zeros(n, api.FP_BI_MERGE_RESULT_DTYPE), np.zeros(2, np.uint64)
        assert f(ctx.h, pw, ph, bd, qp, rm.CUR_POC, num_ref.ctypes.data, pocs.ctypes.data,
                 s.O.h_pic, handles, Rec.h_pic, blocks.ctypes.data, n, ri.ctypes.data,
                 mv.ctypes.data, -1.0, h_choice.ctypes.data, h_cus.ctypes.data, h_ssd.ctypes.data,
                 h_rank.ctypes.data, h_won.ctypes.data, h_chosen.ctypes.data) == 0
        assert not len(differing(h_choice, choice)) and not len(differing(h_cus, cus[:n]))
        assert not len(differing(h_rank, s.fp.merge_rank()))
        assert not len(differing(h_won, won))
        assert not len(differing(h_chosen, s.fp.chosen_results()))
        assert h_ssd.tolist() == [int(v) for v in ssd]
        assert all(np.array_equal(x, y) for x, y in zip(Rec.download(BL), rec))
    finally:
        Rec.destroy()
        s.destroy()
