"""The bit-depth dependent paths of the search and the quantiser, on the GPU against the
oracle.  Above 10 bit the sub-pel search leaves the packed 16-bit SATD sweep (k_subpel.h)
for the 32-bit row-major one, and the 64 class with it the four-wave team kernel for the
wave instance: a decision made per job inside the kernels (me2_subpel_fast, k_me2.h), on
the host for the planned search, and by both the wave instance and the team kernel where
both are launched.  A job neither takes keeps stale memory, a job both take is a race:
every form of the search is run here on poisoned records over a list of every shape, and
every record held against the oracle.  Then: the searches on full-swing residuals at 11
and 12 bit, the RDO quantiser's pipeline at 12 bit, and one pass of the main families at
the odd depths 9 (on the packed path) and 11 (the first depth off it)."""
import numpy as np
import pytest

import oracle_lib as ol
from helpers import (EXTREME_SHAPES, SIZES, bi_struct, extreme_bi_jobs, extreme_blocks,
                     make_pics, me_struct, walsh_pictures)
from test_gpu_parity import BL, gpu, xo  # noqa: F401  (fixtures)
from test_gpu_partition_pass import numpy_bins

pytestmark = pytest.mark.gpu

PW, PH = 352, 288
POISON = 0x5a5a5a5a
UNSUPPORTED = 0xffffffff
LIC, FULLPEL_MV = 2, 1      # XVC_ME_USE_LIC, XVC_ME_FULLPEL_MV
ODD_SHAPES = [(12, 16), (16, 48)]      # sizes the search does not have


def handoff_jobs(api, rng):
    """Every supported shape {4, 8, 16, 32, 64}^2 (64x4 and 4x64, the c64_wave bin, among
    them), each plain, with XVC_ME_FULLPEL_MV, with XVC_ME_USE_LIC and with both; and two
    jobs of sizes no instance takes."""
    shapes = [(w, h, f) for f in (0, FULLPEL_MV, LIC, LIC | FULLPEL_MV) for w in SIZES for h in SIZES]
    shapes += [(w, h, 0) for w, h in ODD_SHAPES]
    me = np.zeros(len(shapes), api.ME_DTYPE)
    for b, (w, h, f) in zip(me, shapes):
        b["w"], b["h"], b["fullpel_mv"] = w, h, f
        b["x"] = int(rng.integers(0, (PW - w) // 4 + 1)) * 4
        b["y"] = int(rng.integers(0, (PH - h) // 4 + 1)) * 4
        b["depth_nonzero"] = int(rng.integers(0, 2))
        b["mvp_x"], b["mvp_y"] = int(rng.integers(-200, 200)), int(rng.integers(-200, 200))
        b["prev_x"], b["prev_y"] = int(rng.integers(-20, 20)), int(rng.integers(-20, 20))
        b["lambda16"] = int(rng.choice([120000, 498000, 1500000]))
        b["search_range"] = int(rng.choice([96, 128]))
    return me


def supported(b, max_size=64, lic_ok=True):
    w, h = int(b["w"]), int(b["h"])
    return w in SIZES and h in SIZES and max(w, h) <= max_size and \
        (lic_ok or not int(b["fullpel_mv"]) & LIC)


class Expect:
    """The records the oracle gives for a job list against one reference picture; the
    searches are cached per job (every form asks for the same ones)."""

    def __init__(self, xo, bd, me, orig, ref):
        self.xo, self.bd, self.me, self.orig, self.ref = xo, bd, me, orig, ref
        self.tz, self.sub = {}, {}

    def fullpel(self, i):
        if i not in self.tz:
            self.tz[i] = self.xo.tz_search(self.bd, me_struct(self.me[i]), PW, PH, self.orig,
                                           self.ref, BL)
        return self.tz[i]

    def subpel(self, i, fp):
        """(mv, dist) from the full-pel vector fp.  XVC_ME_FULLPEL_MV: the vector stays,
        the distortion is GetSubpelDist's (SATD, AC-only for a LIC job) at it."""
        if (i, fp) not in self.sub:
            b = self.me[i]
            s = me_struct(b)
            if int(b["fullpel_mv"]) & FULLPEL_MV:
                mv = (16 * fp[0], 16 * fp[1])
                metric = 2 if int(b["fullpel_mv"]) & LIC else 1    # SATD_ACONLY / SATD
                dist = self.xo.mc_metric(self.bd, metric, 32, 16, s.x, s.y, s.w, s.h, mv, PW, PH,
                                         self.orig, self.ref, BL)
                self.sub[(i, fp)] = (mv, dist)
            else:
                self.sub[(i, fp)] = self.xo.subpel_search(self.bd, s, PW, PH, self.orig, self.ref,
                                                          BL, fp)
        return self.sub[(i, fp)]


def check_records(got, before, exp, idx, phases, max_size, lic_ok, what):
    """got[k] is the record of job idx[k] of exp.me after a search with `phases` over the
    records `before`.  Supported jobs: every field the phases define equals the oracle's,
    so no poisoned field survives; the full-pel fields of a sub-pel only search are its
    input.  Unsupported jobs read 0xffffffff."""
    bad = []
    for k, i in enumerate(idx):
        b, g = exp.me[i], got[k]
        if not supported(b, max_size, lic_ok):
            if int(g["fullpel_cost"]) != UNSUPPORTED or int(g["subpel_dist"]) != UNSUPPORTED:
                bad.append((int(i), "unsupported", tuple(b), tuple(g)))
            continue
        want = {}
        if phases & 1:
            (fx, fy), cost = exp.fullpel(i)
            want.update(fullpel_x=fx, fullpel_y=fy, fullpel_cost=cost)
        else:
            fx, fy = int(before[k]["fullpel_x"]), int(before[k]["fullpel_y"])
            want.update(fullpel_x=fx, fullpel_y=fy, fullpel_cost=int(before[k]["fullpel_cost"]))
        if phases & 2:
            (mx, my), dist = exp.subpel(i, (fx, fy))
            want.update(mv_x=mx, mv_y=my, subpel_dist=dist)
        have = {f: int(g[f]) for f in want}
        # (a full-pel only search leaves no oracle value for the sub-pel fields, but none
        # of them may be what was there)
        stale = [f for f in g.dtype.names if (phases & 1 or f in want) and int(g[f]) == POISON
                 and want.get(f) != POISON]
        if phases == 2:
            stale = [f for f in stale if not f.startswith("fullpel")]
        if have != want or stale:
            bad.append((int(i), "poisoned %s" % stale if stale else "mismatch", tuple(b),
                        have, want))
    assert not bad, (what, len(bad), bad[:6])


def start_records(api, rng, n, phases):
    """Poisoned records; a sub-pel only search starts from given full-pel vectors."""
    r = np.zeros(n, api.MERES_DTYPE)
    for f in r.dtype.names:
        r[f] = POISON
    if phases == 2:
        r["fullpel_x"], r["fullpel_y"] = rng.integers(-8, 9, n), rng.integers(-8, 9, n)
    return r


@pytest.fixture(scope="module")
def handoff(gpu):
    """Per depth: the job list, the two reference pictures and the oracle caches."""
    api, ctx = gpu
    made = {}

    def get(bd):
        if bd not in made:
            rng = np.random.default_rng(8800 + bd)
            orig, ref0 = make_pics(rng, bd, PW, PH, BL, (3, -2))
            ref1 = np.ascontiguousarray(np.roll(ref0, (2, -5), (0, 1)))
            me = handoff_jobs(api, np.random.default_rng(8900))     # one list for every depth
            pics = [ctx.picture(PW, PH, bd) for _ in range(3)]
            for p, host in zip(pics, (orig, ref0, ref1)):
                p.upload([host, None, None], BL)
            xo_ = ol.Lib("xo")
            made[bd] = (me, pics, [Expect(xo_, bd, me, orig, r) for r in (ref0, ref1)])
        return made[bd]

    yield get
    for me, pics, _ in made.values():
        for p in pics:
            p.destroy()


def test_handoff_list_fills_every_plan_bin():
    """(no GPU work: the list of the hand-off tests puts a job in every bin of the plan,
    the LIC bins and the unsupported one included)"""
    from xvc_amd import api
    me = handoff_jobs(api, np.random.default_rng(8900))
    counts = np.bincount(numpy_bins(api, me, 64), minlength=api.ME_PLAN_BINS)
    assert (counts > 0).all(), dict(zip(api.ME_PLAN_BIN_NAMES, counts.tolist()))
    # and below 64: the larger classes become unsupported jobs
    for mbs in (16, 32):
        c = np.bincount(numpy_bins(api, me, mbs), minlength=api.ME_PLAN_BINS)
        assert c[list(api.ME_PLAN_BIN_NAMES).index("unsupported")] > len(ODD_SHAPES)


PHASES = {"both": 3, "fullpel": 1, "subpel": 2}


@pytest.mark.parametrize("phases", list(PHASES))
@pytest.mark.parametrize("bd", [10, 11, 12])
def test_every_job_answered_once_sized(gpu, handoff, bd, phases):
    """xvcgpu_me_search_sized at max_block_size 16, 32 and 64, and its SQ16 hint form."""
    api, ctx = gpu
    me, (O, R0, _), (exp, _) = handoff(bd)
    ph = PHASES[phases]
    rng = np.random.default_rng(17)
    idx = np.arange(len(me))
    forms = [(16, 0), (32, 0), (64, 0)] + ([(64, api.ME_HINT_SQ16)] if ph == 3 else [])
    for mbs, hint in forms:
        before = start_records(api, rng, len(me), ph)
        got = ctx.me_search(O, R0, me, flags=ph | api.ME_LIC_JOBS | hint, results=before,
                            max_size=mbs)
        check_records(got, before, exp, idx, ph, mbs, True, ("sized", bd, phases, mbs, hint))
    # LIC jobs not announced: nobody takes them, they read unsupported
    before = start_records(api, rng, len(me), ph)
    got = ctx.me_search(O, R0, me, flags=ph, results=before, max_size=64)
    check_records(got, before, exp, idx, ph, 64, False, ("sized, LIC not announced", bd, phases))


@pytest.mark.parametrize("phases", list(PHASES))
@pytest.mark.parametrize("bd", [10, 11, 12])
def test_every_job_answered_once_planned(gpu, handoff, bd, phases):
    """xvcgpu_me_search_planned: the host chooses the 64 class's sub-pel kernels by depth."""
    api, ctx = gpu
    me, (O, R0, _), (exp, _) = handoff(bd)
    ph = PHASES[phases]
    rng = np.random.default_rng(18)
    idx = np.arange(len(me))
    d_me = ctx.buffer(me)
    for mbs in (16, 32, 64):
        plan = ctx.me_plan(d_me.ptr, len(me), mbs)
        expect = np.bincount(numpy_bins(api, me, mbs), minlength=api.ME_PLAN_BINS)
        assert np.array_equal(plan.counts, expect), (mbs, plan.counts, expect)
        for lic in (True, False):
            before = start_records(api, rng, len(me), ph)
            d_res = ctx.buffer(before)
            ctx.me_search_planned(O, R0, ph | (api.ME_LIC_JOBS if lic else 0), plan, d_res.ptr)
            ctx.sync()
            got = d_res.to_array(api.MERES_DTYPE, len(me))
            check_records(got, before, exp, idx, ph, mbs, lic, ("planned", bd, phases, mbs, lic))
            d_res.free()
        plan.destroy()
    d_me.free()


@pytest.mark.parametrize("phases", list(PHASES))
@pytest.mark.parametrize("bd", [10, 11, 12])
def test_every_job_answered_once_refs(gpu, handoff, bd, phases):
    """xvcgpu_me_search_refs at its three block classes with two reference slots: the
    class's jobs (the form takes no LIC jobs), each into the picture its slot names; a job
    without a slot keeps its record."""
    api, ctx = gpu
    me, (O, R0, R1), exps = handoff(bd)
    ph = PHASES[phases]
    rng = np.random.default_rng(19)
    mx = np.maximum(me["w"], me["h"]).astype(int)
    plain = (me["fullpel_mv"] & LIC) == 0
    for cls in (16, 32, 64):
        # (a size the search does not have is answered - unsupported - by the 16 class's
        # instances alone: the 12x16 job goes there, the 16x48 one into no call)
        pow2 = np.array([supported(b) for b in me])
        idx = np.flatnonzero(plain & (mx <= cls) & (mx > (cls // 2 if cls > 16 else 0)) &
                             (pow2 | (cls == 16)))
        assert len(idx) >= 12
        slots = rng.integers(0, 2, len(idx)).astype(np.uint8)
        slots[::7] = 255
        before = start_records(api, rng, len(idx), ph)
        got = ctx.me_search_refs(O, [R0, R1], me[idx], slots, cls, flags=ph, results=before)
        for s in (0, 1):
            k = np.flatnonzero(slots == s)
            assert len(k) > 0
            check_records(got[k], before[k], exps[s], idx[k], ph, cls, False,
                          ("refs", bd, phases, cls, s))
        none = slots == 255
        assert np.array_equal(got[none], before[none]), (bd, phases, cls)


def test_subpel_of_the_64_class_is_the_same_on_every_run(gpu, handoff):
    """bd 12, sub-pel only, the sized and the planned form twice each on the same inputs:
    the same bytes.  A job that both the wave instance and the team kernel took would
    usually still be right; that it is also the same every time is cheap evidence that it
    is not written twice (the comparison with the oracle is in the tests above)."""
    api, ctx = gpu
    me, (O, R0, _), _ = handoff(12)
    n = len(me)
    before = start_records(api, np.random.default_rng(21), n, 2)
    d_me = ctx.buffer(me)
    plan = ctx.me_plan(d_me.ptr, n, 64)
    runs = []
    for rep in range(2):
        runs.append(ctx.me_search(O, R0, me, flags=api.ME_SUBPEL | api.ME_LIC_JOBS, results=before))
        d_res = ctx.buffer(before)
        ctx.me_search_planned(O, R0, api.ME_SUBPEL | api.ME_LIC_JOBS, plan, d_res.ptr)
        ctx.sync()
        runs.append(d_res.to_array(api.MERES_DTYPE, n))
        d_res.free()
    assert runs[0].tobytes() == runs[2].tobytes() and runs[1].tobytes() == runs[3].tobytes()
    assert runs[0].tobytes() == runs[1].tobytes()
    plan.destroy()
    d_me.free()


@pytest.mark.parametrize("bd", [11, 12])
def test_searches_on_full_swing_residuals(gpu, xo, bd):
    """The Walsh and random-sign pictures of test_me_search_extreme_residuals (every
    residual +-(2^bd - 1), all 14 shapes) above the packed path's depths: the plain
    search, the AC-only (XVC_ME_USE_LIC) search and the bi-prediction refinement, whose
    2 * orig - pred target reaches -(2^bd - 1) .. 2 * (2^bd - 1) = -4095 .. 8190 at 12 bit,
    the int16 range the kernels hold it in.  The oracle is pinned on these inputs by
    test_oracle_vs_ref.py::test_search_on_full_swing_residuals (same seeds and draws)."""
    api, ctx = gpu
    rng = np.random.default_rng(3100 + bd)
    bi_rng = np.random.default_rng(3200 + bd)
    pw, ph = 256, 192
    O, R = ctx.picture(pw, ph, bd), ctx.picture(pw, ph, bd)
    for trial in range(6):
        orig, ref = walsh_pictures(rng, bd, pw, ph, BL, trial)
        O.upload([orig, None, None], BL)
        R.upload([ref, None, None], BL)
        plain = extreme_blocks(rng, pw, ph)
        for flags, blocks in ((0, plain), (api.ME_LIC_JOBS, extreme_blocks_lic(plain))):
            res = ctx.me_search(O, R, blocks, flags=api.ME_FULLPEL | api.ME_SUBPEL | flags)
            for i, b in enumerate(blocks):
                s = me_struct(b)
                (fx, fy), cost = xo.tz_search(bd, s, pw, ph, orig, ref, BL)
                got = tuple(int(res[i][f]) for f in res.dtype.names)
                (sx, sy), sd = xo.subpel_search(bd, s, pw, ph, orig, ref, BL, (fx, fy))
                assert got == (fx, fy, sx, sy, cost, sd), (trial, flags, tuple(b), got)
        jobs = extreme_bi_jobs(bi_rng, extreme_blocks(bi_rng, pw, ph))
        search, S = (ref, R) if trial % 2 == 0 else (orig, O)
        res = ctx.bipred_search(O, R, S, jobs)
        for i, j in enumerate(jobs):
            mv, dist = xo.bipred_search(bd, bi_struct(j), pw, ph, orig, ref, search, BL)
            got = ((int(res[i]["mv_x"]), int(res[i]["mv_y"])), int(res[i]["subpel_dist"]))
            assert got == (mv, dist), (trial, i, j, got, mv, dist)
    assert len(plain) == len(EXTREME_SHAPES)
    O.destroy()
    R.destroy()


def extreme_blocks_lic(blocks):
    lic = blocks.copy()
    lic["fullpel_mv"] = LIC
    return lic


RDOQ_QPS = (0, 17, 32, 51)


@pytest.mark.parametrize("full_swing", [False, True])
def test_residual_rdoq_pipeline_12bit(gpu, full_swing):
    """xvcgpu_residual_rdoq_batch at 12 bit end to end (the distortion term of the walk
    scales with 2 * (bd - 8)): the tiling of test_gpu_residual_rdoq_pipeline - blocks of
    4..64 a side, square and not, RDOQ and QuantFast blocks mixed - at QP 0, 17, 32 and 51,
    on random residuals and on residuals that are all +-4095."""
    from test_gpu_rdoq import residual_rdoq_pipeline
    api, ctx = gpu
    rng = np.random.default_rng(9412 + full_swing)
    residual_rdoq_pipeline(api, ctx, 12, rng, pw=256, ph=192, full_swing=full_swing, qps=RDOQ_QPS)


# ---- the odd depths, narrow: one pass of each family against the oracle ----
@pytest.mark.parametrize("bd", [9, 11])
def test_odd_depth_me_search(gpu, xo, bd):
    from test_gpu_parity import _me_search
    _me_search(gpu, xo, bd, [(3, -2)])


@pytest.mark.parametrize("bd", [9, 11])
def test_odd_depth_deblock(gpu, xo, bd):
    from test_gpu_parity import test_deblock
    test_deblock(gpu, xo, bd, 1, 4)


@pytest.mark.parametrize("bd", [9, 11])
def test_odd_depth_residual_pipeline(gpu, xo, bd):
    from test_gpu_parity import _residual_pipeline
    _residual_pipeline(gpu, xo, bd, False)


@pytest.mark.parametrize("bd", [9, 11])
def test_odd_depth_frame_pass(gpu, xo, bd):
    from test_gpu_parity import _frame_pass_bitdepth
    _frame_pass_bitdepth(gpu, xo, bd, 27, (136, 72))
