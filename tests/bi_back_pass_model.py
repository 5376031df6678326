"""The expected frame pass of a B picture whose references all lie before it
(xvcgpu_frame_pass_bi_back, pipeline.BiRefsFramePass(low_delay=True)): the composition of
tests/bi_refs_pass_model.py (whose helpers it imports) with the two folds of
InterSearch::SearchMotion under force_l1_mvd_zero (inter_search.cc:410-413, :470-471,
:496-524) in Python integers, worded as include/xvcgpu.h words them, and the predictor cost
EvalStartMvp (:967-997) from xo.mc_block and a SAD.  Its SearchMotion half is pinned to the
reference's own member function, and the predictor cost to xr_eval_start_mvp, by
tests/test_bi_back_pass_model.py.

Also the scene and the reference picture sets the low-delay tests share: its own generator
(make_refs) with its own tables - bi_refs_pass_model's SHIFT / GRAIN / CUR_POC are read by
other tests and stay untouched.

TEST INFRASTRUCTURE."""
import numpy as np

import bi_refs_pass_model as rm
import helpers
import oracle_lib as ol

BL, BC = rm.BL, rm.BC
LAMBDA16, QP, SIDE_BITS, SEARCH_RANGE = rm.LAMBDA16, rm.QP, rm.SIDE_BITS, rm.SEARCH_RANGE
MAX_REFS, NO_JOB, NONE = rm.MAX_REFS, rm.NO_JOB, rm.NONE
CHOICE_DTYPE, INPUTS = rm.CHOICE_DTYPE, rm.INPUTS
CUR_POC = 20
# name -> (list 0's POCs, list 1's POCs), every POC before CUR_POC
SETS = {"E": ((16, 12), (16, 12)),      # the low-delay default: both list-1 pictures re-used
        "F": ((16, 12), (12, 4, 0)),    # Rmax 3 with a no-job third slot, one re-used, two unique
        "G": ((16, 12, 4), (0,)),       # three refinement jobs per CU, one unique picture
        "H": ((16,), (16,))}            # one picture per list
# luma displacement (rows, columns) per POC
SHIFT = {0: (4, -6), 4: (2, -2), 12: (0, 0), 16: (0, 0)}
# grain strength (8-bit units) per POC in each fifth of the width
GRAIN = {16: (1, 10, 4, 8, 8), 12: (4, 1, 4, 8, 8), 4: (8, 8, 8, 8, 1), 0: (8, 8, 8, 1, 8)}

tables, descriptors, eg_bits, mvd_bits, ref_idx_bits = \
    rm.tables, rm.descriptors, rm.eg_bits, rm.mvd_bits, rm.ref_idx_bits


def make_refs(name):
    """bi_refs_pass_model.make_refs with this file's SHIFT and GRAIN: (pw, ph, bd, partition,
    orig, {poc: [Y, U, V] padded planes})."""
    pw, ph, bd, part = INPUTS[name]
    rng = np.random.default_rng(7700 + bd)
    orig = [rm._original(rng, bd, pw >> (c > 0), ph >> (c > 0), BC if c else BL) for c in range(3)]
    part = part() if part else None
    rng = np.random.default_rng(9100 + bd)
    shared = [rng.integers(-64, 65, p.shape) for p in orig]
    refs = {}
    for poc in sorted(SHIFT):
        planes = []
        for c in range(3):
            border = BC if c else BL
            x = np.arange(orig[c].shape[1])[None, :] - border
            band = np.clip(x * 5 // (pw >> (c > 0)), 0, 4)
            amp = np.array(GRAIN[poc])[band] << (bd - 8)
            own = rng.integers(-64, 65, orig[c].shape)
            grain = (np.where((band == 4) & (poc in (12, 16)), shared[c], own) * amp) >> 6
            noisy = np.clip(orig[c].astype(np.int32) + grain, 0, (1 << bd) - 1)
            dy, dx = (v >> (c > 0) for v in SHIFT[poc])
            planes.append(np.ascontiguousarray(np.roll(noisy, (dy, dx), (0, 1)).astype(np.uint16)))
        refs[poc] = planes
    return pw, ph, bd, part, orig, refs


def search_range(poc):
    """InterSearch::GetSearchRangeUniPred (inter_search.cc:1050-1057) at CUR_POC with a
    sub-GOP of 16 and the settings' 96 .. 256"""
    return min(256, max(96, (256 * abs(CUR_POC - poc) + 8) // 16))


def jobs(desc, lists):
    """me[l][r]: the descriptors' jobs with each picture's own search range."""
    me = [[desc.me.copy() for _ in lists[l]] for l in range(2)]
    for l in range(2):
        for r, poc in enumerate(lists[l]):
            me[l][r]["search_range"] = search_range(poc)
    return me


def _cost(dist, bits, lambda16):
    return (dist + ((bits * lambda16) >> 16)) & NONE


def shape_taken(w, h):
    """What xvcgpu_fp_bi_back_mvp_cost takes: both sides 4, 8, 16, 32 or 64."""
    return w in (4, 8, 16, 32, 64) and h in (4, 8, 16, 32, 64)


def mvp_cost(xo, bd, pw, ph, orig_y, ref_y, b):
    """EvalStartMvp with both entries the job's mvp: SAD(orig, MotionCompensationMv(mvp)) +
    ((GetMvpBits(0, 2) * lambda16) >> 16); kSad: the sum shifted by bd - 8."""
    x, y, w, h = (int(b[k]) for k in ("x", "y", "w", "h"))
    if not shape_taken(w, h):
        return NONE
    pred = xo.mc_block(bd, 0, x, y, w, h, int(b["mvp_x"]), int(b["mvp_y"]), pw, ph, ref_y, BL)
    o = orig_y[BL + y:BL + y + h, BL + x:BL + x + w].astype(np.int64)
    sad = int(np.abs(o - pred.astype(np.int64)).sum()) >> (bd - 8)
    return (sad + ((1 * int(b["lambda16"])) >> 16)) & NONE


def l1_mvp_costs(xo, bd, pw, ph, orig_y, refs, lists, me):
    """xvcgpu_fp_bi_back_mvp_cost: [n, MAX_REFS] uint32, NONE beyond list 1's pictures."""
    n = len(me[0][0])
    out = np.full((n, MAX_REFS), NONE, np.uint32)
    for r, poc in enumerate(lists[1]):
        for i in range(n):
            out[i][r] = mvp_cost(xo, bd, pw, ph, orig_y, refs[poc][0], me[1][r][i])
    return out


def uni_fold(lists, me, res, l1_cost, side_bits=SIDE_BITS):
    """xvcgpu_fp_bi_back_uni_fold.  me[l][r]: the jobs; res[l][r]: the search results, None
    for a re-used list-1 picture; l1_cost: l1_mvp_costs' answer.  Returns (choice with the
    fold's fields, jobs [n, Rmax], slot bytes [n, Rmax, 2]); a job nobody writes stays zero."""
    num_ref, same, _, slot = tables(lists)
    rmax, n = max(num_ref), len(me[0][0])
    choice = np.zeros(n, CHOICE_DTYPE)
    jobs = np.zeros((n, rmax), ol.BI_DTYPE)
    slots = np.full((n, rmax, 2), NO_JOB, np.uint8)
    for i in range(n):
        c = choice[i]
        c["cost_uni"] = NONE
        best, best_cost, unique, unique_cost, bad = [-1, -1], [NONE, NONE], -1, NONE, False

        def searched(l, r):
            q, b = res[l][r][i], me[l][r][i]
            mv = (int(q["mv_x"]), int(q["mv_y"]))
            bits = side_bits[l] + ref_idx_bits(num_ref[l], r) + 1 + mvd_bits(b, mv)
            return int(q["subpel_dist"]) == NONE, _cost(int(q["subpel_dist"]), bits,
                                                        int(b["lambda16"]))
        for r in range(num_ref[0]):
            unsupported, cost = searched(0, r)
            bad = bad or unsupported
            c["cost_uni"][0][r] = cost
            if cost < best_cost[0]:
                best[0], best_cost[0] = r, cost
        for r in range(num_ref[1]):
            pc = int(l1_cost[i][r])
            bad = bad or pc == NONE
            c["cost_uni"][1][r] = pc
            if pc < best_cost[1]:                   # :508: strict <, the lower index stays
                best[1], best_cost[1] = r, pc
            if same[r] >= 0:                        # :521-523: a re-used picture is done
                continue
            unsupported, cost = searched(1, r)
            bad = bad or unsupported
            if cost < unique_cost:
                unique, unique_cost = r, cost
        if bad or min(best) < 0:
            choice[i:i + 1].view(np.uint8)[:] = 0xff
            continue
        other = me[1][best[1]][i]
        for k in range(num_ref[0]):
            j = jobs[i][k]
            j["blk"] = me[0][k][i]
            j["boot_mv_x"], j["boot_mv_y"] = res[0][k][i]["mv_x"], res[0][k][i]["mv_y"]
            j["other_mv_x"], j["other_mv_y"] = other["mvp_x"], other["mvp_y"]
            slots[i][k] = (slot[0][k], slot[1][best[1]])
        c["search_list"], c["cost_list"], c["cost_l1_unique"] = 0, best_cost, unique_cost
        c["best_ref"], c["best_ref_l1_unique"] = best, unique
    return choice, jobs, slots


def choice_fold(lists, me, res, bi_res, choice, side_bits=SIDE_BITS):
    """xvcgpu_fp_bi_back_choice: completes a copy of uni_fold's records from the refinement
    results bi_res [n, Rmax].  Returns (choice, the prediction jobs as (x, y, w, h, ref[2],
    mv[2][2]) per CU)."""
    num_ref, _, _, slot = tables(lists)
    choice = choice.copy()
    inter = []
    for i in range(len(choice)):
        c, b00 = choice[i], me[0][0][i]
        rect = tuple(int(b00[k]) for k in ("x", "y", "w", "h"))
        if int(c["search_list"]) != 0:
            inter.append(rect + ((-1, -1), ((0, 0), (0, 0))))
            continue
        best = [int(v) for v in c["best_ref"]]
        p1 = me[1][best[1]][i]
        mvp1 = (int(p1["mvp_x"]), int(p1["mvp_y"]))

        def uni_mv(l, r):
            return (int(res[l][r][i]["mv_x"]), int(res[l][r][i]["mv_y"]))
        # GetForceMvdZero: list 1 adds its index and predictor bits, no vector difference
        bits_1 = side_bits[2] + ref_idx_bits(num_ref[1], best[1]) + 1
        cost_bi, best_k, best_mv = NONE, -1, (0, 0)
        c["bi_cost"], c["bi_mv"] = NONE, 0
        for k in range(num_ref[0]):
            r, b = bi_res[i][k], me[0][k][i]
            mv = (int(r["mv_x"]), int(r["mv_y"]))
            cost = NONE
            if int(r["subpel_dist"]) != NONE:
                cost = _cost(int(r["subpel_dist"]),
                             bits_1 + ref_idx_bits(num_ref[0], k) + 1 + mvd_bits(b, mv),
                             int(b["lambda16"]))
            c["bi_cost"][k], c["bi_mv"][k] = cost, mv
            if cost < cost_bi:
                cost_bi, best_k, best_mv = cost, k, mv
        if best_k < 0:
            best_k, best_mv = best[0], uni_mv(0, best[0])
        c["cost_bi"] = cost_bi
        cost0, cost1u = int(c["cost_list"][0]), int(c["cost_l1_unique"])
        d = 2 if cost_bi <= cost0 and cost_bi <= cost1u else (0 if cost0 <= cost1u else 1)
        ref_idx, mv = [-1, -1], [(0, 0), (0, 0)]
        if d == 2:
            ref_idx[0], mv[0] = best_k, best_mv
            ref_idx[1], mv[1] = best[1], mvp1
            c["cost"] = cost_bi
        elif d == 0:
            ref_idx[0], mv[0] = best[0], uni_mv(0, best[0])
            c["cost"] = cost0
        else:
            u = int(c["best_ref_l1_unique"])
            ref_idx[1], mv[1] = u, uni_mv(1, u)
            c["cost"] = cost1u
        c["inter_dir"], c["ref_idx"], c["mv"] = d, ref_idx, mv
        inter.append(rect + (tuple(slot[l][ref_idx[l]] if ref_idx[l] >= 0 else -1
                                   for l in range(2)), tuple(mv)))
    return choice, inter


def search_motion(xo, bd, pw, ph, orig_y, refs, lists, me, side_bits=SIDE_BITS, key=None):
    """SearchMotion for every CU under force_l1_mvd_zero.  refs: {poc: planes}; me[l][r]: the
    jobs.  Returns (res[l][r] - None where re-used -, the refinement results [n, Rmax] with
    zeros where there is no job, the slot bytes, the choice records, the prediction jobs, the
    predictor costs)."""
    num_ref, same, distinct, _ = tables(lists)
    res = [[None] * num_ref[l] for l in range(2)]
    for l in range(2):
        for r in range(num_ref[l]):
            if l == 0 or same[r] < 0:
                poc = lists[l][r]
                res[l][r] = rm.uni_search(xo, None if key is None else (("back", key), poc), bd,
                                          pw, ph, orig_y, refs[poc][0], me[l][r])
    l1_cost = l1_mvp_costs(xo, bd, pw, ph, orig_y, refs, lists, me)
    choice, jobs, slots = uni_fold(lists, me, res, l1_cost, side_bits)
    bi = np.zeros(jobs.shape, ol.MERES_DTYPE)
    for i in range(jobs.shape[0]):
        for k in range(jobs.shape[1]):
            if slots[i][k][0] == NO_JOB:
                continue
            mv, dist = xo.bipred_search(bd, helpers.bi_struct(jobs[i][k]), pw, ph, orig_y,
                                        refs[distinct[slots[i][k][1]]][0],
                                        refs[distinct[slots[i][k][0]]][0], BL)
            bi[i][k]["mv_x"], bi[i][k]["mv_y"], bi[i][k]["subpel_dist"] = mv[0], mv[1], dist
    choice, inter = choice_fold(lists, me, res, bi, choice, side_bits)
    return res, bi, slots, choice, inter, l1_cost, jobs


def frame_pass(xo, desc, bd, orig, refs, lists, searched):
    """The whole pass over desc (descriptors()); searched: search_motion's answer for its
    jobs.  bi_refs_pass_model.frame_pass's answer (the prediction, the residual pipeline, the
    CU records and the B tail read the choice records only) with the predictor costs and the
    refinement jobs behind it, [10] and [11]."""
    out = rm.frame_pass(xo, desc, bd, orig, refs, lists, searched[:5])
    return out + (searched[5], searched[6])
