"""The expected B frame pass with merge mode (xvcgpu_frame_pass_bi_refs_merge,
pipeline.BiRefsFramePass(merge_cands=...)), composed in numpy / ctypes from pinned pieces and
nothing else: bi_refs_pass_model.search_motion for the plain run, xo.mc_block /
xo.mc_bipred_block + xo.metric_ss with SATD per candidate, merge_pass_model.rank_fold, the
prices of the choice in Python integers, and bi_refs_pass_model.frame_pass for the
prediction, the residual pipeline, the CU records and the tail - each step worded as
include/xvcgpu.h words its kernel.

Also the inputs the B merge-pass tests share (scene, candidates): bi_refs_pass_model's
pictures, one value in the rightmost 16 luma columns of the original and of every reference
(borders included) - there every vector predicts alike, also one so far outside the picture
that ClipMv changes it.

TEST INFRASTRUCTURE."""
import numpy as np

import bi_refs_pass_model as rm
import merge_pass_model as mm

BL, BC = rm.BL, rm.BC
BORDERS = (BL, BC, BC)
LAMBDA16, LAMBDA_SQRT = mm.LAMBDA16, mm.LAMBDA_SQRT
QP = 26                  # (blocks of every component keep levels and some CUs none)
SIDE_BITS, MERGE_SIDE_BITS = rm.SIDE_BITS, 1
NONE = rm.NONE
CANDS, SATD, SIDES, FAR, FLAT = mm.CANDS, mm.SATD, mm.SIDES, mm.FAR, mm.FLAT
INPUTS = rm.INPUTS
SETS = {k: rm.SETS[k] for k in "ACD"}
# the candidate generator's seed per (set, input), chosen on the CPU until the model alone
# meets the conditions of tests/test_bi_merge_pass_model.py
SEEDS = {("A", "grid10"): 9, ("A", "grid8"): 36, ("A", "part10"): 10,
         ("C", "grid10"): 7, ("C", "grid8"): 10, ("C", "part10"): 12,
         ("D", "grid10"): 10, ("D", "grid8"): 10, ("D", "part10"): 10}

_scenes = {}


def scene(name):
    """(pw, ph, bd, partition or None, orig, {poc: planes}): [Y, U, V] padded planes."""
    if name not in _scenes:
        pw, ph, bd, part, orig, refs = rm.make_refs(name)
        orig = [p.copy() for p in orig]
        refs = {poc: [p.copy() for p in planes] for poc, planes in refs.items()}
        for planes in [orig] + list(refs.values()):
            for c in range(3):
                x0 = BORDERS[c] + ((pw - FLAT) >> (1 if c else 0))
                planes[c][:, x0:] = 1 << (bd - 1)
        _scenes[name] = (pw, ph, bd, part, orig, refs)
    return _scenes[name]


def descriptors(name, rdoq=False):
    """pipeline.FrameDescriptors of the input as BiRefsFramePass builds them (a B picture's
    contexts for RDOQ), with the tests' lambda."""
    from xvc_amd import pipeline
    pw, ph, bd, part = INPUTS[name]
    d = pipeline.FrameDescriptors(pw, ph, QP, search_range=rm.SEARCH_RANGE, rdoq=rdoq,
                                  bitdepth=bd, partition=part() if part else None)
    d.me["lambda16"] = LAMBDA16
    if rdoq:
        d.rdoq_contexts = pipeline.rdoq_init_contexts(QP, 0)
    return d


_plain = {}


def plain_search(xo, name, which):
    """bi_refs_pass_model.search_motion over the scene: (res, bi, slots, choice, inter)."""
    if (name, which) not in _plain:
        pw, ph, bd, _, orig, refs = scene(name)
        lists = SETS[which]
        _plain[name, which] = rm.search_motion(xo, bd, pw, ph, orig[0], refs, lists,
                                               rm.jobs(descriptors(name), lists),
                                               key=("bi_merge", name))
    return _plain[name, which]


def true_mv(poc):
    """The scene's displacement into the picture of `poc`, (x, y) in 1/16 pel"""
    return (16 * rm.SHIFT[poc][1], 16 * rm.SHIFT[poc][0])


def candidates(name, which, desc, seed=None):
    """api.FP_MERGE_CAND_DTYPE [n_cus, 5] from a seeded generator.  Per CU a plan: nothing
    that can win; only one good candidate, of list 0, of list 1 or of both; a mix.  Good
    candidates carry the true displacement into a picture of each used list (any index of
    the list), some a vector close to it; a bi-directional one sometimes with one list's
    vector +-FAR outside the picture.  Some CUs hold the same candidate at indices 3 and 4,
    some the good one at index 4 only, some one that is not valid ({-1, -1} or an index >=
    num_ref)."""
    from xvc_amd import api
    lists = SETS[which]
    rng = np.random.default_rng(SEEDS[which, name] if seed is None else seed)
    n = desc.n_cus
    cands = np.zeros((n, CANDS), api.FP_MERGE_CAND_DTYPE)

    def wild():
        return (int(rng.integers(-96 * 16, 96 * 16 + 1)), int(rng.integers(-96 * 16, 96 * 16 + 1)))

    def good(l, near=False):
        r = int(rng.integers(0, len(lists[l])))
        mv = true_mv(lists[l][r])
        if near:
            mv = (mv[0] + int(rng.integers(-2, 3)) * 4, mv[1] + int(rng.integers(-2, 3)) * 4)
        return r, mv

    def cand(kind):
        """((ref_idx0, ref_idx1), (mv0, mv1))"""
        if kind == "bad":
            l = int(rng.integers(0, 3))
            r = [int(rng.integers(0, len(lists[0]))), int(rng.integers(0, len(lists[1])))]
            if l < 2:
                r[1 - l] = -1
            return tuple(r), tuple(wild() if r[k] >= 0 else (0, 0) for k in range(2))
        near = kind.endswith("~")
        r0, mv0 = good(0, near)
        r1, mv1 = good(1, near)
        if kind[:2] == "l0":
            return (r0, -1), (mv0, (0, 0))
        if kind[:2] == "l1":
            return (-1, r1), ((0, 0), mv1)
        if kind[:3] == "far":       # one list's vector outside the picture
            far = (int(rng.choice([-FAR, FAR])), int(rng.choice([-FAR, 0, FAR])))
            return (r0, r1), ((far, mv1) if rng.integers(0, 2) else (mv0, far))
        return (r0, r1), (mv0, mv1)

    for i in range(n):
        plan = ("bad", "l0", "l0", "l1", "l1", "l1", "bi", "bi", "far", "mix", "mix",
                "same")[int(rng.integers(0, 12))]
        cs = [cand("bad") for _ in range(CANDS)]
        if plan == "mix":
            cs = [cand(("bad", "l0", "l1", "bi", "l0~", "l1~", "bi~", "far")[int(rng.integers(0, 8))])
                  for _ in range(CANDS)]
        elif plan == "same":
            cs[3] = cs[4] = cand(("l0", "l1", "bi")[int(rng.integers(0, 3))])
        elif plan != "bad":
            at = 4 if rng.integers(0, 4) == 0 else int(rng.integers(0, CANDS))
            cs[at] = cand(plan)
            if plan == "far":
                cs[0] = cand("far")
        if rng.integers(0, 4) == 0:     # one that is not valid
            at = int(rng.integers(0, CANDS))
            bad = [(-1, -1), (len(lists[0]), -1), (0, len(lists[1])), (-2, 0)][int(rng.integers(0, 4))]
            cs[at] = (bad, cs[at][1])
        for m, (r, mv) in enumerate(cs):
            cands[i][m]["ref_idx"] = r
            cands[i][m]["mv"] = mv
    return cands


def valid(c, num_ref):
    r = [int(v) for v in c["ref_idx"]]
    return all(-1 <= r[l] < num_ref[l] for l in range(2)) and max(r) >= 0


def cand_dist_planes(xo, bd, pw, ph, orig_y, pics, b, c):
    """dist of one valid candidate: the luma prediction of MotionCompensation's branch (both
    oracle functions clip each vector as ClipMv does), SATD against the original.  orig_y:
    the padded luma plane; pics[l]: list l's padded luma plane (None: unused)."""
    x, y, w, h = (int(b[k]) for k in ("x", "y", "w", "h"))
    mv = [(int(c["mv"][l][0]), int(c["mv"][l][1])) for l in range(2)]
    if pics[0] is not None and pics[1] is not None:
        pred = xo.mc_bipred_block(bd, 0, x, y, w, h, mv[0], mv[1], pw, ph, pics[0], pics[1], BL)
    else:
        l = 0 if pics[0] is not None else 1
        pred = xo.mc_block(bd, 0, x, y, w, h, mv[l][0], mv[l][1], pw, ph, pics[l], BL)
    o = orig_y[BL + y:BL + y + h, BL + x:BL + x + w]
    return int(xo.metric_ss(SATD, bd, np.ascontiguousarray(o), pred))


def cand_dist(xo, name, lists, b, c):
    pw, ph, bd, _, orig, refs = scene(name)
    r = [int(v) for v in c["ref_idx"]]
    pics = [refs[lists[l][r[l]]][0] if r[l] >= 0 else None for l in range(2)]
    return cand_dist_planes(xo, bd, pw, ph, orig[0], pics, b, c)


def rank(xo, name, which, desc, cands, listed=None, lambda_sqrt=LAMBDA_SQRT, out=None):
    """xvcgpu_fp_bi_merge_rank: the listed CUs' records; the others as `out` has them."""
    from xvc_amd import api
    lists = SETS[which]
    num_ref = [len(lists[0]), len(lists[1])]
    out = np.zeros(desc.n_cus, api.FP_MERGE_RANK_DTYPE) if out is None else out.copy()
    for i in (range(desc.n_cus) if listed is None else listed):
        b = desc.me[i]
        shape = int(b["w"]) in SIDES and int(b["h"]) in SIDES
        dist = [cand_dist(xo, name, lists, b, c) if shape and valid(c, num_ref) else NONE
                for c in cands[i]]
        cost, order, num = mm.rank_fold(dist, lambda_sqrt)
        out[i] = (dist, order, num, 0, cost)
    return out


def choice_fold(lists, me, plain, inter, cands, ranks, listed=None,
                merge_side_bits=MERGE_SIDE_BITS):
    """xvcgpu_fp_bi_merge_choice.  me: d_me[0][0]; plain: the plain choice records; inter:
    the plain run's prediction jobs (rm.choice_fold's).  Returns (the records with skip = 0,
    the chosen records, the prediction jobs)."""
    from xvc_amd import api
    num_ref, _, _, slot = rm.tables(lists)
    n = len(me)
    choice = np.zeros(n, api.FP_BI_MERGE_RESULT_DTYPE)
    chosen, inter = plain.copy(), list(inter)
    named = set(range(n) if listed is None else [int(v) for v in listed])
    for i in range(n):
        b, q, c = me[i], chosen[i], choice[i]
        if int(plain[i]["search_list"]) not in (0, 1):
            choice[i:i + 1].view(np.uint8)[:] = 0xff
            continue
        c["merge_idx"], c["cost_merge"], c["cost_plain"] = -1, NONE, q["cost"]
        if i in named and not int(b["fullpel_mv"]) & mm.ME_USE_LIC:
            r = ranks[i]
            m0 = int(r["order"][0])
            c["num"] = r["num"]
            d0, cd = int(r["dist"][m0]), cands[i][m0]
            if d0 != NONE and valid(cd, num_ref):
                bits = merge_side_bits + mm.idx_bits(m0)
                c["cost_merge"] = (d0 + ((bits * int(b["lambda16"])) >> 16)) & NONE
                if int(c["cost_merge"]) <= int(c["cost_plain"]):    # (merge on a tie)
                    c["use_merge"], c["merge_idx"] = 1, m0
                    ref = [int(v) for v in cd["ref_idx"]]
                    mv = [tuple(int(v) for v in cd["mv"][l]) if ref[l] >= 0 else (0, 0)
                          for l in range(2)]
                    q["inter_dir"] = 2 if min(ref) >= 0 else (0 if ref[0] >= 0 else 1)
                    q["ref_idx"], q["mv"], q["cost"] = ref, mv, c["cost_merge"]
                    inter[i] = tuple(int(b[k]) for k in ("x", "y", "w", "h")) + (
                        tuple(slot[l][ref[l]] if ref[l] >= 0 else -1 for l in range(2)), tuple(mv))
        c["inter_dir"], c["ref_idx"], c["mv"] = q["inter_dir"], q["ref_idx"], q["mv"]
        c["cost"] = c["cost_merge"] if int(c["use_merge"]) else c["cost_plain"]
    return choice, chosen, inter


def skip_fold(desc, choice, nnz):
    return mm.skip_fold(desc, choice, nnz)


_searched = {}


def search(xo, name, which, listed=None, key=None):
    """The plain run, the ranking and the choice for every CU: (plain_search's answer, cands,
    ranks, choice, chosen, the prediction jobs).  Shared per (input, set, key)."""
    k = (name, which, key)
    if k not in _searched:
        desc = descriptors(name)
        plain = plain_search(xo, name, which)
        cands = candidates(name, which, desc)
        ranks = rank(xo, name, which, desc, cands, listed)
        choice, chosen, inter = choice_fold(SETS[which], desc.me, plain[3], plain[4], cands, ranks,
                                            listed)
        _searched[k] = (plain, cands, ranks, choice, chosen, inter)
    return _searched[k]


def frame_pass(xo, name, which, desc, searched):
    """The whole pass over desc; searched: search()'s answer.  Returns rm.frame_pass's tuple
    made from the chosen state (its choice records are the chosen ones) + (the merge records
    with skip, the plain choice records)."""
    pw, ph, bd, _, orig, refs = scene(name)
    plain, _, _, choice, chosen, inter = searched
    res, bi, slots, plain_choice, _ = plain
    e = rm.frame_pass(xo, desc, bd, orig, refs, SETS[which], (res, bi, slots, chosen, inter))
    return e + (skip_fold(desc, choice, e[2]), plain_choice)
