"""The expected P frame pass with merge mode (xvcgpu_frame_pass_merge,
pipeline.FramePass(merge_cands=...)), composed in numpy / ctypes from the oracle's pinned
pieces and nothing else: xo.tz_search + xo.subpel_search per CU
(bi_refs_pass_model.uni_search), xo.mc_metric with SATD per candidate, the ranking of
InterSearch::SearchMergeCandidates (inter_search.cc:165-197) in Python floats (IEEE doubles,
no fused multiply-add), the two prices of the choice in Python integers, xo.mc_block at the
clipped vector, the residual pipeline per transform block, the CU records with the unclipped
vector, xo.deblock, xo.pad_border, xo.picture_ssd - each step worded as include/xvcgpu.h
words its kernel.

Also the inputs the merge-pass tests share (INPUTS, scene, candidates): the reference is the
original displaced, with grain of a strength that changes over the width, and both are flat
in the rightmost 16 luma columns - there every vector predicts alike, also one so far outside
the picture that ClipMv changes it.

TEST INFRASTRUCTURE."""
import ctypes as C

import numpy as np

import bi_refs_pass_model as rm
import oracle_lib as ol

BL, BC = rm.BL, rm.BC
BORDERS = (BL, BC, BC)
LAMBDA16 = 498000
LAMBDA_SQRT = 498000 / 65536        # dyadic: sqrt(x * x) == x exactly
QP = 26                  # (at this QP blocks of every component keep levels and some CUs none)
SEARCH_RANGE = 64
SIDE_BITS, MERGE_SIDE_BITS = 1, 1
NONE = 0xffffffff
CANDS = 5
SATD = 1                            # XVC_METRIC_SATD
ME_USE_LIC = 2
SIDES = (4, 8, 16, 32, 64)
INPUTS = rm.INPUTS       # grid10, grid8 (104x72 on the 16-sample grid), part10 (partition_128)
REF_POC = 4              # bi_refs_pass_model's picture: displaced by SHIFT[4], grain GRAIN[4]
TRUE_MV = (16 * rm.SHIFT[REF_POC][1], 16 * rm.SHIFT[REF_POC][0])    # (x, y), 1/16 pel
FLAT = 16                # luma columns at the right edge that are one value
FAR = 5000               # 1/16 pel: past every picture's ClipMv bound
# the candidate generator's seed per input, chosen on the CPU until the model alone meets the
# conditions of tests/test_merge_pass_model.py
SEEDS = {"grid10": 11, "grid8": 12, "part10": 13}

assert LAMBDA_SQRT * LAMBDA_SQRT == (498000 * 498000) / 2.0 ** 32
assert np.sqrt(LAMBDA_SQRT * LAMBDA_SQRT) == LAMBDA_SQRT

_scenes = {}


def scene(name):
    """(pw, ph, bd, partition or None, orig, ref): [Y, U, V] padded planes."""
    if name not in _scenes:
        pw, ph, bd, part, orig, refs = rm.make_refs(name)
        orig = [p.copy() for p in orig]
        ref = [p.copy() for p in refs[REF_POC]]
        for c in range(3):
            cs = 1 if c else 0
            x0 = BORDERS[c] + ((pw - FLAT) >> cs)
            orig[c][:, x0:] = 1 << (bd - 1)
            ref[c][:, x0:] = 1 << (bd - 1)
        _scenes[name] = (pw, ph, bd, part, orig, ref)
    return _scenes[name]


def descriptors(name, rdoq=False, cu=16):
    """pipeline.FrameDescriptors of the input with the tests' lambda (and P contexts)."""
    from xvc_amd import pipeline
    pw, ph, bd, part = INPUTS[name]
    d = pipeline.FrameDescriptors(pw, ph, QP, cu=cu, search_range=SEARCH_RANGE, rdoq=rdoq,
                                  bitdepth=bd, partition=part() if part else None)
    d.me["lambda16"] = LAMBDA16
    return d


_searched = {}


def plain_search(xo, name, desc=None):
    """The plain search of every CU of the input, shared per input."""
    if name not in _searched:
        pw, ph, bd, _, orig, ref = scene(name)
        desc = desc or descriptors(name)
        _searched[name] = rm.uni_search(xo, None, bd, pw, ph, orig[0], ref[0], desc.me)
    return _searched[name]


def cand_array(n):
    from xvc_amd import api
    c = np.zeros((n, CANDS), api.FP_MERGE_CAND_DTYPE)
    c["ref_idx"] = (0, -1)
    return c


def candidates(name, desc, res, seed=None):
    """api.FP_MERGE_CAND_DTYPE [n_cus, 5] from a seeded generator: per slot one of the scene's
    true displacement, a vector close to it, zero, the searched vector of the CU to the
    left, a random vector within +-96 samples and, for some CUs, a vector far outside the
    picture; some CUs hold the same candidate at merge indices 3 and 4 (equal bits: only
    the stable sort separates them), some one candidate that is not valid (ref_idx {1, -1});
    some CUs hold the true displacement at index 4 only."""
    rng = np.random.default_rng(SEEDS[name] if seed is None else seed)
    n = desc.n_cus
    cands = cand_array(n)
    for i, b in enumerate(desc.me):
        x, y = int(b["x"]), int(b["y"])
        left = int(desc.cu_map[y // 4][x // 4 - 1]) - desc.cu_base if x else -1
        left_mv = (int(res[left]["mv_x"]), int(res[left]["mv_y"])) if 0 <= left < n else (0, 0)

        def draw():
            k = int(rng.integers(0, 12))
            if k < 2:
                return TRUE_MV
            if k < 5:
                return (TRUE_MV[0] + int(rng.integers(-3, 4)) * 4, TRUE_MV[1] + int(rng.integers(-3, 4)) * 4)
            if k < 6:
                return (0, 0)
            if k < 8:
                return left_mv
            if k < 11:
                return (int(rng.integers(-96 * 16, 96 * 16 + 1)), int(rng.integers(-96 * 16, 96 * 16 + 1)))
            return (int(rng.choice([-FAR, FAR])), int(rng.choice([-FAR, FAR])))
        kind = int(rng.integers(0, 8))
        mvs = [draw() for _ in range(CANDS)]
        if kind == 0:       # the true displacement at the last index only
            mvs = [(int(rng.integers(-96 * 16, 96 * 16 + 1)), int(rng.integers(-96 * 16, 96 * 16 + 1)))
                   for _ in range(4)] + [TRUE_MV]
        elif kind == 1:     # none that can win
            mvs = [(int(rng.integers(-96 * 16, 96 * 16 + 1)), int(rng.integers(-96 * 16, 96 * 16 + 1)))
                   for _ in range(CANDS)]
        elif kind == 2:     # two equal candidates where the index bits are equal
            mvs[4] = mvs[3]
        elif kind == 3:     # in the flat columns a far vector first
            mvs[0] = (FAR, int(rng.choice([-FAR, 0, FAR])))
        cands[i]["mv"][:, 0, :] = mvs
        if kind in (4, 5):
            cands[i]["ref_idx"][int(rng.integers(0, CANDS))] = (1, -1)
    return cands


def valid(c):
    return int(c["ref_idx"][0]) == 0 and int(c["ref_idx"][1]) == -1


def idx_bits(m):
    return m + 1 - (1 if m == CANDS - 1 else 0)


def rank_fold(dist, lambda_sqrt=LAMBDA_SQRT):
    """SearchMergeCandidates' arithmetic (:176-196) on five distortions: (cost sorted, order,
    num).  Python floats are IEEE doubles and a * b + c is two roundings."""
    cost = [float(int(dist[m])) + float(idx_bits(m)) * lambda_sqrt for m in range(CANDS)]
    order = list(range(CANDS))
    for a in range(1, CANDS):       # std::stable_sort: moves only on strictly smaller
        c, o, b = cost[a], order[a], a - 1
        while b >= 0 and c < cost[b]:
            cost[b + 1], order[b + 1] = cost[b], order[b]
            b -= 1
        cost[b + 1], order[b + 1] = c, o
    num = 4
    for k in range(4, -1, -1):
        if cost[k] > cost[0] * 1.25:
            num = k
    return cost, order, num


def rank(xo, name, desc, cands, listed=None, lambda_sqrt=LAMBDA_SQRT, out=None):
    """xvcgpu_fp_merge_rank: the listed CUs' records; the others as `out` has them."""
    from xvc_amd import api
    pw, ph, bd, _, orig, ref = scene(name)
    out = np.zeros(desc.n_cus, api.FP_MERGE_RANK_DTYPE) if out is None else out.copy()
    for i in (range(desc.n_cus) if listed is None else listed):
        b = desc.me[i]
        x, y, w, h = (int(b[k]) for k in ("x", "y", "w", "h"))
        dist = [NONE] * CANDS
        for m in range(CANDS):
            c = cands[i][m]
            if not valid(c) or w not in SIDES or h not in SIDES:
                continue
            mv = xo.clip_mv(x, y, pw, ph, int(c["mv"][0][0]), int(c["mv"][0][1]))
            dist[m] = xo.mc_metric(bd, SATD, 0, 0, x, y, w, h, mv, pw, ph, orig[0], ref[0], BL)
        cost, order, num = rank_fold(dist, lambda_sqrt)
        out[i] = (dist, order, num, 0, cost)
    return out


def _cost(dist, bits, lambda16):
    return (dist + ((bits * lambda16) >> 16)) & NONE


def choice_fold(me, res, cands, ranks, listed=None, side_bits=SIDE_BITS,
                merge_side_bits=MERGE_SIDE_BITS):
    """xvcgpu_fp_merge_choice.  Returns (the records with skip = 0, the chosen results)."""
    from xvc_amd import api
    n = len(me)
    choice = np.zeros(n, api.FP_MERGE_RESULT_DTYPE)
    chosen = res.copy()
    named = set(range(n) if listed is None else [int(v) for v in listed])
    for i in range(n):
        b, q, c = me[i], res[i], choice[i]
        if int(q["subpel_dist"]) == NONE:
            choice[i:i + 1].view(np.uint8)[:] = 0xff
            continue
        mv = (int(q["mv_x"]), int(q["mv_y"]))
        c["merge_idx"], c["cost_merge"] = -1, NONE
        c["cost_plain"] = _cost(int(q["subpel_dist"]), side_bits + 1 + rm.mvd_bits(b, mv),
                                int(b["lambda16"]))
        if i in named and not int(b["fullpel_mv"]) & ME_USE_LIC:
            r = ranks[i]
            m0 = int(r["order"][0])
            c["num"] = r["num"]
            d0 = int(r["dist"][m0])
            if d0 != NONE:
                c["cost_merge"] = _cost(d0, merge_side_bits + idx_bits(m0), int(b["lambda16"]))
                if int(c["cost_merge"]) <= int(c["cost_plain"]):    # (merge on a tie)
                    c["use_merge"], c["merge_idx"] = 1, m0
                    mv = (int(cands[i][m0]["mv"][0][0]), int(cands[i][m0]["mv"][0][1]))
                    chosen[i]["mv_x"], chosen[i]["mv_y"], chosen[i]["subpel_dist"] = mv[0], mv[1], d0
        c["mv"] = mv
        c["cost"] = c["cost_merge"] if int(c["use_merge"]) else c["cost_plain"]
    return choice, chosen


def skip_fold(desc, choice, nnz, from_me=False):
    """xvcgpu_fp_merge_skip on a copy of the records"""
    choice = choice.copy()
    for i in range(len(choice)):
        use = int(choice[i]["use_merge"])
        if use not in (0, 1):
            continue
        t = 3 * i if from_me else int(desc.luma_idx[i])
        choice[i]["skip"] = int(use == 1 and not nnz[t:t + 3].any())
    return choice


def cu_records(desc, chosen, nnz, ref_poc=0):
    """xvcgpu_cu_info_from_me over desc's own CUs: the chosen vector, unclipped"""
    cus = np.zeros(desc.n_cus_total, ol.CU_DTYPE)
    for i, b in enumerate(desc.me):
        c = cus[desc.cu_base + i]
        c["x"], c["y"], c["w"], c["h"] = b["x"], b["y"], b["w"], b["h"]
        c["cbf_luma"] = nnz[desc.luma_idx[i]] != 0
        c["qp_y"], c["qp_c"] = desc.qp, desc.qp_c
        c["ref_poc"] = (ref_poc, -1)
        c["mv"][0][:] = (chosen[i]["mv_x"], chosen[i]["mv_y"])
    return cus


_ranked = {}


def search(xo, name, listed=None, key=None):
    """The search, the ranking and the choice for every CU of the input: (res, cands, ranks,
    choice, chosen).  Shared per (input, key)."""
    k = (name, key)
    if k not in _ranked:
        desc = descriptors(name)
        res = plain_search(xo, name, desc)
        cands = candidates(name, desc, res)
        ranks = rank(xo, name, desc, cands, listed)
        choice, chosen = choice_fold(desc.me, res, cands, ranks, listed)
        _ranked[k] = (res, cands, ranks, choice, chosen)
    return _ranked[k]


def _inner(p, b, w, h):
    return p[b:b + h, b:b + w]


def _ptr(a):
    return a.ctypes.data_as(ol.u16p)


def prediction(xo, desc, bd, ref, chosen):
    """The pass's prediction picture: every CU at ClipMv of its chosen vector"""
    pw, ph = desc.w, desc.h
    pred = [np.zeros((ph >> (c > 0), pw >> (c > 0)), np.uint16) for c in range(3)]
    for i, b in enumerate(desc.me):
        x, y, w, h = (int(b[k]) for k in ("x", "y", "w", "h"))
        mv = xo.clip_mv(x, y, pw, ph, int(chosen[i]["mv_x"]), int(chosen[i]["mv_y"]))
        for c in range(3):
            cs = 1 if c else 0
            pred[c][y >> cs:(y + h) >> cs, x >> cs:(x + w) >> cs] = xo.mc_block(
                bd, c, x, y, w, h, mv[0], mv[1], pw, ph, ref[c], BORDERS[c])
    return pred


def frame_pass(xo, desc, bd, orig, ref, searched, ref_poc=0, from_me=False):
    """The whole pass over desc; searched: search()'s answer for its jobs.  Returns (padded
    rec planes, res, nnz, cus, (ssd, samples), choice with skip, chosen, the levels per
    transform block)."""
    pw, ph = desc.w, desc.h
    res, _, _, choice, chosen = searched
    pred = prediction(xo, desc, bd, ref, chosen)
    rec = [np.zeros_like(p) for p in orig]
    nnz = np.zeros(len(desc.tx), np.int32)
    levels, kept = np.zeros(64 * 64, np.int16), []
    rq = xo.dll.xo_residual_pipeline_rdoq
    rq.restype = C.c_int
    rq.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p] + [ol.u16p, ol.pd] * 3 + [ol.i16p]
    if desc.rdoq:
        ctxs = np.ascontiguousarray(desc.rdoq_contexts)
        prm = np.ascontiguousarray(desc.rdoq_params)
    tx = np.ascontiguousarray(desc.tx)
    for t in range(len(tx)):
        c = int(tx[t]["comp"])
        o = _inner(orig[c], BORDERS[c], pw >> (c > 0), ph >> (c > 0))
        r = _inner(rec[c], BORDERS[c], pw >> (c > 0), ph >> (c > 0))
        planes = (_ptr(o), o.strides[0] // 2, _ptr(pred[c]), pred[c].strides[0] // 2, _ptr(r),
                  r.strides[0] // 2, levels.ctypes.data_as(ol.i16p))
        if desc.rdoq:
            nnz[t] = rq(bd, tx[t:].ctypes.data, ctxs.ctypes.data, prm[t:].ctypes.data, *planes)
        else:
            nnz[t] = xo._residual_pipeline(bd, tx[t:].ctypes.data_as(C.POINTER(ol.TxBlock)),
                                           *planes)
        kept.append(levels[:int(tx[t]["w"]) * int(tx[t]["h"])].copy())
    cus = cu_records(desc, chosen, nnz, ref_poc)
    xo.deblock(bd, pw, ph, 0, 0, 0, 4, cus, desc.cu_map, rec, BORDERS)
    xo.pad_border(pw, ph, rec, BORDERS)
    ssd = xo.picture_ssd(bd, _inner(orig[0], BL, pw, ph), _inner(rec[0], BL, pw, ph))
    return (rec, res, nnz, cus, (int(ssd[0]), int(ssd[1])), skip_fold(desc, choice, nnz, from_me),
            chosen, kept)
