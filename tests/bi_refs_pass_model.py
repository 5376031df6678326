"""The expected frame pass of a B picture (xvcgpu_frame_pass_bi_refs,
pipeline.BiRefsFramePass), composed in numpy / ctypes from the oracle's pinned pieces
(tests/oracle_lib.py): per searched (list, picture) xo.tz_search + xo.subpel_search,
xo.bipred_search per refinement job, xo.mc_block / xo.mc_bipred_block from the chosen
pictures, the residual pipeline per transform block, xo.deblock(bipred=1), xo.pad_border,
xo.picture_ssd - and the two folds of InterSearch::SearchMotion (inter_search.cc:198-259;
uni_fold, choice_fold) in Python integers, worded as include/xvcgpu.h words them.  Its
SearchMotion half is pinned to the reference's own member function by
tests/test_bi_refs_pass_model.py.

Also the inputs (INPUTS, partition_128, descriptors) and the reference picture sets (SETS,
make_refs) the B-pass tests share.

TEST INFRASTRUCTURE."""
import ctypes as C

import numpy as np

import helpers
import oracle_lib as ol

BL, BC = 128, 64          # luma / chroma borders of the padded planes
LAMBDA16, QP = 498000, 32
SIDE_BITS = (3, 3, 5)     # fast_inter_pred_bits: uni L0, uni L1, bi
SEARCH_RANGE = 128        # the descriptors' range (jobs() gives each picture its own)
CUR_POC = 8
MAX_REFS = 3
NO_JOB = 255
NONE = 0xffffffff
# name -> (list 0's POCs, list 1's POCs)
SETS = {"A": ((4, 0), (12, 16)),        # four distinct pictures
        "B": ((4, 12), (12, 4)),        # both list-1 entries re-used: L1 is never chosen
        "C": ((4, 0, 16), (16, 12)),    # Rmax 3, a no-job slot in list 1, one entry re-used
        "D": ((4,), (12,))}             # one picture per list: Rmax 1, every slot a job
# luma displacement (rows, columns; even, so that chroma moves by half) per POC; 12 and 16
# cost the same vector bits
SHIFT = {0: (4, -6), 4: (2, -2), 12: (-2, 4), 16: (2, -4)}
# grain strength (8-bit units) per POC in each fifth of the width: one picture clean and the
# rest coarse (a uni-directional choice, each list and index somewhere), two equally fair
# ones (bi), and in the last fifth 12 and 16 with the SAME fine grain - equal costs up to
# the reference-index bits, which decide between a re-used and a unique list-1 picture
GRAIN = {0: (8, 5, 8, 8, 10), 4: (1, 10, 8, 8, 10), 12: (8, 10, 1, 8, 3), 16: (8, 5, 8, 1, 3)}

CHOICE_DTYPE = np.dtype([
    ("inter_dir", "<i4"), ("search_list", "<i4"), ("ref_idx", "<i4", (2,)),
    ("mv", "<i4", (2, 2)), ("cost_list", "<u4", (2,)), ("cost_l1_unique", "<u4"),
    ("cost_bi", "<u4"), ("cost", "<u4"), ("best_ref", "<i4", (2,)),
    ("best_ref_l1_unique", "<i4"), ("cost_uni", "<u4", (2, MAX_REFS)),
    ("bi_cost", "<u4", (MAX_REFS,)), ("bi_mv", "<i4", (MAX_REFS, 2))])


def partition_128():
    """The 128x128 partition of 111 CUs: every search and refinement class, a side of 4."""
    p = [(0, 0, 64, 64), (64, 0, 32, 32), (96, 0, 32, 32), (64, 32, 32, 16), (64, 48, 32, 16),
         (96, 32, 16, 32), (112, 32, 16, 32)]
    p += [(x, y, 16, 16) for y in (64, 80) for x in range(0, 128, 16)]
    p += [(x, y, 8, 8) for y in (96, 104) for x in range(0, 128, 8)]
    p += [(x, y, 8, 4) for y in (112, 116) for x in range(0, 64, 8)]
    p += [(x, 120, 8, 8) for x in range(0, 64, 8)]
    p += [(x, y, 4, 8) for y in (112, 120) for x in range(64, 128, 4)]
    assert len(p) == 111
    return np.array(p, np.int32)


# name -> (width, height, bit depth, partition or None for the 16-sample grid)
INPUTS = {"grid10": (104, 72, 10, None), "grid8": (104, 72, 8, None),
          "part10": (128, 128, 10, partition_128)}


def _original(rng, bd, pw, ph, border):
    """One component's padded original: between two textured pictures, the first displaced
    on the left quarter, the second displaced on the right quarter, their mean between,
    plus noise."""
    _, ref0 = helpers.make_pics(rng, bd, pw, ph, border, (0, 0))
    _, ref1 = helpers.make_pics(rng, bd, pw, ph, border, (0, 0))
    a = np.roll(ref0, (2, -5), (0, 1)).astype(np.int32)
    b = np.roll(ref1, (-3, 6), (0, 1)).astype(np.int32)
    x = np.arange(a.shape[1])[None, :] - border
    orig = np.where(x < pw // 4, a, np.where(x >= 3 * pw // 4, b, (a + b + 1) // 2))
    orig = np.clip(orig + rng.integers(-2, 3, a.shape), 0, (1 << bd) - 1).astype(np.uint16)
    return np.ascontiguousarray(orig)


def descriptors(name, rdoq=False):
    """pipeline.FrameDescriptors of the input as BiRefsFramePass builds them (the B
    picture's contexts for RDOQ), with the tests' lambda."""
    from xvc_amd import pipeline
    pw, ph, bd, part = INPUTS[name]
    d = pipeline.FrameDescriptors(pw, ph, QP, search_range=SEARCH_RANGE, rdoq=rdoq, bitdepth=bd,
                                  partition=part() if part else None)
    d.me["lambda16"] = LAMBDA16
    if rdoq:
        d.rdoq_contexts = pipeline.rdoq_init_contexts(QP, 0)
    return d


def eg_bits(v):
    """GetNumExpGolombBits (inter_search.cc:1179-1188)"""
    u = ((-v) << 1) + 1 if v <= 0 else v << 1
    n = 1
    while u != 1:
        u >>= 1
        n += 2
    return n


def mvd_bits(b, mv):
    sh = 2 + (2 if int(b["fullpel_mv"]) & 1 else 0)
    return eg_bits((mv[0] - int(b["mvp_x"])) >> sh) + eg_bits((mv[1] - int(b["mvp_y"])) >> sh)


def tables(lists):
    """(num_ref, same_poc_in_l0 per list-1 picture, the distinct POCs in order of first
    mention, slot[l][r] into them): ReferencePictureLists::GetSamePocMappingFor(L1)."""
    l0, l1 = list(lists[0]), list(lists[1])
    same = [l0.index(v) if v in l0 else -1 for v in l1]
    distinct = []
    for v in l0 + l1:
        if v not in distinct:
            distinct.append(v)
    return [len(l0), len(l1)], same, distinct, [[distinct.index(v) for v in l] for l in (l0, l1)]


def make_refs(name):
    """(pw, ph, bd, partition, orig, {poc: [Y, U, V] padded planes}): every reference is the
    input's original with grain of GRAIN's strength, displaced by SHIFT[poc], so that
    different pictures and all directions win in different CUs."""
    pw, ph, bd, part = INPUTS[name]
    rng = np.random.default_rng(7700 + bd)
    orig = [_original(rng, bd, pw >> (c > 0), ph >> (c > 0), BC if c else BL) for c in range(3)]
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


def ref_idx_bits(num_ref, r):
    """The reference-index bits of GetInterPredBits (inter_search.cc:1091-1094)"""
    return 0 if num_ref <= 1 else r + 1 - (1 if r == num_ref - 1 else 0)


def _cost(dist, bits, lambda16):
    return (dist + ((bits * lambda16) >> 16)) & NONE


def uni_fold(lists, me, res, side_bits=SIDE_BITS):
    """xvcgpu_fp_bi_refs_uni_fold.  me[l][r]: the jobs; res[l][r]: the search results, None
    for a re-used list-1 picture.  Returns (choice with the fold's fields, jobs [n, Rmax],
    slot bytes [n, Rmax, 2]); a job nobody writes stays zero."""
    num_ref, same, _, slot = tables(lists)
    rmax, n = max(num_ref), len(me[0][0])
    choice = np.zeros(n, CHOICE_DTYPE)
    jobs = np.zeros((n, rmax), ol.BI_DTYPE)
    slots = np.full((n, rmax, 2), NO_JOB, np.uint8)
    eff = [list(res[0]), [res[0][same[r]] if same[r] >= 0 else res[1][r]
                          for r in range(num_ref[1])]]
    for i in range(n):
        c = choice[i]
        c["cost_uni"] = NONE
        best, best_cost, unique, unique_cost, bad = [-1, -1], [NONE, NONE], -1, NONE, False
        for l in range(2):
            for r in range(num_ref[l]):
                q, b = eff[l][r][i], me[l][r][i]
                bad = bad or int(q["subpel_dist"]) == NONE
                mv = (int(q["mv_x"]), int(q["mv_y"]))
                bits = side_bits[l] + ref_idx_bits(num_ref[l], r) + 1 + mvd_bits(b, mv)
                cost = _cost(int(q["subpel_dist"]), bits, int(b["lambda16"]))
                c["cost_uni"][l][r] = cost
                if cost < best_cost[l]:
                    best[l], best_cost[l] = r, cost
                if l == 1 and same[r] < 0 and cost < unique_cost:
                    unique, unique_cost = r, cost
        if bad or min(best) < 0:
            choice[i:i + 1].view(np.uint8)[:] = 0xff
            continue
        s = 1 if best_cost[0] <= best_cost[1] else 0
        o = 1 - s
        for k in range(num_ref[s]):
            j = jobs[i][k]
            j["blk"] = me[s][k][i]
            j["boot_mv_x"], j["boot_mv_y"] = eff[s][k][i]["mv_x"], eff[s][k][i]["mv_y"]
            j["other_mv_x"] = eff[o][best[o]][i]["mv_x"]
            j["other_mv_y"] = eff[o][best[o]][i]["mv_y"]
            slots[i][k] = (slot[s][k], slot[o][best[o]])
        c["search_list"], c["cost_list"], c["cost_l1_unique"] = s, best_cost, unique_cost
        c["best_ref"], c["best_ref_l1_unique"] = best, unique
    return choice, jobs, slots


def choice_fold(lists, me, res, bi_res, choice, side_bits=SIDE_BITS):
    """xvcgpu_fp_bi_refs_choice: completes a copy of uni_fold's records from the refinement
    results bi_res [n, Rmax].  Returns (choice, the prediction jobs as (x, y, w, h, ref[2],
    mv[2][2]) per CU)."""
    num_ref, same, _, slot = tables(lists)
    n = len(choice)
    choice = choice.copy()
    eff = [list(res[0]), [res[0][same[r]] if same[r] >= 0 else res[1][r]
                          for r in range(num_ref[1])]]
    inter = []
    for i in range(n):
        c, b00 = choice[i], me[0][0][i]
        rect = tuple(int(b00[k]) for k in ("x", "y", "w", "h"))
        if int(c["search_list"]) not in (0, 1):
            inter.append(rect + ((-1, -1), ((0, 0), (0, 0))))
            continue
        s = int(c["search_list"])
        o = 1 - s
        best = [int(v) for v in c["best_ref"]]

        def uni_mv(l, r):
            return (int(eff[l][r][i]["mv_x"]), int(eff[l][r][i]["mv_y"]))
        bits_o = side_bits[2] + ref_idx_bits(num_ref[o], best[o]) + 1 + \
            mvd_bits(me[o][best[o]][i], uni_mv(o, best[o]))
        cost_bi, best_k, best_mv = NONE, -1, (0, 0)
        c["bi_cost"], c["bi_mv"] = NONE, 0
        for k in range(num_ref[s]):
            r, b = bi_res[i][k], me[s][k][i]
            mv = (int(r["mv_x"]), int(r["mv_y"]))
            cost = NONE
            if int(r["subpel_dist"]) != NONE:
                cost = _cost(int(r["subpel_dist"]),
                             bits_o + ref_idx_bits(num_ref[s], k) + 1 + mvd_bits(b, mv),
                             int(b["lambda16"]))
            c["bi_cost"][k], c["bi_mv"][k] = cost, mv
            if cost < cost_bi:
                cost_bi, best_k, best_mv = cost, k, mv
        if best_k < 0:
            best_k, best_mv = best[s], uni_mv(s, best[s])
        c["cost_bi"] = cost_bi
        cost0, cost1u = int(c["cost_list"][0]), int(c["cost_l1_unique"])
        d = 2 if cost_bi <= cost0 and cost_bi <= cost1u else (0 if cost0 <= cost1u else 1)
        ref_idx, mv = [-1, -1], [(0, 0), (0, 0)]
        if d == 2:
            ref_idx[s], mv[s] = best_k, best_mv
            ref_idx[o], mv[o] = best[o], uni_mv(o, best[o])
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


_uni_cache = {}


def uni_search(xo, key, bd, pw, ph, orig_y, ref_y, me):
    """One (list, picture)'s search of every CU; key: what the caller shares it under (the
    jobs of the tests' sets differ in nothing the search reads), None: not shared."""
    if key is not None and key in _uni_cache:
        return _uni_cache[key]
    res = np.zeros(len(me), ol.MERES_DTYPE)
    for i, b in enumerate(me):
        assert not int(b["fullpel_mv"]), "the model searches sub-pel jobs only"
        s = helpers.me_struct(b)
        fp, fcost = xo.tz_search(bd, s, pw, ph, orig_y, ref_y, BL)
        mv, dist = xo.subpel_search(bd, s, pw, ph, orig_y, ref_y, BL, fp)
        res[i] = (fp[0], fp[1], mv[0], mv[1], fcost, dist)
    if key is not None:
        _uni_cache[key] = res
    return res


def search_motion(xo, bd, pw, ph, orig_y, refs, lists, me, side_bits=SIDE_BITS, key=None):
    """SearchMotion for every CU.  refs: {poc: planes}; me[l][r]: the jobs.  Returns (res[l][r]
    - None where re-used -, the refinement results [n, Rmax] with zeros where there is no job,
    the slot bytes, the choice records, the prediction jobs)."""
    num_ref, same, distinct, slot = tables(lists)
    res = [[None] * num_ref[l] for l in range(2)]
    for l in range(2):
        for r in range(num_ref[l]):
            if l == 0 or same[r] < 0:
                poc = lists[l][r]
                res[l][r] = uni_search(xo, None if key is None else (key, poc), bd, pw, ph,
                                       orig_y, refs[poc][0], me[l][r])
    choice, jobs, slots = uni_fold(lists, me, res, side_bits)
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
    return res, bi, slots, choice, inter


def _inner(p, b, w, h):
    return p[b:b + h, b:b + w]


def _ptr(a):
    return a.ctypes.data_as(ol.u16p)


def frame_pass(xo, desc, bd, orig, refs, lists, searched):
    """The whole pass over desc (descriptors()); searched: search_motion's answer for its
    jobs.  Returns (padded rec planes, res, nnz, cus, (ssd, samples), choice, bi, slots,
    the prediction picture's planes, the levels per transform block)."""
    pw, ph = desc.w, desc.h
    _, _, distinct, _ = tables(lists)
    res, bi, slots, choice, inter = searched
    border = (BL, BC, BC)
    pred = [np.zeros((ph >> (c > 0), pw >> (c > 0)), np.uint16) for c in range(3)]
    for x, y, w, h, ref, mv in inter:
        pics = [refs[distinct[k]] if k >= 0 else None for k in ref]
        for c in range(3):
            cs = 1 if c else 0
            if ref[0] >= 0 and ref[1] >= 0:
                blk = xo.mc_bipred_block(bd, c, x, y, w, h, mv[0], mv[1], pw, ph, pics[0][c],
                                         pics[1][c], border[c])
            else:
                l = 0 if ref[0] >= 0 else 1
                blk = xo.mc_block(bd, c, x, y, w, h, mv[l][0], mv[l][1], pw, ph, pics[l][c],
                                  border[c])
            pred[c][y >> cs:(y + h) >> cs, x >> cs:(x + w) >> cs] = blk
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
        o = _inner(orig[c], border[c], pw >> (c > 0), ph >> (c > 0))
        r = _inner(rec[c], border[c], pw >> (c > 0), ph >> (c > 0))
        planes = (_ptr(o), o.strides[0] // 2, _ptr(pred[c]), pred[c].strides[0] // 2, _ptr(r),
                  r.strides[0] // 2, levels.ctypes.data_as(ol.i16p))
        if desc.rdoq:
            nnz[t] = rq(bd, tx[t:].ctypes.data, ctxs.ctypes.data, prm[t:].ctypes.data, *planes)
        else:
            nnz[t] = xo._residual_pipeline(bd, tx[t:].ctypes.data_as(C.POINTER(ol.TxBlock)),
                                           *planes)
        kept.append(levels[:int(tx[t]["w"]) * int(tx[t]["h"])].copy())
    cus = np.zeros(desc.n_cus_total, ol.CU_DTYPE)
    for i, b in enumerate(desc.me):
        c, ch = cus[i], choice[i]
        c["x"], c["y"], c["w"], c["h"] = b["x"], b["y"], b["w"], b["h"]
        c["cbf_luma"] = nnz[desc.luma_idx[i]] != 0
        c["qp_y"], c["qp_c"] = desc.qp, desc.qp_c
        c["ref_idx0"] = ch["ref_idx"][0]
        for l in range(2):
            r = int(ch["ref_idx"][l])
            c["ref_poc"][l] = lists[l][r] if r >= 0 else -1
            c["mv"][l][:] = ch["mv"][l]
    xo.deblock(bd, pw, ph, 1, 0, 0, 4, cus, desc.cu_map, rec, border)
    xo.pad_border(pw, ph, rec, border)
    ssd = xo.picture_ssd(bd, _inner(orig[0], BL, pw, ph), _inner(rec[0], BL, pw, ph))
    return rec, res, nnz, cus, (int(ssd[0]), int(ssd[1])), choice, bi, slots, pred, kept
