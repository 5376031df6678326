"""The expected frame pass of a B picture (xvcgpu_frame_pass_bi, pipeline.BiFramePass),
composed in numpy / ctypes from the oracle's pinned pieces (tests/oracle_lib.py): per list
xo.tz_search + xo.subpel_search, xo.bipred_search, xo.mc_block / xo.mc_bipred_block, the
residual pipeline per transform block, xo.deblock(bipred=1), xo.pad_border and
xo.picture_ssd - and the two folds of InterSearch::SearchMotion (inter_search.cc:198-259)
as Python integer arithmetic.  Its SearchMotion half is pinned to the reference's own
member function by tests/test_bi_pass_model.py.

Also the inputs the B-pass tests share (make_input, PARTITION_128).

TEST INFRASTRUCTURE."""
import ctypes as C

import numpy as np

import helpers
import oracle_lib as ol

BL, BC = 128, 64          # luma / chroma borders of the padded planes
LAMBDA16, QP = 498000, 32
SIDE_BITS = (3, 3, 5)     # fast_inter_pred_bits: uni L0, uni L1, bi
REF_POCS = (0, 2)
SEARCH_RANGE = 128        # GetSearchRangeUniPred for both lists (test_bi_pass_model.py)

CHOICE_DTYPE = np.dtype([("inter_dir", "<i4"), ("search_list", "<i4"),
                         ("cost_uni", "<u4", (2,)), ("cost_bi", "<u4"), ("cost", "<u4"),
                         ("mv", "<i4", (2, 2)), ("bi_mv", "<i4", (2,))])


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


def _planes(rng, bd, pw, ph, border):
    """One component's padded (orig, ref0, ref1): two textured references, the original
    list 0 displaced on the left quarter, list 1 displaced on the right quarter, their mean
    between, plus noise."""
    _, ref0 = helpers.make_pics(rng, bd, pw, ph, border, (0, 0))
    _, ref1 = helpers.make_pics(rng, bd, pw, ph, border, (0, 0))
    a = np.roll(ref0, (2, -5), (0, 1)).astype(np.int32)
    b = np.roll(ref1, (-3, 6), (0, 1)).astype(np.int32)
    x = np.arange(a.shape[1])[None, :] - border
    orig = np.where(x < pw // 4, a, np.where(x >= 3 * pw // 4, b, (a + b + 1) // 2))
    orig = np.clip(orig + rng.integers(-2, 3, a.shape), 0, (1 << bd) - 1).astype(np.uint16)
    return [np.ascontiguousarray(p) for p in (orig, ref0, ref1)]


def make_input(name):
    """(pw, ph, bd, partition, orig, ref0, ref1): the pictures as [Y, U, V] padded planes."""
    pw, ph, bd, part = INPUTS[name]
    rng = np.random.default_rng(7700 + bd)
    comps = [_planes(rng, bd, pw >> (c > 0), ph >> (c > 0), BC if c else BL) for c in range(3)]
    orig, ref0, ref1 = ([comps[c][k] for c in range(3)] for k in range(3))
    return pw, ph, bd, (part() if part else None), orig, ref0, ref1


def descriptors(name, rdoq=False):
    """pipeline.FrameDescriptors of the input as BiFramePass builds them (the B picture's
    contexts for RDOQ), with the tests' lambda."""
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


def search_motion(xo, bd, pw, ph, orig_y, ref_y, me, side_bits=SIDE_BITS):
    """SearchMotion for every CU: me = (list 0's jobs, list 1's), ref_y = the lists' padded
    luma planes.  Returns (the lists' search results, the refinement results by searched
    list with zeros where the CU refined the other one, the choice records)."""
    n = len(me[0])
    res = [np.zeros(n, ol.MERES_DTYPE) for _ in range(2)]
    bi = [np.zeros(n, ol.MERES_DTYPE) for _ in range(2)]
    choice = np.zeros(n, CHOICE_DTYPE)
    for i in range(n):
        cost = []
        for l in range(2):
            b = me[l][i]
            assert not int(b["fullpel_mv"]), "the model searches sub-pel jobs only"
            s = helpers.me_struct(b)
            fp, fcost = xo.tz_search(bd, s, pw, ph, orig_y, ref_y[l], BL)
            mv, dist = xo.subpel_search(bd, s, pw, ph, orig_y, ref_y[l], BL, fp)
            res[l][i] = (fp[0], fp[1], mv[0], mv[1], fcost, dist)
            bits = side_bits[l] + 1 + mvd_bits(b, mv)
            cost.append(dist + ((bits * int(b["lambda16"])) >> 16))
        s = 1 if cost[0] <= cost[1] else 0          # the list that lost is refined
        job = np.zeros(1, ol.BI_DTYPE)[0]
        job["blk"] = me[s][i]
        job["other_mv_x"], job["other_mv_y"] = res[1 - s][i]["mv_x"], res[1 - s][i]["mv_y"]
        job["boot_mv_x"], job["boot_mv_y"] = res[s][i]["mv_x"], res[s][i]["mv_y"]
        bmv, bdist = xo.bipred_search(bd, helpers.bi_struct(job), pw, ph, orig_y, ref_y[1 - s],
                                      ref_y[s], BL)
        bi[s][i]["mv_x"], bi[s][i]["mv_y"], bi[s][i]["subpel_dist"] = bmv[0], bmv[1], bdist
        mv = [(int(res[l][i]["mv_x"]), int(res[l][i]["mv_y"])) for l in range(2)]
        pair = list(mv)
        pair[s] = (int(bmv[0]), int(bmv[1]))
        bits = side_bits[2] + 2 + mvd_bits(me[0][i], pair[0]) + mvd_bits(me[1][i], pair[1])
        cost_bi = bdist + ((bits * int(me[s][i]["lambda16"])) >> 16)
        d = 2 if cost_bi <= cost[0] and cost_bi <= cost[1] else (0 if cost[0] <= cost[1] else 1)
        c = choice[i]
        c["inter_dir"], c["search_list"] = d, s
        c["cost_uni"], c["cost_bi"] = cost, cost_bi
        c["cost"] = cost_bi if d == 2 else cost[d]
        c["bi_mv"] = pair[s]
        for l in range(2):
            c["mv"][l] = (pair[l] if d == 2 else mv[l]) if d in (2, l) else (0, 0)
    return res, bi, choice


def _inner(p, b, w, h):
    return p[b:b + h, b:b + w]


def _ptr(a):
    return a.ctypes.data_as(ol.u16p)


def frame_pass(xo, desc, bd, orig, ref0, ref1, searched=None, ref_pocs=REF_POCS):
    """The whole pass over desc (descriptors()); searched: search_motion's answer for its
    jobs where a caller has it already.  Returns (padded rec planes, (res0, res1), nnz, cus,
    (ssd, samples), choice)."""
    pw, ph = desc.w, desc.h
    if searched is None:
        searched = search_motion(xo, bd, pw, ph, orig[0], (ref0[0], ref1[0]),
                                 (desc.me, desc.me))
    res, _, choice = searched
    border = (BL, BC, BC)
    pred = [np.zeros((ph >> (c > 0), pw >> (c > 0)), np.uint16) for c in range(3)]
    for i, b in enumerate(desc.me):
        x, y, w, h = (int(b[k]) for k in ("x", "y", "w", "h"))
        d = int(choice[i]["inter_dir"])
        mv = [tuple(int(v) for v in choice[i]["mv"][l]) for l in range(2)]
        for c in range(3):
            cs = 1 if c else 0
            if d == 2:
                blk = xo.mc_bipred_block(bd, c, x, y, w, h, mv[0], mv[1], pw, ph, ref0[c],
                                         ref1[c], border[c])
            else:
                blk = xo.mc_block(bd, c, x, y, w, h, mv[d][0], mv[d][1], pw, ph,
                                  (ref0, ref1)[d][c], border[c])
            pred[c][y >> cs:(y + h) >> cs, x >> cs:(x + w) >> cs] = blk
    rec = [np.zeros_like(p) for p in orig]
    nnz = np.zeros(len(desc.tx), np.int32)
    levels = np.zeros(64 * 64, np.int16)
    rq = xo.dll.xo_residual_pipeline_rdoq
    rq.restype = C.c_int
    rq.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p] + \
        [ol.u16p, ol.pd] * 3 + [ol.i16p]
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
    cus = np.zeros(desc.n_cus_total, ol.CU_DTYPE)
    for i, b in enumerate(desc.me):
        c, d = cus[i], int(choice[i]["inter_dir"])
        c["x"], c["y"], c["w"], c["h"] = b["x"], b["y"], b["w"], b["h"]
        c["cbf_luma"] = nnz[desc.luma_idx[i]] != 0
        c["qp_y"], c["qp_c"] = desc.qp, desc.qp_c
        c["ref_idx0"] = 0 if d in (0, 2) else -1
        for l in range(2):
            c["ref_poc"][l] = ref_pocs[l] if d in (2, l) else -1
            c["mv"][l][:] = choice[i]["mv"][l]
    xo.deblock(bd, pw, ph, 1, 0, 0, 4, cus, desc.cu_map, rec, border)
    xo.pad_border(pw, ph, rec, border)
    ssd = xo.picture_ssd(bd, _inner(orig[0], BL, pw, ph), _inner(rec[0], BL, pw, ph))
    return rec, res, nnz, cus, (int(ssd[0]), int(ssd[1])), choice
