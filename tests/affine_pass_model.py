"""The expected P frame pass with affine motion (xvcgpu_frame_pass_affine,
pipeline.FramePass(affine=True)), composed in numpy / ctypes from the oracle's pinned pieces
and nothing else: xo.tz_search + xo.subpel_search per CU (bi_refs_pass_model.uni_search),
xo.clip_mv for the bootstrap, oracle_affine_me.affine_me for the capable CUs, the two prices
of InterSearch::CompressInter's comparison (inter_search.cc:74-99, :563, :1097-1101) in Python
integers, xo.mc_block / xo.mc_affine_block, the residual pipeline per transform block, the CU
records with corners, xo.deblock, xo.pad_border, xo.picture_ssd - each step worded as
include/xvcgpu.h words its kernel.

Also the inputs the affine-pass tests share (INPUTS, scene): the reference picture seen
through a similarity transform on a part of the picture and displaced on the rest, so that
both states win somewhere.

TEST INFRASTRUCTURE."""
import ctypes as C

import numpy as np

import bi_refs_pass_model as rm
import oracle_affine_me as oa
import oracle_lib as ol

BL, BC = rm.BL, rm.BC
BORDERS = (BL, BC, BC)
LAMBDA16 = rm.LAMBDA16
QP = 20                  # (the scene is smooth: at this QP blocks of every component keep levels)
SEARCH_RANGE = 64
SIDE_BITS = 1            # a picture with one list (inter_search.cc:1092)
NONE = 0xffffffff
SIDES = (16, 32, 64)
HAS_BOOTSTRAP, NO_JOB = 1, 4
INTER_AFFINE = 1
INPUTS = rm.INPUTS       # grid10, grid8 (104x72 on the 16-sample grid), part10 (partition_128)
# the similarity transform of the warped part: seed, zoom, rotation, shift (x, y)
SEED, ZOOM, ROT, SHIFT = 7, 1.04, 0.03, (1.5, -0.75)


def _warp_maps(name, pw, ph, border, cs):
    """(zoom, rotation) per sample of a padded plane.  The grids are warped whole (their
    two bit depths give 12 / 12 and 4 / 20 affine / plain winners); on the partition the
    columns from luma x = 96 in the upper half - a 32x32 and two 16x32 CUs - only move, so
    that the 32-high class has plain winners beside the 16-high one."""
    H, W = ph + 2 * border, pw + 2 * border
    zoom, rot = np.full((H, W), ZOOM), np.full((H, W), ROT)
    if name == "part10":
        yy, xx = np.mgrid[0:H, 0:W]
        still = (((xx - border) << cs) >= 96) & (((yy - border) << cs) < 64)
        zoom[still], rot[still] = 1.0, 0.0
    return zoom, rot


_scenes = {}


def scene(name):
    """(pw, ph, bd, partition or None, orig, ref): [Y, U, V] padded planes; every component
    is oracle_affine_me.warped_pics' texture, the original the reference through the
    transform (chroma at half the shift)."""
    if name not in _scenes:
        pw, ph, bd, part = INPUTS[name]
        rng = np.random.default_rng(SEED)
        orig, ref = [], []
        for c in range(3):
            cs = 1 if c else 0
            zoom, rot = _warp_maps(name, pw >> cs, ph >> cs, BORDERS[c], cs)
            o, r = oa.warped_pics(rng, bd, pw >> cs, ph >> cs, BORDERS[c], zoom, rot,
                                  (SHIFT[0] / (1 << cs), SHIFT[1] / (1 << cs)))
            orig.append(np.ascontiguousarray(o))
            ref.append(np.ascontiguousarray(r))
        _scenes[name] = (pw, ph, bd, part() if part else None, orig, ref)
    return _scenes[name]


def descriptors(name, rdoq=False, cu=16):
    """pipeline.FrameDescriptors of the input with the tests' lambda (and P contexts)."""
    from xvc_amd import pipeline
    pw, ph, bd, part = INPUTS[name]
    d = pipeline.FrameDescriptors(pw, ph, QP, cu=cu, search_range=SEARCH_RANGE, rdoq=rdoq,
                                  bitdepth=bd, partition=part() if part else None)
    d.me["lambda16"] = LAMBDA16
    return d


def capable(b):
    """CodingUnit::CanUseAffine on the sides the search has instances for, and a plain job
    without fullpel vectors and LIC"""
    return int(b["w"]) in SIDES and int(b["h"]) in SIDES and not int(b["fullpel_mv"]) & 3


def order_list(me):
    """(d_order, n_class): the capable CUs grouped by height 16, 32, 64, CU order inside"""
    groups = [[i for i, b in enumerate(me) if capable(b) and int(b["h"]) == h] for h in SIDES]
    return np.array(sum(groups, []), np.int32), [len(g) for g in groups]


def boot(xo, res, order, pw, ph, jobs):
    """xvcgpu_fp_affine_boot on a copy of the jobs"""
    jobs = jobs.copy()
    for i in order:
        q, j = res[i], jobs[i]
        if int(q["subpel_dist"]) == NONE:
            j["flags"], j["bootstrap"] = NO_JOB, 0
            continue
        mv = xo.clip_mv(int(j["x"]), int(j["y"]), pw, ph, int(q["mv_x"]), int(q["mv_y"]))
        j["flags"], j["bootstrap"] = HAS_BOOTSTRAP, [mv, mv, mv]
    return jobs


def affine_search(lib, bd, pw, ph, orig_y, ref_y, jobs, order, out=None):
    """xvcgpu_affine_me_listed: the listed jobs' records; the others as `out` has them"""
    out = np.zeros(len(jobs), oa.RESULT_DTYPE) if out is None else out.copy()
    for i in order:
        if int(jobs[i]["flags"]) & NO_JOB:
            continue
        out[i] = oa.affine_me(lib, bd, jobs[i], pw, ph, orig_y, ref_y, BL)
    return out


def _cost(dist, bits, lambda16):
    return (dist + ((bits * lambda16) >> 16)) & NONE


def corner_bits(mvp, mv):
    """The exp-Golomb bits of the quarter-sample difference of corners 0 and 1
    (SetMvd<MotionVector3> :1034-1048, GetInterPredBits :1097-1101)"""
    return sum(rm.eg_bits((int(mv[k][c]) - int(mvp[k][c])) >> 2) for k in (0, 1) for c in (0, 1))


def choice_fold(me, res, jobs, ares, side_bits=SIDE_BITS):
    """xvcgpu_fp_affine_choice.  Returns (the records, the prediction jobs [3 n])."""
    from xvc_amd import api
    n = len(me)
    choice = np.zeros(n, api.FP_AFFINE_RESULT_DTYPE)
    inter = np.zeros(3 * n, api.INTER_DTYPE)
    for i in range(n):
        b, q, c = me[i], res[i], choice[i]
        p = inter[3 * i:3 * i + 3]
        for k in ("x", "y", "w", "h"):
            p[k] = b[k]
        p["comp"] = (0, 1, 2)
        p["ref"] = -1
        if int(q["subpel_dist"]) == NONE:
            choice[i:i + 1].view(np.uint8)[:] = 0xff
            continue
        mv = (int(q["mv_x"]), int(q["mv_y"]))
        c["cost_plain"] = _cost(int(q["subpel_dist"]), side_bits + 1 + rm.mvd_bits(b, mv),
                                int(b["lambda16"]))
        c["cost_affine"] = NONE
        j = jobs[i]
        if capable(b) and int(j["flags"]) & HAS_BOOTSTRAP:
            r = ares[i]
            c["cost_affine"] = _cost(int(r["dist"]), side_bits + 1 + corner_bits(j["mvp"], r["mv"]),
                                     int(j["lambda16"]))
            c["dist_affine"], c["iterations"] = r["dist"], r["iterations"]
            if int(c["cost_affine"]) < int(c["cost_plain"]):    # (the plain state on a tie)
                c["use_affine"], c["mv"] = 1, r["mv"]
        if not int(c["use_affine"]):
            c["mv"] = [mv, mv, mv]
        c["cost"] = c["cost_affine"] if int(c["use_affine"]) else c["cost_plain"]
        p["ref"] = (0, -1)
        p["mv"][:, 0, 0] = c["mv"][0]
        if int(c["use_affine"]):
            p["flags"] = INTER_AFFINE
            p["mv"][:, 0, 1], p["mv"][:, 0, 2] = c["mv"][1], c["mv"][2]
    return choice, inter


def cu_records(desc, choice, nnz, ref_poc=0):
    """xvcgpu_cu_info_from_affine_choice over desc's own CUs"""
    cus = np.zeros(desc.n_cus_total, ol.CU_DTYPE)
    for i, b in enumerate(desc.me):
        c, ch = cus[desc.cu_base + i], choice[i]
        c["x"], c["y"], c["w"], c["h"] = b["x"], b["y"], b["w"], b["h"]
        c["cbf_luma"] = nnz[desc.luma_idx[i]] != 0
        c["qp_y"], c["qp_c"] = desc.qp, desc.qp_c
        c["ref_poc"] = (ref_poc, -1)
        if int(ch["use_affine"]) == 1:
            c["mv"][0][:3] = ch["mv"]
            c["mv"][0][3] = ch["mv"][1] + ch["mv"][2] - ch["mv"][0]
        else:
            c["mv"][0][:] = ch["mv"][0]
    return cus


_searched = {}


def search(xo, name, desc=None, key=None):
    """Both SearchMotion runs and the choice for every CU of the input: (res, the jobs
    after boot, the affine results, choice, the prediction jobs, order, n_class).  Shared
    per input (the descriptors of one input differ in nothing the searches read)."""
    key = key or name
    if key not in _searched:
        pw, ph, bd, _, orig, ref = scene(name)
        desc = desc or descriptors(name)
        res = rm.uni_search(xo, None, bd, pw, ph, orig[0], ref[0], desc.me)
        jobs0, order, n_class = desc.affine_jobs()
        o2, c2 = order_list(desc.me)
        assert (order == o2).all() and list(n_class) == c2
        jobs = boot(xo, res, order, pw, ph, jobs0)
        ares = affine_search(xo, bd, pw, ph, orig[0], ref[0], jobs, order)
        choice, inter = choice_fold(desc.me, res, jobs, ares)
        _searched[key] = (res, jobs, ares, choice, inter, order, n_class)
    return _searched[key]


def _inner(p, b, w, h):
    return p[b:b + h, b:b + w]


def _ptr(a):
    return a.ctypes.data_as(ol.u16p)


def prediction(xo, desc, bd, ref, inter):
    """xvcgpu_inter_pred_batch over the pass's jobs: the unpadded planes"""
    pw, ph = desc.w, desc.h
    pred = [np.zeros((ph >> (c > 0), pw >> (c > 0)), np.uint16) for c in range(3)]
    for p in inter:
        x, y, w, h, c = (int(p[k]) for k in ("x", "y", "w", "h", "comp"))
        cs = 1 if c else 0
        if int(p["ref"][0]) < 0:
            continue
        if int(p["flags"]) & INTER_AFFINE:
            blk = xo.mc_affine_block(bd, c, x, y, w, h, p["mv"][0], pw, ph, ref[c], BORDERS[c])
        else:
            blk = xo.mc_block(bd, c, x, y, w, h, int(p["mv"][0][0][0]), int(p["mv"][0][0][1]),
                              pw, ph, ref[c], BORDERS[c])
        pred[c][y >> cs:(y + h) >> cs, x >> cs:(x + w) >> cs] = blk
    return pred


def frame_pass(xo, desc, bd, orig, ref, searched, ref_poc=0):
    """The whole pass over desc; searched: search()'s answer for its jobs.  Returns (padded
    rec planes, res, nnz, cus, (ssd, samples), choice, the prediction planes, the levels per
    transform block)."""
    pw, ph = desc.w, desc.h
    res, _, _, choice, inter = searched[:5]
    pred = prediction(xo, desc, bd, ref, inter)
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
    cus = cu_records(desc, choice, nnz, ref_poc)
    xo.deblock(bd, pw, ph, 0, 0, 0, 4, cus, desc.cu_map, rec, BORDERS)
    xo.pad_border(pw, ph, rec, BORDERS)
    ssd = xo.picture_ssd(bd, _inner(orig[0], BL, pw, ph), _inner(rec[0], BL, pw, ph))
    return rec, res, nnz, cus, (int(ssd[0]), int(ssd[1])), choice, pred, kept
