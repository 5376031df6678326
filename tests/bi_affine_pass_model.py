"""The expected B frame pass with affine motion (xvcgpu_frame_pass_bi_refs_affine,
pipeline.BiRefsFramePass(affine=True)), composed in numpy / ctypes from the oracle's pinned
pieces: bi_refs_pass_model.search_motion for the plain run, xo.clip_mv for the bootstrap,
oracle_affine_me.affine_me for every uni-directional and BIPRED affine job, the two folds of
the second SearchMotion run (inter_search.cc:484-572, :394-435, :247-257, :90) in Python
integers on bi_refs_pass_model's eg_bits, ref_idx_bits and _cost, xo_inter_pred_block for the
predictions, then the residual pipeline, the CU records with corners, xo.deblock(bipred=1),
xo.pad_border and xo.picture_ssd as bi_refs_pass_model.frame_pass composes them - each step
worded as include/xvcgpu.h words its kernel.

Also the scenes the tests share (scene): every reference POC sees the texture of
oracle_affine_me.warped_pics through its own similarity transform, zoom, rotation and shift
growing with the POC distance, under grain whose strength differs per picture and per fifth
of the width (GRAIN), so that lists, indices, directions and both motion models win
somewhere; a part of each input only moves, so that the plain state wins there.

TEST INFRASTRUCTURE."""
import ctypes as C

import numpy as np

import bi_refs_pass_model as rm
import oracle_affine_me as oa
import oracle_lib as ol

BL, BC = rm.BL, rm.BC
BORDERS = (BL, BC, BC)
QP = 20                   # (the texture is smooth: at this QP blocks of every component keep levels)
LAMBDA16 = 124678         # pipeline.lambda16_for_qp(QP): with zero predictors an affine state
                          # pays twice a plain one's vector bits, which at the B model's
                          # lambda (QP 32) outweigh what the corners gain on 16x16 CUs
SIDE_BITS = rm.SIDE_BITS
CUR_POC = rm.CUR_POC
MAX_REFS = rm.MAX_REFS
NONE = rm.NONE
NO_SLOT = rm.NO_JOB       # XVC_FP_BI_NO_JOB
SIDES = (16, 32, 64)
HAS_BOOTSTRAP, BIPRED, NO_JOB = 1, 2, 4
INTER_AFFINE = 1
SETS = rm.SETS
INPUTS = rm.INPUTS
tables = rm.tables
# per POC of distance: zoom - 1, rotation (radians), shift (x, y in luma samples)
SEED = 11
ZOOM_PER, ROT_PER, SHIFT_PER = 0.01, 0.01, (0.375, -0.1875)
# grain strength (8-bit units) per POC in each fifth of the width
GRAIN = {0: (6, 3, 6, 6, 6), 4: (1, 6, 6, 1, 1), 12: (6, 6, 1, 1, 1), 16: (6, 3, 6, 6, 6)}
# brightness offset (8-bit units) per POC and fifth: where the two nearest pictures carry
# opposite offsets only their mean fits, so that bi-directional states win there
OFFSET = {0: (0, 0, 0, 0, 0), 4: (0, 0, 0, 6, 6), 12: (0, 0, 0, -6, -6), 16: (0, 0, 0, 0, 0)}

INTER_DTYPE = np.dtype([("x", "<i2"), ("y", "<i2"), ("w", "u1"), ("h", "u1"), ("comp", "u1"),
                        ("flags", "u1"), ("ref", "i1", (2,)), ("neighbors", "u1"),
                        ("reserved", "u1"), ("above_x", "<i2"), ("above_y", "<i2"),
                        ("left_x", "<i2"), ("left_y", "<i2"), ("mv", "<i4", (2, 3, 2))])
RESULT_DTYPE = np.dtype([
    ("use_affine", "<i4"), ("inter_dir", "<i4"), ("ref_idx", "<i4", (2,)),
    ("mv", "<i4", (2, 3, 2)), ("cost", "<u4"), ("cost_plain", "<u4"), ("cost_affine", "<u4"),
    ("search_list", "<i4"), ("cost_list", "<u4", (2,)), ("cost_l1_unique", "<u4"),
    ("cost_bi", "<u4"), ("best_ref", "<i4", (2,)), ("best_ref_l1_unique", "<i4"),
    ("cost_uni", "<u4", (2, MAX_REFS)), ("bi_cost", "<u4", (MAX_REFS,))])
assert INTER_DTYPE.itemsize == 68 and RESULT_DTYPE.itemsize == 144


def _tex(x, y):
    """oracle_affine_me.warped_pics' texture"""
    return (np.sin(x / 6.0) * np.cos(y / 8.0) * 0.25 + np.sin((x + y) / 19.0) * 0.2 +
            np.cos((x - 2 * y) / 31.0) * 0.1 + 0.5)


def _still(name, xx, yy, border, cs):
    """The samples that only move (luma coordinates): the lowest CU row of the grids; on the
    partition the columns from x = 96 of the upper half (a 32x32 and two 16x32 CUs) and the
    second row of 16x16 CUs."""
    lx, ly = (xx - border) * (1 << cs), (yy - border) * (1 << cs)
    if name == "part10":
        return ((lx >= 96) & (ly < 64)) | (ly >= 80)
    return ly >= 48


_scenes = {}


def scene(name):
    """(pw, ph, bd, partition or None, orig, {poc: [Y, U, V]}): padded planes."""
    if name in _scenes:
        return _scenes[name]
    pw, ph, bd, part = INPUTS[name]
    rng = np.random.default_rng(SEED + bd)
    mx = (1 << bd) - 1
    orig, refs = [], {poc: [] for poc in sorted(GRAIN)}
    for c in range(3):
        cs = 1 if c else 0
        w, h, border = pw >> cs, ph >> cs, BORDERS[c]
        H, W = h + 2 * border, w + 2 * border
        yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
        orig.append(np.ascontiguousarray(np.clip(
            _tex(xx, yy) * mx + rng.integers(-2, 3, (H, W)), 0, mx).astype(np.uint16)))
        still = _still(name, xx, yy, border, cs)
        band = np.clip((np.arange(W)[None, :] - border) * 5 // w, 0, 4)
        cx, cy = W / 2.0, H / 2.0
        for poc in sorted(GRAIN):
            d = poc - CUR_POC
            zoom = np.where(still, 1.0, 1.0 + ZOOM_PER * d)
            rot = np.where(still, 0.0, ROT_PER * abs(d))    # (two lists' turns do not cancel)
            a, b = zoom * np.cos(rot), zoom * np.sin(rot)
            sx, sy = SHIFT_PER[0] * d / (1 << cs), SHIFT_PER[1] * d / (1 << cs)
            xs = a * (xx - cx) - b * (yy - cy) + cx + sx
            ys = b * (xx - cx) + a * (yy - cy) + cy + sy
            amp = np.array(GRAIN[poc])[band] << (bd - 8)
            grain = (rng.integers(-64, 65, (H, W)) * amp) >> 6
            grain = grain + np.array(OFFSET[poc])[band] * (1 << (bd - 8))
            refs[poc].append(np.ascontiguousarray(
                np.clip(_tex(xs, ys) * mx + grain, 0, mx).astype(np.uint16)))
    _scenes[name] = (pw, ph, bd, part() if part else None, orig, refs)
    return _scenes[name]


def descriptors(name, rdoq=False, cu=16):
    """pipeline.FrameDescriptors of the input as BiRefsFramePass builds them (the B picture's
    contexts for RDOQ), with the tests' lambda and QP."""
    from xvc_amd import pipeline
    pw, ph, bd, part = INPUTS[name]
    d = pipeline.FrameDescriptors(pw, ph, QP, cu=cu, search_range=rm.SEARCH_RANGE, rdoq=rdoq,
                                  bitdepth=bd, partition=part() if part else None)
    d.me["lambda16"] = LAMBDA16
    if rdoq:
        d.rdoq_contexts = pipeline.rdoq_init_contexts(QP, 0)
    return d


def capable(b):
    return int(b["w"]) in SIDES and int(b["h"]) in SIDES and not int(b["fullpel_mv"]) & 3


def order_list(me):
    """(d_order, n_class): the capable CUs grouped by height 16, 32, 64, CU order inside"""
    groups = [[i for i, b in enumerate(me) if capable(b) and int(b["h"]) == h] for h in SIDES]
    return np.array(sum(groups, []), np.int32), [len(g) for g in groups]


def uni_jobs(lists, me, mvp=None):
    """The caller's half of xvcgpu_frame_pass_bi_affine_args: (jobs [n, E], slot bytes
    [n, E, 2]); job [i, l * Rmax + r]."""
    num_ref, same, _, slot = tables(lists)
    rmax, n = max(num_ref), len(me[0][0])
    jobs = np.zeros((n, 2 * rmax), oa.BLOCK_DTYPE)
    slots = np.full((n, 2 * rmax, 2), NO_SLOT, np.uint8)
    for l in range(2):
        for r in range(num_ref[l]):
            for i, b in enumerate(me[l][r]):
                j = jobs[i][l * rmax + r]
                j["x"], j["y"], j["w"], j["h"] = b["x"], b["y"], b["w"], b["h"]
                j["lambda16"] = b["lambda16"]
                j["mvp"] = [(b["mvp_x"], b["mvp_y"])] * 3 if mvp is None else mvp[l][r][i]
            if l == 0 or same[r] < 0:
                slots[:, l * rmax + r, 0] = slot[l][r]
    return jobs, slots


def boot(xo, lists, res, jobs, slots, order, pw, ph):
    """xvcgpu_fp_bi_affine_boot on a copy of the jobs"""
    num_ref, _, _, _ = tables(lists)
    rmax = max(num_ref)
    jobs = jobs.copy()
    for i in order:
        for e in range(2 * rmax):
            if slots[i][e][0] == NO_SLOT:
                continue
            q, j = res[e // rmax][e % rmax][i], jobs[i][e]
            if int(q["subpel_dist"]) == NONE:
                j["flags"], j["bootstrap"] = NO_JOB, 0
                continue
            mv = xo.clip_mv(int(j["x"]), int(j["y"]), pw, ph, int(q["mv_x"]), int(q["mv_y"]))
            j["flags"], j["bootstrap"] = HAS_BOOTSTRAP, [mv, mv, mv]
    return jobs


def listed_search(lib, bd, pw, ph, orig_y, refs, distinct, jobs, slots, order, out=None):
    """xvcgpu_affine_me_listed_refs over jobs [n, per_cu]: the listed CUs' jobs that name a
    picture; the other records as `out` has them (zero without)"""
    out = np.zeros(jobs.shape, oa.RESULT_DTYPE) if out is None else out.copy()
    for i in order:
        for e in range(jobs.shape[1]):
            s0, s1 = (int(v) for v in slots[i][e])
            if s0 >= len(distinct) or int(jobs[i][e]["flags"]) & NO_JOB:
                continue
            other = refs[distinct[s1]][0] if int(jobs[i][e]["flags"]) & BIPRED else None
            out[i][e] = oa.affine_me(lib, bd, jobs[i][e], pw, ph, orig_y, refs[distinct[s0]][0],
                                     BL, other)
    return out


def corner_bits(mvp, mv):
    """The exp-Golomb bits of the quarter-sample difference of corners 0 and 1
    (SetMvd<MotionVector3>, GetInterPredBits :1097-1101)"""
    return sum(rm.eg_bits((int(mv[k][c]) - int(mvp[k][c])) >> 2) for k in (0, 1) for c in (0, 1))


def price(dist, bits, lambda16):
    return rm._cost(int(dist), int(bits), int(lambda16))


def searched(me00, jobs, slots, i):
    """A CU the affine run searched: capable, and each of its jobs that names a picture
    carries the boot kernel's flag"""
    return capable(me00[i]) and all(int(jobs[i][e]["flags"]) & HAS_BOOTSTRAP
                                    for e in range(jobs.shape[1]) if slots[i][e][0] != NO_SLOT)


def _src(same, rmax, l, r):
    return same[r] if l == 1 and same[r] >= 0 else l * rmax + r


def uni_fold(lists, me00, jobs, slots, ures, side_bits=SIDE_BITS):
    """xvcgpu_fp_bi_affine_uni_fold.  Returns (records with the fold's fields - zero for a CU
    that was not searched -, the refinement jobs [n, Rmax], their slot bytes)."""
    num_ref, same, _, _ = tables(lists)
    rmax, n = max(num_ref), len(me00)
    choice = np.zeros(n, RESULT_DTYPE)
    bjobs = np.zeros((n, rmax), oa.BLOCK_DTYPE)
    bslots = np.full((n, rmax, 2), NO_SLOT, np.uint8)
    for i in range(n):
        if not searched(me00, jobs, slots, i):
            continue
        c = choice[i]
        c["cost_uni"] = NONE
        best, best_cost, unique, unique_cost = [-1, -1], [NONE, NONE], -1, NONE
        for l in range(2):
            for r in range(num_ref[l]):
                j, q = jobs[i][l * rmax + r], ures[i][_src(same, rmax, l, r)]
                bits = side_bits[l] + rm.ref_idx_bits(num_ref[l], r) + 1 + \
                    corner_bits(j["mvp"], q["mv"])
                cost = price(q["dist"], bits, j["lambda16"])
                c["cost_uni"][l][r] = cost
                if cost < best_cost[l]:
                    best[l], best_cost[l] = r, cost
                if l == 1 and same[r] < 0 and cost < unique_cost:
                    unique, unique_cost = r, cost
        s = 1 if best_cost[0] <= best_cost[1] else 0
        o = 1 - s
        oe = _src(same, rmax, o, best[o])
        for k in range(num_ref[s]):
            se = _src(same, rmax, s, k)
            bjobs[i][k] = jobs[i][s * rmax + k]
            j = bjobs[i][k]
            j["bootstrap"], j["other_mv"] = ures[i][se]["mv"], ures[i][oe]["mv"]
            j["flags"], j["reserved"] = HAS_BOOTSTRAP | BIPRED, 0
            bslots[i][k] = (slots[i][se][0], slots[i][oe][0])
        c["search_list"], c["cost_list"], c["cost_l1_unique"] = s, best_cost, unique_cost
        c["best_ref"], c["best_ref_l1_unique"] = best, unique
    return choice, bjobs, bslots


def plain_inter(inter):
    """bi_refs_pass_model's prediction jobs as xvcgpu_inter_block [3 n]"""
    out = np.zeros(3 * len(inter), INTER_DTYPE)
    for i, (x, y, w, h, ref, mv) in enumerate(inter):
        p = out[3 * i:3 * i + 3]
        p["x"], p["y"], p["w"], p["h"], p["comp"] = x, y, w, h, (0, 1, 2)
        p["ref"] = ref
        for l in range(2):
            p["mv"][:, l, 0] = mv[l]
    return out


def choice_fold(lists, me00, jobs, slots, ures, bres, fold, plain, inter,
                side_bits=SIDE_BITS):
    """xvcgpu_fp_bi_affine_choice.  fold: uni_fold's records; plain: the plain run's choice
    records; inter: its prediction jobs [3 n] (plain_inter).  Returns (records, jobs)."""
    num_ref, same, _, _ = tables(lists)
    rmax, n = max(num_ref), len(me00)
    out = np.zeros(n, RESULT_DTYPE)
    inter = inter.copy()
    for i in range(n):
        c, pl = out[i], plain[i]
        if int(pl["inter_dir"]) not in (0, 1, 2):
            out[i:i + 1].view(np.uint8)[:] = 0xff
            continue
        c["cost_plain"] = pl["cost"]
        c["cost_affine"] = c["cost_l1_unique"] = c["cost_bi"] = NONE
        c["cost_list"], c["cost_uni"], c["bi_cost"] = NONE, NONE, NONE
        c["search_list"], c["best_ref"], c["best_ref_l1_unique"] = -1, -1, -1
        if searched(me00, jobs, slots, i):
            f = fold[i]
            for k in ("search_list", "cost_list", "cost_l1_unique", "best_ref",
                      "best_ref_l1_unique", "cost_uni"):
                c[k] = f[k]
            s = int(f["search_list"])
            o = 1 - s
            best = [int(v) for v in f["best_ref"]]
            oe = _src(same, rmax, o, best[o])
            bits_o = side_bits[2] + rm.ref_idx_bits(num_ref[o], best[o]) + 1 + \
                corner_bits(jobs[i][o * rmax + best[o]]["mvp"], ures[i][oe]["mv"])
            cost_bi, best_k = NONE, -1
            for k in range(num_ref[s]):
                r, j = bres[i][k], jobs[i][s * rmax + k]
                cost = price(r["dist"], bits_o + rm.ref_idx_bits(num_ref[s], k) + 1 +
                             corner_bits(j["mvp"], r["mv"]), j["lambda16"])
                c["bi_cost"][k] = cost
                if cost < cost_bi:
                    cost_bi, best_k = cost, k
            c["cost_bi"] = cost_bi
            cost0, cost1u = int(c["cost_list"][0]), int(c["cost_l1_unique"])
            d = 2 if cost_bi <= cost0 and cost_bi <= cost1u else (0 if cost0 <= cost1u else 1)
            c["cost_affine"] = (cost0, cost1u, cost_bi)[d]
            if int(c["cost_affine"]) < int(c["cost_plain"]):     # (:90: plain on a tie)
                state = {}      # list -> (ref_idx, job of the CU's E behind its slot, vectors)
                if d == 2:
                    ks = best[s] if best_k < 0 else best_k
                    se = _src(same, rmax, s, ks)
                    state[s] = (ks, se, ures[i][se]["mv"] if best_k < 0 else bres[i][ks]["mv"])
                    state[o] = (best[o], oe, ures[i][oe]["mv"])
                else:
                    r = best[0] if d == 0 else int(f["best_ref_l1_unique"])
                    e = _src(same, rmax, d, r)
                    state[d] = (r, e, ures[i][e]["mv"])
                c["use_affine"], c["inter_dir"], c["cost"] = 1, d, c["cost_affine"]
                c["ref_idx"] = -1
                p = inter[3 * i:3 * i + 3]
                p["flags"], p["ref"], p["mv"] = INTER_AFFINE, -1, 0
                for l, (r, e, mv) in state.items():
                    c["ref_idx"][l], c["mv"][l] = r, mv
                    p["ref"][:, l] = slots[i][e][0]
                    p["mv"][:, l] = mv
        if not int(c["use_affine"]):
            c["inter_dir"], c["ref_idx"], c["cost"] = pl["inter_dir"], pl["ref_idx"], pl["cost"]
            for l in range(2):
                c["mv"][l][:] = pl["mv"][l]
    return out, inter


def cu_records(desc, lists, choice, nnz):
    """xvcgpu_cu_info_from_bi_affine_choice over desc's own CUs"""
    cus = np.zeros(desc.n_cus_total, ol.CU_DTYPE)
    for i, b in enumerate(desc.me):
        c, ch = cus[i], choice[i]
        c["x"], c["y"], c["w"], c["h"] = b["x"], b["y"], b["w"], b["h"]
        c["cbf_luma"] = nnz[desc.luma_idx[i]] != 0
        c["qp_y"], c["qp_c"] = desc.qp, desc.qp_c
        d = int(ch["inter_dir"])
        used = (d in (0, 2), d in (1, 2))
        c["ref_idx0"] = ch["ref_idx"][0] if used[0] else -1
        for l in range(2):
            c["ref_poc"][l] = lists[l][int(ch["ref_idx"][l])] if used[l] else -1
            if not used[l]:
                continue
            if int(ch["use_affine"]) == 1:
                c["mv"][l][:3] = ch["mv"][l]
                c["mv"][l][3] = ch["mv"][l][1] + ch["mv"][l][2] - ch["mv"][l][0]
            else:
                c["mv"][l][:] = ch["mv"][l][0]
    return cus


_searched = {}


def search(xo, name, set_name, desc=None, key=None):
    """Both SearchMotion runs of every CU of the input.  Returns a dict: me, plain = (res, bi,
    slots, choice, inter tuples) of bi_refs_pass_model.search_motion, jobs (after boot),
    slots, order, n_class, ures, fold, bjobs, bslots, bres, choice, inter [3 n].  Shared per
    (input, set): the descriptors of one input differ in nothing the searches read."""
    key = key or (name, set_name)
    if key in _searched:
        return _searched[key]
    pw, ph, bd, _, orig, refs = scene(name)
    lists = SETS[set_name]
    desc = desc or descriptors(name)
    me = rm.jobs(desc, lists)
    _, _, distinct, _ = tables(lists)
    plain = rm.search_motion(xo, bd, pw, ph, orig[0], refs, lists, me, key=("bi_affine", key))
    order, n_class = order_list(me[0][0])
    jobs0, slots = uni_jobs(lists, me)
    jobs = boot(xo, lists, plain[0], jobs0, slots, order, pw, ph)
    ures = listed_search(xo, bd, pw, ph, orig[0], refs, distinct, jobs, slots, order)
    fold, bjobs, bslots = uni_fold(lists, me[0][0], jobs, slots, ures)
    bres = listed_search(xo, bd, pw, ph, orig[0], refs, distinct, bjobs, bslots, order)
    choice, inter = choice_fold(lists, me[0][0], jobs, slots, ures, bres, fold, plain[3],
                                plain_inter(plain[4]))
    _searched[key] = dict(me=me, plain=plain, jobs=jobs, slots=slots, order=order,
                          n_class=n_class, ures=ures, fold=fold, bjobs=bjobs, bslots=bslots,
                          bres=bres, choice=choice, inter=inter)
    return _searched[key]


def _inner(p, b, w, h):
    return p[b:b + h, b:b + w]


def _ptr(a):
    return a.ctypes.data_as(ol.u16p)


def prediction(xo, desc, bd, refs, distinct, inter):
    """xvcgpu_inter_pred_batch over the pass's jobs through xo_inter_pred_block: the
    unpadded planes"""
    pw, ph = desc.w, desc.h
    f = xo.dll.xo_inter_pred_block
    f.restype = None
    f.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                  C.c_void_p]
    planes = [refs[poc][c] for poc in distinct for c in range(3)]
    pred = [np.zeros_like(refs[distinct[0]][c]) for c in range(3)]
    strides = (C.c_ssize_t * 3)(*[p.strides[0] // 2 for p in pred])

    def origin(p, c):
        return p.ctypes.data + 2 * (BORDERS[c] * (p.strides[0] // 2) + BORDERS[c])
    ref_ptrs = (C.c_void_p * len(planes))(*[origin(p, k % 3) for k, p in enumerate(planes)])
    pred_ptrs = (C.c_void_p * 3)(*[origin(p, c) for c, p in enumerate(pred)])
    jobs = np.ascontiguousarray(inter)
    for k in range(len(jobs)):
        if int(jobs[k]["ref"][0]) < 0 and int(jobs[k]["ref"][1]) < 0:
            continue
        f(bd, jobs[k:].ctypes.data, pw, ph, ref_ptrs, pred_ptrs, pred_ptrs, strides)
    return [np.ascontiguousarray(_inner(pred[c], BORDERS[c], pw >> (c > 0), ph >> (c > 0)))
            for c in range(3)]


def frame_pass(xo, desc, bd, orig, refs, lists, found):
    """The whole pass over desc; found: search()'s answer for its jobs.  Returns (padded rec
    planes, nnz, cus, (ssd, samples), the prediction planes, the levels per transform
    block)."""
    pw, ph = desc.w, desc.h
    _, _, distinct, _ = tables(lists)
    pred = prediction(xo, desc, bd, refs, distinct, found["inter"])
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
    cus = cu_records(desc, lists, found["choice"], nnz)
    xo.deblock(bd, pw, ph, 1, 0, 0, 4, cus, desc.cu_map, rec, BORDERS)
    xo.pad_border(pw, ph, rec, BORDERS)
    ssd = xo.picture_ssd(bd, _inner(orig[0], BL, pw, ph), _inner(rec[0], BL, pw, ph))
    return rec, nnz, cus, (int(ssd[0]), int(ssd[1])), pred, kept


def census(found, lists):
    """Who won among the capable CUs: a dict of counts and CU lists for the scene conditions"""
    _, same, _, _ = tables(lists)
    me00, ch = found["me"][0][0], found["choice"]
    cap = [i for i in range(len(me00)) if capable(me00[i])]
    aff = [i for i in cap if int(ch[i]["use_affine"]) == 1]
    return dict(
        capable=len(cap), affine=len(aff), plain=len(cap) - len(aff),
        affine_dir=[sum(int(ch[i]["inter_dir"]) == d for i in aff) for d in range(3)],
        search_list=sorted({int(ch[i]["search_list"]) for i in cap}),
        l1_best_reused=sum(same[int(ch[i]["best_ref"][1])] >= 0 for i in cap),
        unique_differs=sum(int(ch[i]["best_ref_l1_unique"]) != int(ch[i]["best_ref"][1])
                           for i in cap),
        by_height={h: (sum(int(me00[i]["h"]) == h for i in aff),
                       sum(int(me00[i]["h"]) == h for i in cap if i not in aff))
                   for h in SIDES})
