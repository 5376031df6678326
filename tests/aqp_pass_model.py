"""The expected frame passes with adaptive QP (xvcgpu_frame_pass_aqp,
xvcgpu_frame_pass_bi_refs_aqp; pipeline.FramePass / BiRefsFramePass with aqp_strength),
composed of pinned oracle pieces and nothing else: xo_variance_map + xo_ctu_variance give the
CTU statistic, the table's thresholds (pinned to xo_aqp_delta_qp, and through it to the
reference, by tests/test_aqp_pass_model.py) the delta, apply() writes the table's entry into
copies of the job arrays exactly as include/xvcgpu.h words xvcgpu_aqp_apply, and then

  P:  xo_frame_pass (oracle_frame, encode_only) over those arrays, the CU records' QPs set,
      xo_deblock_picture, xo_pad_border, xo_picture_ssd;
  B:  bi_refs_pass_model's composition over those arrays, the CU records' QPs set in front of
      its deblocking call.

Also the inputs the adaptive-QP tests share: the 200x136 scene whose CTUs run from flat to
full-range noise (scene), its partition (partition_200) and the B inputs of
bi_refs_pass_model with a contrast per CTU (b_scene).

TEST INFRASTRUCTURE."""
import copy
import ctypes as C
import math

import numpy as np

import bi_refs_pass_model as rm
import oracle_frame
import oracle_lib as ol
import oracle_stats as st

BL, BC = 128, 64
BORDERS = (BL, BC, BC)
W, H = 200, 136           # 4 x 3 CTUs: the last column 8 samples wide, the last row 8 high
CTU = 64
QP, STRENGTH = 32, 13
SEARCH_RANGE = 64
DELTA_MIN, DELTAS = -3, 11
# the delta each CTU of the scene is built for, [row][column].  The reference reads a block
# that hangs over the right edge on into the next picture row, i.e. into column 0's CTU, and
# one that hangs over the bottom edge on into what lies behind the plane: column 3 repeats
# column 0's noise and the last row is full-range noise (7 whatever the missing half holds),
# so that the reference's reading and the border's agree on every CTU.
SCENE_DELTAS = ((-3, -2, -1, -3), (3, 1, 5, 3), (7, 7, 7, 7))


def table_delta(table, var):
    """xvcgpu_aqp_apply's count of the thresholds the statistic reaches"""
    return DELTA_MIN + sum(1 for k in range(DELTAS - 1) if var >= int(table.var_min[k]))


def amplitude_for(delta, bd, strength=STRENGTH):
    """The amplitude a of uniform noise in [-a, a] whose 16x16 statistic 256 * a (a + 1) / 3
    lies in the middle of the delta's interval of kStrength * (1.5 ln v - 15 - 2 (bd - 8)),
    which the reference truncates towards zero (cu_encoder.cc:359-362): the interval of d > 0
    is [d, d + 1), of d < 0 (d - 1, d].  The lowest delta: flat; the highest: full range."""
    if delta <= DELTA_MIN:
        return 0
    if delta >= DELTA_MIN + DELTAS - 1:
        return (1 << (bd - 1)) - 1
    assert delta != 0
    x = delta + (0.5 if delta > 0 else -0.5)
    v = math.exp((x / (strength / 10.0) + 15 + 2 * (bd - 8)) / 1.5)
    return int(round(math.sqrt(3 * v / 256)))


_scenes = {}


def scene(bd):
    """(orig, ref): [Y, U, V] padded planes of the 200x136 picture.  Mid grey plus, per CTU,
    uniform noise of amplitude_for(SCENE_DELTAS) in luma and a quarter of it in chroma; the
    reference picture is the original displaced by (2, -2) luma samples plus grain of +-48
    (in 8-bit units)."""
    if bd not in _scenes:
        rng = np.random.default_rng(5200 + bd)
        mid = 1 << (bd - 1)
        orig = []
        for c in range(3):
            cs = 1 if c else 0
            w, h, b = W >> cs, H >> cs, BORDERS[c]
            yy, xx = np.mgrid[0:h, 0:w]
            amp = np.zeros((h, w), np.int64)
            for r, row in enumerate(SCENE_DELTAS):
                for q, d in enumerate(row):
                    a = amplitude_for(d, bd) >> (2 * cs)
                    amp[((yy << cs) // CTU == r) & ((xx << cs) // CTU == q)] = a
            noise = rng.integers(-amp, amp + 1)
            p = np.clip(mid + noise, 0, (1 << bd) - 1).astype(np.uint16)
            orig.append(np.ascontiguousarray(np.pad(p, b, mode="edge")))
        ref = []
        for c in range(3):
            cs = 1 if c else 0
            moved = np.roll(orig[c], (2 >> cs, -2 >> cs), (0, 1)).astype(np.int64)
            # (coarse enough that blocks keep levels at every QP of the map, 29 .. 39)
            grain = rng.integers(-(48 << (bd - 8)), (48 << (bd - 8)) + 1, moved.shape)
            ref.append(np.ascontiguousarray(np.clip(moved + grain, 0, (1 << bd) - 1)
                                            .astype(np.uint16)))
        _scenes[bd] = (orig, ref)
    return _scenes[bd]


def partition_200():
    """A partition of the 200x136 picture: a 64x64 CU, 32x32, 32x16, 16x32, 16x16, 16x8 and
    8x8 CUs, 4-wide CUs, and CUs in the cut CTUs of the last column and row."""
    p = [(0, 0, 64, 64)]
    p += [(x, y, 32, 32) for y in (0, 32) for x in (64, 96)]
    p += [(x, y, 16, 16) for y in range(0, 64, 16) for x in range(128, 192, 16)]
    p += [(192, y, 8, 8) for y in range(0, 64, 8)]
    p += [(x, y, 4, 8) for y in (64, 72) for x in range(0, 64, 4)]
    p += [(x, y, 16, 16) for y in range(80, 128, 16) for x in range(0, 64, 16)]
    p += [(64, 64, 32, 16), (64, 80, 32, 16), (96, 64, 16, 32), (112, 64, 16, 32),
          (64, 96, 32, 32), (96, 96, 32, 32)]
    p += [(x, y, 16, 16) for y in range(64, 128, 16) for x in range(128, 192, 16)]
    p += [(192, y, 8, 8) for y in range(64, 128, 8)]
    p += [(x, 128, 16, 8) for x in range(0, 192, 16)] + [(192, 128, 8, 8)]
    return np.array(p, np.int32)


def descriptors(bd, rdoq=False, part=False, qp=QP):
    from xvc_amd import pipeline
    return pipeline.FrameDescriptors(W, H, qp, search_range=SEARCH_RANGE, rdoq=rdoq,
                                     bitdepth=bd, partition=partition_200() if part else None)


def ctu_variances(xo, w, h, luma_padded, ctu=CTU):
    """The CTU statistic as xvcgpu_variance_map writes it, [rows, columns] uint64; blocks
    that hang over the picture edge read the border."""
    vm = st.xo_variance_map(xo, w, h, luma_padded[BL:, BL:])
    rows, cols = (h + ctu - 1) // ctu, (w + ctu - 1) // ctu
    out = np.zeros((rows, cols), np.uint64)
    for r in range(rows):
        for q in range(cols):
            out[r, q] = st.xo_ctu_variance(xo, w, h, q * ctu, r * ctu, ctu, vm)
    return out


def ctu_variances_as_the_reference_reads(luma, ctu=CTU):
    """The CTU statistic of an unpadded h x w luma plane the way CalcDeltaQpFromVariance
    (cu_encoder.cc:319-357) reads it from an original picture without a border, rows lying
    one behind the other and (in oracle/ref_harness.cc's picture) zeroed chroma planes behind
    them: a 16x16 block that hangs over the right edge runs on into the next row, one that
    hangs over the bottom edge into the zeros.  For whole CTUs it is ctu_variances'."""
    h, w = luma.shape
    flat = np.concatenate([luma.astype(np.int64).ravel(), np.zeros(w * h // 2, np.int64)])
    rows, cols = (h + ctu - 1) // ctu, (w + ctu - 1) // ctu
    out = np.zeros((rows, cols), np.uint64)
    kk, ll = np.mgrid[0:16, 0:16]
    for r in range(rows):
        for q in range(cols):
            v = []
            for i in range(ctu // 16):
                for j in range(ctu // 16):
                    x, y = q * ctu + 16 * j, r * ctu + 16 * i
                    if x >= w or y >= h:
                        continue
                    s = flat[(y + kk) * w + x + ll]
                    total, squares = int(s.sum()), int((s * s).sum())
                    v.append((256 * (squares - (total * total) // 256)) // 256)
            out[r, q] = 1 + sorted(v)[len(v) // 2]
    return out


def apply(table, ctu_var, me_arrays, tx, prm, luma_idx):
    """xvcgpu_aqp_apply on copies.  Returns (me arrays, tx, prm or None, cu_qp [n, 2] int8,
    ctu_dqp [n_ctus] int8, written [n_ctus] bool: the CTUs that hold a CU origin)."""
    me_arrays = [m.copy() for m in me_arrays]
    tx, prm = tx.copy(), (prm.copy() if prm is not None else None)
    flat = np.asarray(ctu_var, np.uint64).reshape(-1)
    n = len(me_arrays[0])
    cu_qp = np.zeros((n, 2), np.int8)
    ctu_dqp, written = np.zeros(len(flat), np.int8), np.zeros(len(flat), bool)
    size, per_row = int(table.ctu_size), int(table.ctus_per_row)
    for i in range(n):
        b = me_arrays[0][i]
        ctu = (int(b["y"]) // size) * per_row + int(b["x"]) // size
        d = table_delta(table, int(flat[ctu]))
        k = d - DELTA_MIN
        for m in me_arrays:
            m["lambda16"][i] = table.lambda16[k]
        t0 = int(luma_idx[i])
        for c in range(3):
            tx["qp"][t0 + c] = table.qp_y[k] if c == 0 else table.qp_c[k]
            if prm is not None:
                prm["lambda"][t0 + c] = table.rdoq_lambda[k][c]
                prm["rd_factor"][t0 + c] = table.rdoq_rd_factor[k][c]
        cu_qp[i] = (table.qp_y[k], table.qp_c[k])
        ctu_dqp[ctu], written[ctu] = d, True
    return me_arrays, tx, prm, cu_qp, ctu_dqp, written


def applied_descriptors(desc, table, ctu_var):
    """(a copy of desc whose job arrays carry the per-CU values, cu_qp, ctu_dqp)"""
    (me,), tx, prm, cu_qp, ctu_dqp, _ = apply(table, ctu_var, [desc.me], desc.tx,
                                              desc.rdoq_params, desc.luma_idx)
    d = copy.copy(desc)
    d.me, d.tx, d.rdoq_params = me, tx, prm
    return d, cu_qp, ctu_dqp


def _inner(p, b, w, h):
    return p[b:b + h, b:b + w]


def block_levels(xo, desc, bd, orig, pred):
    """The levels of every transform block of desc (its own qp / RDOQ constants) between
    the padded original and the unpadded prediction planes; a block without levels: zeros."""
    pw, ph = desc.w, desc.h
    rq = xo.dll.xo_residual_pipeline_rdoq
    rq.restype = C.c_int
    rq.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p] + [ol.u16p, ol.pd] * 3 + [ol.i16p]
    tx = np.ascontiguousarray(desc.tx)
    if desc.rdoq:
        ctxs = np.ascontiguousarray(desc.rdoq_contexts)
        prm = np.ascontiguousarray(desc.rdoq_params)
    rec = [np.zeros_like(p) for p in pred]
    levels, kept = np.zeros(64 * 64, np.int16), []
    for t in range(len(tx)):
        c = int(tx[t]["comp"])
        o = _inner(orig[c], BORDERS[c], pw >> (c > 0), ph >> (c > 0))
        planes = (o.ctypes.data_as(ol.u16p), o.strides[0] // 2, pred[c].ctypes.data_as(ol.u16p),
                  pred[c].strides[0] // 2, rec[c].ctypes.data_as(ol.u16p),
                  rec[c].strides[0] // 2, levels.ctypes.data_as(ol.i16p))
        if desc.rdoq:
            nz = rq(bd, tx[t:].ctypes.data, ctxs.ctypes.data, prm[t:].ctypes.data, *planes)
        else:
            nz = xo._residual_pipeline(bd, tx[t:].ctypes.data_as(C.POINTER(ol.TxBlock)), *planes)
        n = int(tx[t]["w"]) * int(tx[t]["h"])
        kept.append(levels[:n].copy() if nz else np.zeros(n, np.int16))
    return kept


def p_pass(xo, desc, bd, orig, ref, table, ref_poc=0, levels=True):
    """The P pass with adaptive QP.  Returns (rec padded planes, res, nnz, cus, (ssd,
    samples), cu_qp, ctu_dqp [rows, columns], levels per transform block or None)."""
    pw, ph = desc.w, desc.h
    ctu_var = ctu_variances(xo, pw, ph, orig[0], int(table.ctu_size))
    d, cu_qp, ctu_dqp = applied_descriptors(desc, table, ctu_var)
    rec, res, nnz, cus, _ = oracle_frame.frame_pass(d, bd, orig, ref, BL, ref_poc=ref_poc,
                                                    lib=xo, encode_only=True)
    own = cus[d.cu_base:d.cu_base + d.n_cus]
    own["qp_y"], own["qp_c"] = cu_qp[:, 0], cu_qp[:, 1]
    xo.deblock(bd, pw, ph, 0, 0, 0, 4, cus, d.cu_map, rec, BORDERS)
    xo.pad_border(pw, ph, rec, BORDERS)
    ssd = xo.picture_ssd(bd, _inner(orig[0], BL, pw, ph), _inner(rec[0], BL, pw, ph))
    kept = None
    if levels:
        pred = [np.zeros((ph >> (c > 0), pw >> (c > 0)), np.uint16) for c in range(3)]
        for b, r in zip(d.me, res):
            x, y, w, h = (int(b[k]) for k in ("x", "y", "w", "h"))
            for c in range(3):
                cs = 1 if c else 0
                pred[c][y >> cs:(y + h) >> cs, x >> cs:(x + w) >> cs] = xo.mc_block(
                    bd, c, x, y, w, h, int(r["mv_x"]), int(r["mv_y"]), pw, ph, ref[c], BORDERS[c])
        kept = block_levels(xo, d, bd, orig, pred)
    return (rec, res, nnz, cus, (int(ssd[0]), int(ssd[1])), cu_qp,
            ctu_dqp.reshape(ctu_var.shape), kept)


# ---- B ---------------------------------------------------------------------------------
class _SetQpThenDeblock:
    """The oracle with one addition: the CU records' QPs are set in front of the deblocking
    call (what xvcgpu_cu_info_set_qp does between the record kernel and the tail)."""

    def __init__(self, xo, cu_qp):
        self._xo, self._cu_qp = xo, cu_qp

    def __getattr__(self, name):
        return getattr(self._xo, name)

    def deblock(self, bd, pw, ph, bipred, beta, tc, sub, cus, *rest):
        cus["qp_y"][:len(self._cu_qp)] = self._cu_qp[:, 0]
        cus["qp_c"][:len(self._cu_qp)] = self._cu_qp[:, 1]
        return self._xo.deblock(bd, pw, ph, bipred, beta, tc, sub, cus, *rest)


# contrast per CTU [row][column] of the B inputs (both are 2 x 2 CTUs)
B_GAIN = ((1.0, 0.3), (0.05, 0.0))
_b_scenes = {}


def b_scene(name):
    """bi_refs_pass_model's input `name` with the contrast around mid grey scaled per CTU
    (the original and every reference alike, by position): (pw, ph, bd, partition, orig,
    {poc: planes})."""
    if name not in _b_scenes:
        pw, ph, bd, part, orig, refs = rm.make_refs(name)
        mid = 1 << (bd - 1)

        def scaled(planes):
            out = []
            for c, p in enumerate(planes):
                cs, b = (1 if c else 0), BORDERS[c]
                yy, xx = np.mgrid[0:p.shape[0], 0:p.shape[1]]
                r = np.clip(((yy - b) << cs) // CTU, 0, 1)
                q = np.clip(((xx - b) << cs) // CTU, 0, 1)
                gain = np.array(B_GAIN)[r, q]
                v = np.rint(mid + (p.astype(np.float64) - mid) * gain)
                out.append(np.ascontiguousarray(v.astype(np.uint16)))
            return out
        _b_scenes[name] = (pw, ph, bd, part, scaled(orig),
                           {poc: scaled(planes) for poc, planes in refs.items()})
    return _b_scenes[name]


_b_searched = {}


def b_pass(xo, name, which, rdoq, table):
    """The B pass with adaptive QP over b_scene(name), set `which` of bi_refs_pass_model.
    Returns (rm.frame_pass's answer, cu_qp, ctu_dqp [rows, columns])."""
    pw, ph, bd, _, orig, refs = b_scene(name)
    lists = rm.SETS[which]
    desc = rm.descriptors(name, rdoq)
    ctu_var = ctu_variances(xo, pw, ph, orig[0], int(table.ctu_size))
    d, cu_qp, ctu_dqp = applied_descriptors(desc, table, ctu_var)
    key = (name, which, bytes(table))   # (the searches read the table's lambda16)
    if key not in _b_searched:
        _b_searched[key] = rm.search_motion(xo, bd, pw, ph, orig[0], refs, lists,
                                            rm.jobs(d, lists), key=("aqp", name, bytes(table)))
    out = rm.frame_pass(_SetQpThenDeblock(xo, cu_qp), d, bd, orig, refs, lists, _b_searched[key])
    return out, cu_qp, ctu_dqp.reshape(ctu_var.shape)
