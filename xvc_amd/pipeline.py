"""Hot-path frame pass on the GPU: the composition bench.py times.

For one picture with a fixed CU partition (16x16 CUs, 16x8 / 8x16 / 8x8 at the
picture edges, as the reference's forced boundary splits produce):

  me_search        T1+T3   TZ full-pel + 9+8 point sub-pel search per CU
  mc_from_me       I1      motion compensation Y,U,V with the searched MV
  residual_batch   X1,Q,Q1,X2,R1  transform -> quant -> dequant -> inverse -> rec
  cu_info_from_me          CU metadata for the in-loop filter (device-side glue)
  deblock          D1-D4   vertical-edge pass, horizontal-edge pass
  pad_border       P1      so the result can serve as the next reference
  picture_ssd      M6      PSNR-Y parts

Everything (pictures, descriptors, decisions) stays resident in HBM; the host
only enqueues ~9 launches per picture.  What the reference derives serially
from neighbouring CUs (AMVP predictor, previous CU's MV, CABAC state for RDOQ)
is an INPUT of the batched kernels: here the predictor is the zero vector and
the quantiser is the reference's non-RDO QuantFast (scope).
"""
import math
import os

import ctypes as C

import numpy as np

from . import api

# Qp::kChromaScale_ for 4:2:0 with chroma_qp_offset_table == 1
# (quantize.cc:34-38)
_CHROMA_SCALE = list(range(30)) + [29, 30, 31, 32, 33, 33, 34, 34, 35, 35, 36,
                                   36, 37, 37, 38, 39, 40, 41, 42, 43, 44, 45,
                                   46, 47, 48, 49, 50, 51]


def chroma_qp(qp):
    return _CHROMA_SCALE[max(0, min(57, qp))]


def lambda16_for_qp(qp):
    """floor(65536*sqrt(lambda)) with lambda = 0.57*2^((qp-12)/3)
    (PictureData::Init, picture_data.cc:96-97; inter_tz_search.cc:98-99)."""
    lam = 0.57 * math.pow(2.0, (qp - 12) / 3.0)
    return int(math.floor(65536.0 * math.sqrt(lam)))


def lambda_sqrt_for_qp(qp):
    """sqrt(lambda) in double, lambda = 0.57*2^((qp-12)/3): the expression lambda16_for_qp
    floors, what SearchMergeCandidates ranks with (qp.GetLambdaSqrt())."""
    return math.sqrt(0.57 * math.pow(2.0, (qp - 12) / 3.0))


_INV_QUANT_SCALES = (40, 45, 51, 57, 64, 72)       # quantize.cc:44-46
_DATA = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data")
_init_ctx_table = None


def rdoq_init_contexts(qp, pic_type=1):
    """The coefficient-coding context states a syntax writer starts a picture of
    this qp / type with (CabacContexts::ResetStates, cabac.cc:311-358), as one
    xvcgpu_rdoq_contexts record.  RDOQ reads the entropy coder's states
    (rdo_quant.cc:254): an integration snapshots its live CABAC contexts per
    batch; this repo's frame pass has no entropy coder and feeds the
    picture-initial states (data/rdoq_init_contexts.npy, captured from the
    reference by tools/gen_rdoq_contexts.py).  pic_type: 0 bi, 1 uni, 2 intra."""
    global _init_ctx_table
    if _init_ctx_table is None:
        _init_ctx_table = np.load(os.path.join(_DATA, "rdoq_init_contexts.npy"))
    raw = _init_ctx_table[max(0, min(63, qp)), pic_type]
    return np.ascontiguousarray(raw).view(api.RDOQ_CTX_DTYPE).copy()


def rdoq_host_params(qp, bitdepth, lam=None):
    """The two double-arithmetic constants of QuantRdo per component, as the
    reference computes them on the host (rdo_quant.cc:251-252, :590-594; Qp,
    quantize.cc:48-92): returns [(lambda_fix, rd_factor)] for Y, U, V.  `lam` =
    the luma lambda (default: PictureData::Init's 0.57 * 2^((qp - 12) / 3))."""
    if lam is None:
        lam = 0.57 * math.pow(2.0, (qp - 12) / 3.0)
    qpc = chroma_qp(qp)
    # Qp::GetChromaDistWeight with table 1, offset 0 (quantize.cc:82-92)
    weight_c = math.pow(2.0, -(qpc - max(0, min(57, qp))) / 3.0)
    out = []
    for c in range(3):
        lam_c = lam if c == 0 else lam / weight_c
        qpb = max(0, (qp if c == 0 else qpc) + 6 * (bitdepth - 8))
        inv_scale = float(_INV_QUANT_SCALES[qpb % 6] << (qpb // 6))
        lambda_fix = int(lam_c * 65536 + 0.5)
        rd_factor = int(inv_scale * inv_scale / lam_c / 16 / (1 << (2 * (bitdepth - 8))) + 0.5)
        out.append((lambda_fix, rd_factor))
    return out


def _aqp_delta(var, bitdepth, strength):
    """CuEncoder::CalcDeltaQpFromVariance's last lines (cu_encoder.cc:359-363) in the
    reference's double expression, truncating cast included."""
    d = (1.0 * strength / 10) * (1.5 * math.log(float(var)) - 15 - 2 * (bitdepth - 8))
    return max(api.AQP_DELTA_MIN, min(api.AQP_DELTA_MIN + api.AQP_DELTAS - 1, int(d)))


def aqp_table(pic_qp, bitdepth, strength, width, ctu_size=64):
    """The xvcgpu_aqp_table (api.AqpTable) of a picture coded at pic_qp with adaptive QP
    of this aqp_strength (CuEncoder::EncodeCtu, cu_encoder.cc:92-97; the reference's
    default is 13, encoder_settings.h:89-90).  The delta does not decrease in the CTU
    statistic v for a strength >= 0, so var_min[k] - the smallest v >= 1 whose delta is
    >= -2 + k, found by bisection over [1, 2^63] with the reference's expression;
    UINT64_MAX: none - says it without a logarithm.  Per delta: the clipped QP
    (PictureData::GetQp, picture_data.h:51-53), its chroma QP and the constants of a
    picture of that QP with recalculate_lambda (picture_data.cc:94-106) as
    lambda16_for_qp and rdoq_host_params compute them.  The same bytes as
    xvc_gpu::AdaptiveQp::Table (host/xvc_gpu_ops.h)."""
    if strength < 0:
        raise ValueError("aqp_strength %d: a negative strength makes the delta fall as the "
                         "variance grows; the thresholds cannot say that" % strength)
    if ctu_size not in (16, 32, 64, 128):
        raise ValueError("ctu_size %r is not 16, 32, 64 or 128" % (ctu_size,))
    t = api.AqpTable()
    t.pic_qp, t.ctu_size = pic_qp, ctu_size
    t.ctus_per_row = (width + ctu_size - 1) // ctu_size
    top = 1 << 63
    for k in range(api.AQP_DELTAS - 1):
        want = api.AQP_DELTA_MIN + 1 + k
        if _aqp_delta(top, bitdepth, strength) < want:
            t.var_min[k] = 0xffffffffffffffff
            continue
        lo, hi = 1, top         # the answer lies in [lo, hi]; delta(hi) >= want
        while lo < hi:
            mid = (lo + hi) // 2
            if _aqp_delta(mid, bitdepth, strength) >= want:
                hi = mid
            else:
                lo = mid + 1
        t.var_min[k] = lo
    for k in range(api.AQP_DELTAS):
        qp = max(0, min(63, pic_qp + api.AQP_DELTA_MIN + k))
        t.qp_y[k], t.qp_c[k], t.lambda16[k] = qp, chroma_qp(qp), lambda16_for_qp(qp)
        for c, (lf, rf) in enumerate(rdoq_host_params(qp, bitdepth)):
            t.rdoq_lambda[k][c], t.rdoq_rd_factor[k][c] = lf, rf
    return t


class _AqpArrays:
    """What an adaptive-QP pass object holds beside the flat pass's state: the table and
    the four arrays of xvcgpu_aqp_args (allocated once; every run writes them)."""

    def __init__(self, ctx, desc, bitdepth, strength, ctu_size=64):
        self.ctx, self.strength, self.ctu_size = ctx, strength, ctu_size
        self.table = aqp_table(desc.qp, bitdepth, strength, desc.w, ctu_size)
        self.ctu_cols = (desc.w + ctu_size - 1) // ctu_size
        self.ctu_rows = (desc.h + ctu_size - 1) // ctu_size
        self.n_cus = desc.n_cus
        self.d_var16 = ctx.alloc(8 * ((desc.w + 15) // 16) * ((desc.h + 15) // 16))
        self.d_ctu_var = ctx.alloc(8 * self.ctu_cols * self.ctu_rows)
        self.d_ctu_dqp = ctx.alloc(self.ctu_cols * self.ctu_rows)
        self.d_cu_qp = ctx.alloc(2 * max(1, desc.n_cus))

    def args(self):
        q = api.AqpArgs()
        q.table = self.table
        q.d_var16, q.d_ctu_var = self.d_var16.ptr, self.d_ctu_var.ptr
        q.d_ctu_dqp, q.d_cu_qp = self.d_ctu_dqp.ptr, self.d_cu_qp.ptr
        return q

    def ctu_delta_qp(self):
        """The last run's delta QP per CTU, [rows, columns] int8."""
        return self.d_ctu_dqp.to_array(np.int8, self.ctu_cols * self.ctu_rows).reshape(
            self.ctu_rows, self.ctu_cols)

    def cu_qp(self):
        """The last run's (qp_y, qp_c) per CU, [n_cus, 2] int8."""
        return self.d_cu_qp.to_array(np.int8, 2 * self.n_cus).reshape(-1, 2)

    def free(self):
        for b in (self.d_var16, self.d_ctu_var, self.d_ctu_dqp, self.d_cu_qp):
            b.free()


class _AffineArrays:
    """What a pass with affine motion holds beside the flat pass's state: the arrays of
    xvcgpu_frame_pass_affine_args (allocated once; every run writes the work arrays)."""

    def __init__(self, ctx, desc, mvp=None, side_bits=1):
        self.ctx, self.n_cus, self.side_bits = ctx, desc.n_cus, side_bits
        self.jobs, self.order, self.n_class = desc.affine_jobs(mvp)
        n = max(1, desc.n_cus)
        self.d_affine = ctx.buffer(self.jobs) if desc.n_cus else ctx.alloc(api.AFFINE_ME_DTYPE.itemsize)
        self.d_affine_res = ctx.buffer(np.zeros(n, api.AFFINE_ME_RESULT_DTYPE))
        self.d_order = ctx.buffer(self.order) if len(self.order) else None
        self.d_choice = ctx.buffer(np.zeros(n, api.FP_AFFINE_RESULT_DTYPE))
        self.d_inter = ctx.buffer(np.zeros(3 * n, api.INTER_DTYPE))

    def args(self):
        f = api.FramePassAffineArgs()
        f.d_affine, f.d_affine_results = self.d_affine.ptr, self.d_affine_res.ptr
        f.d_order = self.d_order.ptr if self.d_order is not None else None
        f.n_class[:] = self.n_class
        f.side_bits = self.side_bits
        f.d_choice, f.d_inter = self.d_choice.ptr, self.d_inter.ptr
        return f

    def choice(self):
        return self.d_choice.to_array(api.FP_AFFINE_RESULT_DTYPE, self.n_cus)

    def affine_results(self):
        return self.d_affine_res.to_array(api.AFFINE_ME_RESULT_DTYPE, self.n_cus)

    def affine_blocks(self):
        return self.d_affine.to_array(api.AFFINE_ME_DTYPE, self.n_cus)

    def inter_jobs(self):
        return self.d_inter.to_array(api.INTER_DTYPE, 3 * self.n_cus)

    def free(self):
        for b in (self.d_affine, self.d_affine_res, self.d_order, self.d_choice, self.d_inter):
            if b is not None:
                b.free()


def merge_cand_array(cands, n_cus):
    """A pass's merge candidates as api.FP_MERGE_CAND_DTYPE [n_cus, 5]: from such an array as
    it is, or from list 0's vectors [n_cus, 5, 2] int32 (1/16 pel, unclipped) - every candidate
    then names picture 0 of list 0 and leaves list 1 unused (ref_idx = {0, -1}).  The same
    bytes as xvc_gpu::FramePass::MergeCands makes."""
    c = np.asarray(cands)
    if c.dtype == api.FP_MERGE_CAND_DTYPE:
        if c.shape != (n_cus, api.FP_MERGE_CANDS):
            raise ValueError("merge_cands: expected %d x %d candidates, got shape %r"
                             % (n_cus, api.FP_MERGE_CANDS, c.shape))
        return np.ascontiguousarray(c)
    if c.shape != (n_cus, api.FP_MERGE_CANDS, 2) or not np.issubdtype(c.dtype, np.integer):
        raise ValueError("merge_cands: expected an integer array [%d, %d, 2] (x, y per "
                         "candidate), got shape %r, dtype %s"
                         % (n_cus, api.FP_MERGE_CANDS, c.shape, c.dtype))
    out = np.zeros((n_cus, api.FP_MERGE_CANDS), api.FP_MERGE_CAND_DTYPE)
    out["ref_idx"] = (0, -1)
    out["mv"][:, :, 0, :] = c
    return out


def merge_order_array(order, n_cus):
    """(d_order or None, n_listed) of xvcgpu_frame_pass_merge_args: None lists every CU (a
    NULL list of n_cus); else the strictly ascending CU indices that try merge."""
    if order is None:
        return None, n_cus
    o = np.asarray(order, np.int64).reshape(-1)
    if len(o) and (o[0] < 0 or o[-1] >= n_cus or (np.diff(o) <= 0).any()):
        raise ValueError("merge_order: strictly ascending indices in [0, %d) expected" % n_cus)
    return o.astype(np.int32), len(o)


class _MergeArrays:
    """What a pass with merge mode holds beside the flat pass's state: the arrays of
    xvcgpu_frame_pass_merge_args (allocated once; every run writes the work arrays)."""

    def __init__(self, ctx, desc, cands, order, side_bits, merge_side_bits, lambda_sqrt):
        self.ctx, self.n_cus = ctx, desc.n_cus
        self.side_bits, self.merge_side_bits = side_bits, merge_side_bits
        self.lambda_sqrt = float(lambda_sqrt)
        self.cands = cands                      # merge_cand_array's
        self.order, self.n_listed = order       # merge_order_array's
        n = max(1, desc.n_cus)
        self.d_cands = ctx.buffer(self.cands) if desc.n_cus else ctx.alloc(api.FP_MERGE_CAND_DTYPE.itemsize)
        self.d_order = ctx.buffer(self.order) if self.order is not None and len(self.order) else None
        self.d_rank = ctx.buffer(np.zeros(n, api.FP_MERGE_RANK_DTYPE))
        self.d_choice = ctx.buffer(np.zeros(n, api.FP_MERGE_RESULT_DTYPE))
        self.d_chosen = ctx.buffer(np.zeros(n, api.MERES_DTYPE))

    def args(self):
        return merge_args(self.n_listed, self.side_bits, self.merge_side_bits, self.lambda_sqrt,
                          self.d_cands.ptr, self.d_order.ptr if self.d_order is not None else None,
                          self.d_rank.ptr, self.d_choice.ptr, self.d_chosen.ptr)

    def free(self):
        for b in (self.d_cands, self.d_order, self.d_rank, self.d_choice, self.d_chosen):
            if b is not None:
                b.free()


def merge_args(n_listed, side_bits, merge_side_bits, lambda_sqrt, d_cands=None, d_order=None,
               d_rank=None, d_choice=None, d_chosen=None):
    """xvcgpu_frame_pass_merge_args from its parts (pointers: integers or None)."""
    m = api.FramePassMergeArgs()
    m.d_cands, m.d_order, m.n_listed = d_cands, d_order, n_listed
    m.side_bits, m.merge_side_bits, m.lambda_sqrt = side_bits, merge_side_bits, lambda_sqrt
    m.d_rank, m.d_choice, m.d_chosen = d_rank, d_choice, d_chosen
    return m


def bi_merge_cand_array(cands, n_cus):
    """A B pass's merge candidates as api.FP_MERGE_CAND_DTYPE [n_cus, 5]: from such an array as
    it is, or from a pair (ref_idx [n_cus, 5, 2], mv [n_cus, 5, 2, 2]) of integer arrays -
    per list the picture's index in that list (-1: list unused) and its vector (x, y; 1/16
    pel, unclipped).  The same bytes as xvc_gpu::FramePassBiRefs::MergeCands makes."""
    if isinstance(cands, np.ndarray) and cands.dtype == api.FP_MERGE_CAND_DTYPE:
        if cands.shape != (n_cus, api.FP_MERGE_CANDS):
            raise ValueError("merge_cands: expected %d x %d candidates, got shape %r"
                             % (n_cus, api.FP_MERGE_CANDS, cands.shape))
        return np.ascontiguousarray(cands)
    try:
        ref_idx, mv = (np.asarray(v) for v in cands)
    except (TypeError, ValueError):
        raise ValueError("merge_cands: api.FP_MERGE_CAND_DTYPE [n_cus, 5] or a pair (ref_idx "
                         "[n_cus, 5, 2], mv [n_cus, 5, 2, 2]) expected")
    want = (n_cus, api.FP_MERGE_CANDS, 2)
    if ref_idx.shape != want or mv.shape != want + (2,) or \
            not np.issubdtype(ref_idx.dtype, np.integer) or not np.issubdtype(mv.dtype, np.integer):
        raise ValueError("merge_cands: expected integer arrays ref_idx %r and mv %r, got %r %s "
                         "and %r %s" % (want, want + (2,), ref_idx.shape, ref_idx.dtype, mv.shape,
                                        mv.dtype))
    if len(ref_idx) and (ref_idx.min() < -128 or ref_idx.max() > 127):
        raise ValueError("merge_cands: ref_idx does not fit the candidate's int8")
    out = np.zeros((n_cus, api.FP_MERGE_CANDS), api.FP_MERGE_CAND_DTYPE)
    out["ref_idx"] = ref_idx
    out["mv"] = mv
    return out


class _BiMergeArrays:
    """What a B pass with merge mode holds beside the plain pass's state: the arrays of
    xvcgpu_frame_pass_bi_merge_args (allocated once; every run writes the work arrays)."""

    def __init__(self, ctx, desc, cands, order, merge_side_bits, lambda_sqrt):
        self.ctx, self.n_cus = ctx, desc.n_cus
        self.merge_side_bits, self.lambda_sqrt = merge_side_bits, float(lambda_sqrt)
        self.cands = cands                      # bi_merge_cand_array's
        self.order, self.n_listed = order       # merge_order_array's
        n = max(1, desc.n_cus)
        self.d_cands = ctx.buffer(self.cands) if desc.n_cus else ctx.alloc(api.FP_MERGE_CAND_DTYPE.itemsize)
        self.d_order = ctx.buffer(self.order) if self.order is not None and len(self.order) else None
        self.d_rank = ctx.buffer(np.zeros(n, api.FP_MERGE_RANK_DTYPE))
        self.d_choice = ctx.buffer(np.zeros(n, api.FP_BI_MERGE_RESULT_DTYPE))
        self.d_chosen = ctx.buffer(np.zeros(n, api.FP_BI_REFS_RESULT_DTYPE))

    def args(self):
        return bi_merge_args(self.n_listed, self.merge_side_bits, self.lambda_sqrt,
                             self.d_cands.ptr, self.d_order.ptr if self.d_order is not None else None,
                             self.d_rank.ptr, self.d_choice.ptr, self.d_chosen.ptr)

    def free(self):
        for b in (self.d_cands, self.d_order, self.d_rank, self.d_choice, self.d_chosen):
            if b is not None:
                b.free()


def bi_merge_args(n_listed, merge_side_bits, lambda_sqrt, d_cands=None, d_order=None,
                  d_rank=None, d_choice=None, d_chosen=None):
    """xvcgpu_frame_pass_bi_merge_args from its parts (pointers: integers or None)."""
    m = api.FramePassBiMergeArgs()
    m.d_cands, m.d_order, m.n_listed = d_cands, d_order, n_listed
    m.merge_side_bits, m.lambda_sqrt = merge_side_bits, lambda_sqrt
    m.d_rank, m.d_choice, m.d_chosen = d_rank, d_choice, d_chosen
    return m


_AQP_FORMS = ("fwd_transform", "residual", "residual_rdoq")


_AFFINE_SIDES = (16, 32, 64)


def affine_order(me):
    """The order list of xvcgpu_frame_pass_affine_args for the jobs `me` (api.ME_DTYPE):
    (d_order int32 - the indices of the CUs the second, affine SearchMotion run takes,
    grouped by CU height 16, 32, 64 and in CU order inside a group -, n_class [3]).  A CU is
    capable if w and h are each 16, 32 or 64 (CodingUnit::CanUseAffine, coding_unit.h:251-257)
    and its job carries neither ME_FULLPEL_MV nor ME_USE_LIC.  The same list as
    xvc_gpu::FramePass::SetAffine makes."""
    ok = np.isin(me["w"], _AFFINE_SIDES) & np.isin(me["h"], _AFFINE_SIDES) & \
        ((me["fullpel_mv"] & 3) == 0)
    groups = [np.flatnonzero(ok & (me["h"] == h)) for h in _AFFINE_SIDES]
    return (np.concatenate(groups).astype(np.int32) if len(me) else np.zeros(0, np.int32),
            [len(g) for g in groups])


def bi_affine_jobs(me, same, slot, mvp=None):
    """What a B pass with affine motion (xvcgpu_frame_pass_bi_refs_affine) takes beside the
    plain pass's jobs me[l][r] (api.ME_DTYPE): (the uni-directional jobs [n, E]
    api.AFFINE_ME_DTYPE, E = 2 * Rmax, job [i, l * Rmax + r] = CU i into picture r of list l -
    x, y, w, h and lambda16 of the plain job, mvp[l][r] [n, 3, 2] or, None, the plain job's
    mvp at every corner, flags 0 -, their slot bytes [n, E, 2] {slot[l][r], 255} with
    FP_BI_NO_JOB first for r >= num_ref[l] and for a re-used list-1 picture, d_order,
    n_class: affine_order(me[0][0])).  The same bytes as xvc_gpu::FramePassBiRefs::SetAffine
    makes."""
    num_ref = [len(me[0]), len(me[1])]
    rmax, n = max(num_ref), len(me[0][0])
    jobs = np.zeros((n, 2 * rmax), api.AFFINE_ME_DTYPE)
    slots = np.full((n, 2 * rmax, 2), api.FP_BI_NO_JOB, np.uint8)
    for l in range(2):
        for r in range(num_ref[l]):
            j, m = jobs[:, l * rmax + r], me[l][r]
            for k in ("x", "y", "w", "h", "lambda16"):
                j[k] = m[k]
            if mvp is None:
                j["mvp"][:, :, 0] = m["mvp_x"][:, None]
                j["mvp"][:, :, 1] = m["mvp_y"][:, None]
            else:
                j["mvp"] = np.asarray(mvp[l][r], np.int32).reshape(n, 3, 2)
            if l == 0 or same[r] < 0:
                slots[:, l * rmax + r, 0] = slot[l][r]
    order, n_class = affine_order(me[0][0])
    return jobs, slots, order, n_class


class _BiAffineArrays:
    """What a B pass with affine motion holds beside the plain pass's state: the arrays of
    xvcgpu_frame_pass_bi_affine_args (allocated once; every run writes the work arrays)."""

    def __init__(self, ctx, n_cus, me, same, slot, mvp=None):
        self.ctx, self.n_cus = ctx, n_cus
        self.rmax = max(len(me[0]), len(me[1]))
        self.jobs, self.slots, self.order, self.n_class = bi_affine_jobs(me, same, slot, mvp)
        n, e = max(1, n_cus), 2 * self.rmax
        self.d_uni = ctx.buffer(self.jobs) if n_cus else ctx.alloc(api.AFFINE_ME_DTYPE.itemsize)
        self.d_uni_res = ctx.buffer(np.zeros(n * e, api.AFFINE_ME_RESULT_DTYPE))
        self.d_uni_slots = ctx.buffer(self.slots) if n_cus else ctx.alloc(2)
        self.d_bi = ctx.buffer(np.zeros(n * self.rmax, api.AFFINE_ME_DTYPE))
        self.d_bi_res = ctx.buffer(np.zeros(n * self.rmax, api.AFFINE_ME_RESULT_DTYPE))
        self.d_bi_slots = ctx.buffer(np.full(2 * n * self.rmax, api.FP_BI_NO_JOB, np.uint8))
        self.d_order = ctx.buffer(self.order) if len(self.order) else None
        self.d_choice = ctx.buffer(np.zeros(n, api.FP_BI_AFFINE_RESULT_DTYPE))

    def args(self):
        f = api.FramePassBiAffineArgs()
        f.d_uni, f.d_uni_results, f.d_uni_slots = \
            self.d_uni.ptr, self.d_uni_res.ptr, self.d_uni_slots.ptr
        f.d_bi, f.d_bi_results, f.d_bi_slots = self.d_bi.ptr, self.d_bi_res.ptr, self.d_bi_slots.ptr
        f.d_order = self.d_order.ptr if self.d_order is not None else None
        f.n_class[:] = self.n_class
        f.d_choice = self.d_choice.ptr
        return f

    def free(self):
        for b in (self.d_uni, self.d_uni_res, self.d_uni_slots, self.d_bi, self.d_bi_res,
                  self.d_bi_slots, self.d_order, self.d_choice):
            if b is not None:
                b.free()


def cu_partition(width, height, cu=16, xcd_tiles=False):
    """List of (x, y, w, h): cu x cu CUs, smaller at right/bottom edge - in raster
    order, or (xcd_tiles) region by region of a 4 x 2 tiling of the picture, raster
    inside a region.  The kernels give XCD k the k-th contiguous eighth of a job
    list (dev_common.h: xcd_job_index), and an XCD's L2 then holds what its jobs
    read: with raster order that is a band 1/8 of the picture tall plus the rows the
    TZ search's far diamonds (+-64) and the filters reach above and below it -
    (135 + 128) / 135 = 1.95 x the band at 1080p; a quarter-by-half region has the
    shorter boundary: (480 + 128)(540 + 128) / (480 * 540) = 1.57 x."""
    cols, rows = (width + cu - 1) // cu, (height + cu - 1) // cu

    def cell(cx, cy):
        x, y = cx * cu, cy * cu
        return (x, y, min(cu, width - x), min(cu, height - y))
    if not xcd_tiles:
        return [cell(cx, cy) for cy in range(rows) for cx in range(cols)]
    parts = []
    xb = [round(k * cols / 4) for k in range(5)]
    yb = [round(k * rows / 2) for k in range(3)]
    for ty in range(2):
        for tx in range(4):
            parts += [cell(cx, cy) for cy in range(yb[ty], yb[ty + 1])
                      for cx in range(xb[tx], xb[tx + 1])]
    return parts


_CU_SIDES = (4, 8, 16, 32, 64)


def check_partition(width, height, parts):
    """A caller's CU partition - (x, y, w, h) luma rectangles in coding order, a sequence
    or an (n, 4) array - as a list of int tuples, after checking that it is one the frame
    pass can run: origins on the 4-sample grid, sides of 4, 8, 16, 32 or 64 (or what the
    right / bottom picture edge leaves of such a side, a multiple of 4), every CU inside
    the picture, no two overlapping, the picture covered.  ValueError names the first
    offending CU (for a hole: the first uncovered 4x4 cell)."""
    arr = np.asarray(parts)
    if arr.size == 0:
        arr = arr.reshape(0, 4)
    if arr.ndim != 2 or arr.shape[1] != 4 or not np.issubdtype(arr.dtype, np.integer):
        raise ValueError("partition: expected n integer rows (x, y, w, h), got an array of "
                         "shape %r, dtype %s" % (arr.shape, arr.dtype))
    cells_w, cells_h = (width + 3) // 4, (height + 3) // 4
    seen = -np.ones((cells_h, cells_w), np.int64)
    out = []
    for i, (x, y, w, h) in enumerate(arr.tolist()):
        name = "partition: CU %d (x=%d, y=%d, w=%d, h=%d)" % (i, x, y, w, h)
        if w <= 0 or h <= 0 or x < 0 or y < 0 or x + w > width or y + h > height:
            raise ValueError("%s lies outside the %dx%d picture" % (name, width, height))
        if x % 4 or y % 4:
            raise ValueError("%s: origin not on the 4-sample grid" % name)
        for side, at, full, what in ((w, x, width, "width"), (h, y, height, "height")):
            cut = at + side == full and side < 64 and side % 4 == 0
            if side not in _CU_SIDES and not cut:
                raise ValueError("%s: %s %d is not 4, 8, 16, 32 or 64 (nor cut by the picture "
                                 "edge)" % (name, what, side))
        cell = seen[y // 4:(y + h + 3) // 4, x // 4:(x + w + 3) // 4]
        if (cell >= 0).any():
            raise ValueError("%s overlaps CU %d" % (name, int(cell[cell >= 0][0])))
        cell[...] = i
        out.append((x, y, w, h))
    if (seen < 0).any():
        cy, cx = np.argwhere(seen < 0)[0]
        raise ValueError("partition: no CU covers the samples at x=%d, y=%d (a gap)"
                         % (4 * cx, 4 * cy))
    return out


class FrameDescriptors:
    """Host-side (numpy) descriptors of one picture's jobs; shared by the GPU
    frame pass and the CPU oracle frame pass in tests / bench.

    With `row_range=(y0, y1)` only the CUs whose top row lies in [y0, y1) get
    motion-search / residual jobs (one CTU-row shard); the CU map and the CU
    metadata array stay global (indices into the whole picture's raster list)
    because the in-loop filter looks across the shard boundary.

    With `partition=` (check_partition: the luma CU tree of a real picture, CUs of any
    mix of sizes in coding order) instead of the cu x cu grid the arrays are filled the
    same way, CU by CU in the order given; whole pictures only (no row_range, no
    xcd_tiles).  cu_size is then the search's block class - the smallest of 16 / 32 / 64
    that holds the largest side - and cu_rows / cus_per_row are None."""

    def __init__(self, width, height, qp=32, cu=16, search_range=96,
                 row_range=None, rdoq=False, bitdepth=10, xcd_tiles=False, partition=None):
        self.w, self.h, self.qp = width, height, qp
        self.rdoq = rdoq
        # (region-major CU order only for a whole picture: a row shard's CUs have to be
        # a contiguous run of the raster list)
        assert not xcd_tiles or row_range is None or tuple(row_range) == (0, height)
        if partition is not None:
            if xcd_tiles or not (row_range is None or tuple(row_range) == (0, height)):
                raise ValueError("partition= describes a whole picture: no row_range, "
                                 "no xcd_tiles")
            parts_all = check_partition(width, height, partition)
        else:
            parts_all = cu_partition(width, height, cu, xcd_tiles)
        self.partition = parts_all if partition is not None else None
        self.n_cus_total = len(parts_all)
        if row_range is None:
            row_range = (0, height)
        self.row_range = (max(0, row_range[0]), min(height, row_range[1]))
        own = [i for i, p in enumerate(parts_all)
               if self.row_range[0] <= p[1] < self.row_range[1]]
        self.cu_base = own[0] if own else 0
        assert own == list(range(self.cu_base, self.cu_base + len(own)))
        n = len(own)
        self.n_cus = n
        me = np.zeros(n, api.ME_DTYPE)
        tx = np.zeros(3 * n, api.TX_DTYPE)
        luma_idx = np.zeros(n, np.int32)
        cmap = -np.ones(((height + 3) // 4, (width + 3) // 4), np.int32)
        qpc = chroma_qp(qp)
        lam = lambda16_for_qp(qp)
        for gi, (x, y, w, h) in enumerate(parts_all):
            cmap[y // 4:(y + h) // 4, x // 4:(x + w) // 4] = gi
        for i, gi in enumerate(own):
            x, y, w, h = parts_all[gi]
            b = me[i]
            b["x"], b["y"], b["w"], b["h"] = x, y, w, h
            b["depth_nonzero"] = 1
            b["lambda16"] = lam
            b["search_range"] = search_range
            luma_idx[i] = 3 * i
            t = tx[3 * i]
            t["x"], t["y"], t["w"], t["h"], t["comp"], t["qp"] = x, y, w, h, 0, qp
            for c in (1, 2):
                t = tx[3 * i + c]
                t["x"], t["y"], t["w"], t["h"] = x // 2, y // 2, w // 2, h // 2
                t["comp"], t["qp"] = c, qpc
        self.me, self.tx, self.luma_idx, self.cu_map = me, tx, luma_idx, cmap
        self.qp_c = qpc
        self.rdoq_contexts = self.rdoq_params = None
        self.rdoq_lambda = 0.57 * math.pow(2.0, (qp - 12) / 3.0)
        if rdoq:
            # the quantiser the reference's encoder runs (transform_encoder.cc:230)
            tx["intra_pic"] |= api.TXF_RDOQ
            self.rdoq_contexts = rdoq_init_contexts(qp, 1)
            prm = np.zeros(3 * n, api.RDOQ_PARAMS_DTYPE)
            for c, (lf, rf) in enumerate(rdoq_host_params(qp, bitdepth, self.rdoq_lambda)):
                prm["lambda"][c::3] = lf
                prm["rd_factor"][c::3] = rf
            self.rdoq_params = prm
        if partition is not None:
            side = max([max(p[2], p[3]) for p in parts_all], default=16)
            self.cu_rows = self.cus_per_row = None
            self.cu_size = 16 if side <= 16 else (32 if side <= 32 else 64)
            self.min_side = min([min(p[2], p[3]) for p in parts_all], default=16)
            self.max_side = side
            return
        self.cu_rows = (height + cu - 1) // cu
        self.cus_per_row = (width + cu - 1) // cu
        self.cu_size = cu

    def affine_jobs(self, mvp=None):
        """What a pass with affine motion (xvcgpu_frame_pass_affine) takes beside these
        descriptors: (one api.AFFINE_ME_DTYPE job per own CU in CU order - x, y, w, h and
        lambda16 of the plain job, mvp [n, 3, 2] or, None, the plain job's mvp at every
        corner; flags and bootstrap are the device's -, d_order, n_class: affine_order)."""
        jobs = np.zeros(self.n_cus, api.AFFINE_ME_DTYPE)
        for k in ("x", "y", "w", "h", "lambda16"):
            jobs[k] = self.me[k]
        if mvp is None:
            jobs["mvp"][:, :, 0] = self.me["mvp_x"][:, None]
            jobs["mvp"][:, :, 1] = self.me["mvp_y"][:, None]
        else:
            jobs["mvp"] = np.asarray(mvp, np.int32).reshape(self.n_cus, 3, 2)
        order, n_class = affine_order(self.me)
        return jobs, order, n_class


def run_multi(passes, origs, refs, recs, ref_pocs=None):
    """The frame passes of len(passes) independent pictures with every kernel
    launched once for all of them (xvcgpu_frame_pass_multi).  passes: FramePass
    objects of one picture size, each on its own Context - the contexts lend their
    scratch, everything is enqueued on passes[0]'s stream (share_stream() puts the
    other contexts on it).  Passes over a partition (FramePass(partition=...)) are not
    batched: with one among them every pass is run by its own single call."""
    n = len(passes)
    if any(getattr(p, "affine", None) is not None for p in passes):
        raise ValueError("run_multi: a pass with affine motion has no multi-picture form")
    if any(getattr(p, "merge", None) is not None for p in passes):
        raise ValueError("merge_cands and run_multi: a pass with merge mode has no "
                         "multi-picture form")
    if any(p.plan is not None for p in passes):
        for i, p in enumerate(passes):
            p.run(origs[i], refs[i], recs[i], ref_pocs[i] if ref_pocs is not None else 0)
        return
    lead = passes[0].ctx
    ctxs = (C.c_void_p * n)(*[p.ctx.h for p in passes])
    args = [p._call_args(origs[i], refs[i], recs[i], ref_pocs[i] if ref_pocs is not None else 0)
            for i, p in enumerate(passes)]
    argv = (C.POINTER(api.FramePassArgs) * n)(*[C.pointer(a) for a in args])
    lead._check(lead.lib.xvcgpu_frame_pass_multi(
        ctxs, argv, n, api.FP_ENCODE | api.FP_DEBLOCK_V | api.FP_DEBLOCK_H | api.FP_PAD |
        api.FP_SSD))


def share_stream(passes):
    """Put the contexts of passes[1:] on passes[0]'s stream (see run_multi)."""
    stream = passes[0].ctx.stream_ptr()
    for p in passes[1:]:
        p.ctx.set_stream(stream)


class FramePass:
    """Device-resident state for running frame passes of one picture size
    (or of one CTU-row shard of it).

    partition=: the pass over a caller's CU partition (FrameDescriptors) instead of the
    cu x cu grid.  The form follows the shapes - all sides 8 ... 16: the fused forms of
    the grid; else prediction picture + residual pipeline (`residual`, `residual_rdoq`,
    or `fwd_transform` for packed RDOQ) -, the fused tail needs CUs without a side of 4,
    and the search runs through a plan made here (xvcgpu_me_plan_create: the jobs sorted
    once by kernel instance, one launch per non-empty bin).

    form=: name the form instead of taking the one the shapes give - "fwd_transform" where
    that would be "fwd_from_me" (the same buffers; the form an adaptive-QP pass can run).

    aqp_strength=: None, or the reference's aqp_strength (13 by default there) for a pass
    with adaptive QP (xvcgpu_frame_pass_aqp): qp is then the picture's QP, every 64x64 CTU
    gets qp + its delta, derived on the device from orig in front of the search and written
    into this object's job arrays; whole pictures, forms `fwd_transform`, `residual` and
    `residual_rdoq` (else ValueError).  ctu_delta_qp() and cu_qp() read the last run's map
    back.

    affine=True: the pass with affine motion (xvcgpu_frame_pass_affine): every CU with both
    sides above 8 is searched a second time with the three-corner model, bootstrapped from
    its translational vector, and keeps the cheaper state (InterSearch::CompressInter).
    Whole pictures, the forms with a prediction picture (`fwd_transform`, `residual`,
    `residual_rdoq`; else ValueError), not together with aqp_strength and not through
    run_multi.  affine_mvp: the jobs' corner predictors [n_cus, 3, 2]; None: the plain
    job's mvp at every corner.  side_bits: 1, a picture with one list.  affine_choice()
    reads the last run's records back.

    merge_cands=: the pass with merge mode (xvcgpu_frame_pass_merge): five candidate motions
    per CU - list 0's vectors [n_cus, 5, 2] int32 in 1/16 pel, unclipped, in merge-index
    order, or api.FP_MERGE_CAND_DTYPE [n_cus, 5] -, an input as a job's mvp is.  Behind the
    search every listed CU ranks them (SearchMergeCandidates) and takes the best where its
    closed-form price is not above the searched state's; a merge CU without levels is a skip
    CU.  Every form, grid or partition, whole pictures; not together with affine, aqp_strength,
    run_multi or a row_range (ValueError).  merge_order: None, every CU, or the ascending
    indices of the CUs that try merge.  merge_side_bits: the merge flag's bit.
    merge_lambda_sqrt: None, sqrt(0.57 * 2^((qp - 12) / 3)) in double, or the picture's.
    merge_rank(), merge_choice() and chosen_results() read the last run's records back;
    results() keeps the search's answer."""

    def __init__(self, ctx, width, height, bitdepth=10, qp=32, cu=16,
                 search_range=96, row_range=None, fused=True, keep_levels=False,
                 rdoq=False, rdoq_packed=None, xcd_tiles=False, partition=None, form=None,
                 aqp_strength=None, affine=False, affine_mvp=None, side_bits=1,
                 merge_cands=None, merge_side_bits=1, merge_lambda_sqrt=None, merge_order=None,
                 desc=None):
        """desc: the FrameDescriptors of exactly these arguments, where the caller has made
        them already (None: made here)."""
        self.ctx = ctx
        self.plan = None
        self.aqp = None
        self.affine = None
        self.merge = None
        if merge_cands is not None:     # (refusals before anything is allocated)
            if affine:
                raise ValueError("merge_cands and affine: not together (out of scope)")
            if aqp_strength is not None:
                raise ValueError("merge_cands and aqp_strength: not together (out of scope)")
            if not (row_range is None or (max(0, row_range[0]), min(height, row_range[1])) ==
                    (0, height)):
                raise ValueError("merge_cands and row_range: whole pictures only")
            if merge_lambda_sqrt is None:
                merge_lambda_sqrt = lambda_sqrt_for_qp(qp)
            if not (math.isfinite(merge_lambda_sqrt) and merge_lambda_sqrt >= 0):
                raise ValueError("merge_lambda_sqrt: a finite value not below 0 expected")
        self.rdoq = rdoq
        # RDOQ keeps only a few lanes of a wave busy per block, so its own kernel
        # packs several blocks into a wave (xvcgpu_quant_rdo_batch) between the
        # forward and the inverse half of the residual pipeline: 5 launches instead
        # of the one fused launch, an order of magnitude less time
        self.rdoq_packed = rdoq and (fused if rdoq_packed is None else rdoq_packed)
        if self.rdoq_packed:
            keep_levels = True
        # keep_levels: also store the quantised coefficients of every TU (what
        # the entropy coder - or DecodePass - consumes); needs the unfused path
        self.fused = fused and width % 8 == 0 and height % 8 == 0 and not keep_levels \
            and not self.rdoq_packed
        self.w, self.h, self.bd = width, height, bitdepth
        self.desc = d = desc if desc is not None else FrameDescriptors(
            width, height, qp, cu, search_range, row_range, rdoq, bitdepth, xcd_tiles, partition)
        # the kernels that take a CU whole hold CUs of 8 ... 16 samples a side (the grid
        # goes by its nominal side: what the picture edge cuts off a CU does not count)
        max_side, small_side = (d.max_side, d.min_side) if partition is not None else (cu, cu)
        whole_cu_kernels = max_side <= 16 and (small_side >= 8 or partition is None)
        # the form (api.FP_FORM_NAMES) of the launches between the search and the tail
        if whole_cu_kernels and self.fused:
            self.form = "recon_from_me"     # fused: QuantFast or the RDOQ kernel
        elif whole_cu_kernels and self.rdoq_packed:
            self.form = "fwd_from_me"       # packed RDOQ
        elif self.rdoq_packed:
            self.form = "fwd_transform"     # packed RDOQ behind mc_from_me
        else:
            self.form = "residual_rdoq" if rdoq else "residual"
        if form is not None and form != self.form:
            if (self.form, form) != ("fwd_from_me", "fwd_transform"):
                raise ValueError("form %r: these shapes and settings run %r" % (form, self.form))
            self.form = form
        if aqp_strength is not None:
            if self.form not in _AQP_FORMS:
                raise ValueError("aqp_strength: the form %r builds its transform blocks from "
                                 "one QP inside its kernels; adaptive QP runs %s" %
                                 (self.form, ", ".join(_AQP_FORMS)))
            if d.row_range != (0, d.h):
                raise ValueError("aqp_strength: whole pictures only (no row_range)")
            aqp_table(qp, bitdepth, aqp_strength, width)    # (a refused strength: before
            #                                                  anything is allocated)
        if affine:
            if aqp_strength is not None:
                raise ValueError("affine: not together with aqp_strength (out of scope)")
            if self.form not in _AQP_FORMS:
                raise ValueError("affine: the form %r predicts inside its kernels; a pass with "
                                 "affine motion runs %s (fused=False, keep_levels=True or "
                                 "form=\"fwd_transform\")" % (self.form, ", ".join(_AQP_FORMS)))
            if d.row_range != (0, d.h):
                raise ValueError("affine: whole pictures only (no row_range)")
        if merge_cands is not None:     # (a refused array: before anything is allocated)
            merge_cands = merge_cand_array(merge_cands, d.n_cus)
            merge_order = merge_order_array(merge_order, d.n_cus)
        self.d_rdoq_ctx = ctx.buffer(d.rdoq_contexts) if rdoq else None
        self.d_rdoq_prm = ctx.buffer(d.rdoq_params) if rdoq else None
        self.d_me = ctx.buffer(d.me)
        # the searches are the CUs of the grid: on the 16-sample grid (almost) all 16x16
        # (the hint only where it is true: the jobs of any other shape go, 64 per wave and one
        # after the other, through the leftover kernel - a pass of 8x8 CUs would crawl)
        sq = (d.me["w"] == 16) & ((d.me["h"] == 16) | (d.me["h"] == 8)) if len(d.me) else np.zeros(0, bool)
        self.me_flags = api.ME_FULLPEL | api.ME_SUBPEL | \
            (api.ME_HINT_SQ16 if len(sq) and sq.mean() >= 0.98 else 0)
        if len(sq) and sq.all():     # ... all of them: no second kernel for other shapes
            self.me_flags |= api.ME_ONLY_SQ16
        self.d_tx = ctx.buffer(d.tx)
        # no block of the quantiser's general class (diagonal scan, 4x4 sub-blocks, sides up
        # to 32, at most sixteen sub-blocks): its launch can be left out (xvcgpu.h)
        t = d.tx
        self.tx_four_lane_only = bool(len(t)) and bool(
            ((t["w"] >= 4) & (t["h"] >= 4) & (t["w"] <= 32) & (t["h"] <= 32) &
             ((t["w"].astype(int) >> 2) * (t["h"].astype(int) >> 2) <= 16) &
             (((t["intra_pic"].astype(int) >> api.TXF_SCAN_SHIFT) & 3) == 0)).all())
        self.d_luma_idx = ctx.buffer(d.luma_idx)
        self.d_map = ctx.buffer(d.cu_map)
        self.d_res = ctx.alloc(api.MERES_DTYPE.itemsize * max(1, d.n_cus))
        self.d_nnz = ctx.alloc(4 * max(1, len(d.tx)))
        self.d_cus = ctx.alloc(api.CU_DTYPE.itemsize * d.n_cus_total)
        ctx._check(ctx.lib.xvcgpu_memset(ctx.h, self.d_cus.ptr, 0,
                                         api.CU_DTYPE.itemsize * d.n_cus_total))
        self.d_ssd = ctx.alloc(16)
        self.pred = ctx.picture(width, height, bitdepth)
        # whole pictures of CUs >= 8x8 end with ONE launch (xvcgpu_deblock_pad_ssd:
        # unfiltered reconstruction in `scratch` -> deblocked, padded `rec` + SSD)
        # instead of deblock V, H, pad, SSD, SSD fold
        if partition is not None:
            self.plan = ctx.me_plan(self.d_me.ptr, d.n_cus, d.cu_size)
            bad = int(self.plan.counts[api.ME_PLAN_BIN_NAMES.index("unsupported")])
            if bad:
                # (a side the picture edge cut to 12, 24, ...: check_partition lets it
                # through, the search would answer it with the unsupported record)
                odd = [p for p in d.partition if (p[2] & (p[2] - 1)) or (p[3] & (p[3] - 1))]
                self.scratch = self.d_levels = self.d_level_off = self.d_coeffs = None
                self.destroy()
                raise ValueError("partition: the motion search has no instance for %d CUs "
                                 "(sides must be 4, 8, 16, 32 or 64), first (x, y, w, h) = %r"
                                 % (bad, odd[0] if odd else None))
        self.fused_tail = small_side >= 8 and width % 8 == 0 and height % 8 == 0 and \
            d.row_range == (0, d.h) and os.environ.get("XVC_TAIL_FUSED", "1") != "0"
        self.scratch = ctx.picture(width, height, bitdepth) if self.fused_tail else None
        self.d_levels, self.d_level_off, self.n_levels = None, None, 0
        if keep_levels:
            off, total = ctx.level_offsets(d.tx)
            self.d_level_off = ctx.buffer(off)
            self.d_levels = ctx.alloc(2 * max(1, total))
            self.n_levels = total
        self.d_coeffs = ctx.alloc(2 * max(1, self.n_levels)) if self.rdoq_packed else None
        if self.rdoq_packed:    # no allocation inside the passes (they may be recorded)
            ctx._check(ctx.lib.xvcgpu_quant_rdo_reserve(ctx.h, len(d.tx), self.n_levels))
        if aqp_strength is not None:
            self.aqp = _AqpArrays(ctx, d, bitdepth, aqp_strength)
        if affine:
            self.affine = _AffineArrays(ctx, d, affine_mvp, side_bits)
        if merge_cands is not None:
            self.merge = _MergeArrays(ctx, d, merge_cands, merge_order, side_bits,
                                      merge_side_bits, merge_lambda_sqrt)

    @property
    def d_cus_own(self):
        return self.d_cus.ptr + api.CU_DTYPE.itemsize * self.desc.cu_base

    def _args(self):
        """The picture-per-call argument block (xvcgpu_frame_pass), built once and
        never written after: a call fills a copy (_call_args)."""
        if getattr(self, "_fp_args", None) is None:
            d, a = self.desc, api.FramePassArgs()
            a.d_me, a.d_results, a.n_cus = self.d_me.ptr, self.d_res.ptr, d.n_cus
            a.max_block_size, a.qp_y, a.qp_c = d.cu_size, d.qp, d.qp_c
            a.d_nnz, a.d_cus_own, a.d_cus = self.d_nnz.ptr, self.d_cus_own, self.d_cus.ptr
            a.n_cus_total, a.d_cu_map = d.n_cus_total, self.d_map.ptr
            a.map_stride = d.cu_map.shape[1]
            a.db_y_begin, a.db_y_end, a.dbh_y_end = 0, d.h, d.h
            a.scratch_rec = self.scratch.h_pic if self.scratch is not None else None
            a.ssd_y_begin, a.ssd_y_end = 0, 1 << 30
            a.shift_bitdepth, a.d_ssd = self.bd, self.d_ssd.ptr
            a.form = api.FP_FORM_NAMES.index(self.form)
            if self.rdoq:
                a.d_rdoq_contexts, a.d_rdoq_params = self.d_rdoq_ctx.ptr, self.d_rdoq_prm.ptr
            if self.form != "recon_from_me":    # the fields of the other forms (xvcgpu.h)
                a.pred, a.d_tx, a.n_tx = self.pred.h_pic, self.d_tx.ptr, len(d.tx)
                a.d_luma_tx_index = self.d_luma_idx.ptr
                if self.d_levels is not None:
                    a.d_level_off, a.d_levels = self.d_level_off.ptr, self.d_levels.ptr
            if self.rdoq_packed:
                a.d_coeffs, a.n_coeffs = self.d_coeffs.ptr, self.n_levels
            a.tx_four_lane_only = int(self.tx_four_lane_only)
            a.me_shape = self.me_flags & (api.ME_HINT_SQ16 | api.ME_ONLY_SQ16)
            self._fp_args = a
        return self._fp_args

    def _call_args(self, orig, ref, rec, ref_poc=0):
        """A copy of _args() with one call's pictures and reference POC."""
        a = api.FramePassArgs.from_buffer_copy(self._args())
        a.orig = orig.h_pic if orig is not None else None
        a.ref = ref.h_pic if ref is not None else None
        a.rec, a.ref_poc = rec.h_pic, ref_poc
        return a

    def run_phases(self, orig, ref, rec, phases, ref_poc=0, rows=None, dbh_end=None,
                   ssd_rows=None, d_ssd=None, fused_tail=True):
        """One call for the selected phases (api.FP_*).  fused_tail=False: end with the
        separate deblocking, padding and SSD launches also where the one launch applies."""
        a = self._call_args(orig, ref, rec, ref_poc)
        if not fused_tail:
            a.scratch_rec = None
        if rows is not None:
            a.db_y_begin, a.db_y_end = rows
            a.dbh_y_end = dbh_end if dbh_end is not None else rows[1]
        if ssd_rows is not None:
            a.ssd_y_begin, a.ssd_y_end = ssd_rows
        if d_ssd is not None:
            a.d_ssd = d_ssd
        if self.aqp is not None:
            q = self.aqp.args()
            self.ctx._check(self.ctx.lib.xvcgpu_frame_pass_aqp(
                self.ctx.h, C.byref(a), C.byref(q), self.plan.h if self.plan is not None else None,
                phases))
            return
        if self.affine is not None:
            f = self.affine.args()
            self.ctx._check(self.ctx.lib.xvcgpu_frame_pass_affine(
                self.ctx.h, C.byref(a), C.byref(f), self.plan.h if self.plan is not None else None,
                phases))
            return
        if self.merge is not None:
            m = self.merge.args()
            self.ctx._check(self.ctx.lib.xvcgpu_frame_pass_merge(
                self.ctx.h, C.byref(a), C.byref(m), self.plan.h if self.plan is not None else None,
                phases))
            return
        if self.plan is not None:
            self.ctx._check(self.ctx.lib.xvcgpu_frame_pass_planned(self.ctx.h, C.byref(a),
                                                                   self.plan.h, phases))
            return
        self.ctx._check(self.ctx.lib.xvcgpu_frame_pass(self.ctx.h, C.byref(a), phases))

    def _launches(self, orig, ref, rec, ref_poc, fused_tail):
        """The pass's launches as (name, callable) in issue order, split into the
        encode part (search -> prediction, transform, quantiser, reconstruction ->
        CU metadata of the own CUs; empty without CUs) and the tail (deblocking,
        padding, SSD).  fused_tail: the encode part reconstructs into `scratch` and
        the tail is the one deblock_pad_ssd launch from there into rec.
        The quant_rdo launches run without the promise xvcgpu_frame_pass gives the
        quantiser for its batch (tx_four_lane_only: the general-class launch left
        out), so that bench.py's per-kernel times stay what they were.
        "quant_rdo" is the class lists and the walk: rdoq_lists_kernel (one launch; batches
        above XVCGPU_RDOQ_ONE_LAUNCH_LISTS_MAX_BLOCKS: rdoq_count_kernel + rdoq_scatter_kernel,
        xvcgpu_quant_rdo_set_list_form) -> quant_rdo_packed4_kernel [-> quant_rdo_packed_kernel]."""
        if self.affine is not None:     # (these are the flat pass's launches)
            raise ValueError("a pass with affine motion runs through run() / run_phases() only")
        if self.merge is not None:
            raise ValueError("a pass with merge mode runs through run() / run_phases() only")
        ctx, d, lib = self.ctx, self.desc, self.ctx.lib
        n, T, bd, form = d.n_cus, len(d.tx), self.bd, self.form
        out = self.scratch if fused_tail else rec
        me, res, nnz, cus = self.d_me.ptr, self.d_res.ptr, self.d_nnz.ptr, self.d_cus_own
        lv = self.d_levels.ptr if self.d_levels else None
        lo = self.d_level_off.ptr if self.d_level_off else None
        rq = (self.d_rdoq_ctx.ptr, self.d_rdoq_prm.ptr) if self.rdoq else ()
        all_cus, stride = self.d_cus.ptr, d.cu_map.shape[1]
        if fused_tail:
            tail = [("deblock_pad_ssd", lambda: ctx.deblock_pad_ssd_dev(
                out, rec, orig, all_cus, d.n_cus_total, self.d_map.ptr, stride, 0, 0, 0, bd,
                self.d_ssd.ptr))]
        else:
            tail = [("deblock", lambda: ctx.deblock_dev(rec, all_cus, d.n_cus_total,
                                                        self.d_map.ptr, stride, 0, 0, 0, 4)),
                    ("pad_border", lambda: ctx.pad_border(rec)),
                    ("picture_ssd", lambda: ctx.picture_ssd_dev(orig, rec, 0, bd,
                                                                self.d_ssd.ptr))]
        if n == 0:
            return [], tail
        if self.plan is not None:
            enc = [("me_search", lambda: ctx.me_search_planned(
                orig, ref, api.ME_FULLPEL | api.ME_SUBPEL, self.plan, res))]
        else:
            enc = [("me_search", lambda: ctx.me_search_dev(orig, ref, self.me_flags, me, n, res,
                                                           d.cu_size))]
        if form == "recon_from_me":
            # MC + transform/quant/recon + CU metadata in one launch; the prediction
            # never leaves LDS
            recon = ctx.recon_from_me_rdoq_dev if self.rdoq else ctx.recon_from_me_dev
            enc.append(("recon_from_me", lambda: recon(orig, ref, out, me, res, n, d.qp, d.qp_c,
                                                       ref_poc, nnz, cus, *rq)))
        elif form == "fwd_from_me":
            # the prediction goes into the reconstruction's picture, the inverse half then
            # works in place (and skips the blocks without levels); on the way the kernel
            # classifies the blocks for the quantiser, proves with the quantiser's contexts
            # which are all zero (xvcgpu_quant_rdo_set_prove_zero) and writes the CU records
            co, nc = self.d_coeffs.ptr, C.c_size_t(self.n_levels)
            enc += [
                ("fwd_from_me", lambda: ctx._check(lib.xvcgpu_fwd_from_me_classify_prove(
                    ctx.h, orig.h_pic, ref.h_pic, out.h_pic, me, res, n, d.qp, d.qp_c, ref_poc,
                    co, lo, nc, lv, nnz, cus, *rq))),
                ("quant_rdo", lambda: ctx._check(lib.xvcgpu_quant_rdo_classified_batch(
                    ctx.h, bd, self.d_tx.ptr, T, co, lo, nc, lv, nnz, *rq, cus))),
                # blocks 3 * cu + comp: U and V of a CU share a wave
                ("inv_transform", lambda: ctx._check(lib.xvcgpu_inv_transform_cu_order(
                    ctx.h, out.h_pic, self.d_tx.ptr, n, lv, lo, nnz)))]
        else:
            enc.append(("mc_from_me", lambda: ctx.mc_from_me_dev(ref, self.pred, me, res, n)))
            if form == "fwd_transform":
                co, nc = self.d_coeffs.ptr, C.c_size_t(self.n_levels)
                enc += [
                    ("fwd_transform", lambda: ctx._check(lib.xvcgpu_fwd_transform_batch(
                        ctx.h, orig.h_pic, self.pred.h_pic, self.d_tx.ptr, T, co, lo))),
                    ("quant_rdo", lambda: ctx._check(lib.xvcgpu_quant_rdo_batch(
                        ctx.h, bd, self.d_tx.ptr, T, co, lo, nc, lv, nnz, *rq))),
                    ("inv_transform", lambda: ctx._check(lib.xvcgpu_inv_transform_batch(
                        ctx.h, self.pred.h_pic, out.h_pic, self.d_tx.ptr, T, lv, lo, nnz)))]
            elif form == "residual_rdoq":
                enc.append(("residual_rdoq", lambda: ctx.residual_rdoq_batch_dev(
                    orig, self.pred, out, self.d_tx.ptr, T, lv, lo, nnz, *rq)))
            else:
                enc.append(("residual", lambda: ctx.residual_batch_dev(
                    orig, self.pred, out, self.d_tx.ptr, T, lv, lo, nnz)))
            enc.append(("cu_info", lambda: ctx.cu_info_from_me_dev(
                me, res, nnz, self.d_luma_idx.ptr, n, d.qp, d.qp_c, ref_poc, cus)))
        return enc, tail

    def encode(self, orig, ref, rec, ref_poc=0):
        """ME -> MC -> residual -> CU metadata for the own CUs (asynchronous)."""
        for _, fn in self._launches(orig, ref, rec, ref_poc, False)[0]:
            fn()

    def kernel_steps(self, orig, ref, rec, ref_poc=0):
        """The launches of one frame pass as (name, callable) in issue order - for
        per-kernel timing (bench.py); run in order they are a frame pass."""
        enc, tail = self._launches(orig, ref, rec, ref_poc, self.fused_tail)
        return enc + tail

    def deblock_rows(self, rec, pass_, y0, y1):
        d = self.desc
        self.ctx.deblock_rows_dev(rec, self.d_cus.ptr, d.n_cus_total, self.d_map.ptr,
                                  d.cu_map.shape[1], pass_, y0, y1)

    def run(self, orig, ref, rec, ref_poc=0, deblock=True, pad=True, ssd=True, fused_tail=True):
        """Enqueue one whole-picture frame pass (asynchronous)."""
        if self.desc.row_range == (0, self.desc.h):
            # the whole sequence behind one C call (xvcgpu_frame_pass), whatever the form
            self.run_phases(orig, ref, rec, api.FP_ENCODE |
                            (api.FP_DEBLOCK_V | api.FP_DEBLOCK_H if deblock else 0) |
                            (api.FP_PAD if pad else 0) | (api.FP_SSD if ssd else 0), ref_poc,
                            fused_tail=fused_tail)
            return
        enc, tail = self._launches(orig, ref, rec, ref_poc,
                                   self.fused_tail and deblock and pad and ssd)
        skip = {"deblock": not deblock, "pad_border": not pad, "picture_ssd": not ssd}
        for name, fn in enc + tail:
            if not skip.get(name):
                fn()

    def results(self):
        d = self.desc
        return (self.d_res.to_array(api.MERES_DTYPE, d.n_cus),
                self.d_nnz.to_array(np.int32, len(d.tx)),
                self.d_cus.to_array(api.CU_DTYPE, d.n_cus_total),
                self.d_ssd.to_array(np.uint64, 2))

    def ctu_delta_qp(self):
        """Adaptive QP: the last run's delta per CTU, [rows, columns] int8."""
        return self.aqp.ctu_delta_qp()

    def cu_qp(self):
        """Adaptive QP: the last run's (qp_y, qp_c) per CU, [n_cus, 2] int8."""
        return self.aqp.cu_qp()

    def affine_choice(self):
        """Affine motion: the last run's api.FP_AFFINE_RESULT_DTYPE record per CU."""
        return self.affine.choice()

    def merge_rank(self):
        """Merge mode: the last run's api.FP_MERGE_RANK_DTYPE record per CU (the CUs outside
        the list: as allocated, zero)."""
        return self.merge.d_rank.to_array(api.FP_MERGE_RANK_DTYPE, self.desc.n_cus)

    def merge_choice(self):
        """Merge mode: the last run's api.FP_MERGE_RESULT_DTYPE record per CU."""
        return self.merge.d_choice.to_array(api.FP_MERGE_RESULT_DTYPE, self.desc.n_cus)

    def chosen_results(self):
        """Merge mode: the results the pass behind the search ran on (api.MERES_DTYPE)."""
        return self.merge.d_chosen.to_array(api.MERES_DTYPE, self.desc.n_cus)

    def destroy(self):
        if self.aqp is not None:
            self.aqp.free()
            self.aqp = None
        if self.merge is not None:
            self.merge.free()
            self.merge = None
        if self.affine is not None:
            self.affine.free()
            self.affine = None
        for b in (self.d_me, self.d_tx, self.d_luma_idx, self.d_map, self.d_res,
                  self.d_nnz, self.d_cus, self.d_ssd, self.d_levels, self.d_level_off,
                  self.d_rdoq_ctx, self.d_rdoq_prm, self.d_coeffs):
            if b is not None:
                b.free()
        self.pred.destroy()
        if self.plan is not None:
            self.plan.destroy()
            self.plan = None
        if self.scratch is not None:
            self.scratch.destroy()
            self.scratch = None


def ref_list_tables(cur_poc, ref_pocs):
    """What a B picture's two POC lists say as xvcgpu_frame_pass_bi_refs wants it:
    (same_poc_in_l0 per list-1 picture - the first list-0 index of the same POC, or -1,
    ReferencePictureLists::GetSamePocMappingFor -, the distinct POCs in order of first
    mention, slot[l][r] into them, force_l1_mvd_zero - every reference before the picture,
    PictureData::DetermineForceBipredL1MvdZero)."""
    l0, l1 = (list(int(v) for v in ref_pocs[l]) for l in range(2))
    same = [l0.index(v) if v in l0 else -1 for v in l1]
    distinct = []
    for v in l0 + l1:
        if v not in distinct:
            distinct.append(v)
    slot = [[distinct.index(v) for v in l] for l in (l0, l1)]
    return same, distinct, slot, all(v < cur_poc for v in l0 + l1)


class BiRefsFramePass:
    """The frame pass of a B picture whose lists name 1 .. api.CS_MAX_REFS pictures each
    (xvcgpu_frame_pass_bi_refs): one search per picture that list 0 has not searched
    already, the SearchBiIterative step into every picture of the list that lost (by block
    class, through the plan on a partition), the choice against the best unique list-1
    picture, prediction from the chosen pictures, the residual pipeline and the B tail - one
    C call, nothing read back in between.  One refinement iteration, closed-form side bits
    (side_bits = uni L0, uni L1, bi).

    The forms are those with a prediction picture: `residual`, `residual_rdoq`, or
    `fwd_transform` for packed RDOQ; the quantiser's contexts are those of a B picture
    (rdoq_init_contexts(qp, 0)).  The state every (list, picture) shares - descriptors,
    transform blocks, CU records, scratch - is a FramePass's (self.p).

    ref_pocs = [[list 0's POCs], [list 1's]] with cur_poc give same_poc_in_l0, the slot
    table and force_l1_mvd_zero (ref_list_tables); a picture with only back references is
    refused here.  run(orig, refs, rec): refs = [[list 0's pictures], [list 1's]] in the
    lists' order, the same object where the lists name the same POC.  me[l][r] / d_me[l][r]:
    the search jobs per (list, picture), copies of the descriptors until set_jobs.

    low_delay=True: the pass of a picture whose references all lie before it
    (xvcgpu_frame_pass_bi_back; every inter picture of a low-delay encode) - list 1's
    candidate per picture is the job's predictor itself, priced on the device into
    d_l1_mvp_cost (l1_mvp_cost()), list 0 is refined against it, a bi-directional CU codes
    list 1 without a vector difference.  It accepts only such lists.

    affine=True: the pass with affine motion (xvcgpu_frame_pass_bi_refs_affine): behind the
    plain run every CU with both sides in 16, 32, 64 is searched with the three-corner model
    into every picture of both lists and refined as SearchBiIterative does, and keeps the
    cheaper state (the plain one on a tie).  Not together with low_delay or aqp_strength.
    affine_mvp: the jobs' corner predictors [l][r] -> [n_cus, 3, 2]; None: the plain job's
    mvp at every corner.  affine_choice(), affine_uni_results(), affine_bi_results(),
    affine_jobs(), affine_bi_jobs(): the last run's records.

    merge_cands: the pass with merge mode (xvcgpu_frame_pass_bi_refs_merge): five candidates
    per CU in merge-index order - a pair (ref_idx [n_cus, 5, 2], mv [n_cus, 5, 2, 2]): per list
    the picture's index in that list, -1 for an unused list, and its vector in 1/16 pel,
    unclipped; or api.FP_MERGE_CAND_DTYPE [n_cus, 5] -, an input as a job's mvp is.  Behind the
    plain choice the listed CUs (merge_order: strictly ascending CU indices; None: every CU)
    are ranked - a candidate of both lists is bi-predicted in the rank kernel's LDS - and a CU
    takes its best candidate where that costs no more than its plain choice.  The prediction,
    the CU records and the tail are the winners'; results()' choice records stay the plain
    run's.  merge_side_bits: the bits of a merge CU in front of its index; merge_lambda_sqrt:
    the ranking's double, None: lambda_sqrt_for_qp(qp).  Not together with affine,
    aqp_strength or low_delay.  merge_rank(), merge_choice(), chosen_results(): the last
    run's records."""

    def __init__(self, ctx, width, height, bitdepth=10, qp=32, cu=16, rdoq=False,
                 rdoq_packed=None, keep_levels=False, partition=None, cur_poc=8,
                 ref_pocs=((4,), (12,)), search_range=96, side_bits=(3, 3, 5),
                 aqp_strength=None, low_delay=False, affine=False, affine_mvp=None,
                 merge_cands=None, merge_side_bits=1, merge_lambda_sqrt=None, merge_order=None):
        self.ctx = ctx
        self.aqp = None
        self.affine = None
        self.merge = None
        desc = None
        if merge_cands is not None:
            for on, name in ((affine, "affine"), (aqp_strength is not None, "aqp_strength"),
                             (low_delay, "low_delay")):
                if on:
                    raise ValueError("merge_cands: not together with %s (out of scope)" % name)
            if merge_lambda_sqrt is None:
                merge_lambda_sqrt = lambda_sqrt_for_qp(qp)
            if not (np.isfinite(merge_lambda_sqrt) and merge_lambda_sqrt >= 0):
                raise ValueError("merge_lambda_sqrt must be finite and not below 0")
            if merge_side_bits < 0:
                raise ValueError("merge_side_bits must not be below 0")
            # the pass's descriptors, made here (on the host) so that a refused array is
            # refused before anything is allocated; the FramePass below takes these
            desc = FrameDescriptors(width, height, qp, cu, search_range, None, rdoq, bitdepth,
                                    False, partition)
            merge_cands = bi_merge_cand_array(merge_cands, desc.n_cus)
            merge_order = merge_order_array(merge_order, desc.n_cus)
        if affine and low_delay:
            raise ValueError("affine: not together with low_delay (force_l1_mvd_zero): pricing "
                             "list 1's affine predictor is a pass of its own")
        if affine and aqp_strength is not None:
            raise ValueError("affine: not together with aqp_strength (out of scope)")
        self.low_delay = bool(low_delay)
        self.d_l1_mvp_cost = None
        if aqp_strength is not None:    # (a refused strength: before anything is allocated)
            aqp_table(qp, bitdepth, aqp_strength, width)
        self.cur_poc, self.side_bits = cur_poc, tuple(side_bits)
        self.ref_pocs = [list(ref_pocs[0]), list(ref_pocs[1])]
        self.num_ref = [len(l) for l in self.ref_pocs]
        if not all(1 <= k <= api.CS_MAX_REFS for k in self.num_ref):
            raise ValueError("ref_pocs: 1 .. %d pictures per list" % api.CS_MAX_REFS)
        self.same, self.distinct, self.slot, force = ref_list_tables(cur_poc, self.ref_pocs)
        if low_delay and not force:
            raise ValueError("ref_pocs %r with low_delay: every reference must lie before POC "
                             "%d (force_l1_mvd_zero)" % (self.ref_pocs, cur_poc))
        if force and not low_delay:
            raise ValueError("ref_pocs %r lie all before POC %d: a picture with only back "
                             "references (force_l1_mvd_zero) is out of this pass's scope"
                             % (self.ref_pocs, cur_poc))
        self.rmax = max(self.num_ref)
        self.p = p = FramePass(ctx, width, height, bitdepth, qp, cu, search_range, None, True,
                               keep_levels, rdoq, rdoq_packed, False, partition, desc=desc)
        self.desc = d = p.desc
        p.form = "fwd_transform" if p.rdoq_packed else ("residual_rdoq" if rdoq else "residual")
        self.form = p.form
        if rdoq:
            d.rdoq_contexts = rdoq_init_contexts(qp, 0)
            ctx.h2d(p.d_rdoq_ctx.ptr, d.rdoq_contexts)
        n = max(1, d.n_cus)
        self.searched = [[l == 0 or self.same[r] < 0 for r in range(self.num_ref[l])]
                         for l in range(2)]
        self.me = [[d.me.copy() for _ in range(self.num_ref[l])] for l in range(2)]
        self.d_me = [[ctx.buffer(m) for m in self.me[l]] for l in range(2)]
        self.d_res = [[ctx.alloc(api.MERES_DTYPE.itemsize * n) if s else None
                       for s in self.searched[l]] for l in range(2)]
        self.d_bi_jobs = ctx.alloc(api.BI_DTYPE.itemsize * n * self.rmax)
        self.d_bi_res = ctx.alloc(api.MERES_DTYPE.itemsize * n * self.rmax)
        self.d_bi_slots = ctx.alloc(2 * n * self.rmax)
        self.d_choice = ctx.alloc(api.FP_BI_REFS_RESULT_DTYPE.itemsize * n)
        self.d_inter = ctx.alloc(api.INTER_DTYPE.itemsize * 3 * n)
        if low_delay:
            self.d_l1_mvp_cost = ctx.alloc(4 * api.CS_MAX_REFS * n)
        self.plans = [[None] * self.num_ref[l] for l in range(2)]
        if aqp_strength is not None:    # (every form of this pass is one adaptive QP runs)
            self.aqp = _AqpArrays(ctx, d, bitdepth, aqp_strength)
        if p.plan is not None:
            for l in range(2):
                for r in range(self.num_ref[l]):
                    if self.searched[l][r]:
                        self.plans[l][r] = ctx.me_plan(self.d_me[l][r].ptr, d.n_cus, d.cu_size)
        self.affine_mvp = affine_mvp
        if affine:
            self.affine = _BiAffineArrays(ctx, d.n_cus, self.me, self.same, self.slot, affine_mvp)
        if merge_cands is not None:
            self.merge = _BiMergeArrays(ctx, d, merge_cands, merge_order, merge_side_bits,
                                        merge_lambda_sqrt)

    def set_jobs(self, me):
        """New search jobs me[l][r] (predictors, flags, lambda, range; the shapes stay);
        None keeps an entry."""
        for l in range(2):
            for r in range(self.num_ref[l]):
                new, old = me[l][r], self.me[l][r]
                if new is not None:
                    assert all(np.array_equal(new[k], old[k]) for k in ("x", "y", "w", "h"))
                    old[...] = new
                    self.ctx.h2d(self.d_me[l][r].ptr, old)
        if self.affine is not None and self.desc.n_cus:    # (lambda and the default mvp follow)
            f = self.affine
            f.jobs, f.slots, f.order, f.n_class = bi_affine_jobs(self.me, self.same, self.slot,
                                                                 self.affine_mvp)
            self.ctx.h2d(f.d_uni.ptr, f.jobs)
            if f.d_order is not None:
                f.d_order.free()
            f.d_order = self.ctx.buffer(f.order) if len(f.order) else None

    def _distinct_pictures(self, refs):
        pics = [None] * len(self.distinct)
        for l in range(2):
            assert len(refs[l]) == self.num_ref[l]
            for r, pic in enumerate(refs[l]):
                k = self.slot[l][r]
                assert pics[k] is None or pics[k] is pic, \
                    "the lists name POC %d with two different pictures" % self.distinct[k]
                pics[k] = pic
        return pics

    def _call_args(self, orig, refs, rec):
        a = api.FramePassBiRefsArgs()
        a.p = self.p._call_args(orig, None, rec, 0)
        pics = self._distinct_pictures(refs)
        a.n_refs = len(pics)
        for k, pic in enumerate(pics):
            a.refs[k] = pic.h_pic if pic is not None else None
        a.force_l1_mvd_zero = int(self.low_delay)
        for r in range(api.CS_MAX_REFS):
            a.same_poc_in_l0[r] = self.same[r] if r < self.num_ref[1] else -1
        for l in range(2):
            a.num_ref[l] = self.num_ref[l]
            for r in range(self.num_ref[l]):
                a.slot[l][r], a.ref_poc[l][r] = self.slot[l][r], self.ref_pocs[l][r]
                a.d_me[l][r] = self.d_me[l][r].ptr
                a.d_results[l][r] = self.d_res[l][r].ptr if self.searched[l][r] else None
        a.side_bits_uni[0], a.side_bits_uni[1], a.side_bits_bi = self.side_bits
        a.d_bi_jobs, a.d_bi_results = self.d_bi_jobs.ptr, self.d_bi_res.ptr
        a.d_bi_slots, a.d_choice, a.d_inter = self.d_bi_slots.ptr, self.d_choice.ptr, \
            self.d_inter.ptr
        return a

    def plan_handles(self, use=True):
        """plans[2][CS_MAX_REFS] as the C call takes it (use=False: all NULL)."""
        h = ((C.c_void_p * api.CS_MAX_REFS) * 2)()
        for l in range(2):
            for r, plan in enumerate(self.plans[l]):
                h[l][r] = plan.h if use and plan is not None else None
        return h

    def run(self, orig, refs, rec, fused_tail=True, planned=True):
        """Enqueue one whole-picture B pass (asynchronous).  fused_tail=False: end with the
        separate deblocking, padding and SSD launches also where the one launch applies;
        planned=False: sized searches and whole-list class launches also on a partition."""
        a = self._call_args(orig, refs, rec)
        if not fused_tail:
            a.p.scratch_rec = None
        phases = api.FP_ENCODE | api.FP_DEBLOCK_V | api.FP_DEBLOCK_H | api.FP_PAD | api.FP_SSD
        if self.low_delay:
            q = self.aqp.args() if self.aqp is not None else None
            self.ctx._check(self.ctx.lib.xvcgpu_frame_pass_bi_back(
                self.ctx.h, C.byref(a), self.d_l1_mvp_cost.ptr,
                C.byref(q) if q is not None else None, self.plan_handles(planned), phases))
            return
        if self.aqp is not None:
            q = self.aqp.args()
            self.ctx._check(self.ctx.lib.xvcgpu_frame_pass_bi_refs_aqp(
                self.ctx.h, C.byref(a), C.byref(q), self.plan_handles(planned), phases))
            return
        if self.affine is not None:
            f = self.affine.args()
            self.ctx._check(self.ctx.lib.xvcgpu_frame_pass_bi_refs_affine(
                self.ctx.h, C.byref(a), C.byref(f), self.plan_handles(planned), phases))
            return
        if self.merge is not None:
            m = self.merge.args()
            self.ctx._check(self.ctx.lib.xvcgpu_frame_pass_bi_refs_merge(
                self.ctx.h, C.byref(a), C.byref(m), self.plan_handles(planned), phases))
            return
        self.ctx._check(self.ctx.lib.xvcgpu_frame_pass_bi_refs(
            self.ctx.h, C.byref(a), self.plan_handles(planned), phases))

    def kernel_steps(self, orig, refs, rec, fused_tail=None, planned=True):
        """The launches of one pass as (name, callable) in issue order, each through its own
        entry point: run in order they are the pass (per-launch timing, tests)."""
        ctx, lib, p, d = self.ctx, self.ctx.lib, self.p, self.desc
        fused_tail = p.fused_tail if fused_tail is None else fused_tail
        n, chk = d.n_cus, ctx._check
        a = self._call_args(orig, refs, rec)
        pics = self._distinct_pictures(refs)
        handles = (C.c_void_p * len(pics))(*[q.h_pic for q in pics])
        out = p.scratch if fused_tail else rec
        planned = planned and p.plan is not None
        steps = []

        def search(l, r):
            pic, res = refs[l][r], self.d_res[l][r].ptr
            if planned:
                return lambda: ctx.me_search_planned(orig, pic, api.ME_FULLPEL | api.ME_SUBPEL,
                                                     self.plans[l][r], res)
            return lambda: ctx.me_search_dev(orig, pic, p.me_flags, self.d_me[l][r].ptr, n, res,
                                             d.cu_size)

        def refine(cls):
            return lambda: chk(lib.xvcgpu_bipred_search_refs(
                ctx.h, orig.h_pic, handles, len(pics), self.d_bi_jobs.ptr, self.d_bi_slots.ptr,
                n * self.rmax, self.d_bi_res.ptr, cls))
        for l in range(2):
            for r in range(self.num_ref[l]):
                if self.searched[l][r]:
                    steps.append(("me_search_l%d_r%d" % (l, r), search(l, r)))
        if self.low_delay:
            cost = self.d_l1_mvp_cost.ptr
            steps += [
                ("l1_mvp_cost", lambda: chk(lib.xvcgpu_fp_bi_back_mvp_cost(ctx.h, C.byref(a),
                                                                           cost))),
                ("uni_fold", lambda: chk(lib.xvcgpu_fp_bi_back_uni_fold(ctx.h, C.byref(a), cost)))]
        else:
            steps.append(("uni_fold", lambda: chk(lib.xvcgpu_fp_bi_refs_uni_fold(ctx.h,
                                                                                 C.byref(a)))))
        if planned:
            first = next(q for q in self.plans[0] if q is not None)
            steps.append(("bipred_planned", lambda: chk(lib.xvcgpu_bipred_search_refs_planned(
                ctx.h, orig.h_pic, handles, len(pics), first.h, self.rmax, self.d_bi_jobs.ptr,
                self.d_bi_slots.ptr, self.d_bi_res.ptr))))
        else:
            steps += [("bipred_c%d" % cls, refine(cls)) for cls in (16, 32, 64)
                      if cls <= d.cu_size]
        choice = lib.xvcgpu_fp_bi_back_choice if self.low_delay else lib.xvcgpu_fp_bi_refs_choice
        steps.append(("choice", lambda: chk(choice(ctx.h, C.byref(a)))))
        if self.affine is not None:
            f, fa = self.affine, self.affine.args()
            order = f.d_order.ptr if f.d_order is not None else None
            n_class = (C.c_int32 * 3)(*f.n_class)

            def listed(jobs, slots, per_cu, res):
                return lambda: chk(lib.xvcgpu_affine_me_listed_refs(
                    ctx.h, orig.h_pic, handles, len(pics), jobs.ptr, slots.ptr, n, per_cu, order,
                    n_class, res.ptr))
            steps += [
                ("affine_boot", lambda: chk(lib.xvcgpu_fp_bi_affine_boot(ctx.h, C.byref(a),
                                                                         C.byref(fa)))),
                ("affine_uni", listed(f.d_uni, f.d_uni_slots, 2 * self.rmax, f.d_uni_res)),
                ("affine_uni_fold", lambda: chk(lib.xvcgpu_fp_bi_affine_uni_fold(
                    ctx.h, C.byref(a), C.byref(fa)))),
                ("affine_bi", listed(f.d_bi, f.d_bi_slots, self.rmax, f.d_bi_res)),
                ("affine_choice", lambda: chk(lib.xvcgpu_fp_bi_affine_choice(
                    ctx.h, C.byref(a), C.byref(fa))))]
        chosen = a
        if self.merge is not None:
            ma = self.merge.args()
            chosen = self._call_args(orig, refs, rec)
            chosen.d_choice = self.merge.d_chosen.ptr
            steps += [
                ("merge_rank", lambda: chk(lib.xvcgpu_fp_bi_merge_rank(ctx.h, C.byref(a),
                                                                       C.byref(ma)))),
                ("merge_choice", lambda: chk(lib.xvcgpu_fp_bi_merge_choice(ctx.h, C.byref(a),
                                                                           C.byref(ma))))]
        steps += [
            ("inter_pred", lambda: chk(lib.xvcgpu_inter_pred_batch(
                ctx.h, handles, len(pics), rec.h_pic, p.pred.h_pic, self.d_inter.ptr, 3 * n)))]
        # the form's residual pipeline: the P pass's launches between its prediction and
        # its CU records
        steps += p._launches(orig, pics[0], rec, 0, fused_tail)[0][2:-1]
        if self.affine is not None:
            steps.append(("cu_info", lambda: chk(lib.xvcgpu_cu_info_from_bi_affine_choice(
                ctx.h, C.byref(a), C.byref(fa)))))
        else:
            steps.append(("cu_info", lambda: chk(lib.xvcgpu_cu_info_from_choice_refs(
                ctx.h, C.byref(chosen)))))
        if self.merge is not None:
            steps.append(("merge_skip", lambda: chk(lib.xvcgpu_fp_bi_merge_skip(
                ctx.h, p.d_nnz.ptr, p.d_luma_idx.ptr, n, self.merge.d_choice.ptr))))
        all_cus, stride = p.d_cus.ptr, d.cu_map.shape[1]
        if fused_tail:
            return steps + [("deblock_pad_ssd", lambda: ctx.deblock_pad_ssd_dev(
                out, rec, orig, all_cus, d.n_cus_total, p.d_map.ptr, stride, 1, 0, 0, p.bd,
                p.d_ssd.ptr))]
        return steps + [
            ("deblock", lambda: ctx.deblock_dev(rec, all_cus, d.n_cus_total, p.d_map.ptr,
                                                stride, 1, 0, 0, 4)),
            ("pad_border", lambda: ctx.pad_border(rec)),
            ("picture_ssd", lambda: ctx.picture_ssd_dev(orig, rec, 0, p.bd, p.d_ssd.ptr))]

    def results(self):
        """(search results res[l][r] - None for a re-used picture -, nnz, cus, ssd, the
        choice records, the refinement results [n_cus, Rmax], the slot bytes [n_cus, Rmax, 2])."""
        d = self.desc
        _, nnz, cus, ssd = self.p.results()
        res = [[b.to_array(api.MERES_DTYPE, d.n_cus) if b is not None else None for b in row]
               for row in self.d_res]
        return (res, nnz, cus, ssd,
                self.d_choice.to_array(api.FP_BI_REFS_RESULT_DTYPE, d.n_cus),
                self.d_bi_res.to_array(api.MERES_DTYPE, d.n_cus * self.rmax).reshape(-1, self.rmax),
                self.d_bi_slots.to_array(np.uint8, 2 * d.n_cus * self.rmax).reshape(-1, self.rmax, 2))

    def affine_choice(self):
        """affine=True: the last run's api.FP_BI_AFFINE_RESULT_DTYPE record per CU."""
        return self.affine.d_choice.to_array(api.FP_BI_AFFINE_RESULT_DTYPE, self.desc.n_cus)

    def affine_uni_results(self):
        """affine=True: the uni-directional affine results [n_cus, 2 * Rmax]."""
        e = 2 * self.rmax
        return self.affine.d_uni_res.to_array(api.AFFINE_ME_RESULT_DTYPE,
                                              self.desc.n_cus * e).reshape(-1, e)

    def affine_bi_results(self):
        """affine=True: the refinement's affine results [n_cus, Rmax]."""
        return self.affine.d_bi_res.to_array(api.AFFINE_ME_RESULT_DTYPE,
                                             self.desc.n_cus * self.rmax).reshape(-1, self.rmax)

    def affine_jobs(self):
        """affine=True: the uni-directional jobs after a run [n_cus, 2 * Rmax] (flags and
        bootstrap are the device's)."""
        e = 2 * self.rmax
        return self.affine.d_uni.to_array(api.AFFINE_ME_DTYPE, self.desc.n_cus * e).reshape(-1, e)

    def affine_bi_jobs(self):
        """affine=True: (the refinement jobs [n_cus, Rmax], their slot bytes [n_cus, Rmax, 2])."""
        k = self.desc.n_cus * self.rmax
        return (self.affine.d_bi.to_array(api.AFFINE_ME_DTYPE, k).reshape(-1, self.rmax),
                self.affine.d_bi_slots.to_array(np.uint8, 2 * k).reshape(-1, self.rmax, 2))

    def merge_rank(self):
        """Merge mode: the last run's api.FP_MERGE_RANK_DTYPE record per CU (the CUs outside
        the list keep what the array held)."""
        return self.merge.d_rank.to_array(api.FP_MERGE_RANK_DTYPE, self.desc.n_cus)

    def merge_choice(self):
        """Merge mode: the last run's api.FP_BI_MERGE_RESULT_DTYPE record per CU."""
        return self.merge.d_choice.to_array(api.FP_BI_MERGE_RESULT_DTYPE, self.desc.n_cus)

    def chosen_results(self):
        """Merge mode: the records the pass behind the choice was made from - the plain
        choice records with the merge winners' direction, pictures, vectors and cost."""
        return self.merge.d_chosen.to_array(api.FP_BI_REFS_RESULT_DTYPE, self.desc.n_cus)

    def inter_jobs(self):
        """The last run's prediction jobs [3 * n_cus]."""
        return self.d_inter.to_array(api.INTER_DTYPE, 3 * self.desc.n_cus)

    def l1_mvp_cost(self):
        """low_delay: the last run's predictor cost per (CU, list-1 picture), [n_cus,
        CS_MAX_REFS] uint32 (UINT32_MAX beyond list 1's pictures)."""
        return self.d_l1_mvp_cost.to_array(np.uint32, api.CS_MAX_REFS * self.desc.n_cus) \
            .reshape(-1, api.CS_MAX_REFS)

    def ctu_delta_qp(self):
        """Adaptive QP: the last run's delta per CTU, [rows, columns] int8."""
        return self.aqp.ctu_delta_qp()

    def cu_qp(self):
        """Adaptive QP: the last run's (qp_y, qp_c) per CU, [n_cus, 2] int8."""
        return self.aqp.cu_qp()

    def destroy(self):
        if self.aqp is not None:
            self.aqp.free()
            self.aqp = None
        if self.affine is not None:
            self.affine.free()
            self.affine = None
        if self.merge is not None:
            self.merge.free()
            self.merge = None
        bufs = [self.d_bi_jobs, self.d_bi_res, self.d_bi_slots, self.d_choice, self.d_inter]
        if self.d_l1_mvp_cost is not None:
            bufs.append(self.d_l1_mvp_cost)
            self.d_l1_mvp_cost = None
        for l in range(2):
            bufs += self.d_me[l] + [b for b in self.d_res[l] if b is not None]
            for plan in self.plans[l]:
                if plan is not None:
                    plan.destroy()
            self.plans[l] = [None] * self.num_ref[l]
        for b in bufs:
            b.free()
        self.p.destroy()


class PipelinedFramePass:
    """The frame pass issued on two queues so that kernels of one half of the
    picture run while kernels of the other half ramp up or drain (a launch is
    only ~2 rounds of waves deep, so each kernel spends a third of its time
    partially filled - tools/trace_me.py).

        ctx_hi (high priority): top CU rows    - search, recon, deblock V
        ctx_lo (low priority):  bottom CU rows - search, recon, deblock V
        ctx_hi: waits for ctx_lo, deblock H over the picture, pad
        ctx_lo: waits for that, picture SSD (overlaps the next picture's search)

    Same kernels, same results as FramePass; only the queueing differs."""

    def __init__(self, ctx_hi, ctx_lo, width, height, bitdepth=10, qp=32, cu=16,
                 search_range=96, rdoq=False):
        self.hi, self.lo = ctx_hi, ctx_lo
        self.w, self.h, self.bd = width, height, bitdepth
        rows = (height + cu - 1) // cu
        self.y_mid = (rows // 2) * cu
        self.top = FramePass(ctx_hi, width, height, bitdepth, qp, cu, search_range,
                             row_range=(0, self.y_mid), rdoq=rdoq)
        self.bot = FramePass(ctx_lo, width, height, bitdepth, qp, cu, search_range,
                             row_range=(self.y_mid, height), rdoq=rdoq)
        # one CU metadata array for the whole picture (the H pass reads both halves)
        self.bot.d_cus.free()
        self.bot.d_cus = self.top.d_cus
        self.desc = FrameDescriptors(width, height, qp, cu, search_range)
        self.d_ssd = self.bot.d_ssd

    def run(self, orig, ref, rec, ref_poc=0):
        hi, lo, top, bot = self.hi, self.lo, self.top, self.bot
        top.encode(orig, ref, rec, ref_poc)
        top.deblock_rows(rec, 0, 0, self.y_mid)
        bot.encode(orig, ref, rec, ref_poc)
        bot.deblock_rows(rec, 0, self.y_mid, self.h)
        hi.wait_for(lo)
        top.deblock_rows(rec, 1, 0, self.h)
        hi.pad_border(rec)
        lo.wait_for(hi)
        lo.picture_ssd_dev(orig, rec, 0, self.bd, self.d_ssd.ptr)

    def sync(self):
        self.hi.sync()
        self.lo.sync()

    def results(self):
        a, b = self.top, self.bot
        res = np.concatenate([a.d_res.to_array(api.MERES_DTYPE, a.desc.n_cus),
                              b.d_res.to_array(api.MERES_DTYPE, b.desc.n_cus)])
        nnz = np.concatenate([a.d_nnz.to_array(np.int32, len(a.desc.tx)),
                              b.d_nnz.to_array(np.int32, len(b.desc.tx))])
        return (res, nnz, a.d_cus.to_array(api.CU_DTYPE, a.desc.n_cus_total),
                self.d_ssd.to_array(np.uint64, 2))

    def destroy(self):
        self.sync()
        self.bot.d_cus = None       # top's: freed once, with top
        self.top.destroy()
        self.bot.destroy()


class DecodePass:
    """The decoder's reconstruction of one inter picture from parsed syntax
    (PictureDecoder::Decode, picture_decoder.cc:
    168-200, and CuDecoder::DecompressInter / DecompressComponent,
    cu_decoder.cc:102-138): per CU the MV, per TU the levels and the cbf;
    motion compensation -> Quantize::Inverse + InverseTransform + AddClip
    (or CopyFrom when cbf == 0) -> deblocking -> PadBorder.  Same kernels as
    the encoder's reconstruction, so encoder rec == decoder output by
    construction - which the tests check."""

    def __init__(self, ctx, desc, bitdepth=10):
        self.ctx, self.desc, self.bd = ctx, desc, bitdepth
        d = desc
        self.d_me = ctx.buffer(d.me)
        self.d_tx = ctx.buffer(d.tx)
        self.d_luma_idx = ctx.buffer(d.luma_idx)
        self.d_map = ctx.buffer(d.cu_map)
        self.d_cus = ctx.alloc(api.CU_DTYPE.itemsize * d.n_cus_total)
        ctx._check(ctx.lib.xvcgpu_memset(ctx.h, self.d_cus.ptr, 0,
                                         api.CU_DTYPE.itemsize * d.n_cus_total))
        self.pred = ctx.picture(d.w, d.h, bitdepth)

    def run(self, ref, rec, d_mvs, d_levels, d_level_off, d_nnz, ref_poc=0,
            deblock=True, pad=True):
        """d_mvs: xvcgpu_me_result per CU (mv_x / mv_y used); d_levels /
        d_level_off / d_nnz: per TU, as xvcgpu_residual_batch lays them out."""
        ctx, d = self.ctx, self.desc
        ctx.mc_from_me_dev(ref, self.pred, self.d_me.ptr, d_mvs, d.n_cus)
        ctx._check(ctx.lib.xvcgpu_inv_transform_batch(
            ctx.h, self.pred.h_pic, rec.h_pic, self.d_tx.ptr, len(d.tx), d_levels,
            d_level_off, d_nnz))
        ctx.cu_info_from_me_dev(self.d_me.ptr, d_mvs, d_nnz, self.d_luma_idx.ptr,
                                d.n_cus, d.qp, d.qp_c, ref_poc, self.d_cus.ptr)
        if deblock:
            ctx.deblock_dev(rec, self.d_cus.ptr, d.n_cus_total, self.d_map.ptr,
                            d.cu_map.shape[1], 0, 0, 0, 4)
        if pad:
            ctx.pad_border(rec)

    def destroy(self):
        for b in (self.d_me, self.d_tx, self.d_luma_idx, self.d_map, self.d_cus):
            b.free()
        self.pred.destroy()


def psnr_from_ssd(dist, samples):
    """SampleMetric::ComputePsnr tail (sample_metric.cc:143-154)."""
    mse = dist / samples if samples else 0.0
    return 10.0 * math.log10(255.0 * 255.0 / mse) if mse > 0 else 99.999


class IntraPictureDescriptors:
    """Host-side plan of an all-intra picture pass: a
    raster of cu x cu CUs coded in raster order.  A CU's prediction reads the
    reconstruction of its left / above-left / above / above-right neighbours,
    so CU (cx, cy) can run once wave cx + 2*cy - 1 is done: the CUs are
    grouped into those anti-diagonal waves, and every wave is one batch per
    kernel.  Jobs and transform blocks are stored wave by wave."""

    def __init__(self, width, height, qp=32, cu=16):
        assert cu in (8, 16, 32, 64)
        self.w, self.h, self.qp, self.cu = width, height, qp, cu
        self.qp_c = chroma_qp(qp)
        parts = cu_partition(width, height, cu)
        order = sorted(range(len(parts)),
                       key=lambda i: (parts[i][0] // cu + 2 * (parts[i][1] // cu), i))
        self.parts = [parts[i] for i in order]
        n = len(parts)
        self.n_cus = n
        self.luma = np.zeros(n, api.INTRA_DTYPE)
        self.chroma = np.zeros(2 * n, api.INTRA_DTYPE)      # U then V of each CU
        self.jobs3 = np.zeros(3 * n, api.INTRA_DTYPE)       # Y, U, V of each CU (= tx order)
        self.tx = np.zeros(3 * n, api.TX_DTYPE)              # Y, U, V of each CU
        wave_of = []
        for i, (x, y, w, h) in enumerate(self.parts):
            nb = (api.INTRA_HAS_LEFT if x else 0) | (api.INTRA_HAS_ABOVE if y else 0) | \
                (api.INTRA_HAS_ABOVE_LEFT if x and y else 0)
            # GetCuSizeAboveRight: the row above is complete; GetCuSizeBelowLeft: 0
            ar = max(0, min(h, width - (x + w))) if y else 0
            self.luma[i] = (x, y, w, h, 0, 0, nb, ar, 0, 0)
            for c in (1, 2):
                self.chroma[2 * i + c - 1] = (x // 2, y // 2, w // 2, h // 2, c, 0, nb,
                                              ar // 2, 0, 0)
            for c in range(3):
                t = self.tx[3 * i + c]
                s = 1 if c else 0
                t["x"], t["y"], t["w"], t["h"] = x >> s, y >> s, w >> s, h >> s
                t["comp"], t["qp"] = c, (self.qp_c if c else qp)
                t["intra_pic"] = api.TXF_INTRA_PIC
            wave_of.append(x // cu + 2 * (y // cu))
        self.jobs3[0::3] = self.luma
        self.jobs3[1::3] = self.chroma[0::2]
        self.jobs3[2::3] = self.chroma[1::2]
        wave_of = np.array(wave_of)
        self.wave_start = np.searchsorted(wave_of, np.arange(wave_of.max() + 2))
        self.level_off, self.level_total = api.Context.level_offsets(self.tx)

    def waves(self):
        for k in range(len(self.wave_start) - 1):
            a, b = int(self.wave_start[k]), int(self.wave_start[k + 1])
            if b > a:
                yield a, b

    def set_modes(self, a, b, modes):
        """Modes of CUs [a, b): luma jobs, chroma jobs (DM: the luma mode) and
        the coefficient scan of small CUs (TransformHelper::DetermineScanOrder,
        transform.cc:1614-1637)."""
        m = np.asarray(modes, np.int64).reshape(-1)
        assert len(m) == b - a
        self.luma["mode"][a:b] = m
        self.chroma["mode"][2 * a:2 * b] = np.repeat(m, 2)
        self.jobs3["mode"][3 * a:3 * b] = np.repeat(m, 3)
        small = (self.luma["w"][a:b] < 16) & (self.luma["h"][a:b] < 16)
        scan = np.where(np.abs(m - 50) < 10, 1, np.where(np.abs(m - 18) < 10, 2, 0))
        scan = np.where(small, scan, 0)
        self.tx["intra_pic"][3 * a:3 * b] = np.repeat(
            api.TXF_INTRA_PIC | (scan << api.TXF_SCAN_SHIFT), 3)


class IntraPicturePass:
    """All-intra picture on the device, wave by wave (IntraPictureDescriptors).

    encode(): per wave the SATD of all 67 luma modes (xvcgpu_intra_satd_batch),
    the mode with the smallest SATD (first on ties; chosen on the host - the
    reference adds CABAC-state dependent mode bits there, which this
    composition leaves out), prediction of Y,U,V (xvcgpu_intra_pred_batch) and
    TransformAndReconstruct with QuantFast (xvcgpu_residual_batch).
    decode(): the decoder's side - modes and levels given, prediction +
    xvcgpu_inv_transform_batch per wave, no host round trip.
    Neither is the reference's intra encoder (no RDO over modes / transforms,
    raster CU order instead of the CTU quad-tree order); the oracle's twin in
    tests/oracle_intra_picture.py is the same composition on the CPU."""

    def __init__(self, ctx, width, height, bitdepth=10, qp=32, cu=16, fused=None):
        self.ctx, self.bd = ctx, bitdepth
        self.desc = d = IntraPictureDescriptors(width, height, qp, cu)
        # CUs up to 16x16: prediction + residual pipeline in one launch per wave
        # (xvcgpu_intra_recon_batch); else prediction picture + separate launches
        self.fused = (cu <= 16) if fused is None else fused
        self.pred = ctx.picture(width, height, bitdepth)
        self.d_luma = ctx.buffer(d.luma)
        self.d_chroma = ctx.buffer(d.chroma)
        self.d_jobs3 = ctx.buffer(d.jobs3)
        self.d_tx = ctx.buffer(d.tx)
        self.d_off = ctx.buffer(d.level_off)
        self.d_levels = ctx.alloc(2 * max(1, d.level_total))
        self.d_nnz = ctx.alloc(4 * len(d.tx))
        self.d_dist = ctx.alloc(4 * api.INTRA_NUM_MODES * d.n_cus)
        self.d_modes = ctx.alloc(4 * d.n_cus)

    def _upload_range(self, buf, arr, a, b):
        sz = arr.dtype.itemsize
        self.ctx.h2d(buf.ptr + a * sz, arr[a:b])

    def encode(self, orig, rec, host_select=False):
        """host_select: fold the SATD table on the host (one round trip per
        wave, the reference's division of labour); default: on the device
        (xvcgpu_intra_select_modes), the whole picture enqueued without a sync."""
        ctx, d, lib = self.ctx, self.desc, self.ctx.lib
        J, T = api.INTRA_DTYPE.itemsize, api.TX_DTYPE.itemsize
        if not host_select and self.fused:
            M = 4 * api.INTRA_NUM_MODES
            for a, b in d.waves():
                n = b - a
                ctx._check(lib.xvcgpu_intra_satd_batch(
                    ctx.h, orig.h_pic, rec.h_pic, self.d_luma.ptr + a * J, n,
                    self.d_dist.ptr + a * M, d.cu))
                ctx._check(lib.xvcgpu_intra_select_modes(
                    ctx.h, self.d_dist.ptr + a * M, None, n, self.d_modes.ptr + 4 * a,
                    self.d_jobs3.ptr + 3 * a * J, self.d_tx.ptr + 3 * a * T, 3))
                self._recon(orig, rec, a, b)
            modes = self.d_modes.to_array(np.int32, d.n_cus)    # synchronises
            d.set_modes(0, d.n_cus, modes)
            return
        for a, b in d.waves():
            n = b - a
            ctx._check(lib.xvcgpu_intra_satd_batch(ctx.h, orig.h_pic, rec.h_pic,
                                                   self.d_luma.ptr + a * J, n,
                                                   self.d_dist.ptr, d.cu))
            dist = self.d_dist.to_array(np.uint32, n * api.INTRA_NUM_MODES) \
                .reshape(n, api.INTRA_NUM_MODES)
            d.set_modes(a, b, dist.argmin(axis=1))
            self._upload_range(self.d_tx, d.tx, 3 * a, 3 * b)
            if self.fused:
                self._upload_range(self.d_jobs3, d.jobs3, 3 * a, 3 * b)
                self._recon(orig, rec, a, b)
                continue
            self._upload_range(self.d_luma, d.luma, a, b)
            self._upload_range(self.d_chroma, d.chroma, 2 * a, 2 * b)
            self._wave(rec, a, b)
            ctx.residual_batch_dev(orig, self.pred, rec, self.d_tx.ptr + 3 * a * T, 3 * n,
                                   self.d_levels.ptr, self.d_off.ptr + 3 * a * 4,
                                   self.d_nnz.ptr + 3 * a * 4)
        ctx.sync()

    def _recon(self, orig, rec, a, b):
        ctx, J, T = self.ctx, api.INTRA_DTYPE.itemsize, api.TX_DTYPE.itemsize
        ctx._check(ctx.lib.xvcgpu_intra_recon_batch(
            ctx.h, orig.h_pic if orig is not None else None, rec.h_pic,
            self.d_jobs3.ptr + 3 * a * J, self.d_tx.ptr + 3 * a * T, 3 * (b - a),
            self.d_levels.ptr, self.d_off.ptr + 3 * a * 4, self.d_nnz.ptr + 3 * a * 4))

    def _wave(self, rec, a, b):
        ctx, lib, J = self.ctx, self.ctx.lib, api.INTRA_DTYPE.itemsize
        ctx._check(lib.xvcgpu_intra_pred_batch(ctx.h, rec.h_pic, self.pred.h_pic,
                                               self.d_luma.ptr + a * J, b - a))
        ctx._check(lib.xvcgpu_intra_pred_batch(ctx.h, rec.h_pic, self.pred.h_pic,
                                               self.d_chroma.ptr + 2 * a * J, 2 * (b - a)))

    def load(self, modes, levels, nnz):
        """Parsed syntax of a picture: mode per CU (wave order), levels / nnz as
        results() returned them."""
        d = self.desc
        d.set_modes(0, d.n_cus, modes)
        for buf, arr in ((self.d_luma, d.luma), (self.d_chroma, d.chroma), (self.d_tx, d.tx),
                         (self.d_jobs3, d.jobs3)):
            self._upload_range(buf, arr, 0, len(arr))
        self.ctx.h2d(self.d_levels.ptr, np.ascontiguousarray(levels, np.int16))
        self.ctx.h2d(self.d_nnz.ptr, np.ascontiguousarray(nnz, np.int32))

    def decode(self, rec):
        ctx, d, T = self.ctx, self.desc, api.TX_DTYPE.itemsize
        for a, b in d.waves():
            if self.fused:
                self._recon(None, rec, a, b)
                continue
            self._wave(rec, a, b)
            ctx._check(ctx.lib.xvcgpu_inv_transform_batch(
                ctx.h, self.pred.h_pic, rec.h_pic, self.d_tx.ptr + 3 * a * T, 3 * (b - a),
                self.d_levels.ptr, self.d_off.ptr + 3 * a * 4, self.d_nnz.ptr + 3 * a * 4))

    def results(self):
        d = self.desc
        return (d.luma["mode"].copy(), self.d_levels.to_array(np.int16, d.level_total),
                self.d_nnz.to_array(np.int32, len(d.tx)))

    def destroy(self):
        for b in (self.d_luma, self.d_chroma, self.d_jobs3, self.d_tx, self.d_off,
                  self.d_levels, self.d_nnz, self.d_dist, self.d_modes):
            b.free()
        self.pred.destroy()


class MixedPictureDecoder:
    """Decoder-side reconstruction of an inter picture whose CUs are a mix of
    uni-pred, bi-pred, LIC and intra CUs: what
    CuDecoder::DecompressInter / DecompressIntra (cu_decoder.cc) do CU by CU,
    scheduled as dependency waves over a raster of cu x cu CUs.  Plain inter
    CUs need no neighbour: wave 0 (prediction + inverse path for all of them).
    A LIC CU reads the reconstruction of its left / above CU, an intra CU that
    of left, above-left, above and above-right: wave = 1 + the latest of those.
    Per wave: xvcgpu_mc_lic_batch + xvcgpu_inv_transform_batch for the LIC CUs,
    one fused xvcgpu_intra_recon_batch for the intra CUs.

    syntax (numpy, CUs in raster order): kind[n] (0 uni L0, 1 bi, 2 LIC, 3 intra,
    4 affine L0), mv0[n,2], mv1[n,2] (1/16 pel), intra_mode[n], mv_affine[n,3,2]
    (corner vectors of the affine CUs), levels / nnz per (CU, comp)."""

    UNI, BI, LIC, INTRA, AFFINE = 0, 1, 2, 3, 4

    def __init__(self, ctx, width, height, bitdepth, qp, kind, mv0, mv1, intra_mode, cu=16,
                 mv_affine=None):
        self.ctx, self.bd, self.w, self.h = ctx, bitdepth, width, height
        self.fused_intra = cu <= 16     # else prediction picture + inverse path
        parts = cu_partition(width, height, cu)
        n = len(parts)
        per_row = (width + cu - 1) // cu
        qpc = chroma_qp(qp)
        wave = np.zeros(n, np.int64)
        for i, (x, y, w, h) in enumerate(parts):
            if kind[i] in (self.UNI, self.BI, self.AFFINE):
                continue
            deps = []
            if x:
                deps.append(i - 1)
            if y:
                deps.append(i - per_row)
            if kind[i] == self.INTRA:
                if x and y:
                    deps.append(i - per_row - 1)
                if y and x + w < width:
                    deps.append(i - per_row + 1)
            wave[i] = 1 + max([wave[d] for d in deps], default=0)
        # CUs ordered by (wave, kind): every (wave, kind) group is one batch
        self.order = order = sorted(range(n), key=lambda i: (wave[i], kind[i], i))
        self.parts = [parts[i] for i in order]
        self.kind = np.asarray(kind)[order]
        self.wave = wave[order]
        tx = np.zeros(3 * n, api.TX_DTYPE)
        jobs3 = np.zeros(3 * n, api.INTRA_DTYPE)
        uni, bi, lic, aff = [], [], [], []
        for k, i in enumerate(order):
            x, y, w, h = parts[i]
            for c in range(3):
                s = 1 if c else 0
                tx[3 * k + c] = (x >> s, y >> s, w >> s, h >> s, c, 0, 0, 0,
                                 qpc if c else qp, 0)
            if kind[i] == self.UNI:
                uni += [(x, y, w, h, c, 0, *mv0[i]) for c in range(3)]
            elif kind[i] == self.BI:
                bi += [(x, y, w, h, c, 0, *mv0[i], *mv1[i]) for c in range(3)]
            elif kind[i] == self.AFFINE:
                aff += [(x, y, w, h, c, 0, np.asarray(mv_affine[i], np.int32)) for c in range(3)]
            elif kind[i] == self.LIC:
                nb = (1 if y else 0) | (2 if x else 0)
                lic += [(x, y, w, h, c, nb, *mv0[i], x, max(0, y - cu), max(0, x - cu), y)
                        for c in range(3)]
            else:
                nb = (api.INTRA_HAS_LEFT if x else 0) | (api.INTRA_HAS_ABOVE if y else 0) | \
                    (api.INTRA_HAS_ABOVE_LEFT if x and y else 0)
                ar = max(0, min(h, width - (x + w))) if y else 0
                for c in range(3):
                    s = 1 if c else 0
                    jobs3[3 * k + c] = (x >> s, y >> s, w >> s, h >> s, c, intra_mode[i], nb,
                                        ar >> s, 0, 0)
        self.tx = tx
        self.level_off, self.level_total = api.Context.level_offsets(tx)
        self.d_tx, self.d_off = ctx.buffer(tx), ctx.buffer(self.level_off)
        self.d_jobs3 = ctx.buffer(jobs3)
        self.d_uni = ctx.buffer(np.array(uni, api.MC_DTYPE)) if uni else None
        self.d_bi = ctx.buffer(np.array(bi, api.MCBI_DTYPE)) if bi else None
        self.d_lic = ctx.buffer(np.array(lic, api.LIC_DTYPE)) if lic else None
        self.d_aff = ctx.buffer(np.array(aff, api.MCAFF_DTYPE)) if aff else None
        self.n_uni, self.n_bi, self.n_aff = len(uni), len(bi), len(aff)
        self.d_levels = ctx.alloc(2 * max(1, self.level_total))
        self.d_nnz = ctx.alloc(4 * 3 * n)
        self.pred = ctx.picture(width, height, bitdepth)
        # batches: (first CU, last CU) in the new order per (wave, kind)
        self.groups = []
        k = 0
        while k < n:
            e = k
            while e < n and self.wave[e] == self.wave[k] and self.kind[e] == self.kind[k]:
                e += 1
            self.groups.append((int(self.wave[k]), int(self.kind[k]), k, e))
            k = e
        self.n_inter = sum(e - a for wv, kd, a, e in self.groups
                           if kd in (self.UNI, self.BI, self.AFFINE))

    def load(self, levels_per_tx, nnz_per_tx):
        """levels_per_tx[3 * i + c]: w*h int16 of CU i (raster order), comp c."""
        lv = np.zeros(self.level_total, np.int16)
        nz = np.zeros(len(self.tx), np.int32)
        for k, i in enumerate(self.order):
            for c in range(3):
                a = np.asarray(levels_per_tx[3 * i + c], np.int16).reshape(-1)
                off = int(self.level_off[3 * k + c])
                lv[off:off + len(a)] = a
                nz[3 * k + c] = nnz_per_tx[3 * i + c]
        self.ctx.h2d(self.d_levels.ptr, lv)
        self.ctx.h2d(self.d_nnz.ptr, nz)

    def _inverse(self, rec, a, e):
        ctx, T = self.ctx, api.TX_DTYPE.itemsize
        ctx._check(ctx.lib.xvcgpu_inv_transform_batch(
            ctx.h, self.pred.h_pic, rec.h_pic, self.d_tx.ptr + 3 * a * T, 3 * (e - a),
            self.d_levels.ptr, self.d_off.ptr + 3 * a * 4, self.d_nnz.ptr + 3 * a * 4))

    def decode(self, ref0, ref1, rec):
        ctx, lib = self.ctx, self.ctx.lib
        J, T, L = api.INTRA_DTYPE.itemsize, api.TX_DTYPE.itemsize, api.LIC_DTYPE.itemsize
        if self.n_uni:
            ctx.mc_batch_dev(ref0, self.pred, self.d_uni.ptr, self.n_uni)
        if self.n_bi:
            ctx._check(lib.xvcgpu_mc_bipred_batch(ctx.h, ref0.h_pic, ref1.h_pic,
                                                  self.pred.h_pic, self.d_bi.ptr, self.n_bi))
        if self.n_aff:
            ctx._check(lib.xvcgpu_mc_affine_batch(ctx.h, ref0.h_pic, self.pred.h_pic,
                                                  self.d_aff.ptr, self.n_aff))
        if self.n_inter:
            self._inverse(rec, 0, self.n_inter)     # all plain inter CUs come first
        lic_done = 0
        for wv, kd, a, e in self.groups:
            if kd == self.LIC:
                ctx._check(lib.xvcgpu_mc_lic_batch(ctx.h, ref0.h_pic, rec.h_pic, self.pred.h_pic,
                                                   self.d_lic.ptr + 3 * lic_done * L,
                                                   3 * (e - a)))
                lic_done += e - a
                self._inverse(rec, a, e)
            elif kd == self.INTRA and not self.fused_intra:
                ctx._check(lib.xvcgpu_intra_pred_batch(ctx.h, rec.h_pic, self.pred.h_pic,
                                                       self.d_jobs3.ptr + 3 * a * J, 3 * (e - a)))
                self._inverse(rec, a, e)
            elif kd == self.INTRA:
                ctx._check(lib.xvcgpu_intra_recon_batch(
                    ctx.h, None, rec.h_pic, self.d_jobs3.ptr + 3 * a * J,
                    self.d_tx.ptr + 3 * a * T, 3 * (e - a), self.d_levels.ptr,
                    self.d_off.ptr + 3 * a * 4, self.d_nnz.ptr + 3 * a * 4))

    def destroy(self):
        for b in (self.d_tx, self.d_off, self.d_jobs3, self.d_uni, self.d_bi, self.d_lic,
                  self.d_aff, self.d_levels, self.d_nnz):
            if b is not None:
                b.free()
        self.pred.destroy()
