"""The transform stages restated in numpy, a counter on every decision.

What `TransformEncoder::TransformAndReconstruct` does around the quantiser (transform_encoder.cc:
203-285), as the device code states it in csrc/k_tx.h (`tx_fwd_1d`, `tx_inv_1d`, the 4x4 DST, the
skip branches, `residual_job`) and csrc/k_tx2.h (`tx2_stage`, `tx2_job`):

  forward   horizontal then vertical, `(M x in + add) >> shift` cast to int16, a 64-point side
            keeps its 32 low rows                                  (transform.cc:869-961)
  dequant   Quantize::Inverse, clipped to 16 bits                  (quantize.cc:94-125)
  inverse   vertical then horizontal, clipped to 16 bits after each stage; the 4x4 DST and the
            transform skip first, then InvDct2Dc for a single level at position 0 of a block
            whose two types are DCT-2                              (transform.cc:83-291)
  AddClip   prediction + residual, clipped to the sample range     (sample_buffer.h:72-87)
  SSD       (orig - pred - residual)^2 summed in 64 bits, >> 2 (depth - 8)
                                                                   (sample_metric.cc:286-290)

Every stage is one matrix product in int64 folded to int32 (the reference accumulates in int32; no
case gets near a wrap, the fold is there so that the model says what the code says).  The matrices
are the oracle's (`xo_transform_matrix`, pinned to the reference's tables by
tests/test_oracle_vs_ref.py); the 4x4 DST is its four output formulas written as a matrix.
QuantFast and its sign hiding are not restated: they have their own suites, the forward cases take
their levels from the oracle's quantiser.

`n` is a collections.Counter; KEYS lists every class.  `device_path` names the code a block of a
batch reaches on the device and EXCLUDED the classes a path cannot reach, each with its reason.
"""
import functools

import numpy as np

import oracle_lib as ol

TX_SKIP, TX_LOW = 6, 7
INV_SCALES = [40, 45, 51, 57, 64, 72]
DST4 = np.array([[29, 55, 74, 84], [74, 74, 0, -74], [84, -29, -74, 55], [55, -84, 74, -29]],
                np.int64)   # FwdPartialDst4's four sums (transform.cc:997-1017), rows = outputs

KEYS = [
    # which inverse / forward form the block took
    "form_matrix", "form_dst4", "form_skip",
    # forward stages (stage 1 horizontal, 2 vertical; the DST's and the matrix form's alike)
    "fwd1_ge_2p14", "fwd1_below_2p14", "fwd2_ge_2p14", "fwd2_below_2p14", "fwd1_wrap", "fwd2_wrap",
    # the 32 kept rows of a 64-point side, per direction (either transform)
    "zero_out_hor", "zero_out_ver",
    # the dequantiser
    "deq_clip_high", "deq_clip_low", "deq_inside",
    # inverse stages of the matrix form (1 vertical, 2 horizontal) and of the 4x4 DST
    "inv1_clip_high", "inv1_clip_low", "inv1_inside",
    "inv2_clip_high", "inv2_clip_low", "inv2_inside",
    "dst1_clip_high", "dst1_clip_low", "dst1_inside",
    "dst2_clip_high", "dst2_clip_low", "dst2_inside",
    # the DC-only decision
    "dc_taken", "dc_refused_type", "dc_refused_position", "dc_refused_count",
    "dc_preempted_skip", "dc_preempted_dst",
    # AddClip
    "add_at_0", "add_at_max", "add_inside",
    # nothing coded
    "nnz0_in_place", "nnz0_copied",
    # the residual-domain SSD in front of its shift
    "dist_ge_2p32", "dist_below_2p32",
    # ... and the largest partial sum one lane holds in front of the fold (tx2_job `dist4`: four
    # neighbours of a row; residual_job: every 256th sample)
    "dist_lane_ge_2p32", "dist_lane_below_2p32",
]


def log2(v):
    assert v > 0 and v & (v - 1) == 0, v
    return v.bit_length() - 1


def fold32(a):
    """int64 -> the int32 the reference's accumulator holds."""
    return ((np.asarray(a, np.int64) + (1 << 31)) & 0xffffffff) - (1 << 31)


def cast16(a):
    return ((np.asarray(a, np.int64) + 32768) & 0xffff) - 32768


@functools.lru_cache(maxsize=None)
def matrix(tx, size):
    """Rows = basis functions, int64.  XVC_TX_DEFAULT is the DCT-2."""
    m = ol.Lib("xo").transform_matrix(tx, size)
    assert m is not None, ("no matrix for", tx, size)
    return m.astype(np.int64)


def is_dct2(t):
    return t in (0, 1, TX_LOW)


def hp(t):
    """kTransformHighPrecisionShift of a stage (k_quant.h tx_stage_shifts): none for the 6-bit DCT-2."""
    return 0 if t == TX_LOW else 2


def valid_type(t, size):
    """What the binding passes (xvcgpu_types.h): the low-precision DCT-2 for sides 4 .. 32, a side
    of 2 with the DCT-2 alone.  Anything else indexes outside the table layout."""
    if t == TX_LOW:
        return 4 <= size <= 32
    if size == 2:
        return t in (0, 1)
    return 0 <= t <= 5


def valid_block(b):
    w, h = b["w"], b["h"]
    if b["tx_hor"] == TX_SKIP:
        return w <= 4 and h <= 4 and not b["dst4x4"]
    if b["dst4x4"]:
        return (w, h, b["comp"], b["tx_hor"], b["tx_ver"]) == (4, 4, 0, 0, 0)
    return valid_type(b["tx_hor"], w) and valid_type(b["tx_ver"], h)


def quant_constants(bd, qp, w, h):
    """block_quant (k_quant.h) / Quantize::Inverse: what the dequantiser reads."""
    lsum = log2(w) + log2(h)
    qpb = max(0, qp + 6 * (bd - 8))
    bias = lsum & 1
    tshift = 15 - bd - (lsum >> 1)
    return dict(bias=bias, tshift=tshift,
                iq_scale=(INV_SCALES[qpb % 6] << (qpb // 6)) * (181 if bias else 1),
                iq_shift=6 - tshift + (8 if bias else 0))


def dequant(bd, qp, w, h, levels, n):
    k = quant_constants(bd, qp, w, h)
    prod = fold32(np.asarray(levels, np.int64) * k["iq_scale"])
    if k["iq_shift"] > 0:
        cf = fold32(prod + (1 << (k["iq_shift"] - 1))) >> k["iq_shift"]
    else:
        cf = fold32(prod << -k["iq_shift"])
    n["deq_clip_high"] += int((cf > 32767).sum())
    n["deq_clip_low"] += int((cf < -32768).sum())
    n["deq_inside"] += int(((cf <= 32767) & (cf >= -32768)).sum())
    return np.clip(cf, -32768, 32767)


def _fwd_stage(m, x, shift, keep, key, n):
    """x: lines x N.  out[k][line] for the min(N, 32) kept rows k and the first `keep` lines, zero
    elsewhere (tx_fwd_1d)."""
    size, lines = m.shape[0], x.shape[0]
    rows = min(size, 32)
    v = fold32(fold32(m[:rows] @ x[:keep].T) + (1 << (shift - 1))) >> shift
    n[key + "_ge_2p14"] += int((np.abs(v) >= 1 << 14).sum())
    n[key + "_below_2p14"] += int((np.abs(v) < 1 << 14).sum())
    n[key + "_wrap"] += int(((v > 32767) | (v < -32768)).sum())
    out = np.zeros((size, lines), np.int64)
    out[:rows, :keep] = cast16(v)
    return out


def _inv_stage(m, c, shift, keep, key, n):
    """c: N x lines.  out[line][k] = clip16 of the sum over the min(N, 32) kept rows, for the first
    `keep` lines, zero beyond (tx_inv_1d)."""
    size, lines = m.shape[0], c.shape[1]
    rows = min(size, 32)
    v = fold32(fold32(c[:rows, :keep].T @ m[:rows]) + (1 << (shift - 1))) >> shift
    n[key + "_clip_high"] += int((v > 32767).sum())
    n[key + "_clip_low"] += int((v < -32768).sum())
    n[key + "_inside"] += int(((v <= 32767) & (v >= -32768)).sum())
    out = np.zeros((lines, size), np.int64)
    out[:keep] = np.clip(v, -32768, 32767)
    return out


def _skip_shift(bd, w, h, fwd):
    k = quant_constants(bd, 0, w, h)
    return k["tshift"] + ((-8 if fwd else 7) if k["bias"] else 0), (181 if k["bias"] else 1)


def forward(bd, b, resi, n):
    """resi: h x w.  Coefficients h x w (row = vertical frequency)."""
    w, h = b["w"], b["h"]
    resi = np.asarray(resi, np.int64)
    if b["tx_hor"] == TX_SKIP:      # ForwardTransform::TransformSkip, transform.cc:963-995
        n["form_skip"] += 1
        sh, sc = _skip_shift(bd, w, h, True)
        v = resi * sc
        return cast16(v * (1 << sh) if sh > 0 else (v + (1 << (-sh - 1))) >> -sh)
    if b["dst4x4"] and (w, h) == (4, 4):
        n["form_dst4"] += 1
        t = _fwd_stage(DST4, resi, 2 + bd - 9, 4, "fwd1", n)
        return _fwd_stage(DST4, t, 2 + 6, 4, "fwd2", n)
    n["form_matrix"] += 1
    n["zero_out_hor"] += w == 64
    n["zero_out_ver"] += h == 64
    t = _fwd_stage(matrix(b["tx_hor"], w), resi, log2(w) + bd - 9 + hp(b["tx_hor"]), h, "fwd1", n)
    return _fwd_stage(matrix(b["tx_ver"], h), t, log2(h) + 6 + hp(b["tx_ver"]), min(w, 32),
                      "fwd2", n)


def inverse(bd, b, coeff, nnz, level0, n):
    """coeff: dequantised, h x w; nnz the block's count as handed over, level0 the level at
    position 0.  The order of the decisions is residual_job's: skip, DST, DC-only, matrices."""
    w, h = b["w"], b["h"]
    coeff = np.asarray(coeff, np.int64)
    dc_candidate = nnz == 1 and level0 != 0       # transform_encoder.cc:241
    if nnz == 1 and level0 == 0:
        n["dc_refused_position"] += 1
    if nnz > 1 and level0 != 0:
        n["dc_refused_count"] += 1
    if b["tx_hor"] == TX_SKIP:      # InverseTransform::TransformSkip, transform.cc:184-215
        n["form_skip"] += 1
        n["dc_preempted_skip"] += dc_candidate
        sh, sc = _skip_shift(bd, w, h, False)
        v = fold32(coeff * sc)
        return cast16((v + (1 << (sh - 1))) >> sh if sh > 0 else v << -sh)
    if b["dst4x4"] and (w, h) == (4, 4):
        n["form_dst4"] += 1
        n["dc_preempted_dst"] += dc_candidate
        u = _inv_stage(DST4, coeff, 7, 4, "dst1", n)
        return _inv_stage(DST4, u, 20 - bd, 4, "dst2", n)
    if dc_candidate:
        if is_dct2(b["tx_hor"]) and is_dct2(b["tx_ver"]):       # InvDct2Dc, transform.cc:279-291
            n["dc_taken"] += 1
            sh = 14 - bd
            cf = cast16((((int(coeff[0, 0]) + 1) >> 1) + (1 << (sh - 1))) >> sh)
            return np.full((h, w), int(cf), np.int64)
        n["dc_refused_type"] += 1
    n["form_matrix"] += 1
    n["zero_out_hor"] += w == 64
    n["zero_out_ver"] += h == 64
    u = _inv_stage(matrix(b["tx_ver"], h), coeff, 7 + hp(b["tx_ver"]), min(w, 32), "inv1", n)
    return _inv_stage(matrix(b["tx_hor"], w), u, 20 - bd + hp(b["tx_hor"]), h, "inv2", n)


def add_clip(bd, pred, resi, n):
    v = np.asarray(pred, np.int64) + resi
    smax = (1 << bd) - 1
    n["add_at_0"] += int((v <= 0).sum())
    n["add_at_max"] += int((v >= smax).sum())
    n["add_inside"] += int(((v > 0) & (v < smax)).sum())
    return np.clip(v, 0, smax).astype(np.uint16)


def ssd(bd, b, orig, pred, resi, n):
    """The distortion output of xvcgpu_inv_transform_dist_batch: python integers, no width."""
    d = np.asarray(orig, np.int64) - np.asarray(pred, np.int64) - resi
    sq = [int(v) * int(v) for v in d.reshape(-1)]
    total = sum(sq)
    n["dist_ge_2p32" if total >= 1 << 32 else "dist_below_2p32"] += 1
    if tx_small_job(b):     # a row is a multiple of four samples: a lane's four never leave it
        lane = max(sum(sq[i:i + 4]) for i in range(0, len(sq), 4))
    else:
        lane = max(sum(sq[i::256]) for i in range(min(256, len(sq))))
    n["dist_lane_ge_2p32" if lane >= 1 << 32 else "dist_lane_below_2p32"] += 1
    return total >> (2 * (bd - 8))


def reconstruct(bd, b, pred, levels, nnz, n, orig=None, in_place=False):
    """Dequantiser, inverse, AddClip (and the SSD where orig is given) of one block.  Returns
    (residual or None, reconstruction, distortion or None)."""
    w, h = b["w"], b["h"]
    if nnz == 0:        # cbf == 0: the level buffer is not read
        n["nnz0_in_place" if in_place else "nnz0_copied"] += 1
        dist = None if orig is None else ssd(bd, b, orig, pred, np.zeros((h, w), np.int64), n)
        return None, np.asarray(pred, np.uint16).copy(), dist
    levels = np.asarray(levels, np.int64).reshape(h, w)
    coeff = dequant(bd, b["qp"], w, h, levels, n)
    resi = inverse(bd, b, coeff, nnz, int(levels[0, 0]), n)
    dist = None if orig is None else ssd(bd, b, orig, pred, resi, n)
    return resi, add_clip(bd, pred, resi, n), dist


# ---- which code a block reaches on the device ---------------------------------------------------

INV_ONE_LAUNCH_MAX = 16384      # XVCGPU_INV_ONE_LAUNCH_MAX (xvcgpu.hip)
PER_JOB_MAX = 65536             # launch_residual: `n <= 65536`
RDOQ_CU_MAX, RDOQ_PER_JOB_MAX = 64, 262144      # launch_residual_rdoq

ENTRIES = ("residual", "fwd", "inv", "inv_dist", "rdoq")
PATHS = ["tx2_job/residual_wave_kernel", "tx2_job/residual_cu_kernel",
         "residual_job/residual_per_job_kernel", "residual_job/residual_kernel",
         "residual_job/residual_cu_kernel"]


def tx_small_job(b):
    """k_tx.h tx_small_job: sides 4, 8 or 16, not the 4x4 DST, not transform skip."""
    return b["w"] in (4, 8, 16) and b["h"] in (4, 8, 16) and \
        not (b["dst4x4"] and b["w"] == 4 and b["h"] == 4) and b["tx_hor"] != TX_SKIP


def device_path(block, entry, n, one_launch=True):
    """'<stage code>/<kernel>' of a block in a batch of n through `entry`.
    launch_residual (xvcgpu.hip): the inverse without distortion is one residual_cu_kernel launch
    up to 16384 blocks where the context was created with XVCGPU_INV_ONE_LAUNCH unset or not "0";
    every other batch is residual_wave_kernel (which leaves the blocks tx_small_job refuses) and
    then residual_per_job_kernel up to 65536 blocks, the scanning residual_kernel beyond.
    launch_residual_rdoq: residual_cu_kernel up to 64 blocks, per-job up to 262144.
    residual_cu_body (k_tx2.h) runs tx2_job for a small job and residual_job for the rest, as the
    two kernels would."""
    assert entry in ENTRIES
    stage = "tx2_job" if tx_small_job(block) else "residual_job"
    if entry == "rdoq":
        cu, per_job = n <= RDOQ_CU_MAX, n <= RDOQ_PER_JOB_MAX
    else:
        cu, per_job = entry == "inv" and one_launch and n <= INV_ONE_LAUNCH_MAX, n <= PER_JOB_MAX
    if cu:
        kernel = "residual_cu_kernel"
    elif stage == "tx2_job":
        kernel = "residual_wave_kernel"
    else:
        kernel = "residual_per_job_kernel" if per_job else "residual_kernel"
    return stage + "/" + kernel


_WRAP = ("no row of a matrix sums to more than 256 N (64 N for the 6-bit DCT-2, 242 for the DST) in "
         "absolute value, so a residual of at most 2^depth - 1 leaves either forward stage at no "
         "more than (2^depth - 1) * 2^(15 - depth) < 32768 (tests/test_tx_model.py evaluates it)")
_DST2 = ("the DST's second inverse stage shifts by 20 - depth >= 8 and its rows sum to 242: at most "
         "32768 * 242 >> 8 = 30976")
_SMALL = "tx_small_job: the one-wave path takes neither %s"
_CU = ("launch_residual gives residual_cu_kernel the inverse without distortion alone; its RDOQ "
       "instance quantises and belongs to the RDOQ suite, whose dispatch test runs it")
_TX2 = dict({k: _SMALL % "a 64-point side" for k in ("zero_out_hor", "zero_out_ver")},
            **{k: _SMALL % "the 4x4 DST nor transform skip"
               for k in ("form_dst4", "form_skip", "dc_preempted_skip", "dc_preempted_dst",
                         "dst1_clip_high", "dst1_clip_low", "dst1_inside", "dst2_inside")})
_NO_FWD = {k: _CU for k in ("fwd1_ge_2p14", "fwd1_below_2p14", "fwd2_ge_2p14", "fwd2_below_2p14",
                            "dist_ge_2p32", "dist_below_2p32", "dist_lane_ge_2p32",
                            "dist_lane_below_2p32")}
EXCLUDED = {
    "*": {"fwd1_wrap": _WRAP, "fwd2_wrap": _WRAP, "dst2_clip_high": _DST2, "dst2_clip_low": _DST2},
    "tx2_job/residual_wave_kernel": _TX2,
    "tx2_job/residual_cu_kernel": dict(_TX2, **_NO_FWD),
    "residual_job/residual_per_job_kernel": {},
    "residual_job/residual_kernel": {},
    "residual_job/residual_cu_kernel": _NO_FWD,
}
