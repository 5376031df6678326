"""numpy restatement of the decoder's output conversion, Resampler::ConvertTo
(xvc_common_lib/resample.cc:94-148) with CopyToWithResize (:340-393), the
shift / dither copies (:304-338, :475-551), resample::Resample (:741-856),
resample::BilinearResample (:891-930) and ConvertColorSpace (:396-474),
written from the algorithm.

Edge rule: positions outside the picture are clamped to the picture's internal
size (what YuvPicture::PadBorder replicates from), so a picture is read as if
it were padded.  Planes are the picture's internal 4:2:0 planes (2-D arrays);
the display size selects the part that is converted.
"""
import numpy as np

SCALE_ONE = 1 << 15  # kScaleFactor (kPositionPrecision 15)
COLOR_BD = 12        # kColorConversionBitdepth

# kUpsampleFilter [phase][tap at -3..4] and kDownsampleFilters
# [filter][phase][tap at -5..6]
UP_FILTER = np.array([
    [  0,   0,   0,  64,   0,   0,   0,   0],
    [  0,   1,  -3,  63,   4,  -2,   1,   0],
    [ -1,   2,  -5,  62,   8,  -3,   1,   0],
    [ -1,   3,  -8,  60,  13,  -4,   1,   0],
    [ -1,   4, -10,  58,  17,  -5,   1,   0],
    [ -1,   4, -11,  52,  26,  -8,   3,  -1],
    [ -1,   3,  -9,  47,  31, -10,   4,  -1],
    [ -1,   4, -11,  45,  34, -10,   4,  -1],
    [ -1,   4, -11,  40,  40, -11,   4,  -1],
    [ -1,   4, -10,  34,  45, -11,   4,  -1],
    [ -1,   4, -10,  31,  47,  -9,   3,  -1],
    [ -1,   3,  -8,  26,  52, -11,   4,  -1],
    [  0,   1,  -5,  17,  58, -10,   4,  -1],
    [  0,   1,  -4,  13,  60,  -8,   3,  -1],
    [  0,   1,  -3,   8,  62,  -5,   2,  -1],
    [  0,   1,  -2,   4,  63,  -3,   1,   0],
], np.int64)

DOWN_FILTER = np.array([
    [
        [  0,   0,   0,   0,   0, 128,   0,   0,   0,   0,   0,   0],
        [  0,   0,   0,   2,  -6, 127,   7,  -2,   0,   0,   0,   0],
        [  0,   0,   0,   3, -12, 125,  16,  -5,   1,   0,   0,   0],
        [  0,   0,   0,   4, -16, 120,  26,  -7,   1,   0,   0,   0],
        [  0,   0,   0,   5, -18, 114,  36, -10,   1,   0,   0,   0],
        [  0,   0,   0,   5, -20, 107,  46, -12,   2,   0,   0,   0],
        [  0,   0,   0,   5, -21,  99,  57, -15,   3,   0,   0,   0],
        [  0,   0,   0,   5, -20,  89,  68, -18,   4,   0,   0,   0],
        [  0,   0,   0,   4, -19,  79,  79, -19,   4,   0,   0,   0],
        [  0,   0,   0,   4, -18,  68,  89, -20,   5,   0,   0,   0],
        [  0,   0,   0,   3, -15,  57,  99, -21,   5,   0,   0,   0],
        [  0,   0,   0,   2, -12,  46, 107, -20,   5,   0,   0,   0],
        [  0,   0,   0,   1, -10,  36, 114, -18,   5,   0,   0,   0],
        [  0,   0,   0,   1,  -7,  26, 120, -16,   4,   0,   0,   0],
        [  0,   0,   0,   1,  -5,  16, 125, -12,   3,   0,   0,   0],
        [  0,   0,   0,   0,  -2,   7, 127,  -6,   2,   0,   0,   0],
    ],
    [
        [  0,   2,   0, -14,  33,  86,  33, -14,   0,   2,   0,   0],
        [  0,   1,   1, -14,  29,  85,  38, -13,  -1,   2,   0,   0],
        [  0,   1,   2, -14,  24,  84,  43, -12,  -2,   2,   0,   0],
        [  0,   1,   2, -13,  19,  83,  48, -11,  -3,   2,   0,   0],
        [  0,   0,   3, -13,  15,  81,  53, -10,  -4,   3,   0,   0],
        [  0,   0,   3, -12,  11,  79,  57,  -8,  -5,   3,   0,   0],
        [  0,   0,   3, -11,   7,  76,  62,  -5,  -7,   3,   0,   0],
        [  0,   0,   3, -10,   3,  73,  65,  -2,  -7,   3,   0,   0],
        [  0,   0,   3,  -9,   0,  70,  70,   0,  -9,   3,   0,   0],
        [  0,   0,   3,  -7,  -2,  65,  73,   3, -10,   3,   0,   0],
        [  0,   0,   3,  -7,  -5,  62,  76,   7, -11,   3,   0,   0],
        [  0,   0,   3,  -5,  -8,  57,  79,  11, -12,   3,   0,   0],
        [  0,   0,   3,  -4, -10,  53,  81,  15, -13,   3,   0,   0],
        [  0,   0,   2,  -3, -11,  48,  83,  19, -13,   2,   1,   0],
        [  0,   0,   2,  -2, -12,  43,  84,  24, -14,   2,   1,   0],
        [  0,   0,   2,  -1, -13,  38,  85,  29, -14,   1,   1,   0],
    ],
    [
        [  0,   5,  -6, -10,  37,  76,  37, -10,  -6,   5,   0,   0],
        [  0,   5,  -4, -11,  33,  76,  40,  -9,  -7,   5,   0,   0],
        [ -1,   5,  -3, -12,  29,  75,  45,  -7,  -8,   5,   0,   0],
        [ -1,   4,  -2, -13,  25,  75,  48,  -5,  -9,   5,   1,   0],
        [ -1,   4,  -1, -13,  22,  73,  52,  -3, -10,   4,   1,   0],
        [ -1,   4,   0, -13,  18,  72,  55,  -1, -11,   4,   2,  -1],
        [ -1,   4,   1, -13,  14,  70,  59,   2, -12,   3,   2,  -1],
        [ -1,   3,   1, -13,  11,  68,  62,   5, -12,   3,   2,  -1],
        [ -1,   3,   2, -13,   8,  65,  65,   8, -13,   2,   3,  -1],
        [ -1,   2,   3, -12,   5,  62,  68,  11, -13,   1,   3,  -1],
        [ -1,   2,   3, -12,   2,  59,  70,  14, -13,   1,   4,  -1],
        [ -1,   2,   4, -11,  -1,  55,  72,  18, -13,   0,   4,  -1],
        [  0,   1,   4, -10,  -3,  52,  73,  22, -13,  -1,   4,  -1],
        [  0,   1,   5,  -9,  -5,  48,  75,  25, -13,  -2,   4,  -1],
        [  0,   0,   5,  -8,  -7,  45,  75,  29, -12,  -3,   5,  -1],
        [  0,   0,   5,  -7,  -9,  40,  76,  33, -11,  -4,   5,   0],
    ],
    [
        [  2,  -3,  -9,   6,  39,  58,  39,   6,  -9,  -3,   2,   0],
        [  2,  -3,  -9,   4,  38,  58,  43,   7,  -9,  -4,   1,   0],
        [  2,  -2,  -9,   2,  35,  58,  44,   9,  -8,  -4,   1,   0],
        [  1,  -2,  -9,   1,  34,  58,  46,  11,  -8,  -5,   1,   0],
        [  1,  -1,  -8,  -1,  31,  57,  47,  13,  -7,  -5,   1,   0],
        [  1,  -1,  -8,  -2,  29,  56,  49,  15,  -7,  -6,   1,   1],
        [  1,   0,  -8,  -3,  26,  55,  51,  17,  -7,  -6,   1,   1],
        [  1,   0,  -7,  -4,  24,  54,  52,  19,  -6,  -7,   1,   1],
        [  1,   0,  -7,  -5,  22,  53,  53,  22,  -5,  -7,   0,   1],
        [  1,   1,  -7,  -6,  19,  52,  54,  24,  -4,  -7,   0,   1],
        [  1,   1,  -6,  -7,  17,  51,  55,  26,  -3,  -8,   0,   1],
        [  1,   1,  -6,  -7,  15,  49,  56,  29,  -2,  -8,  -1,   1],
        [  0,   1,  -5,  -7,  13,  47,  57,  31,  -1,  -8,  -1,   1],
        [  0,   1,  -5,  -8,  11,  46,  58,  34,   1,  -9,  -2,   1],
        [  0,   1,  -4,  -8,   9,  44,  58,  35,   2,  -9,  -2,   2],
        [  0,   1,  -4,  -9,   7,  43,  58,  38,   4,  -9,  -3,   2],
    ],
    [
        [ -2,  -7,   0,  17,  35,  43,  35,  17,   0,  -7,  -5,   2],
        [ -2,  -7,  -1,  16,  34,  43,  36,  18,   1,  -7,  -5,   2],
        [ -1,  -7,  -1,  14,  33,  43,  36,  19,   1,  -6,  -5,   2],
        [ -1,  -7,  -2,  13,  32,  42,  37,  20,   3,  -6,  -5,   2],
        [  0,  -7,  -3,  12,  31,  42,  38,  21,   3,  -6,  -5,   2],
        [  0,  -7,  -3,  11,  30,  42,  39,  23,   4,  -6,  -6,   1],
        [  0,  -7,  -4,  10,  29,  42,  40,  24,   5,  -6,  -6,   1],
        [  1,  -7,  -4,   9,  27,  41,  40,  25,   6,  -5,  -6,   1],
        [  1,  -6,  -5,   7,  26,  41,  41,  26,   7,  -5,  -6,   1],
        [  1,  -6,  -5,   6,  25,  40,  41,  27,   9,  -4,  -7,   1],
        [  1,  -6,  -6,   5,  24,  40,  42,  29,  10,  -4,  -7,   0],
        [  1,  -6,  -6,   4,  23,  39,  42,  30,  11,  -3,  -7,   0],
        [  2,  -5,  -6,   3,  21,  38,  42,  31,  12,  -3,  -7,   0],
        [  2,  -5,  -6,   3,  20,  37,  42,  32,  13,  -2,  -7,  -1],
        [  2,  -5,  -6,   1,  19,  36,  43,  33,  14,  -1,  -7,  -1],
        [  2,  -5,  -7,   1,  18,  36,  43,  34,  16,  -1,  -7,  -2],
    ],
    [
        [ -6,  -3,   5,  19,  31,  36,  31,  19,   5,  -3,  -6,   0],
        [ -6,  -4,   4,  18,  31,  37,  32,  20,   6,  -3,  -6,  -1],
        [ -6,  -4,   4,  17,  30,  36,  33,  21,   7,  -3,  -6,  -1],
        [ -5,  -5,   3,  16,  30,  36,  33,  22,   8,  -2,  -6,  -2],
        [ -5,  -5,   2,  15,  29,  36,  34,  23,   9,  -2,  -6,  -2],
        [ -5,  -5,   2,  15,  28,  36,  34,  24,  10,  -2,  -6,  -3],
        [ -4,  -5,   1,  14,  27,  36,  35,  24,  10,  -1,  -6,  -3],
        [ -4,  -5,   0,  13,  26,  35,  35,  25,  11,   0,  -5,  -3],
        [ -4,  -6,   0,  12,  26,  36,  36,  26,  12,   0,  -6,  -4],
        [ -3,  -5,   0,  11,  25,  35,  35,  26,  13,   0,  -5,  -4],
        [ -3,  -6,  -1,  10,  24,  35,  36,  27,  14,   1,  -5,  -4],
        [ -3,  -6,  -2,  10,  24,  34,  36,  28,  15,   2,  -5,  -5],
        [ -2,  -6,  -2,   9,  23,  34,  36,  29,  15,   2,  -5,  -5],
        [ -2,  -6,  -2,   8,  22,  33,  36,  30,  16,   3,  -5,  -5],
        [ -1,  -6,  -3,   7,  21,  33,  36,  30,  17,   4,  -4,  -6],
        [ -1,  -6,  -3,   6,  20,  32,  37,  31,  18,   4,  -4,  -6],
    ],
    [
        [ -9,   0,   9,  20,  28,  32,  28,  20,   9,   0,  -9,   0],
        [ -9,   0,   8,  19,  28,  32,  29,  20,  10,   0,  -4,  -5],
        [ -9,  -1,   8,  18,  28,  32,  29,  21,  10,   1,  -4,  -5],
        [ -9,  -1,   7,  18,  27,  32,  30,  22,  11,   1,  -4,  -6],
        [ -8,  -2,   6,  17,  27,  32,  30,  22,  12,   2,  -4,  -6],
        [ -8,  -2,   6,  16,  26,  32,  31,  23,  12,   2,  -4,  -6],
        [ -8,  -2,   5,  16,  26,  31,  31,  23,  13,   3,  -3,  -7],
        [ -8,  -3,   5,  15,  25,  31,  31,  24,  14,   4,  -3,  -7],
        [ -7,  -3,   4,  14,  25,  31,  31,  25,  14,   4,  -3,  -7],
        [ -7,  -3,   4,  14,  24,  31,  31,  25,  15,   5,  -3,  -8],
        [ -7,  -3,   3,  13,  23,  31,  31,  26,  16,   5,  -2,  -8],
        [ -6,  -4,   2,  12,  23,  31,  32,  26,  16,   6,  -2,  -8],
        [ -6,  -4,   2,  12,  22,  30,  32,  27,  17,   6,  -2,  -8],
        [ -6,  -4,   1,  11,  22,  30,  32,  27,  18,   7,  -1,  -9],
        [ -5,  -4,   1,  10,  21,  29,  32,  28,  18,   8,  -1,  -9],
        [ -5,  -4,   0,  10,  20,  29,  32,  28,  19,   8,   0,  -9],
    ],
    [
        [ -8,   7,  13,  18,  22,  24,  22,  18,  13,   7,   2, -10],
        [ -8,   7,  13,  18,  22,  23,  22,  19,  13,   7,   2, -10],
        [ -8,   6,  12,  18,  22,  23,  22,  19,  14,   8,   2, -10],
        [ -9,   6,  12,  17,  22,  23,  23,  19,  14,   8,   3, -10],
        [ -9,   6,  12,  17,  21,  23,  23,  19,  14,   9,   3, -10],
        [ -9,   5,  11,  17,  21,  23,  23,  20,  15,   9,   3, -10],
        [ -9,   5,  11,  16,  21,  23,  23,  20,  15,   9,   4, -10],
        [ -9,   5,  10,  16,  21,  23,  23,  20,  15,  10,   4, -10],
        [-10,   5,  10,  16,  20,  23,  23,  20,  16,  10,   5, -10],
        [-10,   4,  10,  15,  20,  23,  23,  21,  16,  10,   5,  -9],
        [-10,   4,   9,  15,  20,  23,  23,  21,  16,  11,   5,  -9],
        [-10,   3,   9,  15,  20,  23,  23,  21,  17,  11,   5,  -9],
        [-10,   3,   9,  14,  19,  23,  23,  21,  17,  12,   6,  -9],
        [-10,   3,   8,  14,  19,  23,  23,  22,  17,  12,   6,  -9],
        [-10,   2,   8,  14,  19,  22,  23,  22,  18,  12,   6,  -8],
        [-10,   2,   7,  13,  19,  22,  23,  22,  18,  13,   7,  -8],
    ],
], np.int64)

# ConvertColorSpace kM: 0 = undefined (the 709 table), 1 = 601, 2 = 709, 3 = 2020
MATRICES = np.array([
    [[1192, 0, 1877], [1192, -223, -558], [1192, 2212, 0]],
    [[1192, 0, 1671], [1192, -410, -851], [1192, 2112, 0]],
    [[1192, 0, 1877], [1192, -223, -558], [1192, 2212, 0]],
    [[1192, 0, 1758], [1192, -196, -681], [1192, 2243, 0]],
], np.int64)


def filter_from_scale(scale):
    """GetFilterFromScale"""
    k = SCALE_ONE
    for lim, f in ((15 * k // 4, 7), (20 * k // 7, 6), (5 * k // 2, 5), (2 * k, 4),
                   (5 * k // 3, 3), (5 * k // 4, 2), (20 * k // 19, 1)):
        if scale > lim:
            return f
    return 0


def scale_of(src, dst):
    return ((src << 15) + (dst >> 1)) // dst


def plane_size(w, h, cf, c):
    """util::ScaleSizeX / ScaleSizeY of plane c of an output format"""
    if c == 0:
        return w, h
    return (w if cf >= 3 else w >> 1), (h if cf >= 2 else h >> 1)


def resolve(fmt, disp_w, disp_h, bd):
    """Decoder's defaults (decoder.cc:162-176) for a 4:2:0 source."""
    f = dict(width=0, height=0, chroma_format=255, color_matrix=0, bitdepth=0, dither=0)
    f.update(fmt)
    f["width"] = f["width"] or disp_w
    f["height"] = f["height"] or disp_h
    if f["chroma_format"] == 255:
        f["chroma_format"] = 1
    f["bitdepth"] = f["bitdepth"] or bd
    return f


def total_samples(f):
    """util::GetTotalNumSamples"""
    w, h, cf = f["width"], f["height"], f["chroma_format"]
    if cf == 4:
        return 4 * w * h
    if cf == 0:
        return w * h
    cw, ch = plane_size(w, h, cf, 1)
    return w * h + 2 * cw * ch


def output_bytes(f):
    return total_samples(f) * (2 if f["bitdepth"] > 8 else 1)


def _filter_1d(get, pos, scale):
    """FilterHor / FilterVer before the shift, along the last axis: get(idx)
    -> the samples at positions idx (one per output sample)."""
    sub, full = pos & 15, pos >> 4
    if scale < SCALE_ONE:
        s = 0
        for k in range(8):
            s = s + get(full + k - 3) * UP_FILTER[sub, k]
        return s
    if scale == SCALE_ONE:
        return get(full) << 6
    coef = DOWN_FILTER[filter_from_scale(scale)][sub]
    s = 0
    for k in range(12):
        s = s + get(full + k - 5) * coef[:, k]
    return s >> 1


def resample(plane, sw, sh, dw, dh, src_bd, dst_bd):
    """resample::Resample of the sw x sh top-left part of `plane` to dw x dh,
    positions clamped to the plane.  Returns int64 samples."""
    p = plane.astype(np.int64)
    ih, iw = p.shape
    sx, sy = scale_of(sw, dw), scale_of(sh, dh)
    shift_hor = max(src_bd - 10, 0)
    rows = p[np.clip(np.arange(-8, sh + 8), 0, ih - 1)]
    pos_x = (np.arange(dw, dtype=np.int64) * sx) >> 11
    tmp = _filter_1d(lambda o: rows[:, np.clip(o, 0, iw - 1)], pos_x, sx)
    tmp = np.clip(tmp >> shift_hor, 0, 0xffff)
    pos_y = (np.arange(dh, dtype=np.int64) * sy) >> 11
    shift_ver = 12 - shift_hor + src_bd - dst_bd
    tmp_t = tmp.T  # tmp row r + 8 = source row r; filter the columns as rows
    out = _filter_1d(lambda o: tmp_t[:, o + 8], pos_y, sy).T
    return np.clip(out >> shift_ver, 0, (1 << dst_bd) - 1)


def bilinear(plane, sw, sh, src_bd, dst_bd):
    """resample::BilinearResample of the sw x sh part to 2sw x 2sh, positions
    clamped to the plane; the result truncated to the output sample type."""
    p = plane.astype(np.int64)
    ih, iw = p.shape
    ys, xs = np.arange(sh), np.arange(sw)
    y1, x1 = np.minimum(ys + 1, ih - 1), np.minimum(xs + 1, iw - 1)
    a = p[np.ix_(ys, xs)]
    b = p[np.ix_(ys, x1)]
    c = p[np.ix_(y1, xs)]
    d = p[np.ix_(y1, x1)]
    shift = dst_bd - src_bd
    assert shift != 1, "undefined in the reference (>> -1)"
    vals = (a, a + b, a + c, a + b + c + d + 2)
    out = np.zeros((2 * sh, 2 * sw), np.int64)
    for (oy, ox), v, sh_ in zip(((0, 0), (0, 1), (1, 0), (1, 1)), vals, (0, 1, 1, 2)):
        out[oy::2, ox::2] = v << (shift - sh_) if shift > 1 else v >> (-shift + sh_)
    return out & (0xffff if dst_bd > 8 else 0xff)


def shift_copy(plane, w, h, src_bd, out_bd, dither):
    """CopyToBytesWithShift of the w x h part (the error feedback of the dither
    runs through the plane in raster order)."""
    v = plane[:h, :w].astype(np.int64)
    smax = (1 << out_bd) - 1
    if out_bd > 8:
        if out_bd >= src_bd:
            return (v << (out_bd - src_bd)) & 0xffff
    elif src_bd <= 8:
        return v & 0xff
    s = src_bd - out_bd
    if not dither:
        return np.minimum((v + (1 << (s - 1))) >> s, smax)
    flat = v.reshape(-1)
    before = (np.concatenate(([0], np.cumsum(flat)[:-1])) & ((1 << s) - 1))
    return np.minimum((before + flat) >> s, smax).reshape(h, w)


def convert_planes(planes, bd, disp_w, disp_h, f):
    """The planes ConvertTo produces (before ARGB's matrix), and the depth."""
    cf = f["chroma_format"]
    dst_bd = COLOR_BD if cf == 4 else f["bitdepth"]
    out = []
    for c in range(1 if cf == 0 else 3):
        sw, sh = (disp_w, disp_h) if c == 0 else (disp_w >> 1, disp_h >> 1)
        dw, dh = plane_size(f["width"], f["height"], 3 if cf == 4 else cf, c)
        if (dw, dh) == (sw, sh):
            out.append(shift_copy(planes[c], sw, sh, bd, dst_bd, f["dither"]))
        elif c and (dw, dh) == (2 * sw, 2 * sh):
            out.append(bilinear(planes[c], sw, sh, bd, dst_bd))
        else:
            out.append(resample(planes[c], sw, sh, dw, dh, bd, dst_bd))
    return out, dst_bd


def color_convert(y, u, v, out_bd, matrix):
    """ConvertColorSpace (and ConvertColorSpace8bit709, the same arithmetic)
    from 12-bit components: (h, w, 4) values R, G, B, alpha."""
    m = MATRICES[matrix]
    smax = (1 << out_bd) - 1
    shift = 10 + COLOR_BD - out_bd
    c = y - (16 << (COLOR_BD - 8))
    d = u - (128 << (COLOR_BD - 8))
    e = v - (128 << (COLOR_BD - 8))
    r = (m[0, 0] * c + m[0, 2] * e) >> shift
    g = (m[1, 0] * c + m[1, 1] * d + m[1, 2] * e) >> shift
    b = (m[2, 0] * c + m[2, 1] * d) >> shift
    return np.stack([np.clip(r, 0, smax), np.clip(g, 0, smax), np.clip(b, 0, smax),
                     np.full_like(r, smax)], axis=-1)


def convert_to(planes, bd, disp_w, disp_h, fmt):
    """Resampler::ConvertTo: the output bytes of one picture.  planes: the
    picture's internal Y, U, V planes; fmt: unresolved fields allowed."""
    f = resolve(fmt, disp_w, disp_h, bd)
    dt = np.dtype("<u2") if f["bitdepth"] > 8 else np.uint8
    out, _ = convert_planes(planes, bd, disp_w, disp_h, f)
    if f["chroma_format"] == 4:
        return color_convert(*out, f["bitdepth"], f["color_matrix"]).astype(dt).tobytes()
    return b"".join(o.astype(dt).tobytes() for o in out)


def _taps_inside(n_dst, n_src, n_int, kind):
    """Per output position: every sample the filter reads lies inside the
    picture's internal size n_int (so the reference's border is not read)."""
    x = np.arange(n_dst, dtype=np.int64)
    if kind == "shift":
        return np.ones(n_dst, bool)
    if kind == "bilinear":
        return (x >> 1) + 1 <= n_int - 1
    s = scale_of(n_src, n_dst)
    full = (x * s) >> 15
    lo, hi = (-3, 4) if s < SCALE_ONE else ((0, 0) if s == SCALE_ONE else (-5, 6))
    return (full + lo >= 0) & (full + hi <= n_int - 1)


def interior_mask(fmt, disp_w, disp_h, bd, int_w, int_h):
    """Per output byte: True where the output depends on picture samples only,
    never on the padded border (for pictures the reference did not pad)."""
    f = resolve(fmt, disp_w, disp_h, bd)
    cf = f["chroma_format"]
    bps = 2 if f["bitdepth"] > 8 else 1
    masks = []
    for c in range(1 if cf == 0 else 3):
        sw, sh = (disp_w, disp_h) if c == 0 else (disp_w >> 1, disp_h >> 1)
        iw, ih = (int_w, int_h) if c == 0 else (int_w >> 1, int_h >> 1)
        dw, dh = plane_size(f["width"], f["height"], 3 if cf == 4 else cf, c)
        if (dw, dh) == (sw, sh):
            kind = "shift"
        elif c and (dw, dh) == (2 * sw, 2 * sh):
            kind = "bilinear"
        else:
            kind = "resample"
        masks.append(_taps_inside(dh, sh, ih, kind)[:, None] &
                     _taps_inside(dw, sw, iw, kind)[None, :])
    if cf == 4:
        m = masks[0] & masks[1] & masks[2]
        return np.repeat(m.reshape(-1), 4 * bps)
    return np.concatenate([np.repeat(m.reshape(-1), bps) for m in masks])
