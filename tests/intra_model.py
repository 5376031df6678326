"""Intra prediction restated in plain integers, with a counter on every decision it takes.

IntraPrediction::ComputeRefSamples / FilterRefSamples / UseFilteredRefSamples / Predict
(planar, DC, the 65 angular modes, both edge filters) and PredLmChroma (4:2:0), written from
oracle/xvc_oracle_intra.c and the description in include/xvcgpu.h.  Scalars are Python
integers; whole rows are numpy int64, which none of this arithmetic leaves.  Every function
takes a collections.Counter and adds to it.
tests/test_intra_model.py pins this file to the oracle on every case of tests/intra_cases.py
and the oracle to the reference's own code; tests/test_gpu_intra_cases.py runs every device
copy of the prediction on the same cases.

Keys:

  refs.none / .full / .partial   the three forms of ComputeRefSamples
  refs.bl.*    below-left: full, partial (0 < below_left < w, last sample repeated), or padded
               from_left / from_corner / from_above / mid (the first side that exists)
  refs.left.* refs.corner.* refs.above.*   present or padded
  refs.ar.*    above-right: full, partial (last sample repeated), padded
  filt.s<k>.on / .off   UseFilteredRefSamples of a luma block of size index k = (log2 w +
               log2 h) >> 1, for the modes that read the choice (all but DC); .at_thr: the
               mode's distance equals the threshold (off), .thr_plus_1: one more (on)
  filt.chroma_never     a chroma block (never filtered)
  pred.planar, pred.dc.post / .plain (with / without the DC edge filter), pred.dc.nonpow2
               (w != h: a division by a sum that is no power of two)
  ang.hor / ang.ver . zero / pos / neg   the angle's sign, per half of the modes
  ang.wt0      a row with weight 0 at a non-zero angle
  ang.proj     a negative angle that projects side samples (num_projected > 0)
  ang.proj_last   the projection reads the side's sample ph - 1, the last of the block's own
  edge.a0.*    a sample of the edge filter of modes 18 / 50 (">> 1"): inside, sat_zero, sat_max
  edge.a1.*    the same of modes 17, 19 / 49, 51 (">> 2")
  edge.off_large   DC or one of those angular modes on a luma block above 16 on a side: no
               edge filter
  lm.nb_<above><left>   which neighbours the model is fitted through
  lm.dx<r> lm.dy<r>     the sub-sampling step of the longer side
  lm.prescale<sh>       the shift that brings the sums to 15 bit + log2(count)
  lm.vxx_neg   the variance came out negative (after the pre-scale's rounding)
  lm.flat      vxx_s < 32: offset only
  lm.vxy_zero, lm.shift_xy.zero / .pos
  lm.clip_lo / lm.clip_hi   the slope clipped at -256 / 255
  lm.slope.neg / .zero / .pos
  lm.out.inside / .sat_zero / .sat_max   a predicted sample

Two properties of the LM arithmetic are asserted: total_shift >= 0 and the product of the
slope computation below 2^31 in magnitude (it is formed in 32 bit).  No case breaks either.

What the case set of tests/intra_cases.py reaches, per device path (all depths together;
test_census_floor asserts at least FLOOR = 8 of every key a path can reach; "-": the key is
exempted for that path by name, intra_cases.EXEMPT gives the reason):

  key                         pred batch    fused wave  SATD general     SATD rows            LM
  refs.none                         5450          2674            73            12
  refs.full                         5184          2527            70            12
  refs.partial                    143327         67443          1925           392
  refs.bl.full                     39127         18898           525           104
  refs.bl.partial                  32369         14476           435           104
  refs.bl.from_left                41881         19836           563           104
  refs.bl.from_corner              20332          9704           273            54
  refs.bl.from_above               14802          7056           199            38
  refs.bl.mid                       5450          2674            73            12
  refs.left.present               113377         53210          1523           312
  refs.left.padded                 40584         19434           545           104
  refs.corner.present              77015         36177          1035           208
  refs.corner.padded               76946         36467          1033           208
  refs.above.present              113671         53396          1527           312
  refs.above.padded                40290         19248           541           104
  refs.ar.full                     40117         19434           539           104
  refs.ar.partial                  32823         14796           441           104
  refs.ar.padded                   81021         38414          1088           208
  filt.s2.off                      13728         13728         13728             -
  filt.s3.on                        5728          4576          5728          1664
  filt.s3.off                      41528         33176         41528         12064
  filt.s3.at_thr                    2864          2288          2864           832
  filt.s3.thr_plus_1                2864          2288          2864           832
  filt.s4.on                       43456         11648         43456         11648
  filt.s4.off                       7760          2080          7760          2080
  filt.s4.at_thr                    3104           832          3104           832
  filt.s4.thr_plus_1                3104           832          3104           832
  filt.s5.on                       20480             -         20480             -
  filt.s5.off                        640             -           640             -
  filt.s5.at_thr                     640             -           640             -
  filt.s5.thr_plus_1                1280             -          1280             -
  filt.s6.off                       3168             -          3168             -
  filt.chroma_never                14220          5952             -             -
  pred.planar                       3253          1484          2068           416
  pred.dc.post                       988           988           988           416
  pred.dc.plain                     2265           496          1080             -
  pred.dc.nonpow2                   2336           828          1428             -
  ang.hor.zero                      3253          1484          2068           416
  ang.hor.pos                      35458         16800         33088          6656
  ang.hor.neg                      33390         15812         31020          6240
  ang.ver.zero                      3253          1484          2068           416
  ang.ver.pos                      35458         16800         33088          6656
  ang.ver.neg                      36643         17296         33088          6656
  ang.wt0                         242386         47008        195152         16640
  ang.proj                         58195         26112         54640         10816
  ang.proj_last                     5652          3924          5148          1248
  edge.a0.hor.inside                9130          9130          9130          4469
  edge.a0.hor.sat_zero               114           114           114            66
  edge.a0.hor.sat_max                916           916           916           457
  edge.a0.ver.inside                8434          8434          8434          4024
  edge.a0.ver.sat_zero              1431          1431          1431           742
  edge.a0.ver.sat_max                311           311           311           226
  edge.a1.hor.inside               19321         19321         19321          9488
  edge.a1.hor.sat_zero               108           108           108            68
  edge.a1.hor.sat_max                891           891           891           428
  edge.a1.ver.inside               18811         18811         18811          9116
  edge.a1.ver.sat_zero              1182          1182          1182           628
  edge.a1.ver.sat_max                359           359           359           240
  edge.off_large                    7560             -          7560             -
  lm.nb_00                                                                                    46
  lm.nb_01                                                                                   138
  lm.nb_10                                                                                   118
  lm.nb_11                                                                                   468
  lm.dx1                                                                                     402
  lm.dx2                                                                                      70
  lm.dx4                                                                                      18
  lm.dx8                                                                                      54
  lm.dx16                                                                                     42
  lm.dy1                                                                                     424
  lm.dy2                                                                                      70
  lm.dy4                                                                                      18
  lm.dy8                                                                                      48
  lm.dy16                                                                                     46
  lm.prescale0                                                                               606
  lm.prescale1                                                                                50
  lm.prescale2                                                                                54
  lm.prescale3                                                                                14
  lm.vxx_neg                                                                                   8
  lm.flat                                                                                    180
  lm.vxy_zero                                                                                187
  lm.shift_xy.zero                                                                           121
  lm.shift_xy.pos                                                                            423
  lm.clip_lo                                                                                  46
  lm.clip_hi                                                                                  53
  lm.slope.neg                                                                               216
  lm.slope.zero                                                                               70
  lm.slope.pos                                                                               258
  lm.out.inside                                                                           138500
  lm.out.sat_zero                                                                          13284
  lm.out.sat_max                                                                           21872

TEST INFRASTRUCTURE."""
import numpy as np

ANGLE = [-32, -29, -26, -23, -21, -19, -17, -15, -13, -11, -9, -7, -5, -3, -2, -1, 0,
         1, 2, 3, 5, 7, 9, 11, 13, 15, 17, 19, 21, 23, 26, 29, 32]
INV_ANGLE = [8192, 4096, 2731, 1638, 1170, 910, 745, 630, 546, 482, 431, 390, 356, 315, 282, 256]
FILTER_THR = [0, 20, 20, 14, 2, 0, 20, 0]
HAS_ABOVE_LEFT, HAS_ABOVE, HAS_LEFT = 1, 2, 4

REFS_KEYS = ["refs.none", "refs.full", "refs.partial", "refs.bl.full", "refs.bl.partial",
             "refs.bl.from_left", "refs.bl.from_corner", "refs.bl.from_above", "refs.bl.mid",
             "refs.left.present", "refs.left.padded", "refs.corner.present",
             "refs.corner.padded", "refs.above.present", "refs.above.padded", "refs.ar.full",
             "refs.ar.partial", "refs.ar.padded"]
MODE_KEYS = ["pred.planar", "pred.dc.post", "pred.dc.plain", "pred.dc.nonpow2"]
ANG_KEYS = ["ang.%s.%s" % (a, b) for a in ("hor", "ver") for b in ("zero", "pos", "neg")] + \
    ["ang.wt0", "ang.proj", "ang.proj_last"]
EDGE_KEYS = ["edge.a%d.%s.%s" % (a, d, o) for a in (0, 1) for d in ("hor", "ver")
             for o in ("inside", "sat_zero", "sat_max")] + ["edge.off_large"]
LM_KEYS = ["lm.nb_%d%d" % (a, b) for a in (0, 1) for b in (0, 1)] + \
    ["lm.d%s%d" % (a, r) for a in "xy" for r in (1, 2, 4, 8, 16)] + \
    ["lm.prescale%d" % s for s in (0, 1, 2, 3)] + \
    ["lm.vxx_neg", "lm.flat", "lm.vxy_zero", "lm.shift_xy.zero", "lm.shift_xy.pos",
     "lm.clip_lo", "lm.clip_hi", "lm.slope.neg", "lm.slope.zero", "lm.slope.pos",
     "lm.out.inside", "lm.out.sat_zero", "lm.out.sat_max"]


def filter_keys(size_indices):
    """The filt.* keys of luma blocks of these size indices (at_thr / thr_plus_1 where a mode
    at that distance exists: the largest distance is 16, planar's is 18)."""
    keys = []
    for k in sorted(size_indices):
        keys += ["filt.s%d.on" % k, "filt.s%d.off" % k]
        if FILTER_THR[k] <= 15:
            keys += ["filt.s%d.at_thr" % k, "filt.s%d.thr_plus_1" % k]
        if FILTER_THR[k] > 18:
            keys.remove("filt.s%d.on" % k)
    return keys


def log2(v):
    assert v > 0 and v & (v - 1) == 0
    return v.bit_length() - 1


def ref_samples(bd, w, h, nb, ar, bl, plane, x, y, n):
    """ComputeRefSamples + FilterRefSamples.  plane[y][x] is the block's first sample.
    -> (top, side, top_f, side_f): top[0] = corner, top[1 + i] above / above-right,
    side[i] left / below-left, i < w + h; the same filtered."""
    dc = 1 << (bd - 1)
    has_al, has_a, has_l = bool(nb & HAS_ABOVE_LEFT), bool(nb & HAS_ABOVE), bool(nb & HAS_LEFT)
    # what DetermineNeighbors guarantees (include/xvcgpu_types.h)
    assert (ar == 0 or has_a) and (bl == 0 or has_l) and 0 <= ar <= h and 0 <= bl <= w
    if not (has_al or has_a or has_l or ar or bl):
        n["refs.none"] += 1
    elif has_al and has_a and has_l and bl == w and ar == h:
        n["refs.full"] += 1
    else:
        n["refs.partial"] += 1
    side, above, corner = [None] * (w + h), [None] * (w + h), None
    if has_al:
        corner = int(plane[y - 1][x - 1])
    if has_l:
        for i in range(h + bl):
            side[i] = int(plane[y + i][x - 1])
        for i in range(bl, w):
            side[h + i] = side[h + bl - 1] if bl else None
    if has_a:
        for i in range(w + ar):
            above[i] = int(plane[y - 1][x + i])
        for i in range(ar, h):
            above[w + i] = above[w + ar - 1] if ar else None
    # padding, in the order below-left <- left <- corner <- above <- above-right
    if bl:
        n["refs.bl.full" if bl == w else "refs.bl.partial"] += 1
    else:
        if has_l:
            r, key = side[h - 1], "from_left"
        elif has_al:
            r, key = corner, "from_corner"
        elif has_a:
            r, key = above[0], "from_above"
        else:
            r, key = dc, "mid"
        n["refs.bl." + key] += 1
        side[h:] = [r] * w
    n["refs.left." + ("present" if has_l else "padded")] += 1
    if not has_l:
        side[:h] = [side[h]] * h
    n["refs.corner." + ("present" if has_al else "padded")] += 1
    if not has_al:
        corner = side[0]
    n["refs.above." + ("present" if has_a else "padded")] += 1
    if not has_a:
        above[:w] = [corner] * w
    n["refs.ar." + ("full" if ar == h else "partial" if ar else "padded")] += 1
    if not ar:
        above[w:] = [above[w - 1]] * h
    top = [corner] + above
    t = w + h
    top_f = [(2 * corner + top[1] + side[0] + 2) >> 2] + \
        [(2 * top[i] + top[i - 1] + top[i + 1] + 2) >> 2 for i in range(1, t)] + [top[t]]
    side_f = [(2 * side[0] + corner + side[1] + 2) >> 2] + \
        [(2 * side[i] + side[i - 1] + side[i + 1] + 2) >> 2 for i in range(1, t - 1)] + \
        [side[t - 1]]
    return top, side, top_f, side_f


def use_filtered(is_luma, w, h, mode, n):
    """UseFilteredRefSamples, 67-mode thresholds; counted for the modes that read it."""
    if not is_luma:
        if mode != 1:
            n["filt.chroma_never"] += 1
        return False
    k = (log2(w) + log2(h)) >> 1
    dist = min(abs(mode - 18), abs(mode - 50))
    on = dist > FILTER_THR[k]
    if mode != 1:
        n["filt.s%d.%s" % (k, "on" if on else "off")] += 1
        if dist == FILTER_THR[k]:
            n["filt.s%d.at_thr" % k] += 1
        if dist == FILTER_THR[k] + 1:
            n["filt.s%d.thr_plus_1" % k] += 1
    return on


def _edge(first, side, corner, shift, bd, key, n):
    """The edge filter of the near-straight modes on the first column (in the mode's frame)."""
    smax = (1 << bd) - 1
    out = []
    for y, v in enumerate(first):
        v = int(v) + ((side[y] - corner) >> shift)
        assert -32768 <= v <= 32767          # the reference holds it in 16 bit
        if v < 0:
            n[key + ".sat_zero"] += 1
            v = 0
        elif v > smax:
            n[key + ".sat_max"] += 1
            v = smax
        else:
            n[key + ".inside"] += 1
        out.append(v)
    return out


def _angular(bd, w, h, mode, post, large, top, side, n):
    hor = mode < 34
    half = "hor" if hor else "ver"
    if hor:    # swapped references, transposed block
        top, side = [top[0]] + side, top[1:]
        w, h = h, w
    angle_offset = 18 - mode if hor else mode - 50
    angle = ANGLE[16 + angle_offset]
    n["ang.%s.%s" % (half, "zero" if angle == 0 else "pos" if angle > 0 else "neg")] += 1
    if large and abs(angle) <= 1:
        n["edge.off_large"] += 1
    if angle == 0:
        tmp = np.tile(np.array(top[1:1 + w], np.int64), (h, 1))
        if post:
            tmp[:, 0] = _edge([top[1]] * h, side, top[0], 1, bd, "edge.a0." + half, n)
    else:
        line, base = top[1:] + [0], 0
        if angle < 0:
            num_projected = -((h * angle) >> 5) - 1
            inv = INV_ANGLE[-angle_offset - 1]
            proj = []
            for i in range(num_projected):
                k = ((128 + (i + 1) * inv) >> 8) - 1
                assert 0 <= k < w + h
                if k == h - 1:
                    n["ang.proj_last"] += 1
                proj.append(side[k])
            if num_projected > 0:
                n["ang.proj"] += 1
            line = proj[::-1] + top[:1 + w] + [0]
            base = num_projected + 1
        asum = angle * np.arange(1, h + 1, dtype=np.int64)
        off, wt = asum >> 5, asum & 31
        n["ang.wt0"] += int((wt == 0).sum())
        idx = base + off[:, None] + np.arange(w, dtype=np.int64)[None, :]
        assert idx.min() >= 0 and idx.max() + 1 < len(line)
        line = np.array(line, np.int64)
        a, b, wt = line[idx], line[idx + 1], wt[:, None]
        tmp = np.where(wt != 0, ((32 - wt) * a + wt * b + 16) >> 5, a)
        if post and abs(angle) == 1:
            tmp[:, 0] = _edge(tmp[:, 0], side, top[0], 2, bd, "edge.a1." + half, n)
    return tmp.T if hor else tmp


def predict(bd, is_luma, mode, w, h, refs, n):
    """IntraPrediction::Predict for mode 0..66 from ref_samples()'s result -> int64 [h, w]."""
    top, side, top_f, side_f = refs
    if use_filtered(is_luma, w, h, mode, n):
        ftop, fside = top_f, side_f
    else:
        ftop, fside = top, side
    post = is_luma and w <= 16 and h <= 16
    large = is_luma and not post
    if mode == 0:
        n["pred.planar"] += 1
        wl, hl = log2(w), log2(h)
        above, left = np.array(ftop[1:1 + w], np.int64), np.array(fside[:h], np.int64)
        top_right, bottom_left = ftop[1 + w], fside[h]
        shift = wl + hl + 1
        ys, xs = np.arange(h, dtype=np.int64)[:, None], np.arange(w, dtype=np.int64)[None, :]
        hor_ = (h - 1 - ys) * above[None, :] + (ys + 1) * bottom_left
        ver_ = (w - 1 - xs) * left[:, None] + (xs + 1) * top_right
        return ((hor_ << wl) + (ver_ << hl) + (1 << (shift - 1))) >> shift
    if mode == 1:    # always the unfiltered references
        total = w + h
        dc = (sum(top[1:1 + w]) + sum(side[:h]) + (total >> 1)) // total
        n["pred.dc.post" if post else "pred.dc.plain"] += 1
        if w != h:
            n["pred.dc.nonpow2"] += 1
        if large:
            n["edge.off_large"] += 1
        out = np.full((h, w), dc, np.int64)
        if post:
            out[1:, 0] = [(side[y] + 3 * dc + 2) >> 2 for y in range(1, h)]
            out[0, 1:] = [(top[1 + x] + 3 * dc + 2) >> 2 for x in range(1, w)]
            out[0, 0] = (top[1] + side[0] + 2 * dc + 2) >> 2
        return out
    return _angular(bd, w, h, mode, post, large, ftop, fside, n)


def _hadamard(k):
    m = np.array([[1]], np.int64)
    while len(m) < k:
        m = np.block([[m, m], [m, -m]])
    return m


_H = {k: _hadamard(k) for k in (2, 4, 8, 16)}


def satd(bd, a, b):
    """SampleMetric(kSatd)::CompareSample of two blocks (the tile shapes and normalisations
    of the oracle's xo_satd)."""
    h, w = a.shape
    if w == 2 or h == 2:
        tw, th = 2, 2
    elif w == 4 and h == 4:
        tw, th = 4, 4
    elif h == 4 and w > h:
        tw, th = 8, 4
    elif w == 4 and h > w:
        tw, th = 4, 8
    elif w > h:
        tw, th = 16, 8
    elif w < h:
        tw, th = 8, 16
    else:
        tw, th = 8, 8
    d = (a.astype(np.int64) - b.astype(np.int64)).reshape(h // th, th, w // tw, tw)
    t = np.einsum("ij,ajbk,kl->aibl", _H[th], d, _H[tw])
    sums = np.abs(t).sum(axis=(1, 3))
    if (tw, th) == (2, 2):
        tiles = sums
    elif (tw, th) == (4, 4):
        tiles = (sums + 1) >> 1
    elif tw == th:
        tiles = (sums + 2) >> 2
    else:     # (int)(2.0 * sum / sqrt(tw * th)): the square root of 32 and 128 is irrational,
        tiles = np.array([[int(2.0 * int(s) / float(np.sqrt(float(tw * th)))) for s in row]
                          for row in sums], np.int64)   # so the same doubles as the oracle's
    return int(tiles.sum()) >> (bd - 8)


def log2_floor(v):
    return v.bit_length() - 1 if v > 1 else 0


def lm_chroma(bd, x, y, w, h, luma, chroma, n):
    """PredLmChroma, 4:2:0: RescaleLuma, DeriveLmParams, AddLinearModel -> uint16 [h, w].
    (x, y, w, h) in chroma samples; availability = the picture's edges."""
    has_above, has_left = y > 0, x > 0
    n["lm.nb_%d%d" % (has_above, has_left)] += 1
    L = np.asarray(luma).astype(np.int64)

    def sub(yy, xx):        # the down-scaled luma at chroma position (y + yy, x + xx)
        r, c = 2 * (y + yy), 2 * (x + xx)
        if xx == 0 and not has_left:
            return int(L[r, c] + L[r + 1, c] + 1) >> 1
        return int(L[r, c - 1] + 2 * L[r, c] + L[r, c + 1] + L[r + 1, c - 1] + 2 * L[r + 1, c] +
                   L[r + 1, c + 1] + 4) >> 3

    scale, shift, offset = 0, 0, 1 << (bd - 1)
    if has_above or has_left:
        pairs = []
        if has_above:
            dx = max(w // h, 1) if has_left else 1
            n["lm.dx%d" % dx] += 1
            pairs += [(sub(-1, xx), int(chroma[y - 1][x + xx])) for xx in range(0, w, dx)]
        if has_left:
            dy = max(h // w, 1) if has_above else 1
            n["lm.dy%d" % dy] += 1
            pairs += [(sub(yy, -1), int(chroma[y + yy][x - 1])) for yy in range(0, h, dy)]
        sx, sy = sum(r for r, _ in pairs), sum(c for _, c in pairs)
        sxx, sxy = sum(r * r for r, _ in pairs), sum(r * c for r, c in pairs)
        assert sxx < 1 << 31 and sxy < 1 << 31
        size_shift = 1
        while (1 << size_shift) < len(pairs):
            size_shift += 1
        sh = max(size_shift + bd - 15, 0)
        n["lm.prescale%d" % sh] += 1
        if sh:
            sx, sy, sxx, sxy = ((v + (1 << (sh - 1))) >> sh for v in (sx, sy, sxx, sxy))
            size_shift -= sh
        avg_x, avg_y = sx >> size_shift, sy >> size_shift
        x_frac, y_frac = sx & ((1 << size_shift) - 1), sy & ((1 << size_shift) - 1)
        vxy = sxy - ((avg_x * avg_y) << size_shift) - avg_x * y_frac - avg_y * x_frac
        vxx = sxx - ((avg_x * avg_x) << size_shift) - 2 * avg_x * x_frac
        if vxx < 0:
            n["lm.vxx_neg"] += 1
        if vxy == 0:
            n["lm.vxy_zero"] += 1
        shift_xy = max(0 if vxy == 0 else log2_floor(abs(vxy)) - bd + 2, 0)
        shift_xx = max(0 if vxx == 0 else log2_floor(abs(vxx)) - 5, 0)
        vxy_s, vxx_s = vxy >> shift_xy, vxx >> shift_xx
        total_shift = bd + shift_xx + 4 + 7 - 13 - shift_xy
        if vxx_s < 32:
            n["lm.flat"] += 1
            offset = avg_y
        else:
            n["lm.shift_xy." + ("pos" if shift_xy else "zero")] += 1
            assert total_shift >= 0
            sc = vxy_s * (((1 << (bd + 4)) + vxx_s // 2) // vxx_s)
            assert abs(sc) < 1 << 31
            sc >>= total_shift
            if sc < -256:
                n["lm.clip_lo"] += 1
            if sc > 255:
                n["lm.clip_hi"] += 1
            sc = max(-256, min(255, sc))
            n["lm.slope." + ("neg" if sc < 0 else "pos" if sc else "zero")] += 1
            scale = 128 * sc
            base_shift = log2_floor(abs(scale) + (-1 if scale < 0 else 0)) - (5 if scale else 0)
            shift = 13 - base_shift
            scale >>= base_shift
            offset = avg_y - ((scale * avg_x) >> shift)
    smax = (1 << bd) - 1
    out = np.zeros((h, w), np.uint16)
    for yy in range(h):
        for xx in range(w):
            v = ((scale * sub(yy, xx)) >> shift) + offset
            if v < 0:
                n["lm.out.sat_zero"] += 1
            elif v > smax:
                n["lm.out.sat_max"] += 1
            else:
                n["lm.out.inside"] += 1
            out[yy, xx] = max(0, min(smax, v))
    return out
