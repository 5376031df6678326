"""Directed cases for the forward and inverse transform stages (csrc/k_tx.h, csrc/k_tx2.h).

Pure numpy and deterministic; the matrices are the oracle's (tx_model.matrix).  A case is a dict:
  family, kind, bd, blk (w, h, comp, tx_hor, tx_ver, dst4x4, qp), orig, pred (h x w, uint16),
  levels (h x w int16) and nnz for the cases that enter behind the quantiser, None for those that
  enter at the residual.
Depths 8, 10, 12 in full, 9 and 11 reduced to one pass of each family.

  1 types     every valid (tx_hor, tx_ver) of {0,1,2,3,4,5,7}^2 at every luma shape, of {0,1,7}^2
              at every chroma shape; the 4x4 DST and transform skip; residual uniform over
              +-(2^bd - 1)
  2 fwd_max   full-swing residuals whose signs follow a basis row of each matrix: DC, the last
              kept row, the row of largest L1 norm
  3 inv_clip  crafted levels whose dequantised coefficients are +32767 / -32768 with the signs of a
              matrix column (both inverse stages pushed both ways), the same pattern scaled so
              that stage 1 stays inside, so that nothing clips, and down to one step; prediction
              0 / maximum / mid-grey; the original opposite the residual, for the largest
              distortion (and, at 16 columns, four saturated neighbours of a row: one lane's
              partial sum beyond 2^32)
  4 dc        nnz = 1 with the level at position 0: +-1, +-the largest unclipped, +-the smallest
              clipped, over the DCT-2 pairs (shortcut) and the pairs that refuse it, the DST and
              skip; the level elsewhere; nnz = 2; a level outside a 64-point side's kept corner
  5 nothing   nnz = 0, the level buffer poisoned
  6 launch    batches beyond the launch thresholds built from a few distinct tiles (launch_batch)

What the binding never passes (tx_model.valid_block) is never generated: EXCLUSIONS names it.
modelled(bd) runs the model over the depth's cases; the frame pass's pictures (swing_pictures) are
family 2's residuals laid over a CU partition.
"""
import functools

import numpy as np

import tx_model as tm

DEPTHS = (8, 10, 12)
REDUCED = (9, 11)
ALL_DEPTHS = DEPTHS + REDUCED
LUMA_SIDES = (64, 32, 16, 8, 4)
CHROMA_SIDES = (32, 16, 8, 4, 2)
LUMA_TYPES = (0, 1, 2, 3, 4, 5, 7)
CHROMA_TYPES = (0, 1, 7)
LUMA_PAIRS = [(a, b) for a in LUMA_TYPES for b in LUMA_TYPES]
CHROMA_PAIRS = [(a, b) for a in CHROMA_TYPES for b in CHROMA_TYPES]
# (w, h, comp)
MAX_SHAPES = [(4, 4, 0), (16, 16, 0), (16, 4, 0), (4, 16, 0), (8, 8, 0), (32, 32, 0), (64, 64, 0),
              (64, 4, 0), (2, 8, 1)]
DC_SHAPES = MAX_SHAPES + [(32, 8, 0), (8, 2, 1), (2, 2, 1), (16, 8, 1)]
CLIP_PAIRS = [(0, 0), (1, 7), (7, 0), (5, 3), (2, 4), (3, 5), (4, 2)]
DC_PAIRS = [(0, 0), (1, 7), (7, 0), (7, 7), (5, 0), (0, 3), (5, 3)]
SKIP_SHAPES = [(4, 4, 0), (4, 4, 1), (4, 2, 1), (2, 4, 1), (2, 2, 1)]
POISON = 0x5a5a

EXCLUSIONS = {
    "low_precision_side_2_or_64": "XVC_TX_DCT2_LOW exists for sides 4 .. 32 (TransformData::"
                                  "kDct2Transform4..32); the table layout has no such entry",
    "side_2_beyond_dct2": "a side of 2 has the DCT-2 matrix alone",
    "dst4x4_elsewhere": "can_dst_4x4 is intra luma 4x4 with the default types",
    "skip_above_4x4": "transform skip is signalled for blocks up to 4x4",
}


def blk(w, h, comp, tx_hor=0, tx_ver=0, dst4x4=0, qp=30):
    return dict(w=w, h=h, comp=comp, tx_hor=tx_hor, tx_ver=tx_ver, dst4x4=dst4x4, qp=qp)


def shapes(comp):
    sides = CHROMA_SIDES if comp else LUMA_SIDES
    return [(w, h, comp) for h in sides for w in sides]


def cell(w, h, comp):
    """Where tests/test_gpu_quant_cases.py::grid_blocks puts the shape: the outer product of the
    sides in descending order inside a 128 x 128 picture, each block aligned to its own size."""
    sides = CHROMA_SIDES if comp else LUMA_SIDES
    off = dict(zip(sides, np.r_[0, np.cumsum(sides)[:-1]].tolist()))
    return off[w], off[h]


def pair_for(pair, w, h, comp):
    """The pair itself where it is valid for the shape, else None."""
    ok = tm.valid_type(pair[0], w) and tm.valid_type(pair[1], h) and \
        (not comp or (pair[0] in CHROMA_TYPES and pair[1] in CHROMA_TYPES))
    return pair if ok else None


def nearest_pair(pair, w, h, comp):
    """The pair with every type the shape cannot take replaced by the high-precision DCT-2."""
    fix = lambda t, size: t if tm.valid_type(t, size) and (not comp or t in CHROMA_TYPES) else 1
    return fix(pair[0], w), fix(pair[1], h)


def case(family, kind, bd, b, orig, pred, levels=None, nnz=None):
    assert tm.valid_block(b), b
    smax = (1 << bd) - 1
    assert 0 <= int(np.min(orig)) and int(np.max(orig)) <= smax
    assert 0 <= int(np.min(pred)) and int(np.max(pred)) <= smax
    return dict(family=family, kind=kind, bd=bd, blk=b, orig=np.asarray(orig, np.uint16),
                pred=np.asarray(pred, np.uint16),
                levels=None if levels is None else np.asarray(levels, np.int16), nnz=nnz)


def uniform_residual(rng, bd, w, h):
    """orig, pred with orig - pred uniform over [-(2^bd - 1), 2^bd - 1]."""
    smax = (1 << bd) - 1
    r = rng.integers(-smax, smax + 1, (h, w))
    lo, hi = np.maximum(0, -r), np.minimum(smax, smax - r)
    pred = lo + (rng.random((h, w)) * (hi - lo + 1)).astype(np.int64)
    return pred + r, pred


def signed_residual(bd, sign):
    """orig, pred at the range ends: orig - pred = +-(2^bd - 1) with the given signs."""
    smax = (1 << bd) - 1
    return np.where(sign >= 0, smax, 0), np.where(sign >= 0, 0, smax)


def stage_matrices(b):
    """(Mh, Mv) of the block's two stages, rows = basis functions: the DST's formulas as a matrix."""
    if b["dst4x4"]:
        return tm.DST4, tm.DST4
    return tm.matrix(b["tx_hor"], b["w"]), tm.matrix(b["tx_ver"], b["h"])


# ---- family 1 -----------------------------------------------------------------------------------

def _special_blocks():
    return [blk(4, 4, 0, dst4x4=1)] + [blk(w, h, c, tm.TX_SKIP) for w, h, c in SKIP_SHAPES]


def type_cases(bd):
    rng = np.random.default_rng(9100 + bd)
    out = []
    if bd in REDUCED:       # one grid: the pairs walk over the shapes
        for comp, pairs in ((0, LUMA_PAIRS), (1, CHROMA_PAIRS)):
            for i, (w, h, _) in enumerate(shapes(comp)):
                p = nearest_pair(pairs[(5 * i + 3) % len(pairs)], w, h, comp)
                out.append(case(1, "types", bd, blk(w, h, comp, p[0], p[1], qp=24 + i % 12),
                                *uniform_residual(rng, bd, w, h)))
    else:
        for i, lp in enumerate(LUMA_PAIRS):
            for comp, pair in ((0, lp), (1, CHROMA_PAIRS[i % len(CHROMA_PAIRS)])):
                for w, h, _ in shapes(comp):
                    p = pair_for(pair, w, h, comp)
                    if p is not None:
                        out.append(case(1, "types", bd, blk(w, h, comp, p[0], p[1], qp=22 + i % 14),
                                        *uniform_residual(rng, bd, w, h)))
    for b in _special_blocks():
        out.append(case(1, "skip" if b["tx_hor"] == tm.TX_SKIP else "dst4", bd, b,
                        *uniform_residual(rng, bd, b["w"], b["h"])))
    return out


# ---- family 2 -----------------------------------------------------------------------------------

def max_rows(m):
    """DC, the last kept row, the row of largest L1 norm."""
    kept = min(m.shape[0], 32)
    return [("dc", 0), ("last", kept - 1), ("l1", int(np.abs(m[:kept]).sum(axis=1).argmax()))]


def fwd_max_cases(bd):
    out = []
    for w, h, comp in MAX_SHAPES:
        pairs = CHROMA_PAIRS if comp else LUMA_PAIRS
        if bd in REDUCED:
            pairs = [(0, 0)]
        blocks = [blk(w, h, comp, p[0], p[1]) for p in pairs if pair_for(p, w, h, comp)]
        if (w, h, comp) == (4, 4, 0):
            blocks.append(blk(4, 4, 0, dst4x4=1))
        for b in blocks:
            mh, mv = stage_matrices(b)
            for (name, kx), (_, ky) in zip(max_rows(mh), max_rows(mv)):
                sign = np.outer(np.where(mv[ky] < 0, -1, 1), np.where(mh[kx] < 0, -1, 1))
                out.append(case(2, name, bd, b, *signed_residual(bd, sign)))
                out.append(case(2, name + "_neg", bd, b, *signed_residual(bd, -sign)))
    for w, h, comp in SKIP_SHAPES[:2] if bd in REDUCED else SKIP_SHAPES:
        sign = np.fromfunction(lambda y, x: 1 - 2 * ((x + y) % 2), (h, w), dtype=np.int64)
        out.append(case(2, "skip", bd, blk(w, h, comp, tm.TX_SKIP), *signed_residual(bd, sign)))
    return out


# ---- the dequantiser's edges --------------------------------------------------------------------

def dequant_scalar(bd, qp, w, h, level):
    import collections
    return int(tm.dequant(bd, qp, w, h, np.array([[level]]), collections.Counter())[0, 0])


@functools.lru_cache(maxsize=None)
def level_edges(bd, qp, w, h):
    """(largest level the dequantiser leaves unclipped, smallest it clips with either sign), both
    positive (the negative clip is at -32768, one further out)."""
    k = tm.quant_constants(bd, qp, w, h)

    def raw(level):     # in front of the clip
        prod = level * k["iq_scale"]
        sh = k["iq_shift"]
        return (prod + (1 << (sh - 1))) >> sh if sh > 0 else prod << -sh

    lo, hi = 0, 32767       # raw(lo) <= 32767 < raw(hi)
    assert raw(hi) > 32768, ("the QP is too low to clip", bd, qp, w, h)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if raw(mid) <= 32767 else (lo, mid)
    while raw(-hi) >= -32768:       # -32768 itself is not clipped
        hi += 1
    assert lo >= 1 and raw(-lo) >= -32768 and hi <= 32767
    assert (hi + 1) * k["iq_scale"] < 1 << 31, ("the product leaves int32", bd, qp, w, h)
    return lo, hi


def level_for(bd, qp, w, h, magnitude):
    """The largest positive level whose dequantised value is at most `magnitude` (0: none)."""
    k = tm.quant_constants(bd, qp, w, h)
    sh = k["iq_shift"]
    level = ((magnitude << sh) if sh > 0 else (magnitude >> -sh)) // k["iq_scale"]
    while level > 0 and dequant_scalar(bd, qp, w, h, level) > magnitude:
        level -= 1
    return int(min(level, 32767))


def clip_qp(bd, w, h):
    """A QP at which the dequantiser's step is a small power of two: qp % 6 == 4 is the scale 64."""
    k = tm.quant_constants(bd, 4, w, h)
    # step = 64 << (qpb / 6) >> iq_shift; raise the QP by sixes until the step is at least 8
    qp = 4
    while (64 << ((qp + 6 * (bd - 8)) // 6)) < (8 << max(0, k["iq_shift"])):
        qp += 6
    return qp


# ---- family 3 -----------------------------------------------------------------------------------

def clip_column(m):
    """The column with entries of both signs among the kept rows whose L1 norm is largest."""
    kept = m[:min(m.shape[0], 32)]
    mixed = (kept > 0).any(axis=0) & (kept < 0).any(axis=0)
    l1 = np.abs(kept).sum(axis=0)
    return int(np.where(mixed, l1, -1).argmax()), int(l1.max())


def clip_levels(bd, b, kind):
    """Levels whose dequantised coefficients are m * sign(Mv[j][y0]) * sign(Mh[k][x0]) inside the
    kept corner: stage 1 leaves +-(m * L1 of the column) at (k, y0) with the sign of Mh[k][x0], so
    stage 2 sums them all into (y0, x0).  kind: 'both' m = the clipped 32767 / -32768; 'stage2'
    the largest m that keeps every stage-1 sum inside; 'none' the largest that keeps both inside;
    'small' one quantiser step, which leaves a mid-grey prediction inside the sample range."""
    w, h, qp = b["w"], b["h"], b["qp"]
    if b["tx_hor"] == tm.TX_SKIP:
        sign = np.fromfunction(lambda y, x: 1 - 2 * ((x + y) % 2), (h, w), dtype=np.int64)
        m = level_edges(bd, qp, w, h)[1] + 1 if kind == "both" else \
            1 if kind == "small" else level_for(bd, qp, w, h, 20000 if kind == "stage2" else 300)
        return sign * max(m, 1)
    mh, mv = stage_matrices(b)
    (x0, l1h), (y0, l1v) = clip_column(mh), clip_column(mv)
    s1 = 7 if b["dst4x4"] else 7 + tm.hp(b["tx_ver"])
    s2 = 20 - bd + (0 if b["dst4x4"] else tm.hp(b["tx_hor"]))
    kw, kh = min(w, 32), min(h, 32)
    sign = np.zeros((h, w), np.int64)
    sign[:kh, :kw] = np.outer(np.where(mv[:kh, y0] < 0, -1, 1), np.where(mh[:kw, x0] < 0, -1, 1))
    if kind == "both":
        return sign * (level_edges(bd, qp, w, h)[1] + 1)
    if kind.startswith("lane"):
        # stage 2 sums the clipped column into four neighbours of row y0 at once: the signs are
        # those of the four columns' sum, negated (with the prediction at 0 and the original at
        # the maximum each of the four differences is then near 32768 + 2^bd)
        g = int(kind[4:])
        s4 = np.where(mh[:kw, g:g + 4].sum(axis=1) < 0, 1, -1)
        sign[:kh, :kw] = np.outer(np.where(mv[:kh, y0] < 0, -1, 1), s4)
        return sign * (level_edges(bd, qp, w, h)[1] + 1)
    if kind == "small":
        return sign
    m = (32767 << s1) // l1v
    if kind == "none":
        m = min(m, (((32767 << s2) // l1h) << s1) // l1v)
    return sign * max(level_for(bd, qp, w, h, m), 1)


def inv_clip_cases(bd):
    import collections
    smax = (1 << bd) - 1
    out = []
    blocks = []
    for w, h, comp in MAX_SHAPES:
        pairs = [(0, 0)] if bd in REDUCED else CLIP_PAIRS
        seen = set()
        for p in pairs:
            p = nearest_pair(p, w, h, comp)
            if p not in seen:
                seen.add(p)
                blocks.append(blk(w, h, comp, p[0], p[1]))
    blocks += [blk(4, 4, 0, dst4x4=1), blk(4, 4, 0, tm.TX_SKIP), blk(2, 2, 1, tm.TX_SKIP)]
    for b in blocks:
        b = dict(b, qp=clip_qp(bd, b["w"], b["h"]))
        for kind in ("both", "stage2", "none", "small"):
            levels = clip_levels(bd, b, kind)
            for pname, pv in (("p0", 0), ("pmax", smax), ("pmid", 1 << (bd - 1))):
                if bd in REDUCED and (kind, pname) not in (("both", "p0"), ("stage2", "pmax"),
                                                           ("none", "pmid"), ("small", "pmid")):
                    continue
                pred = np.full((b["h"], b["w"]), pv, np.int64)
                nnz = int(np.count_nonzero(levels))
                resi = tm.reconstruct(bd, b, pred, levels, nnz, collections.Counter())[0]
                orig = np.where(resi < 0, smax, 0)      # opposite the residual
                out.append(case(3, kind + "_" + pname, bd, b, orig, pred, levels, nnz))
        if tm.tx_small_job(b) and b["w"] == 16:
            # the distortion's partial sum of one lane: four saturated neighbours
            for g in (0, 8):
                levels = clip_levels(bd, b, "lane%d" % g)
                pred = np.zeros((b["h"], b["w"]), np.int64)
                nnz = int(np.count_nonzero(levels))
                resi = tm.reconstruct(bd, b, pred, levels, nnz, collections.Counter())[0]
                out.append(case(3, "lane%d_p0" % g, bd, b, np.where(resi < 0, smax, 0), pred,
                                levels, nnz))
    return out


# ---- family 4 -----------------------------------------------------------------------------------

def dc_cases(bd):
    rng = np.random.default_rng(9400 + bd)
    smax = (1 << bd) - 1
    out = []

    def add(kind, b, levels, nnz):
        h, w = levels.shape
        pred = rng.integers(0, smax + 1, (h, w))
        out.append(case(4, kind, bd, b, rng.integers(0, smax + 1, (h, w)), pred, levels, nnz))

    def single(w, h, y, x, v):
        lv = np.zeros((h, w), np.int64)
        lv[y, x] = v
        return lv

    for w, h, comp in DC_SHAPES:
        pairs = []
        for p in DC_PAIRS:
            if comp and not (p[0] in CHROMA_TYPES and p[1] in CHROMA_TYPES):
                continue
            p = nearest_pair(p, w, h, comp)
            if p not in pairs:
                pairs.append(p)
        blocks = [blk(w, h, comp, p[0], p[1]) for p in pairs]
        if (w, h, comp) == (4, 4, 0):
            blocks.append(blk(4, 4, 0, dst4x4=1))
        if (w, h, comp) in SKIP_SHAPES:
            blocks.append(blk(w, h, comp, tm.TX_SKIP))
        for b in blocks:
            top, over = level_edges(bd, b["qp"], w, h)
            values = [1, -1, top, -top, over, -over]
            if bd in REDUCED:
                values = [1, -top, over]
            for v in values:
                add("at0", b, single(w, h, 0, 0, v), 1)
        # the level elsewhere, and a second level, with the default types (the shortcut's own)
        b = blk(w, h, comp)
        top = level_edges(bd, b["qp"], w, h)[0]
        add("last", b, single(w, h, min(h, 32) - 1, min(w, 32) - 1, 3), 1)
        add("at01", b, single(w, h, 0, 1, -top), 1)
        add("at10", b, single(w, h, 1, 0, 5), 1)
        two = single(w, h, 0, 0, 7)
        two[h - 1, 0] = -2
        add("two", b, two, 2)
        # a single level outside the kept corner of a 64-point side: the inverse reads nothing
        if w == 64:
            add("outside", b, single(w, h, 0, 32, 9), 1)
            add("outside", b, single(w, h, h - 1, 63, -top), 1)
        if h == 64:
            add("outside", b, single(w, h, 32, 0, 9), 1)
    return out


# ---- family 5 -----------------------------------------------------------------------------------

def nothing_cases(bd):
    rng = np.random.default_rng(9500 + bd)
    smax = (1 << bd) - 1
    out = []
    blocks = [blk(w, h, c) for w, h, c in MAX_SHAPES] + \
        [blk(4, 4, 0, dst4x4=1), blk(4, 4, 0, tm.TX_SKIP), blk(2, 2, 1, tm.TX_SKIP)]
    for b in blocks:
        w, h = b["w"], b["h"]
        poison = np.full((h, w), POISON, np.int16)
        out.append(case(5, "nothing", bd, b, rng.integers(0, smax + 1, (h, w)),
                        rng.integers(0, smax + 1, (h, w)), poison, 0))
    return out


@functools.lru_cache(maxsize=None)
def cases(bd):
    """Every case of families 1 - 5 at the depth, each with its index `i`."""
    out = type_cases(bd) + fwd_max_cases(bd) + inv_clip_cases(bd) + dc_cases(bd) + nothing_cases(bd)
    for i, cs in enumerate(out):
        cs["i"] = i
    return out


def in_plane(cs, comp):
    """The case in component plane `comp` (same index `i`: the model does not look at the plane)."""
    return cs if cs["blk"]["comp"] == comp else dict(cs, blk=dict(cs["blk"], comp=comp))


def pack(cs_list, size=128):
    """Batches [(case, x, y)] of non-overlapping blocks inside a size x size picture.  The 'types'
    cases of family 1 keep the grid of cell(): one batch per type pair, the chroma grid in the U
    plane of every even batch and in the V plane of every odd one; every other case goes,
    largest first, to the first free position aligned to its own size in the first batch that
    has one, chroma cases to U and V in turn (in_plane: the case with blk['comp'] replaced)."""
    grids, batches = [], []
    for cs in cs_list:
        if cs["kind"] != "types":
            continue
        key = (cs["blk"]["comp"], cs["blk"]["w"], cs["blk"]["h"])
        for g in grids:
            if key not in g:
                g[key] = cs
                break
        else:
            grids.append({key: cs})
    for k, g in enumerate(grids):
        batches.append([(in_plane(cs, comp and 1 + k % 2),) + cell(w, h, comp)
                        for (comp, w, h), cs in g.items()])
    free, resume = [], {}
    rest = sorted((cs for cs in cs_list if cs["kind"] != "types"),
                  key=lambda cs: -cs["blk"]["w"] * cs["blk"]["h"])
    turn = 0
    for cs in rest:
        comp, w, h = (cs["blk"][k] for k in ("comp", "w", "h"))
        if comp:
            turn += 1
            comp = 1 + turn % 2
            cs = in_plane(cs, comp)
        unit = 2 if comp else 4                     # occupancy in cells of the smallest side
        cells = (size >> (1 if comp else 0)) // unit
        cw, ch = w // unit, h // unit
        nx, ny = cells // cw, cells // ch
        bi, ci = resume.get((comp, cw, ch), (0, 0))
        while True:
            if bi == len(free):
                free.append(({c: np.zeros((size // 4,) * 2, bool) for c in range(3)}, []))
            occ = free[bi][0][comp]
            while ci < nx * ny:
                x, y = (ci % nx) * cw, (ci // nx) * ch
                if not occ[y:y + ch, x:x + cw].any():
                    break
                ci += 1
            if ci < nx * ny:
                occ[y:y + ch, x:x + cw] = True
                free[bi][1].append((cs, x * unit, y * unit))
                resume[(comp, cw, ch)] = (bi, ci + 1)
                break
            bi, ci = bi + 1, 0
    return batches + [items for _, items in free]


# ---- the model over the cases -------------------------------------------------------------------

def quantised(xo_, cs, coeff):
    """QuantFast of the oracle (sign hiding on, inter picture, diagonal scan: flags 0)."""
    lv, nnz = xo_.quant_fast2(cs["bd"], cs["blk"]["qp"], 0, 1, 0,
                              np.ascontiguousarray(coeff.astype(np.int16)))
    return lv, nnz


@functools.lru_cache(maxsize=None)
def modelled(bd):
    """Per case a dict: coeff (forward cases), levels, nnz, resi, rec, dist and the three
    censuses fwd / inv / dist (what the forward half, the inverse half and the SSD decide)."""
    import collections
    import oracle_lib as ol
    xo_ = ol.Lib("xo")
    out = []
    for cs in cases(bd):
        b = cs["blk"]
        n_fwd, n_inv, n_dist = (collections.Counter() for _ in range(3))
        m = dict(coeff=None, fwd=n_fwd, inv=n_inv, dist_n=n_dist)
        if cs["levels"] is None:
            resi = cs["orig"].astype(np.int64) - cs["pred"].astype(np.int64)
            m["coeff"] = tm.forward(bd, b, resi, n_fwd)
            m["levels"], m["nnz"] = quantised(xo_, cs, m["coeff"])
        else:
            m["levels"], m["nnz"] = cs["levels"], cs["nnz"]
        m["resi"], m["rec"], _ = tm.reconstruct(bd, b, cs["pred"], m["levels"], m["nnz"], n_inv)
        r = m["resi"] if m["resi"] is not None else np.zeros(cs["pred"].shape, np.int64)
        m["dist"] = tm.ssd(bd, b, cs["orig"], cs["pred"], r, n_dist)
        out.append(m)
    return out


def describe(cs, m=None):
    d = dict(depth=cs["bd"], case=cs["i"], family=cs["family"], kind=cs["kind"], **cs["blk"])
    if m is not None:
        d["classes"] = sorted(k for n in (m["fwd"], m["inv"]) for k in n if n[k])
    return d


# ---- the frame pass's pictures ------------------------------------------------------------------

FW, FH = 64, 40         # the picture of tests/test_gpu_fwd_inv_paths.py: 16x16 CUs over a row of 16x8
FRAME_QPS = (0, 63)     # the ends of the range the pass clamps its tables to (rdoq_init_contexts,
                        # the adaptive-QP table; kMaxAllowedQp of the reference)


def flat_planes(w, h, value):
    return [np.full((h >> (1 if c else 0), w >> (1 if c else 0)), value, np.uint16)
            for c in range(3)]


def swing_pictures(bd, parts, weak_v):
    """orig, ref: per CU and component orig - ref = +-(2^bd - 1) with the signs of a DCT-2 basis
    function, alternately the DC row and the row of largest L1 norm of each matrix (family 2);
    weak_v: the V block of every second CU has a residual of +-2^(bd - 8) instead, which the lowest
    QP still codes and the highest does not."""
    smax = (1 << bd) - 1
    orig, ref = flat_planes(FW, FH, 0), flat_planes(FW, FH, 0)
    for i, (x, y, w, h) in enumerate(parts):
        for c in range(3):
            s = 1 if c else 0
            bw, bh, bx, by = w >> s, h >> s, x >> s, y >> s
            rows = [max_rows(tm.matrix(0, n))[0 if (i + c) % 2 else 2][1] for n in (bw, bh)]
            sign = np.outer(np.where(tm.matrix(0, bh)[rows[1]] < 0, -1, 1),
                            np.where(tm.matrix(0, bw)[rows[0]] < 0, -1, 1))
            if weak_v and c == 2 and i % 2:
                weak = 1 << (bd - 8)
                o, r = np.where(sign > 0, 8 + weak, 8), np.where(sign > 0, 8, 8 + weak)
            else:
                o, r = signed_residual(bd, sign)
            orig[c][by:by + bh, bx:bx + bw], ref[c][by:by + bh, bx:bx + bw] = o, r
    assert max(int(p.max()) for p in orig + ref) <= smax
    return orig, ref


def partitions(kind):
    """(CUs (x, y, w, h), the partition= argument of the pass) of the 16 grid, the 8 grid and the
    mixed partition of tests/test_gpu_fwd_inv_paths.py."""
    import test_gpu_fwd_inv_paths as fip
    from xvc_amd import pipeline
    assert (fip.W, fip.H) == (FW, FH)
    if kind == "16":
        return [tuple(int(b[k]) for k in ("x", "y", "w", "h"))
                for b in pipeline.FrameDescriptors(FW, FH).me], None
    parts = fip.only_8x8(FW, FH) if kind == "8" else fip.mixed_shapes(FW, FH)
    return parts, parts


def check_frame_pass_counts(qp, nnz):
    """On the oracle's answer: the low QP codes every block, the high QP leaves blocks without a
    level beside coded ones in the same CU."""
    per_cu = np.asarray(nnz).reshape(-1, 3)
    if qp == FRAME_QPS[0]:
        assert (per_cu != 0).all(), np.nonzero(per_cu == 0)
    else:
        assert ((per_cu == 0).any(axis=1) & (per_cu != 0).any(axis=1)).any(), per_cu


# ---- family 6 -----------------------------------------------------------------------------------

LAUNCH_BD = 12      # the depth at which every inverse class of the large blocks can be reached
WINDOW = 256        # descriptors a workgroup of the scanning kernel looks at


def special_indices(n):
    """Where the general-path blocks of a launch batch sit: index 0, 255, 256 and the last, five
    inside window 2, one in every tenth window; every other window holds none."""
    s = {0, WINDOW - 1, WINDOW, n - 1} | {2 * WINDOW + k for k in (3, 17, 64, 200, 255)}
    s |= set(range(3 * WINDOW + 232, n, 10 * WINDOW))
    if n <= WINDOW:     # a batch of one window: a few more, so that it holds every kind of block
        s |= {3, 4, 17, 18, 19, n // 2, n - 2}
    return sorted(i for i in s if 0 <= i < n)


def _pick(bd, **want):
    for cs in cases(bd):
        flat = dict(cs["blk"], family=cs["family"], kind=cs["kind"])
        if all(flat[k] == v for k, v in want.items()):
            return cs
    raise KeyError(want)


def launch_tiles(mode, bd=LAUNCH_BD):
    """(bulk tiles: 4x4 luma blocks of the one-wave path; special tiles: general-path blocks).
    mode 'fwd': cases that enter at the residual; 'inv': crafted levels."""
    s44 = dict(w=4, h=4, comp=0, dst4x4=0)
    if mode == "fwd":
        bulk = [_pick(bd, family=2, kind="dc", tx_hor=0, tx_ver=0, **s44),
                _pick(bd, family=1, tx_hor=5, tx_ver=3, **s44),
                _pick(bd, family=2, kind="l1_neg", tx_hor=7, tx_ver=7, **s44),
                _pick(bd, family=1, tx_hor=2, tx_ver=4, **s44)]
        flat = dict(bulk[0], kind="flat", orig=bulk[0]["pred"])      # nothing to code
        bulk.append(flat)
        special = [_pick(bd, family=2, kind="l1", w=64, h=64, tx_hor=0, tx_ver=0),
                   _pick(bd, family=1, w=32, h=32, tx_hor=3, tx_ver=5),
                   _pick(bd, family=2, kind="dc", w=2, h=8),
                   _pick(bd, family=2, kind="l1", dst4x4=1),
                   _pick(bd, family=2, kind="skip", w=4, h=4, comp=0),
                   _pick(bd, family=1, w=64, h=32, tx_hor=5, tx_ver=7),
                   _pick(bd, family=1, w=8, h=2, comp=1),
                   _pick(bd, family=2, kind="last_neg", w=32, h=32, tx_hor=7, tx_ver=7),
                   _pick(bd, family=1, kind="skip", w=4, h=4, comp=0),
                   _pick(bd, family=1, kind="dst4")]
        special.append(dict(special[1], kind="flat", orig=special[1]["pred"]))
    else:
        bulk = [_pick(bd, family=3, kind="both_p0", tx_hor=0, tx_ver=0, **s44),
                _pick(bd, family=3, kind="none_pmid", tx_hor=5, tx_ver=3, **s44),
                _pick(bd, family=4, kind="at0", tx_hor=0, tx_ver=0, **s44),
                _pick(bd, family=5, **s44),
                _pick(bd, family=4, kind="at0", tx_hor=5, tx_ver=0, **s44),
                _pick(bd, family=4, kind="two", **s44),
                _pick(bd, family=3, kind="stage2_pmax", tx_hor=2, tx_ver=4, **s44)]
        special = [_pick(bd, family=3, kind="both_pmid", w=64, h=64, tx_hor=0, tx_ver=0),
                   _pick(bd, family=3, kind="none_pmid", w=32, h=32, tx_hor=5, tx_ver=3),
                   _pick(bd, family=4, kind="at0", w=2, h=8),
                   _pick(bd, family=4, kind="at0", dst4x4=1),
                   _pick(bd, family=4, kind="at0", w=4, h=4, comp=0, tx_hor=tm.TX_SKIP),
                   _pick(bd, family=4, kind="outside", w=64, h=64),
                   _pick(bd, family=4, kind="two", w=8, h=2),
                   _pick(bd, family=3, kind="stage2_p0", w=32, h=32, tx_hor=0, tx_ver=0),
                   _pick(bd, family=3, kind="both_pmax", dst4x4=1),
                   _pick(bd, family=5, w=32, h=32),
                   _pick(bd, family=4, kind="at0", w=32, h=32, tx_hor=5, tx_ver=0),
                   _pick(bd, family=4, kind="at0", w=64, h=64, tx_hor=1, tx_ver=1),
                   _pick(bd, family=4, kind="at01", w=32, h=32),
                   _pick(bd, family=3, kind="both_p0", w=4, h=4, comp=0, tx_hor=tm.TX_SKIP),
                   _pick(bd, family=5, dst4x4=1)]
    assert all(tm.tx_small_job(t["blk"]) for t in bulk)
    assert not any(tm.tx_small_job(t["blk"]) for t in special)
    return bulk, special


def launch_batch(mode, n, per_row=256, flags=0, bd=LAUNCH_BD):
    """A batch of n non-overlapping blocks: descriptor i is the 4x4 luma tile at
    (4 (i % per_row), 4 (i / per_row)) with one of the bulk tiles' content, except at
    special_indices(n), which hold the special tiles in turn - a 4x4 one at the index's own
    position, a larger luma one in bands of 64 rows under the tiles, a chroma one in the U or the
    V plane in turn (which the tiles leave alone).  Returns dict(pw, ph, blocks[n] of the binding's dtype,
    tile[n] index into tiles, tiles)."""
    import oracle_lib as ol
    bulk, special = launch_tiles(mode, bd)
    tiles = bulk + special
    in_v = {}       # special tile -> its copy in the V plane, appended on first use
    idx = np.arange(n)
    tile = (idx * 5 + idx // WINDOW) % len(bulk)
    blocks = np.zeros(n, ol.TX_DTYPE)
    blocks["x"], blocks["y"] = 4 * (idx % per_row), 4 * (idx // per_row)
    rows = (4 * ((n - 1 + per_row - 1) // per_row) + 63) // 64 * 64    # of the indices 0 .. n - 2
    per_band = 4 * per_row // 64
    slot_l = slot_c = 0
    for k, i in enumerate(special_indices(n)):
        t = len(bulk) + k % len(special)
        b = tiles[t]["blk"]
        tile[i] = t
        if b["comp"]:
            blocks["x"][i], blocks["y"][i] = 32 * (slot_c // 2), 0
            if slot_c % 2:      # every second chroma block goes to the V plane
                if t not in in_v:
                    in_v[t] = len(tiles)
                    tiles.append(in_plane(tiles[t], 2))
                tile[i] = in_v[t]
            slot_c += 1
        elif b["w"] > 4 or b["h"] > 4 or i == n - 1:
            blocks["x"][i], blocks["y"][i] = 64 * (slot_l % per_band), rows + 64 * (slot_l // per_band)
            slot_l += 1
    assert 32 * ((slot_c + 1) // 2) <= 2 * per_row
    bands = (slot_l + per_band - 1) // per_band
    for t, cs in enumerate(tiles):
        sel = tile == t
        for k, v in cs["blk"].items():
            blocks[k][sel] = v
    blocks["intra_pic"] = flags
    return dict(pw=4 * per_row, ph=rows + 64 * bands, bd=bd, n_bulk=len(bulk), blocks=blocks, tile=tile, tiles=tiles)


_PER_JOB = ("residual_wave_kernel", "residual_per_job_kernel")
_SCANNING = ("residual_wave_kernel", "residual_kernel")


def _launch(name, mode, n, entry, kernels, in_place=False, per_row=256):
    return dict(name=name, mode=mode, n=n, entry=entry, kernels=kernels, in_place=in_place,
                per_row=per_row)


# the launch forms of launch_residual / launch_residual_rdoq (xvcgpu.hip) beyond their thresholds
LAUNCHES = [
    _launch("inv_16640_in_place", "inv", 16640, "inv", _PER_JOB, True),
    _launch("inv_16640", "inv", 16640, "inv", _PER_JOB),
    _launch("inv_65537_in_place", "inv", 65537, "inv", _SCANNING, True),
    _launch("inv_65537", "inv", 65537, "inv", _SCANNING),
    _launch("inv_dist_65537", "inv", 65537, "inv_dist", _SCANNING),
    _launch("fwd_65537", "fwd", 65537, "fwd", _SCANNING),
    _launch("residual_65537", "fwd", 65537, "residual", _SCANNING),
    _launch("rdoq_64", "fwd", 64, "rdoq", ("residual_cu_kernel",)),
    _launch("rdoq_65", "fwd", 65, "rdoq", _PER_JOB),
    _launch("rdoq_262145", "fwd", 262145, "rdoq", _SCANNING, per_row=512),
]
