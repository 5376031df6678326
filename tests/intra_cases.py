"""The directed case set of intra prediction: every size, mode and neighbour configuration on
reference lines that make a wrong index, weight, tap or clip visible.

A *target* is one block with its own painted L-shaped neighbourhood: (bit depth, component,
x, y, w, h, neighbours, above_right, below_left, content) and the list of modes it is
predicted with.  Targets lie in the slots of a *sheet* (three planes, 768 x 768 luma): pitch
48 for blocks up to 16, 96 up to 32, 192 above (chroma: 48 up to 16, 96 for 32), the block a
margin inside its slot, so that no job's reference line lies in another job's block and a
block that declares a side unavailable still has samples there - random ones, which neither
the device nor the oracle may read into the result.

Content of the reference line (the line is painted over its whole declared-or-not extent):
  steps     runs of 0 and the maximum of lengths 1, 2, 3, 5, the left line phase-shifted
  sat_high  one side within 2 of the maximum, the other rising from a low corner: the edge
            filters' above + ((left - corner) >> 1) and ">> 2" forms leave the range
            (blocks up to 16x16; alternately the left side high and the above side rising)
  sat_low   the same mirrored at 0
  full      uniformly random over the whole range
The original plane of the SATD pass holds, per target, the steps pattern in opposite phase
or full-range noise.

LM chroma targets lie on sheets of their own (chroma 160 x 160, slots of 40): slot column 0
starts at x = 0 and slot row 0 at y = 0, so all four neighbour availabilities occur.  Kinds:
chroma = a * luma + b for a in -5, -2, -3/4, 0, 1/8, 3/4, 2, 5 on luma levels with edges;
flat luma under varying chroma; flat chroma; nearly flat luma (a few samples one off: the
variance after the pre-scale's rounding can come out negative); neighbours in a narrow band
and the block's own luma at the other end of the range (the model extrapolates past the
maximum / below 0).

Depths 8, 10, 12 in full; 9 and 11 reduced (every kernel path of the device tests).

TEST INFRASTRUCTURE."""
import functools

import numpy as np

import intra_model as im
import oracle_intra as oi

FLOOR = 8
DEPTHS, ODD_DEPTHS = (8, 10, 12), (9, 11)
LUMA_SIZES, CHROMA_SIZES = (4, 8, 16, 32, 64), (2, 4, 8, 16, 32)
CHROMA_MODES = (0, 1, 2, 17, 18, 19, 33, 34, 35, 49, 50, 51, 66)
LM_MODE = 67
SHEET = 768          # luma samples a side; chroma planes half of it
LM_SHEET, LM_PITCH = 160, 40     # chroma samples
PATHS = ("pred", "wave", "satd", "rows", "lm")
PATH_TITLES = {"pred": "pred batch", "wave": "fused wave", "satd": "SATD general",
               "rows": "SATD rows", "lm": "LM"}

_LUMA_ONLY = "luma only: the SATD pass takes no chroma job"
_TO_16 = "the path stops at 16x16"
_SQUARE = "square 8x8 / 16x16 blocks only"
EXEMPT = {
    "pred": {},
    "wave": {"edge.off_large": _TO_16, "filt.s5.on": _TO_16, "filt.s5.off": _TO_16,
             "filt.s5.at_thr": _TO_16, "filt.s5.thr_plus_1": _TO_16, "filt.s6.off": _TO_16},
    "satd": {"filt.chroma_never": _LUMA_ONLY},
    "rows": {"filt.chroma_never": _LUMA_ONLY, "edge.off_large": _SQUARE,
             "pred.dc.plain": _SQUARE + ", always with the DC edge filter",
             "pred.dc.nonpow2": _SQUARE, "filt.s2.off": _SQUARE, "filt.s5.on": _SQUARE,
             "filt.s5.off": _SQUARE, "filt.s5.at_thr": _SQUARE, "filt.s5.thr_plus_1": _SQUARE,
             "filt.s6.off": _SQUARE},
}
PRED_KEYS = im.REFS_KEYS + im.filter_keys(range(2, 7)) + ["filt.chroma_never"] + im.MODE_KEYS + \
    im.ANG_KEYS + im.EDGE_KEYS


def path_keys(path):
    """The census keys a device path must reach."""
    if path == "lm":
        return list(im.LM_KEYS)
    assert set(EXEMPT[path]) <= set(PRED_KEYS)
    return [k for k in PRED_KEYS if k not in EXEMPT[path]]


def in_wave(t):
    """xvcgpu_intra_recon_batch takes it: sides 4, 8, 16 (the jobs carry dst4x4 = 0)."""
    return t["w"] in (4, 8, 16) and t["h"] in (4, 8, 16)


def in_rows(t):
    """intra_row8: square 8x8 / 16x16 luma at max_block_size 16."""
    return t["comp"] == 0 and t["w"] == t["h"] and t["w"] in (8, 16)


# ---- neighbour configurations -------------------------------------------------------------
def configs(w, h, step):
    """(neighbors, above_right, below_left): all eight availabilities, each with the extents
    a CU map can produce - above_right > 0 only with HAS_ABOVE, below_left > 0 only with
    HAS_LEFT."""
    def extents(n):
        half = n // 2
        return [0] + ([half] if half and half % step == 0 else []) + [n]

    out = []
    for nb in range(8):
        for ar in (extents(h) if nb & oi.HAS_ABOVE else [0]):
            for bl in (extents(w) if nb & oi.HAS_LEFT else [0]):
                assert (ar == 0 or nb & oi.HAS_ABOVE) and (bl == 0 or nb & oi.HAS_LEFT)
                out.append((nb, ar, bl))
    return out


REDUCED_LUMA = ((4, 4), (8, 8), (16, 16), (16, 8), (4, 16), (32, 32), (64, 16), (8, 32))
REDUCED_CHROMA = ((2, 2), (4, 4), (8, 8), (16, 4), (32, 32), (2, 32), (4, 8))


def _targets(bd, comp, reduced):
    luma = comp == 0
    sizes = LUMA_SIZES if luma else CHROMA_SIZES
    pairs = [(w, h) for w in sizes for h in sizes]
    if reduced:
        pairs = list(REDUCED_LUMA if luma else REDUCED_CHROMA)
    out = []
    for si, (w, h) in enumerate(pairs):
        cfgs = configs(w, h, 4 if luma else 2)
        if reduced:                               # eight of them, other ones per size
            cfgs = cfgs[si % 4::4][:8]
        elif not luma or max(w, h) == 64:         # every other one, alternating with the size
            cfgs = cfgs[si % 2::2]
        if luma and not reduced and w == h and w in (8, 16):
            cfgs = cfgs + cfgs[1:] + cfgs[:1]     # the register path's sizes: each one twice,
        for ci, (nb, ar, bl) in enumerate(cfgs):  # on other content
            if luma and max(w, h) <= 16:
                content = ("steps", "sat_high", "sat_low", "full")[(ci + si) % 4]
            else:
                content = ("steps", "full")[(ci + si) % 2]
            out.append(dict(bd=bd, comp=comp, w=w, h=h, nb=nb,
                            ar=ar, bl=bl, content=content, variant=ci + 3 * si,
                            modes=tuple(range(oi.NUM_MODES)) if luma else CHROMA_MODES))
    return out


def _steps(n, phase, smax):
    seq, v = [], 0
    while len(seq) < n + phase:
        for run in (1, 2, 3, 5):
            seq += [v] * run
            v = smax - v
    return seq[phase:phase + n]


def _paint(rng, plane, t):
    """The reference line of target t: above row from the corner on, left column."""
    bd, x, y, n = t["bd"], t["x"], t["y"], t["w"] + t["h"]
    smax, kind, var = (1 << bd) - 1, t["content"], t["variant"]
    if kind == "full":
        above, left = rng.integers(0, smax + 1, n + 1), rng.integers(0, smax + 1, n)
    elif kind == "steps":
        above, left = _steps(n + 1, var % 11, smax), _steps(n, var % 11 + 4, smax)
    else:
        corner = smax // 2
        high = [corner] + [smax - (i + 2) % 3 for i in range(n)]      # within 2 of the maximum
        rising = [min(smax, corner + 5 + 3 * j) for j in range(n)]   # more than 2 * 2 above
        above, left = (high, rising) if var % 2 == 0 else ([corner] + rising, high[1:])
        if kind == "sat_low":
            above, left = [smax - v for v in above], [smax - v for v in left]
    plane[y - 1, x - 1:x + n] = above
    plane[y:y + n, x - 1] = left


def _paint_orig(rng, plane, t):
    bd, x, y, w, h = t["bd"], t["x"], t["y"], t["w"], t["h"]
    smax = (1 << bd) - 1
    if t["variant"] % 2:
        return       # the sheet's full-range noise
    seq = _steps(w + h, t["variant"] % 11 + 1, smax)
    plane[y:y + h, x:x + w] = [[smax - seq[i + j] for i in range(w)] for j in range(h)]


def _pitch(t):
    side = max(t["w"], t["h"])
    return 48 if side <= 16 else (96 if side <= 32 else 192)


def _pack(targets, size, margin):
    """Slots in raster order, one pitch per plane -> the planes' target lists."""
    planes = []
    for pitch in (48, 96, 192):
        group = [t for t in targets if _pitch(t) == pitch]
        per_row = size // pitch
        for i in range(0, len(group), per_row * per_row):
            chunk = group[i:i + per_row * per_row]
            for k, t in enumerate(chunk):
                t["x"], t["y"] = pitch * (k % per_row) + margin, pitch * (k // per_row) + margin
                # the whole reference line inside the slot, whatever the job declares
                assert margin + t["w"] + t["h"] <= pitch and margin >= 1
            planes.append(chunk)
    return planes


@functools.lru_cache(maxsize=None)
def sheets(bd, reduced=False):
    """The prediction cases of one depth: [dict(bd, planes [Y, U, V] (the reconstruction),
    orig (the SATD pass's original luma), targets)]."""
    rng = np.random.default_rng(7000 + bd)
    yp = _pack(_targets(bd, 0, reduced), SHEET, 8)
    cp = _pack(_targets(bd, 1, reduced), SHEET // 2, 4)
    out = []
    for s in range(max(len(yp), (len(cp) + 1) // 2)):
        per = [yp[s] if s < len(yp) else [], cp[2 * s] if 2 * s < len(cp) else [],
               cp[2 * s + 1] if 2 * s + 1 < len(cp) else []]
        planes = [rng.integers(0, 1 << bd, (SHEET >> (c > 0),) * 2).astype(np.uint16)
                  for c in range(3)]
        orig = rng.integers(0, 1 << bd, (SHEET, SHEET)).astype(np.uint16)
        targets = []
        for c in range(3):
            for t in per[c]:
                t["comp"] = c
                _paint(rng, planes[c], t)
                if c == 0:
                    _paint_orig(rng, orig, t)
                targets.append(t)
        for p in planes + [orig]:
            p.setflags(write=False)
        out.append(dict(bd=bd, planes=planes, orig=orig, targets=targets))
    return out


def _all_jobs(sheet):
    if "jobs" not in sheet:
        ts = sheet["targets"]
        jobs = np.zeros(len(ts), oi.INTRA_DTYPE)
        for j, t in zip(jobs, ts):
            j["x"], j["y"], j["w"], j["h"], j["comp"] = t["x"], t["y"], t["w"], t["h"], t["comp"]
            j["neighbors"], j["above_right"], j["below_left"] = t["nb"], t["ar"], t["bl"]
        sheet["jobs"] = jobs
    return sheet["jobs"]


def round_jobs(sheet, r, keep=None):
    """The jobs of round r of a sheet: every target (that `keep` takes) with its r-th mode -
    mutually disjoint blocks.  -> INTRA_DTYPE array."""
    ts = sheet["targets"]
    take = [i for i, t in enumerate(ts) if r < len(t["modes"]) and (keep is None or keep(t))]
    jobs = _all_jobs(sheet)[take]
    jobs["mode"] = [ts[i]["modes"][r] for i in take]
    return jobs


def rounds(sheet):
    return max(len(t["modes"]) for t in sheet["targets"])


def luma_jobs(sheet):
    """The SATD pass's jobs of a sheet (mode unused)."""
    return round_jobs(sheet, 0, lambda t: t["comp"] == 0)


# ---- LM chroma ------------------------------------------------------------------------------
SLOPES = ((-5, 1), (-2, 1), (-3, 4), (0, 1), (1, 8), (3, 4), (2, 1), (5, 1))
LM_KINDS = ["slope%d" % i for i in range(8)] + ["flat_luma", "flat_chroma", "near_flat",
                                                "extrap_hi", "extrap_lo", "extrap_lo_pos"]


def _lm_targets(bd, reduced):
    pairs = [(w, h) for w in CHROMA_SIZES for h in CHROMA_SIZES]
    # the neighbour counts of the deepest pre-scales and the 16:1 steps need inside slots
    extra = [(32, 32), (32, 16), (16, 32), (32, 2), (2, 32), (16, 16), (32, 4), (4, 32)]
    if reduced:
        pairs, extra = [(2, 2), (4, 4), (8, 2), (16, 16), (32, 32), (2, 32), (32, 16), (4, 8)], []
    out = []
    for rep in range(1 if reduced else 3):
        for si, (w, h) in enumerate(pairs + extra * 2):
            k = len(out)
            out.append(dict(bd=bd, w=w, h=h, kinds=(LM_KINDS[(k + 5 * rep) % len(LM_KINDS)],
                                                    LM_KINDS[(k + 5 * rep + 9) % len(LM_KINDS)]),
                            variant=k, inside=(w, h) in extra and si >= len(pairs)))
    return out


def _levels(n, phase, values):
    """n values from `values` in runs of 1, 2, 3, 5."""
    seq, i = [], 0
    while len(seq) < n + phase:
        for run in (1, 2, 3, 5):
            seq += [values[i % len(values)]] * run
            i += 1 + (len(seq) % 3 == 0)
    return np.array(seq[phase:phase + n], np.int64)


def _paint_lm(planes, t):
    """Luma in 2x2 cells of one level per chroma sample over the block and a border of two
    chroma samples (U's kind shapes it); U and V from that level by their kinds."""
    bd, x, y, w, h, var = t["bd"], t["x"], t["y"], t["w"], t["h"], t["variant"]
    smax = (1 << bd) - 1
    x0, y0, x1, y1 = max(x - 2, 0), max(y - 2, 0), x + w + 1, y + h + 1
    cw, ch = x1 - x0, y1 - y0
    lo, step = smax // 8, max(smax // 32, 1)
    # four levels across in runs of 1, 2, 3, 5, smaller steps down: at most 4 * step above lo
    cells = _levels(cw, var % 7, [lo, lo + step, lo + 2 * step, lo + 3 * step])[None, :] + \
        _levels(ch, var % 5 + 2, [0, step // 2, 0, step])[:, None]
    inside = np.zeros((ch, cw), bool)
    inside[y - y0:y - y0 + h, x - x0:x - x0 + w] = True
    shape = t["kinds"][0]
    if shape == "flat_luma":
        cells[:] = lo + (var % 3) * step
    elif shape == "near_flat":
        cells[:] = lo + 5 * (var % 4) + 3
        for i in range(1 + var % 8):     # a few neighbour cells two above the rest
            if y > 0 and (i % 2 == 0 or x == 0):
                cells[y - y0 - 1, x - x0 + (3 * i) % w] += 2
            elif x > 0:
                cells[y - y0 + (3 * i) % h, x - x0 - 1] += 2
    elif shape in ("extrap_hi", "extrap_lo"):        # the block's own luma at the top
        cells[inside] = smax - (cells[inside] - lo) // 4
    elif shape == "extrap_lo_pos":                   # neighbours high, the block at 0
        cells += smax - 4 * step - lo
        cells[inside] = (cells[inside] - (smax - 4 * step)) // 4
    assert cells.min() >= 0 and cells.max() <= smax
    planes[0][2 * y0:2 * y1, 2 * x0:2 * x1] = np.repeat(np.repeat(cells, 2, 0), 2, 1)
    outside = cells[~inside]
    base = cells - (outside.min() if outside.size else cells.min())
    for comp, kind in ((1, t["kinds"][0]), (2, t["kinds"][1])):
        if kind in ("flat_luma", "near_flat"):       # chroma varies on its own
            chroma = (_levels(cw, var % 3, [0, smax, smax // 2, smax // 5])[None, :] +
                      _levels(ch, var % 4, [0, smax // 7, 3])[:, None]) % (smax + 1)
        elif kind == "flat_chroma":
            chroma = np.full((ch, cw), smax // 3 + var)
        else:
            num, den = SLOPES[int(kind[5:])] if kind.startswith("slope") else \
                ((-2, 1) if kind == "extrap_lo" else (2, 1))
            chroma = (smax // 32 if num >= 0 else smax - smax // 32) + (num * base) // den
        planes[comp][y0:y1, x0:x1] = np.clip(chroma, 0, smax)


@functools.lru_cache(maxsize=None)
def lm_sheets(bd, reduced=False):
    """[dict(bd, planes, targets)]: an LM target is a block; both chroma components predict
    it (jobs of comp 1 and 2)."""
    rng = np.random.default_rng(7100 + bd)
    targets = _lm_targets(bd, reduced)
    per_row = LM_SHEET // LM_PITCH
    wants = [t for t in targets if t["inside"]]      # inner slots only
    free = [t for t in targets if not t["inside"]]
    out, turn = [], 0
    while wants or free:
        planes = [rng.integers(0, 1 << bd, (LM_SHEET << (c == 0),) * 2).astype(np.uint16)
                  for c in range(3)]
        placed = []
        for k in range(per_row * per_row):
            sx, sy = k % per_row, k // per_row
            if sx and sy and wants and (turn % 2 == 0 or not free):
                t = wants.pop(0)
            elif free:
                t = free.pop(0)
            else:
                continue
            turn += bool(sx and sy)
            t["x"], t["y"] = LM_PITCH * sx + (4 if sx else 0), LM_PITCH * sy + (4 if sy else 0)
            assert t["x"] + t["w"] + 1 <= LM_PITCH * (sx + 1) and \
                t["y"] + t["h"] + 1 <= LM_PITCH * (sy + 1)
            _paint_lm(planes, t)
            placed.append(t)
        for p in planes:
            p.setflags(write=False)
        out.append(dict(bd=bd, planes=planes, targets=placed))
    return out


def lm_jobs(sheet, comp):
    jobs = np.zeros(len(sheet["targets"]), oi.INTRA_DTYPE)
    for j, t in zip(jobs, sheet["targets"]):
        j["x"], j["y"], j["w"], j["h"], j["comp"], j["mode"] = \
            t["x"], t["y"], t["w"], t["h"], comp, LM_MODE
    return jobs


def all_depths():
    """(bd, reduced) of every pass."""
    return [(bd, False) for bd in DEPTHS] + [(bd, True) for bd in ODD_DEPTHS]
