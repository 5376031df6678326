"""The directed inputs of the deblocking tests (tests/test_deblock_model.py on the CPU,
tests/test_gpu_deblock_cases.py on the device): seeded, generated, nothing stored.

Two pictures, 136x72 and 72x136 (3x2 / 2x3 tiles of the fused tail, remainder tiles of 8,
every rim and corner), and two families of partitions: "g4" with CUs down to 4x4 and 4xN /
Nx4 strips (chains of edges four samples apart: the two-pass kernels), "g8" on the 8-sample
grid (what the fused tail takes).  Per family, bit depth and picture the recipes of RECIPES:
QPs over 0..63, the deblocking offsets at both ends of their 6-bit range, the last indices
inside the reference's tables, a narrow high band; plane levels 0 / mid / max; vectors from
a palette around the 16-unit threshold; reference lists that share a POC.  Two hand-built
cases per depth on top: "lowdelay" (every CU bi-predicted from lists with equal POCs) and
"strongclip" (edges at which the strong filter's +-2 tc clip binds, on either side of the
edge, in either sign, in both passes).

The generators do not go through numpy.random.default_rng: the census floors
(test_deblock_model.py) are a statement about exactly these inputs.

TEST INFRASTRUCTURE."""
import functools

import numpy as np

import helpers
import oracle_lib as ol

SIZES = [(136, 72), (72, 136)]
FAMILIES = ("g4", "g8")
DEPTHS = (8, 10, 12, 9, 11)
L0, L1 = [8, 0], [8, 16]
# name: ((beta_offset, tc_offset), (lowest, highest QP of a CU))
RECIPES = [
    ("zero", (0, 0), (0, 63)),
    ("lo_hi", (-32, 31), (0, 63)),      # beta index < 0, tc index > 53, chroma tc index 54
    ("hi_lo", (31, -32), (0, 63)),      # beta index 64, tc index < 0
    ("last", (3, 0), (60, 60)),         # qp + beta_off == 63, cqp + tc_off + 2 == 53 exactly
    ("band", (0, 0), (56, 63)),
    ("neg", (-20, -20), (0, 63)),       # both indices below 0 at low QPs, inside the tables
    ("mid", (6, 4), (8, 51)),
    ("tc_neg", (10, -32), (10, 53)),    # tc index < 0 under a beta that lets groups through
]
# vector components around MotionVector::kScale = 16, the boundary-strength threshold
PALETTE = [-17, -16, -15, -1, 0, 1, 15, 16, 17, 32]


def _rng(*seed):
    return np.random.Generator(np.random.PCG64(list(seed)))


def _strips(rng, parts):
    """Some CUs of at least 8x8 cut into 4-wide strips, 4-tall strips or 4x4 CUs."""
    out = []
    for (x, y, w, h) in parts:
        kind = int(rng.integers(0, 8)) if w >= 8 and h >= 8 and w * h <= 1024 else 3
        if kind == 0:
            out += [(x + dx, y, 4, h) for dx in range(0, w, 4)]
        elif kind == 1:
            out += [(x, y + dy, w, 4) for dy in range(0, h, 4)]
        elif kind == 2:
            out += [(x + dx, y + dy, 4, 4) for dy in range(0, h, 4) for dx in range(0, w, 4)]
        else:
            out.append((x, y, w, h))
    return out


def _partition(rng, family, pw, ph):
    if family == "g8":
        return helpers.random_partition(rng, pw, ph, 8)
    return _strips(rng, helpers.random_partition(rng, pw, ph, 4))


def _cu_map(parts, pw, ph):
    cmap = -np.ones((ph // 4, pw // 4), np.int32)
    for i, (x, y, w, h) in enumerate(parts):
        assert (cmap[y // 4:(y + h) // 4, x // 4:(x + w) // 4] == -1).all()
        cmap[y // 4:(y + h) // 4, x // 4:(x + w) // 4] = i
    assert (cmap >= 0).all()
    return cmap


def _vector(rng, pal):
    return [int(rng.choice(pal)), int(rng.choice(pal))]


def _make_cus(rng, parts, bipred, l0, l1, qp_range, p_intra=0.15, p_cbf=0.3, all_bi=False):
    cus = np.zeros(len(parts), ol.CU_DTYPE)
    # a few vectors per picture, so that neighbours often agree or differ by one palette step
    pal = [int(v) for v in rng.choice(PALETTE, 3, replace=False)] + [0]
    for c, (x, y, w, h) in zip(cus, parts):
        c["x"], c["y"], c["w"], c["h"] = x, y, w, h
        c["intra"] = rng.random() < p_intra
        c["cbf_luma"] = rng.random() < p_cbf
        qp = int(rng.integers(qp_range[0], qp_range[1] + 1))
        c["qp_y"], c["qp_c"] = qp, ol.chroma_qp(qp)
        d = 2 if all_bi else (int(rng.integers(0, 3)) if bipred else 0)     # L0, L1, both
        i0 = int(rng.random() < 0.35) % len(l0)
        i1 = int(rng.random() < 0.35) % len(l1)
        c["ref_idx0"] = i0 if d != 1 else 0
        c["ref_poc"][0] = l0[i0] if d != 1 else -1
        c["ref_poc"][1] = l1[i1] if d != 0 else -1
        for lst in range(2):
            base = _vector(rng, pal)
            for corner in range(4):
                # four different corner vectors for some CUs (an affine CU's)
                c["mv"][lst][corner] = _vector(rng, pal) if rng.random() < 0.3 else base
    return cus


def _planes(rng, bd, pw, ph, level):
    """4-sample cells with steps of up to 96 (scaled by the depth; a step between flat cells
    gives the weak filter a delta of 6/16 of it, so its +-tc clip binds under the largest tc,
    24, from a step of 70 on, and the strong filter gives way at 2.5 tc) and noise of 0..6,
    both drawn per 16x16 region, at level 0 (half of the steps clipped to 0), mid or max (half of
    them clipped to the maximum)."""
    smax, s = (1 << bd) - 1, 1 << (bd - 8)
    planes = []
    for c in range(3):
        w, h = (pw, ph) if c == 0 else (pw // 2, ph // 2)
        rw, rh = (w + 15) // 16, (h + 15) // 16
        def per_region(values):
            return np.kron(rng.choice(values, (rh, rw)), np.ones((16, 16), np.int64))[:h, :w]

        def per_cell(values, dtype):
            return np.kron(values, np.ones((4, 4), dtype))[:h, :w]

        amp, noise, nscale = per_region([0, 2, 6, 15, 40, 96]), per_region([0, 1, 3, 6]), \
            per_region([1, s])
        cell = per_cell(rng.random(((h + 3) // 4, (w + 3) // 4)), np.float64)
        # half of the largest steps at full height: flat cells the whole range (97) apart
        full = per_cell(rng.random(((h + 3) // 4, (w + 3) // 4)) < 0.5, bool)
        cell = np.where(full & (amp == 96), np.round(cell), cell)
        v = np.floor(cell * (amp + 1)).astype(np.int64) * s + \
            np.floor(rng.random((h, w)) * (noise + 1)).astype(np.int64) * nscale
        if level == 0:      # the lower half of the steps flattened at 0
            p = v - (amp * s + 1) // 2
        elif level == 2:
            p = smax - v + (amp * s + 1) // 2
        else:
            p = (1 << (bd - 1)) + v - (amp * s + noise * nscale) // 2
        planes.append(np.clip(p, 0, smax).astype(np.uint16))
    return planes


def _random_case(family, bd, size, recipe, level, bipred, seed):
    name, (beta, tc), qp_range = recipe
    pw, ph = size
    rng = _rng(7100, seed)
    parts = _partition(rng, family, pw, ph)
    cus = _make_cus(rng, parts, bipred, L0, L1, qp_range)
    return dict(name="%s-%s-bd%d-%dx%d" % (family, name, bd, pw, ph), family=family, bd=bd,
                pw=pw, ph=ph, bipred=bipred, beta=beta, tc=tc, l0=L0, l1=L1, cus=cus,
                cu_map=_cu_map(parts, pw, ph), planes=_planes(rng, bd, pw, ph, level),
                recipe=name)


def _lowdelay_case(family, bd, size, seed):
    """A low-delay B picture's shape: every CU bi-predicted, the two lists hold the same
    POCs, few distinct vectors, little intra and few coded residuals - the same-POC and the
    swapped branch of GetBoundaryStrength in all their outcomes."""
    pw, ph = size
    rng = _rng(7200, seed)
    parts = _partition(rng, family, pw, ph)
    l0 = l1 = [8, 0]
    cus = _make_cus(rng, parts, 1, l0, l1, (24, 44), p_intra=0.03, p_cbf=0.08, all_bi=True)
    # two vectors one threshold apart (and a near miss), whole CUs: cond1 / cond2 each go
    # both ways between neighbours
    pal = [[0, 0], [16, 0], [15, 0], [0, -16]]
    for c in cus:
        for lst in range(2):
            c["mv"][lst][:] = pal[int(rng.choice(4, p=[0.4, 0.4, 0.1, 0.1]))]
    return dict(name="%s-lowdelay-bd%d-%dx%d" % (family, bd, pw, ph), family=family, bd=bd,
                pw=pw, ph=ph, bipred=1, beta=0, tc=0, l0=l0, l1=l1, cus=cus,
                cu_map=_cu_map(parts, pw, ph), planes=_planes(rng, bd, pw, ph, 1),
                recipe="lowdelay")


def _strongclip_case(family, bd, size, seed):
    """Edges at which the strong filter's +-2 tc clip binds.  QP 40 with offsets (23, -20):
    beta index 63 (beta 88), tc index 20 / 22 (tc 1).  At 8 bit p3 = L + 10, p2 = p1 = p0 =
    L, q0 .. q3 = L gives np2 - p2 = 3 > 2 tc; p3 = L - 10 with q0 .. q3 = L - 2 gives -3;
    the same mirrored onto the q side; all scaled by the depth.  8x8 CUs; the left (136x72)
    or upper (72x136) part of the picture carries the pattern across vertical edges, the
    rest across horizontal edges and constant along x, where the vertical pass changes
    nothing.  Edges alternate between the p and the q side, pairs of edges and bands of
    four lines between the signs.  ("g4": the rightmost CU column and the lowest CU row
    are cut into 4x4 CUs and hold noise.)"""
    pw, ph = size
    rng = _rng(7300, seed)
    s, L = 1 << (bd - 8), (1 << (bd - 1)) + 3
    parts = []
    for y in range(0, ph, 8):
        for x in range(0, pw, 8):
            if family == "g4" and (x + 8 == pw or y + 8 == ph):
                parts += [(x + dx, y + dy, 4, 4) for dy in (0, 4) for dx in (0, 4)]
            else:
                parts.append((x, y, 8, 8))
    cus = _make_cus(rng, parts, 0, L0, L1, (40, 40), p_intra=0.3, p_cbf=1.0)
    split = (pw // 16 * 8, ph) if pw > ph else (pw, ph // 16 * 8)   # the vertical-edge part
    luma = np.full((ph, pw), L, np.int64)

    def pattern(n_across, n_along):
        """rows = lines (bands of four alternate the sign), columns across the edges"""
        a = np.full((n_along, n_across), L, np.int64)
        for line in range(n_along):
            for e in range(8, n_across, 8):
                sign = 1 if ((line >> 2) ^ (e >> 4)) & 1 else -1
                if (e >> 3) & 1:      # p side: p3 out, the q side level with it or 2 off
                    a[line, e - 4] = L + sign * 10 * s
                    a[line, e:e + 4] = L if sign > 0 else L - 2 * s
                else:                 # q side, mirrored
                    a[line, e + 3] = L + sign * 10 * s
                    a[line, e - 4:e] = L if sign > 0 else L - 2 * s
        return a

    if pw > ph:
        luma[:, :split[0]] = pattern(split[0], ph)
        luma[:, split[0]:] = pattern(ph, 1).T.repeat(pw - split[0], axis=1)
    else:
        luma[:split[1], :] = pattern(pw, split[1])
        luma[split[1]:, :] = pattern(ph - split[1], 1).T.repeat(pw, axis=1)
    planes = _planes(rng, bd, pw, ph, 1)
    if family == "g4":
        keep = np.zeros((ph, pw), bool)
        keep[:, pw - 12:] = keep[ph - 12:, :] = True
        luma = np.where(keep, planes[0], luma)
    planes[0] = luma.astype(np.uint16)
    return dict(name="%s-strongclip-bd%d-%dx%d" % (family, bd, pw, ph), family=family, bd=bd,
                pw=pw, ph=ph, bipred=0, beta=23, tc=-20, l0=L0, l1=L1, cus=cus,
                cu_map=_cu_map(parts, pw, ph), planes=planes, recipe="strongclip")


@functools.lru_cache(maxsize=None)
def cases(family):
    """The family's cases (dicts: name, family, bd, pw, ph, bipred, beta, tc, l0, l1, cus,
    cu_map, planes without border, recipe).  Shared: treat them as read-only."""
    out = []
    fam = FAMILIES.index(family)
    for bi, bd in enumerate(DEPTHS):
        if bd in (9, 11):     # the odd depths once each
            ri = 6 if bd == 9 else 0
            out.append(_random_case(family, bd, SIZES[bd == 9], RECIPES[ri], 1, int(bd == 11),
                                    1000 * fam + 100 * bi + 90))
            out.append((_strongclip_case if bd == 9 else _lowdelay_case)(
                family, bd, SIZES[bd == 11], 1000 * fam + 100 * bi + 91))
            continue
        for si, size in enumerate(SIZES):
            for ri, recipe in enumerate(RECIPES):
                out.append(_random_case(family, bd, size, recipe, (ri + si + bi) % 3,
                                        (ri + si) % 2, 1000 * fam + 100 * bi + 10 * si + ri))
        for si, size in enumerate(SIZES):
            out.append(_lowdelay_case(family, bd, size, 1000 * fam + 100 * bi + 70 + si))
        out.append(_strongclip_case(family, bd, SIZES[(bi + 1) % 2], 1000 * fam + 100 * bi + 81))
    for c in out:
        for p in c["planes"]:
            p.setflags(write=False)
        c["cus"].setflags(write=False)
        c["cu_map"].setflags(write=False)
    return out


def padded(case, borders, rng=None):
    """The case's planes inside borders of zeros (rng: of random samples) - fresh arrays."""
    out = []
    for c, p in enumerate(case["planes"]):
        b = borders[c]
        h, w = p.shape
        if rng is None:
            full = np.zeros((h + 2 * b, w + 2 * b), np.uint16)
        else:
            full = rng.integers(0, 1 << case["bd"], (h + 2 * b, w + 2 * b)).astype(np.uint16)
        full[b:b + h, b:b + w] = p
        out.append(full)
    return out
