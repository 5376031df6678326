"""Shared input generators for the parity tests (seeded, numpy only)."""
import numpy as np

import oracle_lib as ol

SIZES = [4, 8, 16, 32, 64]


def rnd_samples(rng, bd, h, w, smooth=False):
    if smooth:
        base = rng.integers(0, 1 << bd)
        a = base + rng.integers(-6, 7, size=(h, w))
        return np.clip(a, 0, (1 << bd) - 1).astype(np.uint16)
    return rng.integers(0, 1 << bd, size=(h, w), dtype=np.uint16)


def random_partition(rng, pw, ph, min_size=4):
    """Random quad/binary partition of the picture into CUs (x,y,w,h)."""
    out = []

    def split(x, y, w, h, depth):
        if x >= pw or y >= ph:
            return
        inside = x + w <= pw and y + h <= ph
        r = rng.random()
        can_h = h > min_size
        can_w = w > min_size
        if not inside or depth < 1 or (depth < 2 and r < 0.8) or (r < 0.45 and (can_h or can_w)):
            mode = rng.integers(0, 3) if inside else 0
            if mode == 0 and can_h and can_w:
                for (dx, dy) in ((0, 0), (w // 2, 0), (0, h // 2), (w // 2, h // 2)):
                    split(x + dx, y + dy, w // 2, h // 2, depth + 1)
                return
            if mode == 1 and can_w:
                split(x, y, w // 2, h, depth + 1)
                split(x + w // 2, y, w // 2, h, depth + 1)
                return
            if can_h:
                split(x, y, w, h // 2, depth + 1)
                split(x, y + h // 2, w, h // 2, depth + 1)
                return
            if can_w:
                split(x, y, w // 2, h, depth + 1)
                split(x + w // 2, y, w // 2, h, depth + 1)
                return
        out.append((x, y, w, h))

    for cy in range(0, ph, 64):
        for cx in range(0, pw, 64):
            split(cx, cy, 64, 64, 0)
    return out


def make_cus(rng, parts, bipred, l0, l1, pw, ph):
    cus = np.zeros(len(parts), ol.CU_DTYPE)
    cmap = -np.ones(((ph + 3) // 4, (pw + 3) // 4), np.int32)
    for i, (x, y, w, h) in enumerate(parts):
        c = cus[i]
        c["x"], c["y"], c["w"], c["h"] = x, y, w, h
        c["intra"] = rng.random() < 0.15
        c["cbf_luma"] = rng.random() < 0.4
        qp = int(rng.integers(20, 45))
        c["qp_y"] = qp
        c["qp_c"] = ol.chroma_qp(qp)
        if bipred:
            d = rng.integers(0, 3)
        else:
            d = 0
        i0 = int(rng.integers(0, len(l0)))
        i1 = int(rng.integers(0, len(l1)))
        c["ref_idx0"] = i0 if d != 1 else 0
        c["ref_poc"][0] = l0[i0] if d != 1 else -1
        c["ref_poc"][1] = l1[i1] if d != 0 else -1
        base = rng.integers(-40, 41, size=(2, 1, 2))
        if rng.random() < 0.2:
            mv = base + rng.integers(-20, 21, size=(2, 4, 2))
        else:
            mv = np.repeat(base, 4, axis=1)
        c["mv"] = mv
        cmap[y // 4:(y + h) // 4, x // 4:(x + w) // 4] = i
    return cus, cmap


def make_pics(rng, bd, pw, ph, border, motion=(3, -2), noise=3):
    """orig = shifted ref + noise over a textured plane -> searches do real work."""
    H, W = ph + 2 * border, pw + 2 * border
    yy, xx = np.mgrid[0:H, 0:W]
    tex = (np.sin(xx / 7.0) * np.cos(yy / 9.0) * 0.25 + np.sin((xx + yy) / 23.0) * 0.2 + 0.5)
    tex = tex * ((1 << bd) - 1) + rng.integers(-noise * 4, noise * 4 + 1, size=(H, W))
    ref = np.clip(tex, 0, (1 << bd) - 1).astype(np.uint16)
    orig = np.roll(ref, (-motion[1], -motion[0]), axis=(0, 1)).astype(np.int32)
    orig = np.clip(orig + rng.integers(-noise, noise + 1, size=(H, W)), 0,
                   (1 << bd) - 1).astype(np.uint16)
    return orig, ref


# The tile shapes of the packed sub-pel path (k_subpel.h), rectangles first
EXTREME_SHAPES = [(16, 8), (8, 16), (32, 16), (16, 32), (64, 32), (32, 64), (64, 16), (16, 64),
                  (8, 8), (16, 16), (32, 32), (64, 64), (32, 8), (8, 32)]


def walsh_pictures(rng, bd, pw, ph, border, trial):
    """The inputs of test_me_search_extreme_residuals (test_gpu_parity.py), draw for draw:
    the original and the reference are opposite Walsh patterns at full swing (trial 5: a
    random sign pattern), so every residual is +-(2^bd - 1).  Returns the padded luma
    planes (orig, ref)."""
    smax = (1 << bd) - 1
    yy, xx = np.mgrid[0:ph, 0:pw]
    kx, ky = int(rng.integers(0, 16)), int(rng.integers(0, 16))
    walsh = (np.bitwise_count((xx & kx).astype(np.uint8)).astype(np.int64) +
             np.bitwise_count((yy & ky).astype(np.uint8))) & 1
    if trial == 5:
        walsh = rng.integers(0, 2, (ph, pw))
    orig = np.ascontiguousarray(np.pad((walsh * smax).astype(np.uint16), border, mode="edge"))
    ref = np.ascontiguousarray(np.pad(((1 - walsh) * smax).astype(np.uint16), border,
                                      mode="edge"))
    return orig, ref


def extreme_blocks(rng, pw, ph, flags=0):
    """One search job per shape of EXTREME_SHAPES on the 16-sample grid (the draws of
    test_me_search_extreme_residuals); `flags` goes to fullpel_mv (XVC_ME_USE_LIC = 2)."""
    blocks = np.zeros(len(EXTREME_SHAPES), ol.ME_DTYPE)
    for b, (w, h) in zip(blocks, EXTREME_SHAPES):
        b["w"], b["h"] = w, h
        b["x"] = int(rng.integers(0, (pw - w) // 16 + 1)) * 16
        b["y"] = int(rng.integers(0, (ph - h) // 16 + 1)) * 16
        b["lambda16"], b["search_range"] = 498000, 96
        b["fullpel_mv"] = flags
    return blocks


def me_struct(b):
    s = ol.MeBlock()
    for name in ol.ME_DTYPE.names:
        setattr(s, name, int(b[name]))
    return s


def bi_struct(j):
    s = ol.BiBlock()
    for name in ol.ME_DTYPE.names:
        setattr(s.blk, name, int(j["blk"][name]))
    for name in ("other_mv_x", "other_mv_y", "boot_mv_x", "boot_mv_y"):
        setattr(s, name, int(j[name]))
    return s


def extreme_bi_jobs(rng, blocks):
    """One bi-prediction refinement job per block: the other list's vector full-pel for
    every second job (then the 2 * orig - pred target sits at its ends, -(2^bd - 1) and
    2 * (2^bd - 1), when that picture is the opposite pattern), sub-pel for the rest."""
    jobs = np.zeros(len(blocks), ol.BI_DTYPE)
    jobs["blk"] = blocks
    jobs["blk"]["search_range"] = 4
    for k, j in enumerate(jobs):
        if k % 2:
            j["other_mv_x"], j["other_mv_y"] = int(rng.integers(-40, 40)), int(rng.integers(-40, 40))
        else:
            j["other_mv_x"], j["other_mv_y"] = 16 * int(rng.integers(-2, 3)), 16 * int(rng.integers(-2, 3))
        j["boot_mv_x"], j["boot_mv_y"] = int(rng.integers(-48, 48)), int(rng.integers(-48, 48))
    return jobs
