"""The paths of the 16x16 / 16x8 search job (k_me2.h) against the C oracle, through the three
entries that share the job: the plain search, XVCGPU_ME_HINT_SQ16 and XVCGPU_ME_ONLY_SQ16.

64x40 pictures: a 4 x 3 grid of 16-wide CUs whose bottom row is 16x8.  Every field of every
result is compared with xo.tz_search / xo.subpel_search, and the three entries with each other.
What the inputs are for:

  planted   every offset in [-3, 3]^2 between the predictor and the true motion, on low-passed
            texture, 16x16 and 16x8, three lambdas: the range-1 hit, the neighbour step and
            the range-2 diagonals decide these
  window    search ranges 1, 2, 4, 8, 96, 256 (fewer than three rounds ... all nine), the true
            motion exactly on each bound of the window and one outside it, the previous CU's
            vector outside the window (bounds a candidate does not test)
  grid      planted motions (40, 26) and (-17, 9) far from the predictor (step-5 grid),
            full-pel-only jobs, depth_nonzero 0 / 1 with the previous vector winning
  zero      the zero vector winning against predictor and previous vector
  subpel    per-CU fractional motion: every half-pel position, quarter-pel components
  clip8/10/12  motion onto the picture's vector limits, so that d_clip_mv changes sub-pel
            candidates; bit depths 8 and 10 (packed path) and 12 (32-bit path)

The coverage test looks at the oracle's answers only.
"""
import numpy as np
import pytest

import oracle_lib as ol
from helpers import make_pics, me_struct

BL = 128
PW, PH = 64, 40
LAMBDAS = (120000, 498000, 1500000)
CUS = [(x, y, 8 if y == 32 else 16) for y in (0, 16, 32) for x in (0, 16, 32, 48)]
# per CU of the grid: fractional motion in quarter pels (the nine half-pel positions, then
# three with quarter-pel parts)
FRAC = [(-2, -2), (0, -2), (2, -2), (-2, 0), (0, 0), (2, 0), (-2, 2), (0, 2), (2, 2),
        (1, -1), (-1, 3), (3, 1)]


def _blur(a, width, axis):
    a = np.moveaxis(a, axis, 0)
    c = np.cumsum(np.concatenate([a[:1] * 0, a, a[:width]]), axis=0)   # periodic plane
    return np.moveaxis((c[width:width + len(a)] - c[:len(a)]) / width, 0, axis)


def smooth_pics(rng, bd, motion, frac=False):
    """Low-passed texture at four times the resolution; ref = every fourth sample, orig = the
    same plane displaced by `motion` (plus the CU's FRAC quarter pels) and a little noise."""
    H, W = PH + 2 * BL, PW + 2 * BL
    hi = rng.random((4 * H, 4 * W))
    for _ in range(2):
        hi = _blur(_blur(hi, 13, 0), 13, 1)
    hi = (hi - hi.min()) / (hi.max() - hi.min()) * ((1 << bd) - 1)

    def shifted(qx, qy):
        return np.roll(hi, (-(4 * motion[1] + qy), -(4 * motion[0] + qx)), (0, 1))[::4, ::4]

    ref = np.clip(np.rint(hi[::4, ::4]), 0, (1 << bd) - 1).astype(np.uint16)
    orig = shifted(0, 0).copy()
    if frac:
        for (x, y, h), (qx, qy) in zip(CUS, FRAC):
            orig[BL + y:BL + y + h, BL + x:BL + x + 16] = \
                shifted(qx, qy)[BL + y:BL + y + h, BL + x:BL + x + 16]
    orig = orig + rng.integers(-1, 2, size=orig.shape) * (1 << (bd - 8))
    return np.clip(np.rint(orig), 0, (1 << bd) - 1).astype(np.uint16), ref


def job(cu, mvp=(0, 0), prev=(0, 0), lam=498000, rng=96, depth=0, fp=0, h=None):
    x, y, hh = cu
    return (x, y, 16, h or hh, depth, fp, mvp[0], mvp[1], prev[0], prev[1], lam, rng)


def to_blocks(jobs):
    b = np.zeros(len(jobs), ol.ME_DTYPE)
    for name, col in zip(("x", "y", "w", "h", "depth_nonzero", "fullpel_mv", "mvp_x", "mvp_y",
                          "prev_x", "prev_y", "lambda16", "search_range"), zip(*jobs)):
        b[name] = col
    return b


def planted_jobs(m):
    jobs, k = [], 0
    for h in (16, 8):
        for lam in LAMBDAS:
            for oy in range(-3, 4):
                for ox in range(-3, 4):
                    cu = CUS[k % 8] if h == 16 else CUS[k % 12]
                    k += 1
                    jobs.append(job(cu, mvp=((m[0] - ox) * 16, (m[1] - oy) * 16), lam=lam, h=h))
    return jobs


def window_jobs(m):
    jobs, k = [], 0
    for r in (1, 2, 4, 8):
        for d in (r, r + 1):           # the motion on the bound, one outside
            for sx, sy in ((-1, 0), (1, 0), (0, -1), (0, 1), (-1, -1), (1, 1)):
                for rep in range(2):
                    cu = CUS[k % 12]
                    k += 1
                    mvp = ((m[0] - sx * d) * 16 + 3 * rep, (m[1] - sy * d) * 16 - 5 * rep)
                    jobs.append(job(cu, mvp=mvp, rng=r, lam=LAMBDAS[k % 3]))
        # the previous CU's vector (the true motion) wins from outside the window
        for sx, sy in ((-1, 0), (1, 0), (0, -1), (0, 1), (1, -1)):
            cu = CUS[k % 12]
            k += 1
            mvp = ((m[0] - sx * (r + 2)) * 16, (m[1] - sy * (r + 2)) * 16)
            jobs.append(job(cu, mvp=mvp, prev=m, rng=r, depth=1))
    for r in (96, 256):                 # cut by the picture's vector limits on every CU
        for cu in CUS:
            jobs.append(job(cu, mvp=(m[0] * 16 + 7, m[1] * 16 - 9), rng=r))
            jobs.append(job(cu, mvp=((m[0] + 6) * 16, (m[1] - 7) * 16), rng=r, lam=LAMBDAS[0]))
    return jobs


def grid_jobs(m):
    jobs = []
    for i, cu in enumerate(CUS):
        jobs.append(job(cu, lam=LAMBDAS[i % 3]))                              # far from (0, 0)
        jobs.append(job(cu, mvp=(-40, 24), fp=1))                             # one evaluation
        jobs.append(job(cu, mvp=((m[0] + 11) * 16, (m[1] - 12) * 16), prev=m, depth=1))
        jobs.append(job(cu, mvp=((m[0] + 11) * 16, (m[1] - 12) * 16), prev=m, depth=0))
    return jobs


def zero_jobs():
    jobs = []
    for i, cu in enumerate(CUS):
        jobs.append(job(cu, mvp=(37 * 16, -22 * 16), prev=(9, -6), depth=i & 1, lam=LAMBDAS[i % 3]))
        jobs.append(job(cu, mvp=(-3 * 16 + 5, 2 * 16 - 3), prev=(-2, 1), depth=1))
    return jobs


def subpel_jobs(m):
    return [job(cu, mvp=(m[0] * 16 + dx, m[1] * 16 + dy), lam=lam, fp=fp)
            for cu in CUS for lam in LAMBDAS[:2]
            for (dx, dy, fp) in ((0, 0, 0), (-21, 13, 0), (16, -16, 1))]


def clip_jobs(m):
    # (23, 15) are the largest vectors d_clip_mv leaves the CU at (48, 32): the CUs of the last
    # column / the bottom row end on a limit, their sub-pel candidates beyond it are clipped
    return [job(cu, mvp=(m[0] * 16 - dx, m[1] * 16 - dy), lam=lam, rng=r)
            for cu in CUS for lam in LAMBDAS[1:] for (dx, dy, r) in ((0, 0, 96), (40, 24, 8))]


M1, MC = (5, -4), (23, 15)
INPUTS = {
    "planted": (10, lambda r: smooth_pics(r, 10, M1), planted_jobs(M1)),
    "window": (10, lambda r: smooth_pics(r, 10, M1), window_jobs(M1)),
    "grid_a": (10, lambda r: make_pics(r, 10, PW, PH, BL, (40, 26)), grid_jobs((40, 26))),
    "grid_b": (10, lambda r: make_pics(r, 10, PW, PH, BL, (-17, 9)), grid_jobs((-17, 9))),
    "zero": (10, lambda r: smooth_pics(r, 10, (0, 0)), zero_jobs()),
    "subpel": (10, lambda r: smooth_pics(r, 10, M1, frac=True), subpel_jobs(M1)),
    "clip8": (8, lambda r: smooth_pics(r, 8, MC, frac=True), clip_jobs(MC)),
    "clip10": (10, lambda r: smooth_pics(r, 10, MC, frac=True), clip_jobs(MC)),
    "clip12": (12, lambda r: smooth_pics(r, 12, MC, frac=True), clip_jobs(MC)),
}
SEED = 8160
_cache = {}


def case(name):
    """(bd, orig, ref, blocks, the oracle's results): computed once, never changed"""
    if name not in _cache:
        xo = _cache.setdefault("xo", ol.Lib("xo"))
        bd, pics, jobs = INPUTS[name]
        orig, ref = pics(np.random.default_rng(SEED + sorted(INPUTS).index(name)))
        orig, ref = np.ascontiguousarray(orig), np.ascontiguousarray(ref)
        blocks = to_blocks(jobs)
        want = np.zeros(len(blocks), ol.MERES_DTYPE)
        for i, b in enumerate(blocks):
            s = me_struct(b)
            (fx, fy), cost = xo.tz_search(bd, s, PW, PH, orig, ref, BL)
            w = want[i]
            w["fullpel_x"], w["fullpel_y"], w["fullpel_cost"] = fx, fy, cost
            if b["fullpel_mv"] & 1:   # one evaluation; the oracle has no distortion for it
                w["mv_x"], w["mv_y"] = fx * 16, fy * 16
            else:
                (sx, sy), sd = xo.subpel_search(bd, s, PW, PH, orig, ref, BL, (fx, fy))
                w["mv_x"], w["mv_y"], w["subpel_dist"] = sx, sy, sd
        _cache[name] = (bd, orig, ref, blocks, want)
    return _cache[name]


def test_oracle_coverage():
    """What the inputs reach, on the oracle's answers alone."""
    xo = _cache.setdefault("xo", ol.Lib("xo"))
    half, qx, qy, bounds = set(), set(), set(), set()
    for name in INPUTS:
        bd, orig, ref, blocks, want = case(name)
        for b, w in zip(blocks, want):
            fx, fy = int(w["fullpel_x"]), int(w["fullpel_y"])
            mn, mx = xo.min_max_mv(int(b["x"]), int(b["y"]), PW, PH, int(b["mvp_x"]),
                                   int(b["mvp_y"]), int(b["search_range"]))
            for hit, tag in ((fx == mn[0], "left"), (fx == mx[0], "right"), (fy == mn[1], "up"),
                             (fy == mx[1], "down")):
                if hit:
                    bounds.add(tag)
            if b["fullpel_mv"] & 1:
                continue
            dx, dy = int(w["mv_x"]) - 16 * fx, int(w["mv_y"]) - 16 * fy
            assert abs(dx) <= 12 and abs(dy) <= 12
            # the half-pel position of the final vector: the outer one from 8 on
            half.add((np.sign(dx) * (abs(dx) >= 8), np.sign(dy) * (abs(dy) >= 8)))
            qx.add(dx % 8 != 0)
            qy.add(dy % 8 != 0)
    assert len(half) == 9, sorted(half)
    assert qx == {False, True} and qy == {False, True}
    assert bounds == {"left", "right", "up", "down"}, bounds


@pytest.fixture(scope="module")
def gpu():
    from xvc_amd import api
    ctx = api.Context(0)
    yield api, ctx
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(INPUTS))
def test_paths(gpu, name):
    api, ctx = gpu
    bd, orig, ref, blocks, want = case(name)
    O, R = ctx.picture(PW, PH, bd), ctx.picture(PW, PH, bd)
    O.upload([orig, None, None], BL)
    R.upload([ref, None, None], BL)
    both = api.ME_FULLPEL | api.ME_SUBPEL
    got = {"plain": ctx.me_search(O, R, blocks, flags=both),
           "hint": ctx.me_search(O, R, blocks, flags=both | api.ME_HINT_SQ16),
           "only": ctx.me_search(O, R, blocks, flags=both | api.ME_ONLY_SQ16, max_size=16)}
    O.destroy()
    R.destroy()
    searched = (blocks["fullpel_mv"] & 1) == 0
    for entry, res in got.items():
        for field in want.dtype.names:
            differs = res[field] != want[field]
            if field == "subpel_dist":
                differs &= searched
            bad = np.flatnonzero(differs)
            assert bad.size == 0, (name, entry, field, int(bad[0]), tuple(blocks[bad[0]]),
                                   tuple(res[bad[0]]), tuple(want[bad[0]]))
    assert np.array_equal(got["plain"], got["hint"]) and np.array_equal(got["plain"], got["only"])
