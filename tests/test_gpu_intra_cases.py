"""Every device copy of intra prediction on the directed cases of tests/intra_cases.py,
bit exact against the oracle (which tests/test_intra_model.py pins to the reference and to
the counted model of tests/intra_model.py):

  xvcgpu_intra_pred_batch    intra_build_refs<true> / intra_predict<true>, intra_lm_chroma
  xvcgpu_intra_recon_batch   decoder form without coefficients: the one-wave, barrier-free
                             instantiation, whose reconstruction is then the prediction
  xvcgpu_intra_satd_batch    max_block_size 16 (square 8x8 / 16x16: intra_row8; the rest:
                             intra_predict<false>), 32 and 64
  xvcgpu_intra_select_modes  the fold and the scan bits, against three lines of numpy

A sheet's jobs of one round are mutually disjoint blocks with their own painted
neighbourhoods: one launch per round, whole planes compared (so nothing outside the blocks
may change).  Depths 8, 10, 12 in full, 9 and 11 reduced.
"""
import numpy as np
import pytest

import intra_cases as ic
import oracle_intra as oi
import oracle_lib as ol

pytestmark = pytest.mark.gpu
PASSES = ic.all_depths()
SENTINEL = 0xa5a5
UNSUPPORTED = 0xffffffff
SCAN_CLEAR = 0xff ^ (3 << 2)      # every bit of intra_pic but XVC_TXF_SCAN_SHIFT's two


@pytest.fixture(scope="module")
def gpu():
    from xvc_amd import api
    ctx = api.Context(0)
    yield api, ctx
    ctx.close()


@pytest.fixture(scope="module")
def xo():
    return ol.Lib("xo")


def upload(ctx, planes, bd):
    P = ctx.picture(planes[0].shape[1], planes[0].shape[0], bd)
    P.upload(planes)
    return P


def assert_planes(got, exp, jobs, what):
    for c in range(3):
        if np.array_equal(got[c], exp[c]):
            continue
        for j in jobs[jobs["comp"] == c]:
            x, y, w, h = (int(j[k]) for k in "xywh")
            assert np.array_equal(got[c][y:y + h, x:x + w], exp[c][y:y + h, x:x + w]), (what, j)
        assert False, (what, c, "changed outside the jobs' blocks")


@pytest.mark.parametrize("bd,reduced", PASSES)
def test_pred_batch(gpu, xo, bd, reduced):
    """All cases, all components: a launch per round of every sheet; the prediction picture
    starts as a sentinel and must equal the oracle's planes everywhere."""
    api, ctx = gpu
    jobs_seen = 0
    for sheet in ic.sheets(bd, reduced):
        R = upload(ctx, sheet["planes"], bd)
        exp = [np.full_like(p, SENTINEL) for p in sheet["planes"]]
        P = upload(ctx, exp, bd)
        for r in range(ic.rounds(sheet)):
            jobs = ic.round_jobs(sheet, r)
            ctx.intra_pred_batch(R, P, jobs)
            for c in range(3):
                oi.pred_jobs(xo, "xo", bd, jobs[jobs["comp"] == c], sheet["planes"][c], exp[c],
                             ic.SHEET, ic.SHEET)
            assert_planes(P.download(), exp, jobs, ("round", r))
            jobs_seen += len(jobs)
        R.destroy()
        P.destroy()
    assert jobs_seen > 1000


@pytest.mark.parametrize("bd,reduced", PASSES)
def test_lm_chroma(gpu, xo, bd, reduced):
    """The LM jobs of the prediction batch: both chroma components of every target."""
    api, ctx = gpu
    for sheet in ic.lm_sheets(bd, reduced):
        R = upload(ctx, sheet["planes"], bd)
        exp = [np.full_like(p, SENTINEL) for p in sheet["planes"]]
        P = upload(ctx, exp, bd)
        jobs = np.concatenate([ic.lm_jobs(sheet, 1), ic.lm_jobs(sheet, 2)])
        ctx.intra_pred_batch(R, P, jobs)
        for j in jobs:
            x, y, w, h, comp = (int(j[k]) for k in ("x", "y", "w", "h", "comp"))
            exp[comp][y:y + h, x:x + w] = oi.lm_chroma(xo, "xo", bd, comp, x, y, w, h,
                                                       sheet["planes"])
        assert_planes(P.download(), exp, jobs, "lm")
        R.destroy()
        P.destroy()


@pytest.mark.parametrize("bd,reduced", PASSES)
def test_recon_batch_without_coefficients(gpu, xo, bd, reduced):
    """xvcgpu_intra_recon_batch, decoder form, nnz = 0 and zero levels for every job: the
    reconstruction is the prediction.  Every case the entry point takes (sides 4, 8, 16, all
    three components; the 4x4 luma jobs carry dst4x4 = 0), in place on the painted picture."""
    api, ctx = gpu
    jobs_seen = 0
    for sheet in ic.sheets(bd, reduced):
        if not any(ic.in_wave(t) for t in sheet["targets"]):
            continue
        R = upload(ctx, sheet["planes"], bd)
        exp = [p.copy() for p in sheet["planes"]]
        for r in range(ic.rounds(sheet)):
            jobs = ic.round_jobs(sheet, r, ic.in_wave)
            if not len(jobs):
                continue
            blocks = np.zeros(len(jobs), api.TX_DTYPE)
            for k in ("x", "y", "w", "h", "comp"):
                blocks[k] = jobs[k]
            blocks["tx_hor"] = blocks["tx_ver"] = 1      # XVC_TX_DCT2
            blocks["qp"], blocks["intra_pic"] = 32, api.TXF_INTRA_PIC
            off, total = ctx.level_offsets(blocks)
            bufs = [ctx.buffer(jobs), ctx.buffer(blocks), ctx.buffer(np.zeros(total, np.int16)),
                    ctx.buffer(off), ctx.buffer(np.zeros(len(jobs), np.int32))]
            ctx._check(ctx.lib.xvcgpu_intra_recon_batch(
                ctx.h, None, R.h_pic, bufs[0].ptr, bufs[1].ptr, len(jobs), bufs[2].ptr,
                bufs[3].ptr, bufs[4].ptr))
            ctx.sync()
            for b in bufs:
                b.free()
            for c in range(3):      # the reference lines lie outside every block: unchanged
                oi.pred_jobs(xo, "xo", bd, jobs[jobs["comp"] == c], sheet["planes"][c], exp[c],
                             ic.SHEET, ic.SHEET)
            assert_planes(R.download(), exp, jobs, ("round", r))
            jobs_seen += len(jobs)
        R.destroy()
    assert jobs_seen > 1000


@pytest.mark.parametrize("bd,reduced", PASSES)
def test_satd_batch(gpu, xo, bd, reduced):
    """The luma targets at max_block_size 16, 32 and 64: all 67 distances per job; a job
    larger than max_block_size is answered with XVCGPU_INTRA_SATD_UNSUPPORTED."""
    api, ctx = gpu
    rows = general = 0
    for sheet in ic.sheets(bd, reduced):
        jobs = ic.luma_jobs(sheet)
        if not len(jobs):
            continue
        mid = np.full_like(sheet["planes"][1], 1 << (bd - 1))
        O = upload(ctx, [sheet["orig"], mid, mid], bd)
        R = upload(ctx, sheet["planes"], bd)
        exp = np.array([oi.satd_modes(xo, "xo", bd, j, sheet["orig"], sheet["planes"][0])
                        for j in jobs])
        d_jobs, d_dist = ctx.buffer(jobs), ctx.alloc(4 * 67 * len(jobs))
        side = np.maximum(jobs["w"], jobs["h"])
        for ms in (16, 32, 64):
            ctx._check(ctx.lib.xvcgpu_intra_satd_batch(ctx.h, O.h_pic, R.h_pic, d_jobs.ptr,
                                                       len(jobs), d_dist.ptr, ms))
            got = d_dist.to_array(np.uint32, 67 * len(jobs)).reshape(-1, 67)
            assert got.shape == (len(jobs), 67)
            for j, g, e, s in zip(jobs, got, exp, side):
                if s > ms:
                    assert (g == UNSUPPORTED).all(), (ms, j)
                else:
                    assert np.array_equal(g, e), (ms, j, np.flatnonzero(g != e))
            if ms == 16:
                rows += int(((jobs["w"] == jobs["h"]) & np.isin(jobs["w"], (8, 16))).sum())
            general += int((side <= ms).sum())
        for b in (d_jobs, d_dist):
            b.free()
        O.destroy()
        R.destroy()
    assert rows >= 16 and general > rows


# ---- xvcgpu_intra_select_modes ------------------------------------------------------------
def select(ctx, api, dist, cost, per_cu, modes=True, jobs=None, blocks=None):
    n = len(dist)
    bufs = {"dist": ctx.buffer(dist)}
    if cost is not None:
        bufs["cost"] = ctx.buffer(cost)
    if modes:
        bufs["modes"] = ctx.buffer(np.full(n + 2, -7, np.int32))
    if jobs is not None:
        bufs["jobs"] = ctx.buffer(jobs)
    if blocks is not None:
        bufs["blocks"] = ctx.buffer(blocks)

    def ptr(k):
        return bufs[k].ptr if k in bufs else None

    ctx._check(ctx.lib.xvcgpu_intra_select_modes(ctx.h, ptr("dist"), ptr("cost"), n, ptr("modes"),
                                                 ptr("jobs"), ptr("blocks"), per_cu))
    ctx.sync()
    out = (bufs["modes"].to_array(np.int32, n + 2) if modes else None,
           bufs["jobs"].to_array(oi.INTRA_DTYPE, len(jobs)) if jobs is not None else None,
           bufs["blocks"].to_array(api.TX_DTYPE, len(blocks)) if blocks is not None else None)
    for b in bufs.values():
        b.free()
    return out


def expected_modes(dist, cost):
    total = dist.astype(np.uint64) + (0 if cost is None else cost.astype(np.uint64))
    return total.argmin(axis=1)          # the first minimum


def expected_scan(mode, w, h):
    """TransformHelper::DetermineScanOrder: below 16 on both luma sides, within 10 modes of
    vertical -> horizontal scan (1), else within 10 of horizontal -> vertical scan (2)."""
    small = (w < 16) & (h < 16)
    return np.where(small & (np.abs(mode - 50) < 10), 1,
                    np.where(small & (np.abs(mode - 18) < 10), 2, 0))


def select_tables():
    """Distortion / cost tables whose minimum sits where the fold can go wrong."""
    rng = np.random.default_rng(7200)
    rows, costs = [], []

    def add(d, c=None):
        rows.append(np.asarray(d, np.uint32))
        costs.append(np.zeros(67, np.uint32) if c is None else np.asarray(c, np.uint32))

    for m in list(range(67)):                       # a single minimum at every mode
        d = rng.integers(1000, 1 << 20, 67)
        d[m] = 999
        add(d)
    for a, b in ((0, 64), (1, 65), (2, 66), (0, 66), (3, 4), (63, 64), (65, 66), (0, 1)):
        d = rng.integers(1000, 1 << 20, 67)         # ties: the first wins; k and k + 64 lie
        d[a] = d[b] = 7                             # in one lane
        add(d)
    add(np.full(67, 0xffffffff))                    # every entry all ones: mode 0
    d = np.full(67, 0xffffffff)
    d[66] = 0xfffffffe
    add(d)
    add(np.zeros(67))
    for m in (0, 1, 2, 40, 64, 66):                 # dist + cost above 2^32: no wrap
        d = rng.integers(0xfff00000, 0x100000000, 67)
        c = rng.integers(0xfff00000, 0x100000000, 67)
        d[m], c[m] = 0xfff00000, 0x000fffff         # the smallest sum; wrapped sums are smaller
        add(d, c)
    d, c = np.full(67, 0xffffffff), np.full(67, 0xffffffff)
    add(d, c)                                       # all ones plus all ones
    d, c = rng.integers(0, 1 << 16, 67), rng.integers(0, 1 << 16, 67)
    c[:] = (1 << 16) - d                            # a tie of the sums only
    add(d, c)
    return np.array(rows), np.array(costs)


@pytest.mark.parametrize("per_cu", [1, 2, 3])
def test_select_modes(gpu, per_cu):
    api, ctx = gpu
    dist, cost = select_tables()
    assert len(dist) % 4
    for use_cost in (False, True):
        n = len(dist)
        c = cost if use_cost else None
        exp = expected_modes(dist, c)
        if use_cost:        # the 64-bit sums matter: folded in 32 bit the choice differs
            wrapped = (dist + cost).argmin(axis=1)
            assert (wrapped != exp).sum() >= 4
        assert set(exp.tolist()) == set(range(67))
        # per_cu jobs / blocks per CU and two CUs more, which must stay as they are
        sizes = [(w, h) for w in (4, 8, 16) for h in (4, 8, 16)]
        jobs = np.zeros(per_cu * (n + 2), oi.INTRA_DTYPE)
        blocks = np.zeros(per_cu * (n + 2), api.TX_DTYPE)
        rng = np.random.default_rng(7300 + per_cu)
        jobs["mode"] = 99
        jobs["reserved"] = rng.integers(0, 256, len(jobs))
        blocks["intra_pic"] = rng.integers(0, 256, len(blocks))
        blocks["qp"] = rng.integers(-20, 52, len(blocks))
        for i in range(n + 2):
            w, h = sizes[(i + i // 9) % 9]
            for k in range(per_cu):
                b = blocks[i * per_cu + k]
                b["w"], b["h"], b["comp"] = (w, h, 0) if k == 0 else (w // 2, h // 2, k)
        got_modes, got_jobs, got_blocks = select(ctx, api, dist, c, per_cu, True, jobs, blocks)
        assert np.array_equal(got_modes[:n], exp) and (got_modes[n:] == -7).all()
        e_jobs, e_blocks = jobs.copy(), blocks.copy()
        e_jobs["mode"][:per_cu * n] = np.repeat(exp, per_cu)
        lw, lh = blocks["w"][::per_cu][:n].astype(int), blocks["h"][::per_cu][:n].astype(int)
        scan = np.repeat(expected_scan(exp, lw, lh), per_cu)
        e_blocks["intra_pic"][:per_cu * n] = \
            (blocks["intra_pic"][:per_cu * n] & SCAN_CLEAR) | (scan << api.TXF_SCAN_SHIFT)
        assert np.array_equal(got_jobs, e_jobs)
        assert np.array_equal(got_blocks, e_blocks)
        # d_modes NULL; jobs and blocks NULL
        _, got_jobs, got_blocks = select(ctx, api, dist, c, per_cu, False, jobs, blocks)
        assert np.array_equal(got_jobs, e_jobs) and np.array_equal(got_blocks, e_blocks)
        got_modes, _, _ = select(ctx, api, dist, c, per_cu)
        assert np.array_equal(got_modes[:n], exp) and (got_modes[n:] == -7).all()


def test_select_modes_scan_bits(gpu):
    """Every chosen mode 0..66 on every luma size of {4, 8, 16}^2: the scan bits."""
    api, ctx = gpu
    sizes = [(w, h) for w in (4, 8, 16) for h in (4, 8, 16)]
    n = 67 * len(sizes)
    dist = np.full((n, 67), 5000, np.uint32)
    mode = np.arange(n) % 67
    dist[np.arange(n), mode] = 17
    blocks = np.zeros(3 * n, api.TX_DTYPE)
    for i in range(n):
        w, h = sizes[i // 67]
        for k in range(3):
            b = blocks[3 * i + k]
            b["w"], b["h"], b["comp"] = (w, h, 0) if k == 0 else (w // 2, h // 2, k)
            b["intra_pic"] = (0xf3, 0x01, 0xff)[k]
    got_modes, _, got_blocks = select(ctx, api, dist, None, 3, True, None, blocks)
    assert np.array_equal(got_modes[:n], mode)
    lw, lh = blocks["w"][::3].astype(int), blocks["h"][::3].astype(int)
    scan = np.repeat(expected_scan(mode, lw, lh), 3)
    exp = blocks.copy()
    exp["intra_pic"] = (blocks["intra_pic"] & SCAN_CLEAR) | (scan << api.TXF_SCAN_SHIFT)
    assert np.array_equal(got_blocks, exp)
    assert {0, 1, 2} == set(scan.tolist())
    for m, s in ((40, 0), (41, 1), (59, 1), (60, 0), (8, 0), (9, 2), (27, 2), (28, 0)):
        assert int(expected_scan(np.array(m), np.array(8), np.array(8))) == s
