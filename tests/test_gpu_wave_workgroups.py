"""The kernels whose workgroup shape is a constant of its own - recon_from_me_kernel
(RECON_WAVES), inv_cu_pairs_kernel (INV_PAIRS_WAVES), rdoq_lists_kernel (RDOQ_LISTS_WAVES)
and picture_ssd_sum_kernel (SSD_SUM_WAVES) - at the job counts where the indexing of
workgroups and waves has an edge, whatever the constants are set to.

Whole frame passes, as chains of three (each reconstruction is the next reference), byte
for byte against the oracle's frame pass: 16x16 (one CU, two jobs, the rest of the grid
padding), 48x32 (12 jobs: fewer than two a XCD), 80x48 (30 jobs: no multiple of 4 or 8),
64x40 (a bottom row of 16x8 CUs: the any-size path) and 144x80 (45 CUs: uneven eighths).
With RDOQ the class lists of every pass are those numpy builds from the oracle's own
coefficients.  The class lists alone at the batch sizes around a workgroup's chunk, and the
SSD fold at 1, 2 and 12 tiles."""
import functools

import numpy as np
import pytest

import oracle_frame
import oracle_lib as ol
import test_gpu_fwd_inv_paths as fi
import test_gpu_prove_decisions as pd
import test_gpu_rdoq_lists as rl
import test_rdoq_zero_proof as zp

BORDER = 128
QP = 32
CHAIN = 3
PICTURES = [(16, 16), (48, 32), (80, 48), (64, 40), (144, 80)]
DEPTHS = [8, 10]


@pytest.fixture(scope="module")
def gpu():
    from xvc_amd import api
    ctx = api.Context(0)
    yield api, ctx
    ctx.close()


def _pad(planes):
    return [np.ascontiguousarray(np.pad(p, BORDER if c == 0 else BORDER // 2, mode="edge"))
            for c, p in enumerate(planes)]


@functools.lru_cache(maxsize=None)
def _xo():
    return ol.Lib("xo")


def _tx_class(t):
    """rq_class_of (k_rdoq.h) for the blocks of these passes: diagonal scan, 4x4 sub-blocks."""
    n_sb = (int(t["w"]) >> 2) * (int(t["h"]) >> 2)
    return 0 if n_sb <= 4 else (1 if n_sb <= 16 else 2)


def _expected_lists(xo, desc, bd, orig, ref, res):
    """The class lists of an RDOQ pass from the oracle alone: a block is listed unless
    nothing of its forward transform quantises to a level or the bound of
    tests/test_rdoq_zero_proof.py proves the quantiser's answer zero.  Returns (the three
    lists, blocks proved)."""
    ent = zp.entropy_table(xo)
    pw, ph = desc.w, desc.h
    pred = [np.zeros((ph >> (c > 0), pw >> (c > 0)), np.uint16) for c in range(3)]
    for b, r in zip(desc.me, res):
        x, y, w, h = int(b["x"]), int(b["y"]), int(b["w"]), int(b["h"])
        for c in range(3):
            s = 1 if c else 0
            pred[c][y >> s:(y + h) >> s, x >> s:(x + w) >> s] = xo.mc_block(
                bd, c, x, y, w, h, int(r["mv_x"]), int(r["mv_y"]), pw, ph, ref[c],
                BORDER >> s)
    lists, proved_n = [[], [], []], 0
    for i, t in enumerate(desc.tx):
        c, x, y, w, h = (int(t[k]) for k in ("comp", "x", "y", "w", "h"))
        bb = BORDER >> (c > 0)
        o = orig[c][bb + y:bb + y + h, bb + x:bb + x + w].astype(np.int32)
        resi = np.ascontiguousarray((o - pred[c][y:y + h, x:x + w]).astype(np.int16))
        src = xo.fwd_transform(bd, resi)
        nc = pd.n_candidates(bd, int(t["qp"]), src)
        proved = bool(nc) and zp.proves_zero(ent, bd, int(t["qp"]), c, 0, desc.rdoq_contexts[0],
                                             desc.rdoq_params[i], src)
        proved_n += proved
        if nc and not proved:
            lists[_tx_class(t)].append(i)
    return [np.asarray(a, np.int32) for a in lists], proved_n


@functools.lru_cache(maxsize=None)
def oracle_chain(pw, ph, bd, rdoq):
    """The chain on the CPU, computed once per case: per pass the oracle's padded
    reconstruction, search results, counts, CU records and SSD, and with RDOQ the levels
    of every block and the expected class lists."""
    from xvc_amd import pipeline, synth
    xo = _xo()
    desc = pipeline.FrameDescriptors(pw, ph, QP, rdoq=rdoq, bitdepth=bd)
    clip = synth.SyntheticClip(pw, ph, bd)
    ref = _pad(clip.frame(0))
    out = []
    for k in range(1, CHAIN + 1):
        orig = _pad(clip.frame(k))
        rec, res, nnz, cus, ssd = oracle_frame.frame_pass(desc, bd, orig, ref, BORDER, lib=xo)
        p = dict(rec=rec, res=res, nnz=nnz, cus=cus, ssd=ssd)
        if rdoq:
            mvs = [(int(r["mv_x"]), int(r["mv_y"])) for r in res]
            _, nnz2, _, p["levels"] = fi.oracle_encode(xo, desc, bd, orig, ref, mvs)
            assert np.array_equal(nnz2, nnz)
            p["lists"], p["proved"] = _expected_lists(xo, desc, bd, orig, ref, res)
        out.append(p)
        ref = rec
    return desc, out


def test_cases_meet_every_class():
    """(no GPU) the oracle alone: every picture runs, its CU and job counts are the ones
    named above, and over the set there are coded and uncoded blocks, blocks the proof
    takes off the lists, and blocks on each list the passes have (classes 0 and 1); a coded
    block is always listed."""
    seen = dict(coded=0, uncoded=0, proved=0, listed=[0, 0, 0])
    for pw, ph in PICTURES:
        for bd in DEPTHS:
            for rdoq in (True, False):
                desc, passes = oracle_chain(pw, ph, bd, rdoq)
                assert len(passes) == CHAIN
                for p in passes:
                    seen["coded"] += int(np.count_nonzero(p["nnz"]))
                    seen["uncoded"] += int(np.count_nonzero(p["nnz"] == 0))
                    if rdoq:
                        seen["proved"] += p["proved"]
                        listed = np.concatenate(p["lists"])
                        assert np.isin(np.nonzero(p["nnz"])[0], listed).all()
                        for c in range(3):
                            seen["listed"][c] += len(p["lists"][c])
    print(seen)
    n_cus = {(pw, ph): oracle_chain(pw, ph, 10, True)[0].n_cus for pw, ph in PICTURES}
    assert n_cus == {(16, 16): 1, (48, 32): 6, (80, 48): 15, (64, 40): 12, (144, 80): 45}
    shapes = {(int(b["w"]), int(b["h"])) for b in oracle_chain(64, 40, 10, True)[0].me}
    assert shapes == {(16, 16), (16, 8)}
    assert seen["coded"] and seen["uncoded"] and seen["proved"]
    assert seen["listed"][0] and seen["listed"][1] and not seen["listed"][2]


@pytest.mark.gpu
@pytest.mark.parametrize("rdoq", [True, False])
@pytest.mark.parametrize("bd", DEPTHS)
@pytest.mark.parametrize("pw,ph", PICTURES)
def test_frame_pass_chain(gpu, pw, ph, bd, rdoq):
    """Three passes in a row equal the oracle's: reconstruction planes (borders included),
    search results, counts, CU records, SSD and samples; with RDOQ also every block's
    levels and the three class lists."""
    api, ctx = gpu
    from xvc_amd import pipeline, synth
    desc, passes = oracle_chain(pw, ph, bd, rdoq)
    clip = synth.SyntheticClip(pw, ph, bd)
    O, R, Rec = (ctx.picture(pw, ph, bd) for _ in range(3))
    fp = pipeline.FramePass(ctx, pw, ph, bd, qp=QP, rdoq=rdoq)
    assert fp.form == ("fwd_from_me" if rdoq else "recon_from_me")
    assert fp.desc.n_cus == desc.n_cus and len(fp.desc.tx) == 3 * desc.n_cus
    try:
        R.upload(_pad(clip.frame(0)), BORDER)
        for k, e in enumerate(passes):
            O.upload(_pad(clip.frame(k + 1)), BORDER)
            fp.run(O, R, Rec)
            ctx.sync()
            res, nnz, cus, ssd = fp.results()
            assert np.array_equal(res, e["res"]), k
            assert np.array_equal(nnz, e["nnz"]), (k, np.nonzero(nnz != e["nnz"])[0][:8])
            assert cus.tobytes() == e["cus"].tobytes(), k
            assert (int(ssd[0]), int(ssd[1])) == e["ssd"], k
            got = Rec.download(BORDER)
            for c in range(3):
                assert np.array_equal(got[c], e["rec"][c]), (k, c)
            if rdoq:
                levels = fp.d_levels.to_array(np.int16, max(1, fp.n_levels))
                off = np.asarray(ctx.level_offsets(fp.desc.tx)[0], np.int64)
                for i, lv in enumerate(e["levels"]):
                    g = levels[off[i]:off[i] + len(lv)]
                    if e["nnz"][i]:
                        assert np.array_equal(g, lv), (k, i)
                    else:       # cbf = 0: the reference's level buffer is unspecified, zeros here
                        assert not g.any(), (k, i)
                lists = ctx.debug_rdoq_lists(len(fp.desc.tx))
                for c in range(3):
                    assert np.array_equal(lists[c], e["lists"][c]), (k, c)
            R, Rec = Rec, R
    finally:
        fp.destroy()
        for p in (O, R, Rec):
            p.destroy()


# ---- the class lists alone ---------------------------------------------------------------
# around a chunk of one wave (256 blocks), of two (512) and of four (1024); the 1080p pass
LIST_SIZES = [1, 255, 256, 257, 511, 512, 513, 1023, 1025, rl.POOL]


@pytest.fixture(scope="module")
def class_pool():
    """rl.POOL blocks in the layout of tests/test_gpu_rdoq_lists.py's pool with the class of
    every block known without a quantiser: a coded block carries one coefficient far above
    the threshold (class by shape and scan: 4x4 and 8x8 diagonal 0, 16x16 1, horizontal scan
    2), one block in four carries none and is on no list (class -1).  (The all-zero proof
    is off in these runs: what is listed is the classification alone.)"""
    from xvc_amd import api, pipeline
    rng = np.random.default_rng(4242)
    n = rl.POOL
    lam, rdf = pipeline.rdoq_host_params(rl.QP, rl.BD)[0]
    shape = rng.choice(3, n, p=[0.5, 0.3, 0.2])
    scan = np.where((shape < 2) & (rng.random(n) < 0.1), 1, 0)
    coded = rng.random(n) >= 0.25
    blocks = np.zeros(n, api.TX_DTYPE)
    prm = np.zeros(n, api.RDOQ_PARAMS_DTYPE)
    prm["lambda"], prm["rd_factor"] = lam, rdf
    sides = np.array([4, 8, 16])[shape]
    blocks["w"] = blocks["h"] = sides
    blocks["qp"] = rl.QP
    blocks["intra_pic"] = api.TXF_RDOQ | (scan << api.TXF_SCAN_SHIFT)
    off = np.zeros(n, np.uint32)
    off[1:] = np.cumsum(sides[:-1].astype(np.int64) ** 2)
    coeffs = np.zeros(int(off[-1]) + int(sides[-1]) ** 2, np.int16)
    coeffs[off[coded]] = np.where(rng.random(int(coded.sum())) < 0.5, 3000, -3000)
    cls = np.where(coded, np.where(scan == 1, 2, np.where(shape == 2, 1, 0)), -1)
    return dict(blocks=blocks, prm=prm, ctxs=pipeline.rdoq_init_contexts(rl.QP, 1),
                coeffs=coeffs, off=off, cls=cls)


@pytest.mark.gpu
@pytest.mark.parametrize("n", LIST_SIZES)
def test_class_lists_equal_numpy(gpu, class_pool, n):
    """One launch (rdoq_lists_kernel) and two (count + scatter): the lists of the first n
    blocks are numpy's - for every class the ascending indices of its blocks - and so are
    the counts; every class and the unlisted blocks occur from n = 255 on."""
    api, ctx = gpu
    cls = class_pool["cls"][:n]
    want = [np.nonzero(cls == c)[0].astype(np.int32) for c in range(3)]
    if n >= 255:
        assert all(len(w) for w in want) and (cls < 0).any()
    ctx.set_rdoq_prove_zero(0)
    try:
        for form in (1, 0):
            lists = rl.run_form(ctx, class_pool, n, form)[2]
            for c in range(3):
                assert len(lists[c]) == len(want[c]), (n, form, c)
                assert np.array_equal(lists[c], want[c]), (n, form, c)
    finally:
        ctx.set_rdoq_prove_zero(-1)


# ---- the SSD fold ------------------------------------------------------------------------
def _ssd_parts(w, h):
    """ssd_items (xvcgpu.hip): the blocks ComparePicture visits - 64-sample steps while more
    than 64 samples are left, then blocks of the largest power of two dividing the side."""
    def along(n):
        return (max(n - 64 + 63, 0) // 64 if n > 64 else 0) + (n - (n & ~63)) // (n & -n)
    return along(w) * along(h)


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,parts", [(64, 64, 0), (72, 40, 10), (200, 136, 12)])
def test_picture_ssd_fold(gpu, w, h, parts):
    """xvcgpu_picture_ssd (a block per workgroup, then picture_ssd_sum_kernel) against the
    oracle's ComparePicture on pictures of 1, 2 and 12 tiles of 64x64: the fold of no part
    at all (a 64x64 picture: ComparePicture visits nothing of it, the sum is (0, 0)), of ten
    remainder blocks, and of twelve parts, whole and remainder blocks mixed."""
    api, ctx = gpu
    xo = _xo()
    assert _ssd_parts(w, h) == parts
    bd = 10
    rng = np.random.default_rng(w * 1000 + h)
    pa = [rng.integers(0, 1 << bd, (h >> (c > 0), w >> (c > 0))).astype(np.uint16)
          for c in range(3)]
    pb = [np.clip(p.astype(np.int32) + rng.integers(-40, 41, size=p.shape), 0,
                  (1 << bd) - 1).astype(np.uint16) for p in pa]
    A, B = ctx.picture(w, h, bd), ctx.picture(w, h, bd)
    try:
        A.upload(_pad(pa), BORDER)
        B.upload(_pad(pb), BORDER)
        for sbd in (8, bd):
            got = ctx.picture_ssd(A, B, 0, sbd)
            exp = xo.picture_ssd(sbd, pa[0], pb[0])
            assert got == exp and (exp[0] > 0) == (parts > 0), (sbd, got, exp)
    finally:
        A.destroy()
        B.destroy()
