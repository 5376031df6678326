"""The quantiser's class lists, built in one launch (rdoq_lists_kernel) or two
(rdoq_count_kernel + rdoq_scatter_kernel): xvcgpu_quant_rdo_set_list_form forces either
form on any batch size.  Both must give the same lists - ascending, disjoint, covering
every block the classification and the all-zero proof left - and the quantiser's levels
and counts must equal the oracle's under both; a frame pass must not change either."""
import numpy as np
import pytest

import oracle_lib as ol
import oracle_rdoq as oq

pytestmark = pytest.mark.gpu
BD, QP = 10, 30
POOL = 3 * 8160           # the 1080p frame pass's own batch
SHAPES = [(4, 4), (8, 8), (16, 16)]
# the partial uint32 of class bytes; one chunk of 1024, its edge, the first workgroup
# that reads a prefix; a prefix of exactly two chunks; a prefix longer than one 16-byte
# load per thread (more than four chunks); the workload's own n
SIZES = [1, 3, 4, 5, 1023, 1024, 1025, 2049, 4097, POOL]


@pytest.fixture(scope="module")
def gpu():
    from xvc_amd import api
    ctx = api.Context(0)
    yield api, ctx
    ctx.close()


@pytest.fixture(scope="module")
def pool(gpu):
    """POOL blocks of 4x4 / 8x8 / 16x16 mixed (a few with the horizontal scan: the general
    class), their coefficients - strong, around the quantiser's threshold, or all zero -
    and the oracle's levels and counts, computed once; a case of n blocks takes the first
    n (a block's result does not depend on its batch).  The first three blocks are a
    coded 16x16, an all-zero 4x4 and a coded 8x8, so that n = 3 already holds two classes
    and a removed block."""
    api, _ = gpu
    from xvc_amd import pipeline
    rng = np.random.default_rng(20480)
    ctxs = pipeline.rdoq_init_contexts(QP, 1)
    lam, rdf = pipeline.rdoq_host_params(QP, BD)[0]
    shape = rng.choice(3, POOL, p=[0.6, 0.3, 0.1])
    kind = rng.choice(3, POOL, p=[0.5, 0.25, 0.25])    # strong / near threshold / all zero
    scan = np.where((shape < 2) & (rng.random(POOL) < 0.05), 1, 0)
    shape[:3], kind[:3], scan[:3] = [2, 0, 1], [0, 2, 0], 0
    blocks = np.zeros(POOL, api.TX_DTYPE)
    prm = np.zeros(POOL, api.RDOQ_PARAMS_DTYPE)
    prm["lambda"], prm["rd_factor"] = lam, rdf
    coeffs, off, pos = [], np.zeros(POOL, np.uint32), 0
    for i in range(POOL):
        w, h = SHAPES[shape[i]]
        blocks[i]["w"], blocks[i]["h"], blocks[i]["qp"] = w, h, QP
        blocks[i]["intra_pic"] = api.TXF_RDOQ | (int(scan[i]) << api.TXF_SCAN_SHIFT)
        # the quantiser's step on a coefficient of this shape (QP 30, 10 bits): 2^(26 -
        # log2 w) / 26214; strong = levels of a few, near threshold = mostly 0, some 1
        step = 2.0 ** (26 - int(np.log2(w))) / 26214.0
        amp = (2.0, 0.25, 0.0)[kind[i]] * step
        coeffs.append(np.clip(np.rint(rng.laplace(0, 1, w * h) * amp), -32768, 32767)
                      .astype(np.int16))
        off[i] = pos
        pos += w * h
    xo = ol.Lib("xo")
    e_nnz = np.zeros(POOL, np.int32)
    e_lv = np.zeros(pos, np.int16)
    for i in range(POOL):
        if kind[i] == 2:
            continue                                    # no coefficient: nothing to code
        w, h = SHAPES[shape[i]]
        nz, lv = oq.quant_rdo_oracle(xo, BD, QP, 0, int(scan[i]), 1, ctxs, prm[i:i + 1],
                                     coeffs[i].reshape(h, w))
        e_nnz[i] = nz
        if nz:      # (cbf = 0: the reference's level buffer is unspecified, zeros here)
            e_lv[off[i]:off[i] + w * h] = lv.reshape(-1)
    return dict(blocks=blocks, prm=prm, ctxs=ctxs, coeffs=np.concatenate(coeffs), off=off,
                e_nnz=e_nnz, e_lv=e_lv)


def run_form(ctx, p, n, form):
    """The first n blocks of the pool through xvcgpu_quant_rdo_batch with the list form
    forced: levels, counts and the three class lists."""
    end = int(p["off"][n]) if n < POOL else len(p["coeffs"])
    ctx.set_rdoq_list_form(form)
    try:
        levels, nnz = ctx.quant_rdo_batch(BD, p["blocks"][:n], p["coeffs"][:end], p["off"][:n],
                                          p["ctxs"], p["prm"][:n])
        lists = ctx.debug_rdoq_lists(n)
    finally:
        ctx.set_rdoq_list_form(-1)
    return levels, nnz, lists, end


@pytest.mark.parametrize("n", SIZES)
def test_lists_one_launch_equals_two(gpu, pool, n):
    """Form 1 and form 0 build byte-identical lists; each list strictly ascending, the
    lists disjoint, and with the removed blocks they cover 0 .. n - 1; levels and counts
    equal the oracle's under both forms.  (n = 1 can hold one block only: it must be on a
    list; from n = 3 on at least two classes and the removed set are non-empty.)"""
    api, ctx = gpu
    ctx.set_rdoq_prove_zero(1)
    try:
        lv1, nnz1, lists1, end = run_form(ctx, pool, n, 1)
        lv0, nnz0, lists0, _ = run_form(ctx, pool, n, 0)
    finally:
        ctx.set_rdoq_prove_zero(-1)
    sizes = [len(a) for a in lists0]
    print("n = %d: class sizes %s (one launch %s), removed %d" %
          (n, sizes, [len(a) for a in lists1], n - sum(sizes)))
    for c in range(3):
        assert np.array_equal(lists1[c], lists0[c]), (n, c)
        assert np.all(np.diff(lists1[c]) > 0), (n, c)
    listed = np.concatenate(lists1)
    assert len(np.unique(listed)) == len(listed), n
    assert len(listed) == 0 or (listed.min() >= 0 and listed.max() < n), n
    removed = np.setdiff1d(np.arange(n), listed)
    # a block leaves the lists only when nothing of it is coded, and every coded block is listed
    assert not pool["e_nnz"][removed].any(), n
    assert len(listed) + len(removed) == n
    if n >= 3:
        assert sum(s > 0 for s in sizes) >= 2 and len(removed) > 0, (n, sizes)
    else:
        assert len(listed) == 1
    for lv, nnz in ((lv1, nnz1), (lv0, nnz0)):
        assert np.array_equal(nnz, pool["e_nnz"][:n]), n
        assert np.array_equal(lv, pool["e_lv"][:end]), n


def test_frame_pass_same_under_both_forms(gpu):
    """One 64x48 QP 32 RDOQ frame pass with the one-launch lists against the same pass with
    count + scatter: reconstruction, counts, CU records and SSD."""
    api, ctx = gpu
    from xvc_amd import pipeline, synth
    pw, ph, border = 64, 48, 128
    clip = synth.SyntheticClip(pw, ph, BD)

    def pad(planes):
        return [np.ascontiguousarray(np.pad(p, border if c == 0 else border // 2, mode="edge"))
                for c, p in enumerate(planes)]

    O, R, Rec = (ctx.picture(pw, ph, BD) for _ in range(3))
    O.upload(pad(clip.frame(1)), border)
    R.upload(pad(clip.frame(0)), border)
    fp = pipeline.FramePass(ctx, pw, ph, BD, qp=32, rdoq=True)
    got = []
    try:
        for form in (1, 0):
            ctx.set_rdoq_list_form(form)
            fp.run(O, R, Rec)
            ctx.sync()
            res, nnz, cus, ssd = fp.results()
            got.append((Rec.download(border), res, nnz, cus, ssd))
    finally:
        ctx.set_rdoq_list_form(-1)
        fp.destroy()
        for p in (O, R, Rec):
            p.destroy()
    (rec1, res1, nnz1, cus1, ssd1), (rec0, res0, nnz0, cus0, ssd0) = got
    assert nnz0.any()                       # the pass codes something
    for c in range(3):
        assert np.array_equal(rec1[c], rec0[c]), c
    assert np.array_equal(res1, res0) and np.array_equal(nnz1, nnz0)
    assert cus1.tobytes() == cus0.tobytes()
    assert np.array_equal(ssd1, ssd0)
