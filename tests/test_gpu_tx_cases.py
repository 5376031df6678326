"""The directed transform cases (tests/tx_cases.py) on the device, bit exact against the counted
model (tests/tx_model.py, which tests/test_tx_model.py ties to the oracle and the reference).

Every case runs through every entry point that takes it:
  residual_batch            levels, counts, reconstruction        (cases that enter at the residual)
  fwd_transform_batch       coefficients                          (the same)
  inv_transform_batch       reconstruction; the default context: residual_cu_kernel
  inv_transform_batch       on a context created with XVCGPU_INV_ONE_LAUNCH=0: the wave kernel
                            and the per-job kernel
  inv_transform_dist_batch  reconstruction and the uint64 distortion
The cases that enter at the residual reach the three inverse entry points with the quantiser's
levels.  Nothing coded (family 5) runs out of place - onto a reconstruction picture that holds
neither the prediction nor the answer - and in place, with and without the distortion.
Family 6 (the launch forms) runs through the entry points tx_cases.LAUNCHES names; the frame
pass's own instances are driven by pictures whose residuals are family 2's.

A batch is a 128 x 128 picture of non-overlapping blocks (tx_cases.pack); the whole picture is
compared, so a write outside a block shows too.
"""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as ol
import test_gpu_fwd_inv_paths as fip
import tx_cases as tc
import tx_model as tm

pytestmark = pytest.mark.gpu

SIZE = 128
BL = 128                # device border (luma)
CANVAS = 0x15           # what an out-of-place reconstruction picture holds beforehand


@pytest.fixture(scope="module")
def gpu():
    """(api, default context, a context created with XVCGPU_INV_ONE_LAUNCH=0)."""
    from xvc_amd import api
    ctx = api.Context(0)
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("XVCGPU_INV_ONE_LAUNCH", "0")
        two = api.Context(0)
    import os
    assert "XVCGPU_INV_ONE_LAUNCH" not in os.environ
    yield api, ctx, two
    two.close()
    ctx.close()


@pytest.fixture(scope="module")
def xo():
    return ol.Lib("xo")


def pad(planes):
    return [np.ascontiguousarray(np.pad(p, BL >> (1 if c else 0), mode="edge"))
            for c, p in enumerate(planes)]


flat_planes = tc.flat_planes


def batch_inputs(bd, items, models):
    """blocks, orig / pred planes (unpadded), the expected pieces per block."""
    blocks = np.zeros(len(items), ol.TX_DTYPE)
    orig, pred = flat_planes(SIZE, SIZE, 1 << (bd - 1)), flat_planes(SIZE, SIZE, 1 << (bd - 1))
    for i, (cs, x, y) in enumerate(items):
        b = cs["blk"]
        for k, v in b.items():
            blocks[i][k] = v
        blocks[i]["x"], blocks[i]["y"] = x, y
        orig[b["comp"]][y:y + b["h"], x:x + b["w"]] = cs["orig"]
        pred[b["comp"]][y:y + b["h"], x:x + b["w"]] = cs["pred"]
    ms = [models[cs["i"]] for cs, _, _ in items]
    return blocks, orig, pred, ms


def expected_rec(base, items, ms):
    exp = [p.copy() for p in base]
    for (cs, x, y), m in zip(items, ms):
        b = cs["blk"]
        exp[b["comp"]][y:y + b["h"], x:x + b["w"]] = m["rec"]
    return exp


def same_planes(pic, exp, tag):
    got = pic.download(0)
    for c in range(3):
        if not np.array_equal(got[c], exp[c]):
            ys, xs = np.nonzero(got[c] != exp[c])
            raise AssertionError((tag, "plane", c, "first differences (x, y)",
                                  list(zip(xs[:6].tolist(), ys[:6].tolist()))))


def tag_of(cs, what):
    return dict(tc.describe(cs), entry=what)


def run_batch(gpu, pics, bd, items, models):
    api, ctx, two = gpu
    (O, P, R), (P2, R2) = pics
    blocks, orig, pred, ms = batch_inputs(bd, items, models)
    canvas = flat_planes(SIZE, SIZE, CANVAS)
    O.upload(pad(orig), BL)
    P.upload(pad(pred), BL)
    P2.upload(pad(pred), BL)
    off, total = ctx.level_offsets(blocks)
    exp = expected_rec(canvas, items, ms)
    forward = items[0][0]["levels"] is None
    if forward:
        R.upload(pad(canvas), BL)
        levels, off_, nnz = ctx.residual_batch(O, P, R, blocks)
        for i, ((cs, _, _), m) in enumerate(zip(items, ms)):
            got = levels[off[i]:off[i] + cs["blk"]["w"] * cs["blk"]["h"]]
            assert int(nnz[i]) == m["nnz"], tag_of(cs, "residual_batch nnz")
            # cbf = 0: the reference never reads the level buffer; the device writes zeros
            assert np.array_equal(got, np.asarray(m["levels"]).reshape(-1)) if m["nnz"] \
                else not got.any(), tag_of(cs, "residual_batch levels")
        same_planes(R, exp, "residual_batch")
        coeffs, _ = ctx.fwd_transform_batch(O, P, blocks)
        for i, ((cs, _, _), m) in enumerate(zip(items, ms)):
            got = coeffs[off[i]:off[i] + cs["blk"]["w"] * cs["blk"]["h"]]
            assert np.array_equal(got, m["coeff"].reshape(-1)), tag_of(cs, "fwd_transform_batch")
    lv = np.zeros(max(1, total), np.int16)
    for i, m in enumerate(ms):
        flat = np.asarray(m["levels"], np.int16).reshape(-1)
        lv[off[i]:off[i] + len(flat)] = flat
    counts = np.array([m["nnz"] for m in ms], np.int32)
    want_dist = np.array([m["dist"] for m in ms], np.uint64)
    places = (False, True) if items[0][0]["family"] == 5 else (False,)
    for in_place in places:
        start = pred if in_place else canvas
        exp = expected_rec(start, items, ms)
        for name, c, p, r in (("inv_transform_batch", ctx, P, R),
                              ("inv_transform_batch, two launches", two, P2, R2)):
            r.upload(pad(start), BL)
            c.inv_transform_batch(r if in_place else p, r, blocks, lv, off, counts)
            same_planes(r, exp, (name, "in place" if in_place else "out of place",
                                 tc.describe(items[0][0])))
        R.upload(pad(start), BL)
        dist = ctx.inv_transform_dist_batch(O, R if in_place else P, R, blocks, lv, off, counts)
        same_planes(R, exp, ("inv_transform_dist_batch", in_place, tc.describe(items[0][0])))
        bad = np.nonzero(dist != want_dist)[0]
        assert not len(bad), (tag_of(items[bad[0]][0], "distortion"), int(dist[bad[0]]),
                              int(want_dist[bad[0]]))


@pytest.fixture(scope="module")
def pictures(gpu):
    """Per depth, made on first use: (O, P, R) of the default context, (P, R) of the second."""
    _, ctx, two = gpu
    made = {}

    def get(bd):
        if bd not in made:
            made[bd] = ([ctx.picture(SIZE, SIZE, bd) for _ in range(3)],
                        [two.picture(SIZE, SIZE, bd) for _ in range(2)])
        return made[bd]
    yield get
    for a, b in made.values():
        for pic in a + b:
            pic.destroy()


@pytest.mark.parametrize("family", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("bd", tc.ALL_DEPTHS)
def test_cases(gpu, pictures, bd, family):
    models = tc.modelled(bd)
    cases = [cs for cs in tc.cases(bd) if cs["family"] == family]
    batches = tc.pack(cases, SIZE)
    assert sum(len(b) for b in batches) == len(cases) > 0
    for items in batches:
        run_batch(gpu, pictures(bd), bd, items, models)


# ---- family 6: the launch forms -----------------------------------------------------------------

def rdoq_inputs(api, bd, tiles):
    """One context snapshot; per tile the parameters of its QP at the picture lambda of QP 30 (the
    middle of the range), formed as tests/test_gpu_quant_cases.py::rdoq_params forms them."""
    import oracle_rdoq as oq
    ctxs = oq.random_contexts(np.random.default_rng(9600)).view(api.RDOQ_CTX_DTYPE)
    params = np.zeros(len(tiles), api.RDOQ_PARAMS_DTYPE)
    lam = 0.57 * 2.0 ** ((30 - 12) / 3.0)
    for i, cs in enumerate(tiles):
        qpb = cs["blk"]["qp"] + 6 * (bd - 8)
        inv_scale = tm.INV_SCALES[qpb % 6] << (qpb // 6)
        params[i]["lambda"] = int(lam * 65536 + 0.5)
        params[i]["rd_factor"] = int(inv_scale * inv_scale / lam / 16 / (1 << (2 * (bd - 8))) + 0.5)
    return ctxs, params


def rdoq_tile_oracle(xo, bd, cs, flags, ctxs, prm):
    """xo_residual_pipeline_rdoq on the tile alone: (nnz, levels, reconstruction)."""
    f = xo.dll.xo_residual_pipeline_rdoq
    f.restype = C.c_int
    vp = C.c_void_p
    b = cs["blk"]
    blk = np.zeros(1, ol.TX_DTYPE)
    for k, v in b.items():
        blk[0][k] = v
    blk[0]["intra_pic"] = flags
    o, p = np.ascontiguousarray(cs["orig"]), np.ascontiguousarray(cs["pred"])
    rec = np.zeros_like(p)
    lv = np.zeros(b["w"] * b["h"], np.int16)
    st = C.c_ssize_t(b["w"])
    nnz = f(bd, vp(blk.ctypes.data), vp(ctxs.ctypes.data), vp(prm.ctypes.data), vp(o.ctypes.data),
            st, vp(p.ctypes.data), st, vp(rec.ctypes.data), st, vp(lv.ctypes.data))
    return nnz, lv if nnz else np.zeros_like(lv), rec


def paste(planes, batch, content):
    """content[t]: the h x w array every descriptor of tile t gets at its position."""
    blocks, tile = batch["blocks"], batch["tile"]
    for t, arr in enumerate(content):
        sel = np.nonzero(tile == t)[0]
        if len(sel):
            h, w = arr.shape
            ys = blocks["y"][sel].astype(np.int64)[:, None, None] + np.arange(h)[None, :, None]
            xs = blocks["x"][sel].astype(np.int64)[:, None, None] + np.arange(w)[None, None, :]
            planes[batch["tiles"][t]["blk"]["comp"]][ys, xs] = arr[None]


def per_block(batch, off, content, total, dtype=np.int16):
    """The level / coefficient buffer in which every descriptor of tile t holds content[t]."""
    out = np.zeros(max(1, total), dtype)
    for t, arr in enumerate(content):
        sel = np.nonzero(batch["tile"] == t)[0]
        if len(sel):
            flat = np.asarray(arr, dtype).reshape(-1)
            out[off[sel].astype(np.int64)[:, None] + np.arange(len(flat))[None]] = flat[None]
    return out


def first_bad(batch, off, got, want):
    i = int(np.nonzero(got != want)[0][0])
    bi = int(np.searchsorted(off, i, side="right") - 1)
    return dict(block=bi, descriptor=tuple(batch["blocks"][bi]),
                kind=batch["tiles"][batch["tile"][bi]]["kind"])


@pytest.mark.parametrize("run", tc.LAUNCHES, ids=lambda r: r["name"])
def test_launch_forms(gpu, xo, run):
    api, ctx, _ = gpu
    rdoq = run["entry"] == "rdoq"
    flags = api.TXF_RDOQ if rdoq else 0
    batch = tc.launch_batch(run["mode"], run["n"], run["per_row"], flags)
    bd, tiles, blocks, n = batch["bd"], batch["tiles"], batch["blocks"], run["n"]
    assert len(blocks) == n and int((batch["tile"] >= batch["n_bulk"]).sum()) >= 9
    paths = {tm.device_path(cs["blk"], run["entry"], n) for cs in tiles}
    assert len(paths) == 2 and all(p.split("/")[1] in run["kernels"] for p in paths), paths
    if rdoq:
        ctxs, tprm = rdoq_inputs(api, bd, tiles)
        ms = []
        for t, cs in enumerate(tiles):
            nnz, lv, rec = rdoq_tile_oracle(xo, bd, cs, flags, ctxs, tprm[t:t + 1])
            ms.append(dict(nnz=nnz, levels=lv, rec=rec))
        assert any(m["nnz"] for m in ms) and not all(m["nnz"] for m in ms)
    else:
        models = tc.modelled(bd)
        ms = []
        for cs in tiles:
            if cs["kind"] == "flat":
                ms.append(dict(nnz=0, levels=np.zeros(cs["pred"].shape, np.int16), rec=cs["pred"],
                               coeff=np.zeros(cs["pred"].shape, np.int64), dist=0))
            else:
                ms.append(models[cs["i"]])
    pw, ph = batch["pw"], batch["ph"]
    orig, pred = flat_planes(pw, ph, 1 << (bd - 1)), flat_planes(pw, ph, 1 << (bd - 1))
    paste(orig, batch, [cs["orig"] for cs in tiles])
    paste(pred, batch, [cs["pred"] for cs in tiles])
    start = pred if run["in_place"] else flat_planes(pw, ph, CANVAS)
    exp = [p.copy() for p in start]
    paste(exp, batch, [np.asarray(m["rec"]) for m in ms])
    off, total = ctx.level_offsets(blocks)
    want_nnz = np.array([m["nnz"] for m in ms], np.int32)[batch["tile"]]
    want_lv = per_block(batch, off, [np.asarray(m["levels"]) if m["nnz"] else
                                     np.zeros(tiles[t]["pred"].shape, np.int16)
                                     for t, m in enumerate(ms)], total)
    O, P, R = (ctx.picture(pw, ph, bd) for _ in range(3))
    try:
        O.upload(orig)
        P.upload(pred)
        R.upload(start)
        entry = run["entry"]
        if entry == "fwd":
            coeffs, _ = ctx.fwd_transform_batch(O, P, blocks)
            want = per_block(batch, off, [m["coeff"] for m in ms], total)
            assert np.array_equal(coeffs, want), first_bad(batch, off, coeffs, want)
            return
        if entry in ("residual", "rdoq"):
            if rdoq:
                levels, _, nnz = ctx.residual_rdoq_batch(O, P, R, blocks, ctxs, tprm[batch["tile"]])
            else:
                levels, _, nnz = ctx.residual_batch(O, P, R, blocks)
            assert np.array_equal(nnz, want_nnz), np.nonzero(nnz != want_nnz)[0][:8]
            assert np.array_equal(levels, want_lv), first_bad(batch, off, levels, want_lv)
        else:
            given = per_block(batch, off, [np.asarray(cs["levels"]) for cs in tiles], total)
            if entry == "inv":
                ctx.inv_transform_batch(R if run["in_place"] else P, R, blocks, given, off, want_nnz)
            else:
                dist = ctx.inv_transform_dist_batch(O, P, R, blocks, given, off, want_nnz)
                want = np.array([m["dist"] for m in ms], np.uint64)[batch["tile"]]
                assert np.array_equal(dist, want), np.nonzero(dist != want)[0][:8]
        same_planes(R, exp, run["name"])
    finally:
        for pic in (O, P, R):
            pic.destroy()


# ---- the frame pass's own instances -------------------------------------------------------------

@pytest.mark.parametrize("bd", [8, 10, 12])
@pytest.mark.parametrize("kind", ["16", "8", "mixed"])
def test_frame_pass_instances(gpu, xo, kind, bd):
    """recon_from_me_kernel (exact 16x16 / 8x8 + 8x8, any size) and inv_cu_pairs_kernel (exact
    16x16, exact 8x8 half-waves, the generic wave for 16x8 luma, generic half-waves for 8x4
    chroma) on full-swing residuals, zero vectors, at QP 0 and 63: the ends of the range the
    pass clamps its tables to."""
    api, ctx, _ = gpu
    parts, partition = tc.partitions(kind)
    if kind != "8":
        assert (16, 16) in {(p[2], p[3]) for p in parts} and (16, 8) in {(p[2], p[3]) for p in parts}
    for qp in tc.FRAME_QPS:
        orig, ref = tc.swing_pictures(bd, parts, weak_v=True)
        nnz = fip.forced_pass(api, ctx, xo, tc.FW, tc.FH, bd, qp, orig, ref,
                              lambda n: [(0, 0)] * n, partition=partition)
        tc.check_frame_pass_counts(qp, nnz)
