"""The forward (fwd_from_me) and inverse (inv_transform) launches of the packed-RDOQ frame
pass on their own: the motion results are written into the pass's result array instead of
searched, so every filter case of both interpolators, every clip of the vector, the exact
16x16 / 8x8 + 8x8 instances, the any-size paths beside them and the inverse's early exit
are reached on purpose.  Expected values: the oracle's block functions in the order
xo_frame_pass calls them (xo_mc_block per component, xo_residual_pipeline_rdoq per
transform block, the CU records) - xo_frame_pass itself always searches.  Where the search
runs (the 32x32 CU), oracle_frame.frame_pass is the reference as in
tests/test_gpu_partition_pass.py."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as ol

BL, BC = 128, 64  # device borders

# (mv_x, mv_y) in 1/16 luma samples; the chroma phase is mv & 31
MVS = [
    (0, 0), (32, -16),                       # integer in luma and chroma
    (4, 0), (-20, 16),                       # horizontal phase only
    (0, 8), (16 * 2, -12),                   # vertical phase only
    (4, 8), (-7, 13), (12, -4), (15, 1),     # both phases: the two-stage filter
    (16, 32), (-48, 64),                     # luma integer, chroma phase in x only
    (32, 16), (0, -80),                      # luma integer, chroma phase in y only
    (-5000, 3), (5000, -3), (5, -5000), (-5, 5000),   # clipped at the four edges
]


@pytest.fixture(scope="module")
def gpu():
    from xvc_amd import api
    ctx = api.Context(0)
    yield api, ctx
    ctx.close()


@pytest.fixture(scope="module")
def xo():
    return ol.Lib("xo")


def pad_planes(planes):
    return [np.ascontiguousarray(np.pad(p, BL if c == 0 else BC, mode="edge"))
            for c, p in enumerate(planes)]


def clip_planes(w, h, bd, n):
    from xvc_amd import synth
    return synth.SyntheticClip(w, h, bd).frame(n)


def noise_planes(w, h, bd, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 1 << bd, (h >> (c > 0), w >> (c > 0))).astype(np.uint16)
            for c in range(3)]


def mvs_for(n, shift):
    return [MVS[(i + shift) % len(MVS)] for i in range(n)]


def oracle_encode(xo, desc, bd, orig, ref, mvs, ref_poc=0):
    """orig / ref: padded planes.  Returns (rec planes, nnz, cus, levels per block)."""
    from xvc_amd import api
    f = xo.dll.xo_residual_pipeline_rdoq
    f.restype = C.c_int
    vp = C.c_void_p
    pw, ph = desc.w, desc.h
    pred = [np.zeros((ph >> (c > 0), pw >> (c > 0)), np.uint16) for c in range(3)]
    for b, (mx, my) in zip(desc.me, mvs):
        x, y, w, h = int(b["x"]), int(b["y"]), int(b["w"]), int(b["h"])
        for c in range(3):
            s = 1 if c else 0
            pred[c][y >> s:(y + h) >> s, x >> s:(x + w) >> s] = xo.mc_block(
                bd, c, x, y, w, h, mx, my, pw, ph, ref[c], BC if c else BL)
    rec = [np.zeros_like(p) for p in pred]
    tx = np.ascontiguousarray(desc.tx)
    prm = np.ascontiguousarray(desc.rdoq_params)
    ctxs = np.ascontiguousarray(desc.rdoq_contexts)
    nnz = np.zeros(len(tx), np.int32)
    levels = []
    coeff = np.zeros(64 * 64, np.int16)
    for i, t in enumerate(tx):
        c = int(t["comp"])
        bb = BC if c else BL
        o = orig[c]
        st = o.strides[0] // 2
        nnz[i] = f(bd, vp(tx[i:i + 1].ctypes.data), vp(ctxs.ctypes.data),
                   vp(prm[i:i + 1].ctypes.data),
                   vp(o.ctypes.data + 2 * (bb * st + bb)), C.c_ssize_t(st),
                   vp(pred[c].ctypes.data), C.c_ssize_t(pred[c].strides[0] // 2),
                   vp(rec[c].ctypes.data), C.c_ssize_t(rec[c].strides[0] // 2),
                   vp(coeff.ctypes.data))
        levels.append(coeff[:int(t["w"]) * int(t["h"])].copy())
    cus = np.zeros(desc.n_cus_total, api.CU_DTYPE)
    for i, (b, (mx, my)) in enumerate(zip(desc.me, mvs)):
        c = cus[desc.cu_base + i]
        c["x"], c["y"], c["w"], c["h"] = b["x"], b["y"], b["w"], b["h"]
        c["cbf_luma"] = nnz[desc.luma_idx[i]] != 0
        c["qp_y"], c["qp_c"] = desc.qp, desc.qp_c
        c["ref_poc"] = (ref_poc, -1)
        c["mv"][0, :, 0], c["mv"][0, :, 1] = mx, my
    return rec, nnz, cus, levels


MIDDLE = ("fwd_from_me", "mc_from_me", "fwd_transform", "quant_rdo", "inv_transform", "cu_info")


def gpu_encode(api, ctx, fp, O, R, Rec, mvs):
    """The launches between the search and the tail, on the given motion results.  Returns
    (unfiltered reconstruction planes, nnz, cus, levels, level offsets)."""
    res = np.zeros(fp.desc.n_cus, api.MERES_DTYPE)
    res["mv_x"], res["mv_y"] = [m[0] for m in mvs], [m[1] for m in mvs]
    res["fullpel_x"], res["fullpel_y"] = res["mv_x"] >> 4, res["mv_y"] >> 4
    ctx.h2d(fp.d_res.ptr, res)
    ctx.h2d(fp.d_nnz.ptr, np.full(len(fp.desc.tx), 0x5a5a5a5a, np.int32))
    ctx.h2d(fp.d_levels.ptr, np.full(max(1, fp.n_levels), 0x5a5a, np.int16))
    names = []
    for name, fn in fp.kernel_steps(O, R, Rec):
        if name in MIDDLE:
            names.append(name)
            fn()
    ctx.sync()
    assert "me_search" not in names and "inv_transform" in names
    out = fp.scratch if fp.fused_tail else Rec
    _, nnz, cus, _ = fp.results()
    levels = fp.d_levels.to_array(np.int16, max(1, fp.n_levels))
    off = np.asarray(ctx.level_offsets(fp.desc.tx)[0], np.int64)
    return out.download(0), nnz, cus, levels, off


def check_against_oracle(got, exp, desc):
    g_rec, g_nnz, g_cus, g_levels, off = got
    e_rec, e_nnz, e_cus, e_levels = exp
    assert np.array_equal(g_nnz, e_nnz), np.nonzero(g_nnz != e_nnz)[0][:8]
    for i, lv in enumerate(e_levels):
        g = g_levels[off[i]:off[i] + len(lv)]
        if e_nnz[i]:
            assert np.array_equal(g, lv), (i, tuple(desc.tx[i]))
        else:       # cbf = 0: level buffer unspecified in the reference, zeros here
            assert not g.any(), (i, tuple(desc.tx[i]))
    assert g_cus.tobytes() == e_cus.tobytes()
    for c in range(3):
        assert np.array_equal(g_rec[c], e_rec[c]), c


def forced_pass(api, ctx, xo, w, h, bd, qp, orig, ref, mvs_of, partition=None,
                form="fwd_from_me", twice=False):
    """orig / ref: unpadded planes; mvs_of(n_cus) -> vectors.  Returns the oracle's nnz."""
    from xvc_amd import pipeline
    orig_host, ref_host = pad_planes(orig), pad_planes(ref)
    O, R, Rec = (ctx.picture(w, h, bd) for _ in range(3))
    O.upload(orig_host, BL)
    R.upload(ref_host, BL)
    fp = pipeline.FramePass(ctx, w, h, bd, qp=qp, rdoq=True, partition=partition)
    assert fp.form == form and fp.rdoq_packed
    mvs = mvs_of(fp.desc.n_cus)
    got = gpu_encode(api, ctx, fp, O, R, Rec, mvs)
    exp = oracle_encode(xo, fp.desc, bd, orig_host, ref_host, mvs)
    check_against_oracle(got, exp, fp.desc)
    if twice:
        again = gpu_encode(api, ctx, fp, O, R, Rec, mvs)
        for a, b in zip(got[:4], again[:4]):
            if isinstance(a, list):
                assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
            else:
                assert a.tobytes() == b.tobytes()
    fp.destroy()
    for p in (O, R, Rec):
        p.destroy()
    return exp[1]


W, H = 64, 40    # 16 grid: two rows of 16x16 CUs and a bottom row of 16x8


@pytest.mark.gpu
@pytest.mark.parametrize("bd", [10, 8, 12])
@pytest.mark.parametrize("shift", [0, 6, 12])
def test_filter_phases(gpu, xo, bd, shift):
    """Every branch of both interpolators (integer, horizontal, vertical, two-stage; chroma
    phases with an integer luma vector) and vectors ClipMv cuts at each picture edge, on
    16x16 and 16x8 CUs; shift moves every vector to another CU (and CU shape).  Twice: the
    same bytes."""
    api, ctx = gpu
    from xvc_amd import pipeline
    assert {(int(b["w"]), int(b["h"])) for b in pipeline.FrameDescriptors(W, H).me} == \
        {(16, 16), (16, 8)}
    nnz = forced_pass(api, ctx, xo, W, H, bd, 32, clip_planes(W, H, bd, 1),
                      clip_planes(W, H, bd, 0), lambda n: mvs_for(n, shift), twice=True)
    assert np.count_nonzero(nnz) > 0


def only_8x8(w, h):
    return [(x, y, 8, 8) for y in range(0, h, 8) for x in range(0, w, 8)]


def mixed_shapes(w, h):
    parts = []
    for y in range(0, h, 16):
        for x in range(0, w, 16):
            k = (x // 16 + y // 16) % 4
            if h - y < 16:
                parts.append((x, y, 16, 8) if k % 2 else (x, y, 8, 8))
                if not k % 2:
                    parts.append((x + 8, y, 8, 8))
            elif k == 0:
                parts.append((x, y, 16, 16))
            elif k == 1:
                parts += [(x, y, 8, 16), (x + 8, y, 8, 16)]
            elif k == 2:
                parts += [(x, y, 16, 8), (x, y + 8, 16, 8)]
            else:
                parts += [(x, y, 8, 8), (x + 8, y, 8, 8), (x, y + 8, 8, 8), (x + 8, y + 8, 8, 8)]
    return parts


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["8x8", "mixed"])
def test_shapes(gpu, xo, kind):
    """The same picture on an 8x8-only partition (luma 8x8, chroma 4x4 + 4x4) and on a mix
    of 16x16 / 8x8 / 16x8 / 8x16: the any-size paths of the same kernels."""
    api, ctx = gpu
    parts = only_8x8(W, H) if kind == "8x8" else mixed_shapes(W, H)
    if kind == "mixed":
        assert {(p[2], p[3]) for p in parts} == {(16, 16), (8, 8), (16, 8), (8, 16)}
    nnz = forced_pass(api, ctx, xo, W, H, 10, 32, clip_planes(W, H, 10, 1),
                      clip_planes(W, H, 10, 0), lambda n: mvs_for(n, 3), partition=parts)
    assert np.count_nonzero(nnz) > 0


@pytest.mark.gpu
def test_cu_above_16_takes_the_any_size_form(gpu, xo):
    """A 48x48 picture with one 32x32 CU: the pass is the fwd_transform form (prediction
    picture, residual_wave_kernel / residual_kernel) and equals the oracle's frame pass,
    search included."""
    import oracle_frame
    from xvc_amd import pipeline
    api, ctx = gpu
    w = h = 48
    bd, qp = 10, 32
    parts = [(0, 0, 32, 32), (32, 0, 16, 16), (32, 16, 16, 16), (0, 32, 16, 16), (16, 32, 16, 16),
             (32, 32, 16, 16)]
    orig_host, ref_host = pad_planes(clip_planes(w, h, bd, 1)), pad_planes(clip_planes(w, h, bd, 0))
    O, R, Rec = (ctx.picture(w, h, bd) for _ in range(3))
    O.upload(orig_host, BL)
    R.upload(ref_host, BL)
    fp = pipeline.FramePass(ctx, w, h, bd, qp=qp, rdoq=True, partition=parts)
    assert fp.form == "fwd_transform"
    fp.run(O, R, Rec)
    ctx.sync()
    res, nnz, cus, ssd = fp.results()
    e_rec, e_res, e_nnz, e_cus, e_ssd = oracle_frame.frame_pass(fp.desc, bd, orig_host, ref_host,
                                                                BL, lib=xo)
    assert np.array_equal(res, e_res) and np.array_equal(nnz, e_nnz)
    assert cus.tobytes() == e_cus.tobytes() and (int(ssd[0]), int(ssd[1])) == e_ssd
    got = Rec.download(BL)
    for c in range(3):
        assert np.array_equal(got[c], e_rec[c]), c
    assert np.count_nonzero(nnz) > 0
    fp.destroy()
    for p in (O, R, Rec):
        p.destroy()


def early_exit_inputs(kind, w, h, bd=10):
    """(qp, orig, ref) of the inverse's three cases; the vectors are zero."""
    ref = noise_planes(w, h, bd, 1)
    if kind == "all_zero":       # the picture is its reference: no residual at all
        return 51, [p.copy() for p in ref], ref
    noise = noise_planes(w, h, bd, 2)
    if kind == "all_coded":
        return 0, noise, ref
    orig = [p.copy() for p in ref]
    for c in range(3):
        orig[c][:, orig[c].shape[1] // 2:] = noise[c][:, orig[c].shape[1] // 2:]
    return 32, orig, ref


EW, EH = 96, 40   # six CUs a row: the picture's middle falls inside a workgroup's CU pair


@pytest.mark.parametrize("kind", ["all_zero", "all_coded", "halves"])
def test_early_exit_inputs_are_what_they_say(xo, kind):
    """CPU only: the oracle alone on the inverse's cases - none vacuous."""
    from xvc_amd import pipeline
    qp, orig, ref = early_exit_inputs(kind, EW, EH)
    desc = pipeline.FrameDescriptors(EW, EH, qp, rdoq=True, bitdepth=10)
    nnz = oracle_encode(xo, desc, 10, pad_planes(orig), pad_planes(ref),
                        [(0, 0)] * desc.n_cus)[1]
    _check_early_exit_counts(kind, desc, nnz)



def _check_early_exit_counts(kind, desc, nnz):
    if kind == "all_zero":
        assert not nnz.any()
    elif kind == "all_coded":
        assert (nnz != 0).all()
    else:
        left = np.repeat(desc.me["x"] < EW // 2, 3)
        assert not nnz[left].any() and (nnz[~left] != 0).all()
        # CUs 2 (left) and 3 (right) of a row share a workgroup of four waves
        assert left[3 * 2] and not left[3 * 3]


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["all_zero", "all_coded", "halves"])
def test_inverse_early_exit(gpu, xo, kind):
    """Nothing coded (the reconstruction is the prediction), everything coded, and coded and
    skipped blocks side by side in the same workgroups."""
    api, ctx = gpu
    qp, orig, ref = early_exit_inputs(kind, EW, EH)
    nnz = forced_pass(api, ctx, xo, EW, EH, 10, qp, orig, ref, lambda n: [(0, 0)] * n)
    from xvc_amd import pipeline
    _check_early_exit_counts(kind, pipeline.FrameDescriptors(EW, EH, qp, rdoq=True), nnz)
