"""Every case of the transform block's quantiser constants (csrc/k_quant.h),
enumerated instead of drawn: every (w, h) with both sides in {64, 32, 16, 8, 4}
(luma) or {32, 16, 8, 4, 2} (chroma) - so both parities of the log-size sum at every
size class, and both block paths: one wave up to 16x16, the workgroup path above
that and for 2-wide blocks - at every qp % 6 for two values of qp / 6, at bit depths
8, 10 and 12, each compared bit-exactly with the oracle through every entry point
that reads the constants:

  QuantFast  residual_batch; fwd_transform_batch + inv_transform_batch;
             inv_transform_dist_batch
  RDOQ       residual_rdoq_batch (the walks inside the forward kernels);
             fwd_transform_batch + quant_rdo_batch with the all-zero proof off and
             on (the classify kernel, the proof, the packed walks)

The 25 blocks of a component are the outer product of the sizes in descending order,
so every block is aligned to its own size and all of them fit one batch per QP.  The
prediction is mid-grey; input (a) is pred +- AMP << (bd - 8) with a random sign per
sample, input (b) a flat residual of 40 << (bd - 8), whose only level is the DC
(the DC-only inverse).  So that no cell passes vacuously the oracle alone must code
every cell of (a), find exactly one level in every cell of (b), and with RDOQ code
every (w, h) at one QP of the twelve at least.
"""
import contextlib

import numpy as np
import pytest

import oracle_lib as ol
import oracle_rdoq as oq
import test_gpu_rdoq as tr

pytestmark = pytest.mark.gpu

PW = PH = 128
BL = 128                       # device border (luma)
QPS = list(range(20, 26)) + list(range(38, 44))
AMP = 100                      # input (a), at 8 bits
FLAT = 40                      # input (b), at 8 bits


@pytest.fixture(scope="module")
def gpu():
    from xvc_amd import api
    ctx = api.Context(0)
    yield api, ctx
    ctx.close()


@pytest.fixture(scope="module")
def xo():
    return ol.Lib("xo")


def grid_blocks(qp, flags=0):
    """The 25 luma and 25 chroma (U) blocks of one QP."""
    out = []
    for comp, sizes in ((0, (64, 32, 16, 8, 4)), (1, (32, 16, 8, 4, 2))):
        offs = np.r_[0, np.cumsum(sizes)[:-1]]
        for y, h in zip(offs, sizes):
            for x, w in zip(offs, sizes):
                out.append((x, y, w, h, comp, 0, 0, 0, qp, flags))
    return np.array(out, ol.TX_DTYPE)


def planes(bd, kind, rng):
    """orig, pred: [Y, U, V] padded by the device border."""
    pad = lambda p, c: np.ascontiguousarray(np.pad(p, BL >> (1 if c else 0), mode="edge"))
    orig, pred = [], []
    for c in range(3):
        shape = (PH >> (1 if c else 0), PW >> (1 if c else 0))
        p = np.full(shape, 1 << (bd - 1), np.int64)
        if kind == "a":
            o = p + (rng.integers(0, 2, shape) * 2 - 1) * (AMP << (bd - 8))
        else:
            o = p + (FLAT << (bd - 8))
        orig.append(pad(o.astype(np.uint16), c))
        pred.append(pad(p.astype(np.uint16), c))
    return orig, pred


def inner(padded, comp):
    b = BL >> (1 if comp else 0)
    return np.ascontiguousarray(padded[comp][b:-b, b:-b])


def tx_struct(b):
    s = ol.TxBlock()
    for name in ol.TX_DTYPE.names:
        setattr(s, name, int(b[name]))
    return s


def oracle_fast(xo, bd, orig, pred, blocks):
    """The oracle's TransformAndReconstruct with QuantFast: the reconstruction of the
    three planes and per block (count, levels)."""
    exp = [inner(pred, c).copy() for c in range(3)]
    out = []
    for b in blocks:
        c = int(b["comp"])
        rec, coeff, n = xo.residual_pipeline(bd, tx_struct(b), inner(orig, c), inner(pred, c))
        x, y, w, h = int(b["x"]), int(b["y"]), int(b["w"]), int(b["h"])
        exp[c][y:y + h, x:x + w] = rec[y:y + h, x:x + w]
        out.append((n, coeff.reshape(-1)))
    return exp, out


def rdoq_params(api, bd, blocks):
    """lambda and rd_factor of the block's QP as test_gpu_rdoq.rdoq_pipeline_inputs
    forms them; inter CUs, one context snapshot."""
    params = np.zeros(len(blocks), api.RDOQ_PARAMS_DTYPE)
    for i, b in enumerate(blocks):
        qp = int(b["qp"])
        lam = 0.57 * 2.0 ** ((qp - 12) / 3.0)
        qpb = qp + 6 * (bd - 8)
        inv_scale = [40, 45, 51, 57, 64, 72][qpb % 6] << (qpb // 6)
        params[i]["lambda"] = int(lam * 65536 + 0.5)
        params[i]["rd_factor"] = int(inv_scale * inv_scale / lam / 16 / (1 << (2 * (bd - 8))) + 0.5)
    return params


def oracle_rdoq(bd, orig, pred, blocks, params, ctxs):
    """The same with QuantRdo: test_gpu_rdoq.rdoq_pipeline_oracle, its blocks laid over the
    prediction (the grid leaves a rim of the picture uncovered)."""
    rec, out = tr.rdoq_pipeline_oracle(bd, PW, PH, orig, pred, blocks, params, ctxs)
    exp = [inner(pred, c).copy() for c in range(3)]
    for b in blocks:
        c, x, y, w, h = (int(b[k]) for k in ("comp", "x", "y", "w", "h"))
        exp[c][y:y + h, x:x + w] = rec[c][y:y + h, x:x + w]
    return exp, out


@contextlib.contextmanager
def pictures(ctx, bd):
    pics = [ctx.picture(PW, PH, bd) for _ in range(3)]
    try:
        yield pics
    finally:
        for pic in pics:
            pic.destroy()


def check_levels(levels, off, nnz, blocks, records, tag):
    for i, (b, (e_n, e_lv)) in enumerate(zip(blocks, records)):
        n = int(b["w"]) * int(b["h"])
        got = levels[off[i]:off[i] + n]
        assert int(nnz[i]) == e_n, (tag, tuple(b), int(nnz[i]), e_n)
        # cbf = 0: the reference never reads the level buffer; the device writes zeros
        assert np.array_equal(got, e_lv) if e_n else not got.any(), (tag, tuple(b))


def check_rec(R, exp, tag):
    got = R.download(0)
    assert all(np.array_equal(got[c], exp[c]) for c in range(3)), tag


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_quant_fast_cases(gpu, xo, bd):
    api, ctx = gpu
    rng = np.random.default_rng(7100 + bd)
    with pictures(ctx, bd) as (O, P, R):
        for kind in "ab":
            orig, pred = planes(bd, kind, rng)
            O.upload(orig, BL)
            P.upload(pred, BL)
            for qp in QPS:
                blocks = grid_blocks(qp)
                exp, records = oracle_fast(xo, bd, orig, pred, blocks)
                counts = np.array([n for n, _ in records])
                assert (counts > 0).all() if kind == "a" else (counts == 1).all(), (kind, qp, counts)
                R.upload(pred, BL)
                levels, off, nnz = ctx.residual_batch(O, P, R, blocks)
                check_levels(levels, off, nnz, blocks, records, (kind, qp))
                check_rec(R, exp, (kind, qp, "residual"))
                # the split path: forward alone against the oracle's forward transform ...
                coeffs, off2 = ctx.fwd_transform_batch(O, P, blocks)
                for i, b in enumerate(blocks):
                    c, x, y, w, h = (int(b[k]) for k in ("comp", "x", "y", "w", "h"))
                    resi = (inner(orig, c)[y:y + h, x:x + w].astype(np.int32) -
                            inner(pred, c)[y:y + h, x:x + w].astype(np.int32)).astype(np.int16)
                    want = xo.fwd_transform(bd, np.ascontiguousarray(resi))
                    assert np.array_equal(coeffs[off2[i]:off2[i] + w * h].reshape(h, w), want), \
                        (kind, qp, "forward", tuple(b))
                # ... then the two inverse entry points on the quantiser's levels
                R.upload(pred, BL)
                ctx.inv_transform_batch(P, R, blocks, levels, off, nnz)
                check_rec(R, exp, (kind, qp, "inverse"))
                R.upload(pred, BL)
                ctx.inv_transform_dist_batch(O, P, R, blocks, levels, off, nnz)
                check_rec(R, exp, (kind, qp, "inverse+dist"))


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_quant_rdoq_cases(gpu, bd):
    api, ctx = gpu
    rng = np.random.default_rng(7200 + bd)
    ctxs = oq.random_contexts(rng).view(api.RDOQ_CTX_DTYPE)
    orig, pred = planes(bd, "a", rng)
    coded = np.zeros(50, bool)
    with pictures(ctx, bd) as (O, P, R):
        O.upload(orig, BL)
        P.upload(pred, BL)
        try:
            for qp in QPS:
                blocks = grid_blocks(qp, api.TXF_RDOQ)
                params = rdoq_params(api, bd, blocks)
                exp, records = oracle_rdoq(bd, orig, pred, blocks, params, ctxs)
                coded |= np.array([n > 0 for n, _ in records])
                R.upload(pred, BL)
                levels, off, nnz = ctx.residual_rdoq_batch(O, P, R, blocks, ctxs, params)
                check_levels(levels, off, nnz, blocks, records, (qp, "residual_rdoq"))
                check_rec(R, exp, (qp, "residual_rdoq"))
                coeffs, off2 = ctx.fwd_transform_batch(O, P, blocks)
                for mode in (0, 1):
                    ctx.set_rdoq_prove_zero(mode)
                    lv, n2 = ctx.quant_rdo_batch(bd, blocks, coeffs, off2, ctxs, params)
                    check_levels(lv, off2, n2, blocks, records, (qp, "quant_rdo", mode))
        finally:
            ctx.set_rdoq_prove_zero(-1)
    assert coded.all(), [tuple(b)[2:5] for b in grid_blocks(0)[~coded]]
