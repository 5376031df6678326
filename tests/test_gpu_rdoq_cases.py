"""The RDO quantiser's directed cases on the device: every walk instance, bit exact.

The cases of tests/rdoq_cases.py (their census: tests/test_rdoq_model.py, counted on the CPU)
  - through xvcgpu_quant_rdo_batch - the packed kernels - with the all-zero proof forced off
    and on, every block at a 16-byte aligned coefficient offset and at one 8 bytes off it,
    four equal blocks side by side (a wave's groups share one key: one round) and the cases in
    their own order (a wave's groups differ: several rounds, class counts of any remainder);
    levels and counts equal the oracle's, and xvcgpu_quant_rdo_class_counts equals what
    rdoq_model.device_walk and the plain quantiser predict;
  - the class-1 cases once more in a list longer than RDOQ4_LATENCY_BLOCKS, which the packed
    kernel walks with a lane per sub-block (wave_rdoq<16>);
  - through xvcgpu_residual_rdoq_batch - the one-wave forward kernels and the workgroup
    kernel, and both as the one launch of a batch of at most 64 blocks - on one picture pair
    per depth: levels, counts and reconstruction equal xo_residual_pipeline_rdoq.
"""
import ctypes as C
import functools
import time

import numpy as np
import pytest

import rdoq_cases as rc
import rdoq_model as rm
import test_rdoq_model as tm

pytestmark = pytest.mark.gpu
BORDER = 128


@pytest.fixture(scope="module")
def gpu():
    from xvc_amd import api
    ctx = api.Context(0)
    yield api, ctx
    ctx.close()


@functools.lru_cache(maxsize=None)
def taken(bd):
    """The depth's cases xvcgpu_quant_rdo_batch takes, with the oracle's result and the class
    list each lands on (None: no coefficient quantises to a level, it is never listed)."""
    out = []
    for cs, (e_nnz, e_lv) in zip(rc.cases(bd), tm.oracle_results(bd)):
        if rm.device_walk("packed", cs["w"], cs["h"], cs["scan"], cs["flags"]) is None:
            continue
        cls = rm.rq_class_of(cs["w"], cs["h"], cs["scan"]) if min(cs["w"], cs["h"]) > 2 else 2
        out.append((cs, e_nnz, e_lv, cls if rm.any_level(bd, cs["qp"], cs["w"], cs["h"], cs["src"])
                    else None))
    return out


def build_batch(api, items, misaligned):
    """Blocks, coefficients, offsets and parameters of a list of taken() items; every block
    starts on 16 bytes, or 8 bytes behind that."""
    n = len(items)
    blocks = np.zeros(n, api.TX_DTYPE)
    params = np.zeros(n, api.RDOQ_PARAMS_DTYPE)
    off = np.zeros(n, np.uint32)
    pos = 0
    for k, (cs, _, _, _) in enumerate(items):
        blocks[k] = (0, 0, cs["w"], cs["h"], cs["comp"], 0, 0, 0, cs["qp"],
                     api.TXF_RDOQ | (0 if cs["sign_hide"] else api.TXF_NO_SIGN_HIDING) |
                     (cs["scan"] << api.TXF_SCAN_SHIFT))
        params[k]["lambda"], params[k]["rd_factor"] = cs["lam_fix"], cs["rd_factor"]
        params[k]["ctx_index"], params[k]["flags"] = cs["ctx"], cs["flags"]
        off[k] = (pos + 7) // 8 * 8 + (4 if misaligned else 0)
        pos = int(off[k]) + cs["w"] * cs["h"]
    coeffs = np.zeros(pos, np.int16)
    for k, (cs, _, _, _) in enumerate(items):
        coeffs[off[k]:off[k] + cs["w"] * cs["h"]] = cs["src"].reshape(-1)
    return blocks, coeffs, off, params


def check_levels(items, off, levels, nnz, what):
    for k, (cs, e_nnz, e_lv, _) in enumerate(items):
        got = levels[off[k]:off[k] + cs["w"] * cs["h"]].reshape(cs["h"], cs["w"])
        assert nnz[k] == e_nnz and np.array_equal(got, e_lv), (what, k, tm.describe(cs, {}))


def class_counts(ctx):
    cc = (C.c_int32 * 3)()
    ctx._check(ctx.lib.xvcgpu_quant_rdo_class_counts(ctx.h, cc))
    return list(cc)


@pytest.mark.parametrize("order", ["run", "interleaved"])
@pytest.mark.parametrize("misaligned", [False, True])
@pytest.mark.parametrize("prove_zero", [0, 1])
@pytest.mark.parametrize("bd", rc.DEPTHS)
def test_packed_entry(gpu, bd, prove_zero, misaligned, order):
    api, ctx = gpu
    items = taken(bd)
    if order == "run":
        items = [it for it in items for _ in range(4)]
    blocks, coeffs, off, params = build_batch(api, items, misaligned)
    t0 = time.perf_counter()
    ctx.set_rdoq_prove_zero(prove_zero)
    try:
        levels, nnz = ctx.quant_rdo_batch(bd, blocks, coeffs, off, rc.snapshots(bd), params)
        got = class_counts(ctx)
    finally:
        ctx.set_rdoq_prove_zero(-1)
    print("%d blocks, class lists %s, %.3f s" % (len(items), got, time.perf_counter() - t0))
    check_levels(items, off, levels, nnz, (bd, prove_zero, misaligned, order))
    listed = [sum(1 for it in items if it[3] == c) for c in range(3)]
    coded = [sum(1 for it in items if it[3] == c and it[1]) for c in range(3)]
    if prove_zero:      # the proof takes blocks off the lists, never one that codes a level
        assert all(c <= g <= l for c, g, l in zip(coded, got, listed)), (coded, got, listed)
    else:
        assert got == listed
    if order == "interleaved":      # a last wave with idle groups
        assert listed[0] % 4 and min(listed) > 100


@pytest.mark.parametrize("bd", rc.DEPTHS)
def test_packed_long_list(gpu, bd):
    """More class-1 blocks than RDOQ4_LATENCY_BLOCKS: quant_rdo_packed_wave<16, 16, false>, a
    lane per sub-block and four blocks a wave, the 16x16 arm and the any-size one."""
    api, ctx = gpu
    pool = [it for it in taken(bd) if it[3] == 1]
    assert {(it[0]["w"], it[0]["h"]) for it in pool} >= {(16, 16), (16, 8), (8, 32), (32, 4)}
    items = [pool[k % len(pool)] for k in range(rm.LATENCY_BLOCKS + 7)]
    blocks, coeffs, off, params = build_batch(api, items, False)
    ctx.set_rdoq_prove_zero(0)
    try:
        levels, nnz = ctx.quant_rdo_batch(bd, blocks, coeffs, off, rc.snapshots(bd), params)
        got = class_counts(ctx)
    finally:
        ctx.set_rdoq_prove_zero(-1)
    assert got == [0, len(items), 0] and got[1] > rm.LATENCY_BLOCKS
    check_levels(items, off, levels, nnz, (bd, "long list"))


@pytest.mark.parametrize("n_blocks", [None, 64])
@pytest.mark.parametrize("bd", rc.DEPTHS)
def test_residual_entry(gpu, bd, n_blocks):
    """The depth's picture: all of its blocks (the one-wave kernel and the workgroup kernel, one
    launch each), and its first 64 alone - the large luma shapes and the first small ones -,
    which the entry runs as one launch of a workgroup per block (residual_cu_kernel)."""
    api, ctx = gpu
    orig, pred, blocks, params, snaps = rc.residual_picture(bd)
    e_rec, records = tm.residual_oracle(bd)
    blocks, params, records = blocks[:n_blocks], params[:n_blocks], records[:n_blocks]
    pad = lambda planes: [np.ascontiguousarray(np.pad(p, BORDER >> (1 if c else 0), mode="edge"))
                          for c, p in enumerate(planes)]
    O, P, R = (ctx.picture(128, 128, bd) for _ in range(3))
    try:
        O.upload(pad(orig), BORDER)
        P.upload(pad(pred), BORDER)
        levels, off, nnz = ctx.residual_rdoq_batch(O, P, R, blocks, snaps, params)
        got = R.download(0)
    finally:
        for p in (O, P, R):
            p.destroy()
    walks = [m[0] for m in tm.residual_modelled(bd)]
    assert len(set(walks[:len(blocks)])) >= 3
    for i, (b, (e_nnz, e_lv)) in enumerate(zip(blocks, records)):
        x, y, w, h, c = (int(b[k]) for k in ("x", "y", "w", "h", "comp"))
        assert nnz[i] == e_nnz and np.array_equal(levels[off[i]:off[i] + w * h], e_lv), \
            (bd, i, tuple(b), walks[i])
        assert np.array_equal(got[c][y:y + h, x:x + w], e_rec[c][y:y + h, x:x + w]), \
            (bd, i, tuple(b), walks[i])
