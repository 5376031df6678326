"""The four-lane RDOQ walk (wave_rdoq4, k_rdoq4.h) on sparse blocks: planted coefficients.

Step 1 of the walk visits only the anti-diagonals of a sub-block on which a coefficient has
a choice, decides a trip whose candidates all quantise to 1 with the one-against-zero form,
and carries the greater-1 / greater-2 budget and the count of levels through the quad as
three packed counts.  The blocks here put coefficients where that can go wrong - 16x16 luma
(a block per wave) and 8x8 chroma (four blocks per wave) at 8 and 10 bits through
xvcgpu_quant_rdo_batch, levels and counts byte for byte against the oracle (oracle_rdoq.py):

  - one candidate: at DC, at scan offset 15 of sub-block 0, at the DC of sub-block 1 (its
    significance flag is inferred);
  - two candidates on one anti-diagonal of a sub-block, in different rows; three on
    consecutive anti-diagonals, each inside the others' templates;
  - q = 1, 2 and 3, and the magnitudes just under and just at the level-2 threshold;
  - a sub-block full of ones - the ninth falls inside an anti-diagonal, so a lane decides
    again with the greater-1 budget spent -, the same with twos among them (the general
    form decides again), and two levels >= 2 on one anti-diagonal (greater-2 budget);
  - the last position in sub-block 0, in the second and in the last sub-block of the scan;
  - a lambda above 2^32 (64-bit prices);
  - four 8x8 blocks of one wave whose numbers of occupied anti-diagonals differ.

test_planted_cases_on_the_cpu needs no GPU: the python model (rdoq_model.py) agrees with the
oracle on every block and its census shows that the cases reach the decisions they are for.
"""
import collections
import functools

import numpy as np
import pytest

import oracle_lib as ol
import oracle_rdoq as oq
import rdoq_cases as rc
import rdoq_model as rm
import test_rdoq_model as tm

DEPTHS = (8, 10)
SHAPES = ((16, 16, 0), (8, 8, 1))      # (w, h, component)
QP_LUMA = {8: 30, 10: 32}
# scan offset -> (x, y) inside a sub-block (diagonal scan); anti-diagonal x + y
SB = [(c & 3, c >> 2) for c in rm.SCAN4[0]]
DIAG3 = [k for k in range(16) if sum(SB[k]) == 3]       # four offsets, four rows


def level2_threshold(k):
    """The smallest magnitude that quantises to 2."""
    a = 1
    while rm.plain_level(k, a) < 2:
        a += 1
    return a


def plants(w, h, k):
    """name -> {scan index: level in quantiser steps, or ("raw", coefficient)}."""
    n_sb = (w >> 2) * (h >> 2)
    last_sb = 16 * (n_sb - 1)
    a2 = level2_threshold(k)
    ones = {i: (1.45 if i % 3 else -1.45) for i in range(16)}
    p = collections.OrderedDict()
    p["dc"] = {0: 1.3}
    p["offset15"] = {15: -1.4}
    p["dc_of_sb1"] = {16: 1.4}
    p["dc_of_sb1_under_sb2"] = {16: 1.4, 32 + 2: -2.3}
    p["two_on_a_diagonal"] = {DIAG3[0]: 1.3, DIAG3[2]: -1.6}
    p["four_on_a_diagonal"] = {i: 1.35 + 0.1 * n for n, i in enumerate(DIAG3)}
    # (1, 1), (2, 1), (2, 2): anti-diagonals 2, 3, 4, each a neighbour of the others
    p["three_consecutive"] = {SB.index((1, 1)): 1.3, SB.index((2, 1)): -1.45, SB.index((2, 2)): 1.6}
    p["three_consecutive_sb1"] = {16 + SB.index((1, 1)): 2.3, 16 + SB.index((2, 1)): 1.45,
                                  16 + SB.index((2, 2)): -1.3, 0: 3.2}
    p["ones_that_go_to_zero"] = {0: 2.2, 3: 0.6, 5: -0.55, 9: 0.7, 16 + 4: 0.6}
    p["one_weak_one"] = {5: 0.6}
    p["one_weak_one_far"] = {last_sb + 9: -0.7}
    p["q123"] = {0: 3.1, 1: -2.2, 2: 1.2, 4: 1.0, 5: -2.0, 7: 3.0}
    p["level2_threshold"] = {1: ("raw", a2 - 1), 2: ("raw", -a2), 4: ("raw", a2), 8: ("raw", 1 - a2),
                             0: 2.6}
    p["ones_fill_a_sub_block"] = dict(ones)
    p["ones_fill_sb1"] = {16 + i: v for i, v in ones.items()}
    p["ones_and_twos"] = {**ones, 12: 2.4, 11: -2.45, 7: 2.3}
    p["two_twos_on_a_diagonal"] = {14: 2.4, 13: -2.45, 12: 1.3, 0: 1.2}
    p["twos_then_ones"] = {15: 2.4, 14: 1.4, 13: 2.4, 11: -1.4, 10: 2.45, 5: 1.4, 4: -1.45}
    p["last_in_sb0"] = {11: 1.4, 3: -1.2, 0: 2.2}
    p["last_in_second_sb"] = {16 + 6: 1.45, 16: -1.2, 5: 1.3, 0: 2.2}
    p["last_in_last_sb"] = {last_sb + 3: 1.45, last_sb: 1.3, 16 + 9: -1.4, 2: 1.3, 0: -4.3}
    p["every_sb_one_candidate"] = {16 * s + (5 * s) % 16: (1.4 if s & 1 else -1.45)
                                   for s in range(n_sb)}
    p["strong"] = {i: (9.3 - 0.5 * i if i & 1 else 0.4 * i - 8.2) for i in range(0, 24)}
    return p


def make_block(bd, w, h, comp, name, plant, lam_fix=None, mult=0.25, ctx=6, sign_hide=1, qp_luma=None):
    from xvc_amd import pipeline
    qp_luma = QP_LUMA[bd] if qp_luma is None else qp_luma
    qp = qp_luma if comp == 0 else pipeline.chroma_qp(qp_luma)
    k = rm.quant_constants(bd, qp, w, h)
    step = float(1 << k["fq_shift"]) / k["scale"]
    P = rm.scan_positions(w, h, 0)
    src = np.zeros((h, w), np.int16)
    for i, lvl in plant.items():
        x, y = P[i]
        src[y, x] = lvl[1] if isinstance(lvl, tuple) else int(np.clip(np.rint(lvl * step), -32767, 32767))
    lam = 0.57 * 2.0 ** ((qp_luma - 12) / 3.0) * mult if lam_fix is None else lam_fix / 65536.0
    fix, rdf = pipeline.rdoq_host_params(qp_luma, bd, lam)[comp]
    if lam_fix is not None:
        fix = lam_fix
    return dict(bd=bd, i=name, qp_luma=qp_luma, lam=lam, comp=comp, qp=qp, luma=comp == 0, scan=0,
                sign_hide=sign_hide, flags=0, w=w, h=h, src=src, ctx=ctx, lam_fix=fix,
                rd_factor=rdf, kind=name, v=0)


@functools.lru_cache(maxsize=None)
def blocks_of(bd):
    """The depth's blocks.  The 8x8 blocks of one key stand together, a multiple of four of
    them: a wave's four groups walk blocks whose trips differ.  (That holds as long as the
    class lists keep the batch's order, which rdoq_lists_kernel's compaction does and
    tests/test_gpu_rdoq_lists.py checks; nothing here asserts it.  Were the order another,
    the four groups of a wave would still hold blocks of different trips - consecutive
    plants differ - only not these four.)  The walk with four units per lane (more than
    sixteen sub-blocks) keeps the exchange it had and is left to tests/test_gpu_rdoq_cases.py,
    whose 32x16 ... 64x64 cases walk it on both packed kernels."""
    from xvc_amd import pipeline
    out = []
    for w, h, comp in SHAPES:
        qp = QP_LUMA[bd] if comp == 0 else pipeline.chroma_qp(QP_LUMA[bd])
        k = rm.quant_constants(bd, qp, w, h)
        group = []
        for n, (name, plant) in enumerate(plants(w, h, k).items()):
            group.append(make_block(bd, w, h, comp, name, plant, mult=1.0))
            group.append(make_block(bd, w, h, comp, name + "/quarter", plant, ctx=8))
            # a weaker lambda keeps more of the ones; without sign hiding; another snapshot
            group.append(make_block(bd, w, h, comp, name + "/weak", plant, mult=0.05,
                                    sign_hide=n & 1, ctx=7))
        while len(group) % 4:
            group.append(make_block(bd, w, h, comp, "dc/fill", {0: 1.3}))
        out += group
        # 64-bit prices: coefficients up to the int16 limit at the highest QP against a lambda
        # above 2^32
        big = {0: 17.4, 1: -9.4, 2: 5.45, 4: 3.3, 5: -4.6, 16: -6.3, 17: 2.4, 19: 7.5, 33: 1.45}
        for lam_fix in ((1 << 32) + 12345, (5 << 32) + 1, (1 << 32) - 1):
            for _ in range(4):
                out.append(make_block(bd, w, h, comp, "lambda_%x" % lam_fix, big, lam_fix=lam_fix,
                                      qp_luma=51))
    return out


@functools.lru_cache(maxsize=None)
def oracle_of(bd):
    xo, snaps = ol.Lib("xo"), rc.snapshots(bd)
    out = []
    for cs in blocks_of(bd):
        nnz, lv = oq.quant_rdo_oracle(xo, bd, cs["qp"], cs["comp"], 0, cs["sign_hide"],
                                      snaps[cs["ctx"]:cs["ctx"] + 1], tm.case_params(cs), cs["src"])
        out.append((nnz, lv if nnz else np.zeros_like(lv)))
    return out


@pytest.mark.parametrize("bd", DEPTHS)
def test_planted_cases_on_the_cpu(bd):
    """The model equals the oracle, and the blocks go where they were sent."""
    snaps = rc.snapshots(bd)
    by_name = {}
    for cs, (e_nnz, e_lv) in zip(blocks_of(bd), oracle_of(bd)):
        n = collections.Counter()
        nnz, lv = rm.quant_rdo(tm.entropy(), bd, cs["qp"], cs["luma"], 0, cs["sign_hide"], 0,
                               cs["w"], cs["h"], cs["src"].tolist(), tm.ctx_dict(snaps[cs["ctx"]]),
                               cs["lam_fix"], cs["rd_factor"], n)
        assert nnz == e_nnz and np.array_equal(np.array(lv, np.int16) if nnz else 0 * e_lv, e_lv), \
            (bd, cs["i"], cs["w"])
        by_name[(cs["w"], cs["i"])] = (n, e_nnz, e_lv, cs)
    for w, _, _ in SHAPES:
        def n_of(name):
            return by_name[(w, name)][0]
        k = rm.quant_constants(bd, by_name[(w, "dc")][3]["qp"], w, w)
        # every candidate quantises to what its name says
        src = by_name[(w, "level2_threshold")][3]["src"]
        assert sorted(rm.plain_level(k, int(v)) for v in src.reshape(-1) if v) == [1, 1, 2, 2, 3]
        src = by_name[(w, "ones_fill_a_sub_block")][3]["src"]
        assert [rm.plain_level(k, int(v)) for v in src[:4, :4].reshape(-1)] == [1] * 16
        # the budgets run out where a lane has to decide again
        assert n_of("ones_fill_a_sub_block/weak")["g1_budget_spent"] >= 1
        assert n_of("ones_fill_sb1/weak")["g1_budget_spent"] >= 1
        assert n_of("ones_and_twos/weak")["g1_budget_spent"] >= 1
        assert n_of("ones_and_twos/weak")["g2_budget_spent"] >= 1
        assert n_of("two_twos_on_a_diagonal/weak")["g2_budget_spent"] >= 1
        assert n_of("dc_of_sb1/weak")["sig_inferred"] + n_of("dc_of_sb1_under_sb2/weak")["sig_inferred"] >= 1
        seen = collections.Counter()
        for (bw, _), (n, _, _, _) in by_name.items():
            if bw == w:
                seen.update(k_ for k_ in n if n[k_])
        for key in ("q1_to_0", "q1_to_1", "q2_to_1", "q2_to_2", "q3up_kept", "sb_empty", "sb_kept",
                    "last_moved", "last_stays", "block_zeroed"):
            assert seen[key], (bd, w, key)
        # the last position stays where it was planted
        for name, sb in (("last_in_sb0/weak", 0), ("last_in_second_sb/weak", 1),
                         ("last_in_last_sb/weak", (w >> 2) ** 2 - 1)):
            lv = by_name[(w, name)][2]
            P = rm.scan_positions(w, w, 0)
            last = max(i for i, (x, y) in enumerate(P) if lv[y, x])
            assert last >> 4 == sb, (bd, w, name, last)
        # the large lambdas leave levels to decide, and the high half of the lambda decides
        a = by_name[(w, "lambda_%x" % ((1 << 32) + 12345))]
        b = by_name[(w, "lambda_%x" % ((5 << 32) + 1))]
        assert a[1] > 0 and not np.array_equal(a[2], b[2])


@pytest.fixture(scope="module")
def gpu():
    from xvc_amd import api
    ctx = api.Context(0)
    yield api, ctx
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("prove_zero", [0, -1])
@pytest.mark.parametrize("misaligned", [False, True])
@pytest.mark.parametrize("bd", DEPTHS)
def test_sparse_walk(gpu, bd, misaligned, prove_zero):
    import test_gpu_rdoq_cases as tg
    api, ctx = gpu
    items = [(cs, e_nnz, e_lv, None) for cs, (e_nnz, e_lv) in zip(blocks_of(bd), oracle_of(bd))]
    blocks, coeffs, off, params = tg.build_batch(api, items, misaligned)
    ctx.set_rdoq_prove_zero(prove_zero)
    try:
        levels, nnz = ctx.quant_rdo_batch(bd, blocks, coeffs, off, rc.snapshots(bd), params)
        got = tg.class_counts(ctx)
    finally:
        ctx.set_rdoq_prove_zero(-1)
    for k, (cs, e_nnz, e_lv, _) in enumerate(items):
        lv = levels[off[k]:off[k] + cs["w"] * cs["h"]].reshape(cs["h"], cs["w"])
        assert nnz[k] == e_nnz and np.array_equal(lv, e_lv), (bd, cs["w"], cs["i"], misaligned)
    n16 = sum(1 for it in items if it[0]["w"] == 16)
    if prove_zero == 0:     # every block is walked: a block per wave, and four per wave
        assert got == [len(items) - n16, n16, 0]
    else:
        assert got[0] <= len(items) - n16 and got[1] <= n16 and got[2] == 0
