"""The RDO quantiser's directed cases.  TEST INFRASTRUCTURE.

cases(depth): blocks of coefficients for xvcgpu_quant_rdo_batch, enumerated - shape x scan x
construction, the QP, lambda multiplier, component and context snapshot rotating with the
case's number; nothing is drawn at test time (the few generators below are seeded with the
case's own number).  Each construction (KINDS) is written in units of the block's quantiser
step, so that it means the same at every QP, depth and shape, and is aimed at the decision
classes of tests/rdoq_model.py named beside it; tests/test_rdoq_model.py asserts that every
class is reached on every device walk.  A case keeps the luma QP and the lambda as a double,
from which the reference derives the component's QP, the fixed-point lambda and rd_factor
(pipeline.rdoq_host_params does the same here): the oracle is pinned to the reference build on
the cases the reference can express (a non-diagonal scan only in an intra CU below 16x16).

residual_picture(depth): one 128x128 picture pair per depth for xvcgpu_residual_rdoq_batch -
impulses, checkerboards, ramps and full-swing sign patterns under a fixed tiling of every
shape, per-block QP and lambda.
"""
import functools

import numpy as np

import oracle_rdoq as oq
import rdoq_model as rm

DEPTHS = (8, 10, 12)
QP_LOW, QP_HIGH = [0, 1, 2, 3, 4, 5], [46, 47, 48, 49, 50, 51]
QP_ANY = QP_LOW + QP_HIGH + [13, 26, 39, 63]
LAMBDA_MULT = (0.25, 1.0, 4.0, 16.0)

# instance -> shapes (the issue's table; both orientations are generated)
SHAPES_4 = [(4, 4), (8, 4), (8, 8), (16, 4)]
SHAPES_16 = [(16, 8), (16, 16), (32, 4), (32, 8)]
SHAPES_64 = [(32, 16), (32, 32), (64, 4), (64, 16), (64, 64)]
SHAPES_2 = [(2, 2), (2, 4), (2, 8), (2, 16), (2, 32)]


def both(shapes):
    out = []
    for w, h in shapes:
        out += [(w, h)] if w == h else [(w, h), (h, w)]
    return out


def scans_of(w, h):
    return (0, 1, 2) if max(w, h) <= 16 else (0,)


@functools.lru_cache(maxsize=None)
def snapshots(bd):
    """The context snapshots a depth's cases index: every state at 0, 62 and 63 with either
    MPS, a picture's initial states, three seeded ones, and 0 / 63 alternating."""
    from xvc_amd import pipeline
    pool = []
    for byte in (0, 1, 124, 125, 126, 127):
        c = np.zeros(1, oq.RDOQ_CTX_DTYPE)
        c.view(np.uint8)[:] = byte
        pool.append(c)
    pool.append(pipeline.rdoq_init_contexts(30, 1).view(oq.RDOQ_CTX_DTYPE).reshape(1))
    for seed in range(3):
        pool.append(oq.random_contexts(np.random.default_rng(7700 + 10 * bd + seed)))
    c = np.zeros(1, oq.RDOQ_CTX_DTYPE)
    c.view(np.uint8)[:] = np.where(np.arange(oq.RDOQ_CTX_DTYPE.itemsize) & 1, 127, 0)
    pool.append(c)
    out = np.concatenate(pool)
    out["reserved"] = 0
    return out


# ---- the constructions: scan index -> level in quantiser steps ------------------------------
# f(g) returns {scan index: level (float; "max" / "min" / "-max": the int16 limits)}; g: the
# block's geometry() - S coefficients per sub-block, sbs: the scan indices of the sub-blocks
# that hold coefficients (the 32x32 corner), P: scan index -> (x, y), ok(i): the position
# holds a coefficient, v: the variant's number.

def _sb_list(g):
    """Scan indices (of sub-blocks) inside the corner, ascending."""
    return g["sbs"]


def k_dense(g):
    """nine and more levels a sub-block, a level >= 2 early: both budgets; parity either way"""
    rng = np.random.default_rng(g["v"])
    out = {}
    for sb in _sb_list(g)[:2]:
        for k in range(g["S"]):
            out[sb * g["S"] + k] = float(rng.choice([1.3, 1.6, 2.2, 2.8])) * \
                (1 if rng.integers(2) else -1)
    return out


def _decay(g, a, r):
    out = {}
    for i, (x, y) in enumerate(g["P"]):
        lvl = a * r ** -(x + y)
        if g["ok"](i) and lvl >= 0.4:
            out[i] = lvl * (-1 if (x + 2 * y + g["v"]) % 3 == 0 else 1)
    return out


def k_decay2(g):
    """steep decay: the level outruns its neighbours' sum - escape codes at every rice k"""
    return _decay(g, (8, 60, 500, 4000)[g["v"] % 4], 2.0)


def k_decay125(g):
    """flat decay: the rice parameter walks 0 -> 4 and beyond without escapes"""
    return _decay(g, (20, 300, 3000)[g["v"] % 3], 1.25)


def k_flat_max(g):
    """the int16 limits: +-32767 everywhere, -32768 off the last position; rice k at its cap,
    the dequantiser's clip at high QP"""
    out = {}
    for sb in _sb_list(g)[:2]:
        for k in range(g["S"]):
            out[sb * g["S"] + k] = ("max", "-max", "min")[(k + g["v"]) % 3]
    out[max(out)] = "max"
    return out


def _sweep(g, lo, hi):
    s = g["S"]
    out = {k: (lo + (hi - lo) * k / (s - 1)) * (-1 if k & 1 else 1) for k in range(s)}
    last = _sb_list(g)[1] * s + 1 if len(_sb_list(g)) > 1 else s - 1
    out[last] = 3.2
    return out


def k_sweep01(g):
    """a hair either side of zero | one"""
    return _sweep(g, 0.45, 1.2)


def k_sweep12(g):
    """a hair either side of one | two, and of two -> zero under the large lambdas"""
    return _sweep(g, 1.45, 2.2)


def k_sweep23(g):
    """a hair either side of q - 1 | q above two"""
    return _sweep(g, 2.45, 4.6)


def k_sb_struct(g):
    """sub-blocks inside the last position: empty, weak (zeroed), strong (kept), DC only
    (inferred significance)"""
    s, sbs = g["S"], _sb_list(g)
    out = {sbs[-1] * s + min(5, s - 1): 3.0, 1: 2.0}
    for j, sb in enumerate(sbs[1:-1]):
        kind = (j + g["v"]) % 4
        if kind == 1:
            out.update({sb * s + k: 0.8 for k in (1, s - 1)})
        elif kind == 2:
            out.update({sb * s + k: 4.0 + k for k in range(s)})
        elif kind == 3:
            out[sb * s] = 2.0
    return out


def k_tail_ones(g):
    """ones behind a level above one: the last-position walk stops there, the last moves"""
    s = g["S"]
    out = {k: 3.0 for k in range(min(3, s - 1))}
    out.update({k: (0.7, 0.85, 1.0)[(k + g["v"]) % 3] for k in range(min(3, s - 1), s)})
    if len(_sb_list(g)) > 1:
        out[_sb_list(g)[1] * s + 2] = 0.75
    return out


def k_ones_to_dc(g):
    """ones down to DC: the walk reaches it"""
    n = g["S"] + (3 if len(_sb_list(g)) > 1 else 0)
    return {_sb_list(g)[i // g["S"]] * g["S"] + i % g["S"]: (0.8, 1.0, 1.2)[(i + g["v"]) % 3]
            for i in range(n)}


def k_weak_all(g):
    """a few weak levels: the whole block goes to zero at the larger lambdas"""
    s = g["S"]
    out = {0: 0.9, s - 1: 0.7}
    if len(_sb_list(g)) > 1:
        out[_sb_list(g)[-1] * s + 1] = 0.8
    return out


def _far(g, fx, fy):
    out = {0: 5.0}
    tx, ty = (g["rw"] - 1 if fx else 0), (g["rh"] - 1 if fy else 0)
    out[g["P"].index((tx, ty))] = 5.0 + g["v"] % 3
    return out


def k_far_x(g):
    """last position at the far x: bypass suffix in x (in y under the vertical scan)"""
    return _far(g, 1, 0)


def k_far_y(g):
    """... at the far y"""
    return _far(g, 0, 1)


def k_far_xy(g):
    """... in the corner"""
    return _far(g, 1, 1)


def k_single(g):
    """one level: nothing to hide a sign in"""
    return {(0, 1, g["S"] - 1)[g["v"] % 3]: 3.0}


# sign hiding on one 4x4 sub-block: {offset: level}; v & 1 flips the sign of `first` (the
# parity matches or not), v & 2 codes a later sub-block (the adjusted one is then not the last)
SH_PATTERNS = {
    "sh_d3": {2: 2.0, 5: 3.0},                         # distance 3: left alone
    "sh_d4": {2: 2.0, 6: 2.0},                         # distance 4: the shortest that hides
    "sh_inc": {2: 2.0, 6: 2.45, 9: 2.0},               # + 1 on an existing level is cheapest
    "sh_dec": {2: 3.0, 6: 3.55, 9: 3.0},               # - 1 ...
    "sh_one_to_zero": {2: 3.0, 6: 2.0, 9: 0.62, 12: 2.0},
    "sh_zero_below": {0: 0.45, 3: 2.0, 8: 3.0},        # a zero below first, sign as first's
    "sh_zero_barred": {0: -0.45, 3: 2.0, 8: 3.0},      # ... the barred sign
    "sh_zero_above": {2: 2.0, 7: 3.0, 10: 0.45},       # a zero above last (not the last sb)
    "sh_first_one": {2: 0.9, 6: 2.0, 9: 2.0},          # first at level 1: no decrement
    "sh_last_one": {2: 2.0, 5: 2.0, 9: 0.9},           # last at level 1: the 4 * bypass bonus
}


def _sh_kind(name):
    def f(g):
        pat = dict(SH_PATTERNS[name])
        first = min(k for k, v in pat.items() if abs(v) >= 0.5)
        if g["v"] & 1:
            pat[first] = -pat[first]
            if name in ("sh_zero_below", "sh_zero_barred"):
                pat[0] = -pat[0]
        if g["v"] & 4:      # the same one level up: other greater-1 / rice states
            pat = {k: (v + (1 if v > 0 else -1) if abs(v) >= 0.5 else v) for k, v in pat.items()}
        out = {k: v for k, v in pat.items()}
        if g["v"] & 2 and len(_sb_list(g)) > 1:
            out[_sb_list(g)[1] * 16 + 4] = 3.0
        return out
    f.__doc__ = "sign hiding: " + name
    return f


KINDS = {f.__name__[2:]: f for f in (
    k_dense, k_decay2, k_decay125, k_flat_max, k_sweep01, k_sweep12, k_sweep23, k_sb_struct,
    k_tail_ones, k_ones_to_dc, k_weak_all, k_far_x, k_far_y, k_far_xy, k_single)}
KINDS.update({name: _sh_kind(name) for name in SH_PATTERNS})
# construction -> the classes of rdoq_model.KEYS it is there for (test_rdoq_model.py: its cases
# reach each of them, and every class has a construction; the context-state and chroma
# last-position classes belong to the rotation of snapshots and components, not to a kind)
SERVES = {
    "dense": ["g1_budget_spent", "g2_budget_spent", "sh_parity_ok", "sh_parity_fix", "sh_off"],
    "decay2": ["escape_k0", "escape_k1", "escape_k2", "escape_k3", "escape_k4_9", "iq_shift_left"],
    "decay125": ["rice_k0", "rice_k1", "rice_k2", "rice_k3", "rice_k4", "rice_k5_8",
                 "rice_update_cap4"],
    "flat_max": ["src_32767", "src_m32767", "src_m32768", "deq_clip", "rice_k9_cap"],
    "sweep01": ["q1_to_0", "q1_to_1"], "sweep12": ["q2_to_0", "q2_to_1", "q2_to_2"],
    "sweep23": ["q3up_to_qm1", "q3up_kept"],
    "sb_struct": ["sb_empty", "sb_zeroed", "sb_kept", "sig_inferred"],
    "tail_ones": ["last_stop_gt1", "last_moved"], "ones_to_dc": ["last_reach_dc"],
    "weak_all": ["block_zeroed"], "far_x": ["lastpos_suffix_x"], "far_y": ["lastpos_suffix_y"],
    "far_xy": ["lastpos_suffix_x", "lastpos_suffix_y", "lastpos_swapped"],
    "single": ["sh_single_level", "last_stays"],
    "sh_d3": ["sh_dist_3"], "sh_d4": ["sh_dist_4"], "sh_inc": ["sh_adj_inc"],
    "sh_dec": ["sh_adj_dec"], "sh_one_to_zero": ["sh_adj_1_to_0"],
    "sh_zero_below": ["sh_adj_zero_below_first"],
    "sh_zero_barred": ["sh_barred_sign", "sh_bar_decides"],
    "sh_zero_above": ["sh_adj_zero_above_last", "sh_in_later_sb"],
    "sh_first_one": ["sh_first_barred"], "sh_last_one": ["sh_last_sb_bonus", "sh_in_last_sb"],
    "tie_zero_level": ["tie_zero_level"], "tie_qm1_q": ["tie_qm1_q"],
}
UNSERVED = ["ctx_state_0", "ctx_state_62_63", "ctx_mps_0", "ctx_mps_1", "chroma_last_4",
            "chroma_last_8", "chroma_last_16", "chroma_last_32", "sh_saturated"]
# (kind, variants, QPs): the magnitudes of the first group need the small steps of a low QP
PLAN_SMALL = [("dense", 4, QP_ANY), ("decay2", 4, QP_LOW), ("decay125", 3, QP_LOW),
              ("flat_max", 3, QP_ANY), ("sweep01", 4, QP_ANY), ("sweep12", 4, QP_ANY),
              ("sweep23", 4, QP_ANY), ("sb_struct", 4, QP_ANY), ("tail_ones", 3, QP_ANY),
              ("ones_to_dc", 3, QP_ANY), ("weak_all", 4, QP_ANY), ("far_x", 1, QP_ANY),
              ("far_y", 1, QP_ANY), ("far_xy", 1, QP_ANY), ("single", 3, QP_ANY)] + \
    [(name, 8, QP_ANY) for name in SH_PATTERNS]
PLAN_LARGE = [(k, v if k == "decay2" else min(v, 2), q) for k, v, q in PLAN_SMALL]
PLAN_2 = [(k, v, q) for k, v, q in PLAN_SMALL if not k.startswith("sh_")]


def geometry(w, h, scan, v):
    P = rm.scan_positions(w, h, scan)
    S = 4 if (w == 2 or h == 2) else 16
    rw, rh = min(w, 32), min(h, 32)
    inside = [x < rw and y < rh for x, y in P]
    sbs = [i // S for i in range(0, len(P), S) if inside[i]]
    return dict(w=w, h=h, rw=rw, rh=rh, S=S, P=P, v=v, sbs=sbs, ok=lambda i: inside[i])


def coefficients(bd, qp, w, h, scan, kind, v):
    """The kind's block for this quantiser: levels in steps -> int16 coefficients."""
    k = rm.quant_constants(bd, qp, w, h)
    step = float(1 << k["fq_shift"]) / k["scale"]
    g = geometry(w, h, scan, v)
    src = np.zeros((h, w), np.int16)
    for i, lvl in KINDS[kind](g).items():
        if i >= len(g["P"]) or not g["ok"](i):
            continue
        x, y = g["P"][i]
        if isinstance(lvl, str):
            src[y, x] = {"max": 32767, "-max": -32767, "min": -32768}[lvl]
        else:
            src[y, x] = int(np.clip(np.rint(lvl * step), -32767, 32767))
    return src


def make_case(bd, i, w, h, scan, kind, v, qps, flags=0):
    """Case number i of a depth: what rotates with i, and the host-side constants."""
    from xvc_amd import pipeline
    qp_luma = qps[(5 * i + bd) % len(qps)]
    comp = 0 if max(w, h) > 32 else (0, 1, 0, 2)[(i // 3) % 4]
    mult = LAMBDA_MULT[(i + i // 4) % 4]
    lam = 0.57 * 2.0 ** ((qp_luma - 12) / 3.0) * mult
    qp = qp_luma if comp == 0 else pipeline.chroma_qp(qp_luma)
    lam_fix, rdf = pipeline.rdoq_host_params(qp_luma, bd, lam)[comp]
    if scan or (i // 5) % 2:
        flags |= rm.INTRA_CU
    return dict(bd=bd, i=i, qp_luma=qp_luma, lam=lam, comp=comp, qp=qp, luma=comp == 0,
                scan=scan, sign_hide=0 if i % 7 == 3 else 1, flags=flags, w=w, h=h,
                src=coefficients(bd, qp, w, h, scan, kind, v),
                ctx=(i + i // 11) % len(snapshots(bd)),
                lam_fix=lam_fix, rd_factor=rdf, kind=kind, v=v)


# Exact ties of the two comparisons that decide a level (the zero wins a tie against the level,
# q wins one against q - 1): found once by scanning lambda over the model (find_ties below,
# `python tests/rdoq_cases.py ties`) and kept as numbers, (w, h, scan, luma qp, coefficient in
# 1/64 steps, lambda as the fixed-point integer), one shape per walk.  A luma block, the
# coefficient at scan index 2 under a strong one at index 9; every context at state 0, MPS 0.
TIE_SHAPES = [(4, 4, 0), (16, 16, 0), (32, 32, 0), (4, 4, 1), (8, 8, 2), (2, 8, 0), (32, 8, 0)]
TIES = {"tie_zero_level": [(4, 4, 0, 4, 40, 8005), (16, 16, 0, 4, 40, 8005),
                           (32, 32, 0, 4, 48, 16010), (4, 4, 1, 4, 40, 8005), (8, 8, 2, 4, 40, 8005),
                           (2, 8, 0, 4, 40, 8005), (32, 8, 0, 4, 40, 8005)],
        "tie_qm1_q": [(4, 4, 0, 4, 100, 7552), (16, 16, 0, 4, 170, 16384),
                      (32, 32, 0, 4, 170, 32767), (4, 4, 1, 4, 100, 7552), (8, 8, 2, 4, 100, 7552),
                      (2, 8, 0, 4, 100, 7826), (32, 8, 0, 4, 170, 16384)]}


def tie_case(bd, i, w, h, scan, qp, c64, lam_fix, kind="tie"):
    from xvc_amd import pipeline
    k = rm.quant_constants(bd, qp, w, h)
    step = float(1 << k["fq_shift"]) / k["scale"]
    src = np.zeros((h, w), np.int16)
    P = rm.scan_positions(w, h, scan)
    src[P[2][1], P[2][0]] = int(np.rint(c64 / 64.0 * step))
    src[P[9][1], P[9][0]] = int(np.rint(3.0 * step))
    lam = lam_fix / 65536.0
    got_fix, rdf = pipeline.rdoq_host_params(qp, bd, lam)[0]
    assert got_fix == lam_fix
    return dict(bd=bd, i=i, qp_luma=qp, lam=lam, comp=0, qp=qp, luma=True, scan=scan,
                sign_hide=1, flags=rm.INTRA_CU if scan else 0, w=w, h=h, src=src, ctx=0,
                lam_fix=lam_fix, rd_factor=rdf, kind=kind, v=0)


@functools.lru_cache(maxsize=None)
def cases(bd):
    out = []

    def add(w, h, scan, kind, v, qps, flags=0):
        out.append(make_case(bd, len(out), w, h, scan, kind, v, qps, flags))

    for w, h in both(SHAPES_4 + [s for s in SHAPES_16 if max(s) <= 16]):
        for scan in scans_of(w, h):
            for kind, nv, qps in PLAN_SMALL:
                for v in range(nv):
                    add(w, h, scan, kind, v, qps)
    for w, h in both([s for s in SHAPES_16 if max(s) > 16] + SHAPES_64):
        for kind, nv, qps in PLAN_LARGE:
            for v in range(nv):
                add(w, h, 0, kind, v, qps)
    for w, h in both(SHAPES_2):
        for scan in scans_of(w, h):
            for kind, nv, qps in PLAN_2:
                for v in range(nv):
                    add(w, h, scan, kind, v, qps)
            add(w, h, scan, "dense", 0, QP_ANY, rm.NO_2X2)
    # the 2x2 block at 8 bits: the only dequantiser that shifts left
    if bd == 8:
        for v in range(4):
            add(2, 2, 0, "decay2", v, QP_LOW)
    for key, ties in TIES.items():
        for w, h, scan, qp, c64, lam_fix in ties:
            out.append(tie_case(bd, len(out), w, h, scan, qp, c64, lam_fix, key))
    return out


def find_ties(bd=8, qp=4):
    """Scan lambda for exact ties of the model's two level comparisons (see TIES); the
    quantiser's constants move together with the depth, so a tie at one depth is one at all."""
    import collections
    import oracle_lib as ol
    import test_rdoq_zero_proof as zp
    ent = [int(v) for v in zp.entropy_table(ol.Lib("xo"))]
    c = {k: snapshots(bd)[0][k].tolist() for k in oq.RDOQ_CTX_DTYPE.names}
    base = int(0.57 * 2.0 ** ((qp - 12) / 3.0) * 65536)
    found = {"tie_zero_level": [], "tie_qm1_q": []}
    for w, h, scan in TIE_SHAPES:
        for key, c64s in (("tie_zero_level", (40, 48, 56)), ("tie_qm1_q", (100, 170, 110))):
            for c64 in c64s:
                hit = None
                for lam_fix in range(max(base // 4, 1), base * 6):
                    case = tie_case(bd, 0, w, h, scan, qp, c64, lam_fix)
                    n = collections.Counter()
                    rm.quant_rdo(ent, bd, qp, True, scan, 1, case["flags"], w, h,
                                 case["src"].tolist(), c, lam_fix, case["rd_factor"], n)
                    if n[key]:
                        hit = (w, h, scan, qp, c64, lam_fix)
                        break
                if hit:
                    found[key].append(hit)
                    break
    return found


# ---- the residual entry: one picture pair per depth ------------------------------------------
# A fixed tiling of every shape: luma 128x128 as four 64x64 tiles, the chroma planes 64x64.
def _rows(x0, y0, w, h, nx, ny=1):
    return [(x0 + i * w, y0 + j * h, w, h) for j in range(ny) for i in range(nx)]


LUMA_TILING = (
    [(0, 0, 64, 64)] +
    # (64, 0): the 64-wide and 32-wide shapes
    _rows(64, 0, 64, 16, 1) + _rows(64, 16, 64, 4, 1, 4) + [(64, 32, 32, 32), (96, 32, 32, 16)] +
    _rows(96, 48, 32, 8, 1, 2) +
    # (0, 64): the tall ones
    [(0, 64, 16, 64)] + _rows(16, 64, 4, 64, 4) + _rows(32, 64, 8, 32, 4) + _rows(32, 96, 16, 32, 2) +
    # (64, 64): the one-wave kernel's shapes
    _rows(64, 64, 16, 16, 4) + _rows(64, 80, 16, 8, 4, 2) + _rows(64, 96, 8, 16, 8) +
    _rows(64, 112, 8, 8, 8) + _rows(64, 120, 16, 4, 4) + _rows(64, 124, 8, 4, 8))
_CHROMA_TOP = _rows(0, 0, 4, 16, 16) + _rows(0, 16, 4, 8, 16) + _rows(0, 24, 4, 4, 16) + \
    _rows(0, 28, 8, 4, 8)
_TWO_WIDE = _rows(32, 32, 32, 2, 1, 2) + _rows(32, 36, 8, 2, 4) + _rows(32, 38, 4, 2, 8) + \
    _rows(32, 40, 2, 2, 16, 2) + _rows(32, 44, 2, 4, 16) + _rows(32, 48, 2, 8, 16) + \
    [(32, 56, 16, 8)] + _rows(48, 56, 16, 2, 1, 4)
CHROMA_TILING = (
    _CHROMA_TOP + [(0, 32, 32, 32)] + _TWO_WIDE,
    _CHROMA_TOP + _rows(0, 32, 32, 4, 1, 2) + [(0, 40, 32, 8), (0, 48, 32, 16)] + _rows(32, 32, 2, 32, 4) +
    [(40, 32, 8, 32)] + _rows(48, 32, 4, 32, 3) + _rows(60, 32, 2, 16, 2, 2))
CONTENT = ("impulse", "checker", "ramp", "full_swing", "near_threshold", "mixture", "sparse",
           "flat_swing", "near_threshold", "synth", "sparse", "impulse", "synth")
# "synth": a construction of the packed entry, brought here through the oracle's inverse
# transform (the forward transform returns it up to its rounding)
SYNTH_KINDS = ("sh_d3", "sh_d4", "sh_last_one", "sh_zero_below", "sh_zero_barred", "sh_first_one",
               "sh_one_to_zero", "sh_zero_above", "sb_struct", "tail_ones", "weak_all", "single",
               "sweep01", "ones_to_dc")
# the workgroup kernel's four-lane walks see few blocks a picture: every other one is a "synth"
CONTENT_LARGE = ("synth", "impulse", "synth", "full_swing", "synth", "near_threshold", "synth",
                 "flat_swing", "synth", "ramp", "synth", "checker", "synth", "mixture", "synth",
                 "sparse")
RES_QPS_SYNTH = [13, 16, 20, 23, 26, 30]
RES_QPS = [0, 3, 5, 8, 13, 1, 4, 20, 2, 26, 10, 16, 23]
RES_QPS_HIGH = [39, 40, 41, 42, 43, 44, 45, 46, 47, 48, 49, 50, 51]


def _content(kind, bd, w, h, j, qp=0, scan=0, synth=0):
    """(orig, pred) of a w x h block, content number j (qp, scan: the block's, for "synth")."""
    smax, mid = (1 << bd) - 1, 1 << (bd - 1)
    rng = np.random.default_rng(9000 + j)
    yy, xx = np.mgrid[0:h, 0:w]
    pred = np.full((h, w), mid, np.int64)
    orig = pred.copy()
    if kind == "impulse":
        for t in range(1 + j % 3):
            orig[(j + 3 * t) % h, (2 * j + 5 * t) % w] = smax if (j + t) & 1 else 0
    elif kind == "checker":
        period = 1 << (j % 3)
        board = ((xx // period + yy // period) & 1)
        orig, pred = board * smax, (1 - board) * smax
    elif kind == "ramp":
        d = (xx, yy, xx + yy)[j % 3]
        orig = np.clip(mid + (d - d.max() // 2) * ((smax // 2) // max(int(d.max()), 1)) * (1 + j % 2),
                       0, smax)
    elif kind == "full_swing":
        sign = rng.integers(0, 2, (h, w))
        orig, pred = sign * smax, (1 - sign) * smax
    elif kind == "near_threshold":
        a = 1 + j % 4
        orig = np.clip(mid + (rng.integers(-a, a + 1, (h, w)) << (bd - 8)), 0, smax)
    elif kind == "sparse":
        for t in range(1 + j % 4):
            orig[(3 * j + 5 * t) % h, (j + 7 * t) % w] += (2 + (j + t) % 9) * (1 if t & 1 else -1) << (bd - 8)
    elif kind == "synth":
        import oracle_lib as ol
        name = SYNTH_KINDS[synth % len(SYNTH_KINDS)]
        if min(w, h) == 2 and name.startswith("sh_"):
            name = "sb_struct"
        coeff = coefficients(bd, qp, w, h, scan, name, synth // len(SYNTH_KINDS))
        orig = np.clip(mid + ol.Lib("xo").inv_transform(bd, coeff).astype(np.int64), 0, smax)
    elif kind == "rice_cap":
        # a 2x32 block whose energy sits in the four neighbours of one coefficient, equal and
        # as large as samples allow (then half as much again, clipped): the rice parameter's
        # cap of 9 needs their levels to sum to 4092
        import oracle_lib as ol
        xo, best = ol.Lib("xo"), None
        for y0 in range(6):
            for signs in range(16):
                c = np.zeros((h, w), np.int16)
                pts = [(1, y0), (1, y0 + 1), (0, y0 + 1), (0, y0 + 2)]
                for i, (px, py) in enumerate(pts + [(0, y0)]):
                    px, py = (px, py) if w == 2 else (py, px)
                    c[py, px] = (8000 if (signs >> i) & 1 else -8000) // (1 if i < 4 else 40)
                r = xo.inv_transform(bd, c).astype(np.int64)
                if best is None or np.abs(r).max() < np.abs(best).max():
                    best = r
        r = np.clip(best * (1.5 * smax) / np.abs(best).max(), -smax, smax).astype(np.int64)
        orig, pred = np.maximum(r, 0), np.maximum(-r, 0)
    elif kind == "flat_swing":
        orig, pred = (orig * 0 + smax, pred * 0) if j & 1 else (orig * 0, pred * 0 + smax)
    else:
        orig = np.clip(mid + (xx - yy) * (smax // (4 * max(w, h))) +
                       (rng.integers(-6, 7, (h, w)) << (bd - 8)), 0, smax)
        orig[j % h, j % w] = smax
    return orig.astype(np.uint16), pred.astype(np.uint16)


# (depth, block) -> the lambda at which one of the block's coefficients ties zero against its
# level, one block per walk: found by scanning lambda over the model, as TIES above
RES_TIES = {(8, 9): 14624, (8, 19): 1443153, (8, 22): 3410, (8, 39): 9061, (8, 183): 19865}


def _clip_qp(bd, comp, w, h, j):
    """A high luma QP at which the full-swing DC's level dequantises beyond 32767 (the
    dequantiser's clip), the first from a start that rotates with j; else that start."""
    from xvc_amd import pipeline
    c = ((1 << bd) - 1) << (15 - bd)
    order = RES_QPS_HIGH[j % len(RES_QPS_HIGH):] + RES_QPS_HIGH[:j % len(RES_QPS_HIGH)]
    for qp_luma in order:
        k = rm.quant_constants(bd, qp_luma if comp == 0 else pipeline.chroma_qp(qp_luma), w, h)
        deq = rm.plain_level(k, c) * k["iq_scale"]
        if k["iq_shift"] > 0 and (deq + (1 << (k["iq_shift"] - 1))) >> k["iq_shift"] > 32767:
            return qp_luma
    return order[0]


@functools.lru_cache(maxsize=None)
def residual_picture(bd):
    """orig, pred: [Y, U, V] planes (128x128, 64x64, 64x64); blocks: the tiling as tuples of
    api.TX_DTYPE; params: RDOQ_PARAMS_DTYPE per block; the depth's snapshots()."""
    from xvc_amd import api, pipeline
    orig = [np.zeros((128 >> (c > 0), 128 >> (c > 0)), np.uint16) for c in range(3)]
    pred = [np.zeros_like(p) for p in orig]
    blocks, params = [], []
    n_ctx = len(snapshots(bd))
    seen, synths = {}, {}      # per walk: its blocks, its "synth" blocks so far
    for comp, tiling in enumerate((LUMA_TILING,) + CHROMA_TILING):
        cover = np.zeros(orig[comp].shape, np.uint8)
        for x, y, w, h in tiling:
            j = len(blocks) + 7 * bd
            assert x % min(w, 4) == 0 and not cover[y:y + h, x:x + w].any()
            cover[y:y + h, x:x + w] = 1
            scan = (j // 2) % 3 if max(w, h) <= 16 else 0
            scan = (j // 2) % 3 if max(w, h) <= 16 else 0
            flags = (rm.INTRA_CU if scan or j % 3 == 0 else 0) | \
                (rm.NO_2X2 if min(w, h) == 2 and j % 4 == 0 else 0)
            walk = rm.device_walk("residual", w, h, scan, flags)
            content = CONTENT_LARGE if walk.startswith("workgroup/wave_rdoq4") else CONTENT
            kind = content[(seen.get(walk, 0) + 3 * bd) % len(content)]
            seen[walk] = seen.get(walk, 0) + 1
            if walk.endswith("2x2") and max(w, h) == 32 and seen[walk] % 2:
                kind = "rice_cap"
            if kind == "synth":
                synths[walk] = synths.get(walk, 5 * ((bd - 8) // 2) - 1) + 1
            qps = {"flat_swing": RES_QPS_HIGH, "synth": RES_QPS_SYNTH}.get(kind, RES_QPS)
            qp_luma = qps[(j // 3) % len(qps)]
            mult = LAMBDA_MULT[(j + j // 5) % 4]
            large_synth = kind == "synth" and content is CONTENT_LARGE
            if kind == "rice_cap":
                qp_luma = 0
            elif kind == "flat_swing":
                qp_luma = _clip_qp(bd, comp, w, h, j)
            elif large_synth:      # few of them: each as its construction means it
                mult = LAMBDA_MULT[0]
            lam = 0.57 * 2.0 ** ((qp_luma - 12) / 3.0) * mult
            qp = qp_luma if comp == 0 else pipeline.chroma_qp(qp_luma)
            lam_fix, rdf = pipeline.rdoq_host_params(qp_luma, bd, lam)[min(comp, 1)]
            o, p = _content(kind, bd, w, h, j // len(CONTENT) + j, qp, scan, synths.get(walk, 0))
            orig[comp][y:y + h, x:x + w], pred[comp][y:y + h, x:x + w] = o, p
            blocks.append((x, y, w, h, comp, 0, 0, 0, qp,
                           api.TXF_RDOQ | (scan << api.TXF_SCAN_SHIFT) |
                           (api.TXF_NO_SIGN_HIDING if seen[walk] % 5 == 3 and not large_synth else 0)))
            prm = np.zeros(1, oq.RDOQ_PARAMS_DTYPE)
            if (bd, len(blocks) - 1) in RES_TIES:      # (a luma lambda: the integer is exact)
                lam_fix = RES_TIES[(bd, len(blocks) - 1)]
                got, rdf = pipeline.rdoq_host_params(qp_luma, bd, lam_fix / 65536.0)[min(comp, 1)]
                assert got == lam_fix
            prm["lambda"], prm["rd_factor"], prm["flags"] = lam_fix, rdf, flags
            prm["ctx_index"] = (j + j // 9) % n_ctx
            params.append(prm[0])
    return orig, pred, np.array(blocks, api.TX_DTYPE), np.array(params, oq.RDOQ_PARAMS_DTYPE), \
        snapshots(bd)


if __name__ == "__main__":
    import sys
    if sys.argv[1:] == ["ties"]:
        print(find_ties())
