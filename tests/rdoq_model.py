"""The RDO quantiser in plain integers, a counter on every decision.  TEST INFRASTRUCTURE.

quant_rdo() restates RdoQuant::QuantRdo with CoeffSignHideRdo (the extended residual
context set) from the project's oracle, oracle/xvc_oracle_rdoq.c, and the codec's documented
behaviour; python integers, no vector arithmetic, so that each branch can carry a named
counter (KEYS).  tests/test_rdoq_model.py holds it against the oracle on the directed cases
of tests/rdoq_cases.py and asserts that every class is reached on every device walk that can
reach it; device_walk() restates which walk instance of xvc_amd/csrc serves a block.

Where C arithmetic matters it is kept: the forward quantiser's level and the sign hiding's
error term are int16 values, |-32768| stays -32768 (the reference takes abs() into an int16),
costs are 64-bit.  Two inputs are outside the model and refused by an assertion: a coefficient
of -32768 that is the block's last one (its cost is INT64_MAX plus something in C), and a
level times the inverse scale beyond 31 bits.

The walk instances (device_walk) and what the source holds besides them
----------------------------------------------------------------------
xvcgpu_quant_rdo_batch (rdoq_classify_kernel -> rq_class_of, k_rdoq.h):
  packed4/wave_rdoq4<16,1>   class 0: diagonal scan, sides >= 4, at most four sub-blocks
                             (4x4, 8x4, 8x8, 16x4), four blocks of a wave side by side
  packed4/wave_rdoq4<64,1>   class 1: up to sixteen sub-blocks (16x8, 16x16, 32x4, 32x8), a
                             block per wave, while the list holds at most RDOQ4_LATENCY_BLOCKS
  packed4/wave_rdoq<16>      class 1 on a longer list: a lane per sub-block, four blocks side
                             by side; its 16x16 arm (G == 16 && NSB == 16) and the any-size one
  packed/wave_rdoq4<64,4>    class 2, diagonal: more than sixteen sub-blocks or a 64-point side
  packed/wave_rdoq<64>/scan  class 2, horizontal and vertical scan, 4x4 sub-blocks
  packed/wave_rdoq<64>/2x2   class 2, 2-wide blocks (2x2 sub-blocks)
  (a 2-wide block with XVC_RDOQ_NO_2X2 is not this entry's: device_walk returns None)
xvcgpu_residual_rdoq_batch (tx_small_job: sides 4, 8, 16 -> tx2_job, else residual_job):
  wave/wave_rdoq4<64,1>      one-wave forward kernel, diagonal scan
  wave/wave_rdoq<64>/scan    one-wave forward kernel, the other scans
  workgroup/wave_rdoq4<64,1> workgroup kernel, at most sixteen sub-blocks in the 32x32 corner
                             (32x4, 32x8, 64x4, 64x8)
  workgroup/wave_rdoq4<64,4> workgroup kernel, more (32x16 ... 64x64)
  workgroup/wave_rdoq<64>/2x2  workgroup kernel, 2-wide blocks
  QuantFast                  2-wide with XVC_RDOQ_NO_2X2 (not the RDO quantiser: no census)
Not a walk of these two entries' directed cases: the workgroup kernel's wave_rdoq<64> on 4x4
sub-blocks (a non-diagonal scan above 16x16, which DetermineScanOrder never gives, or the 4x4
DST / transform-skip blocks, tests/test_gpu_fwd_inv_paths.py) and wave_rdoq<32> (two small
blocks side by side in recon_from_me_kernel, the frame pass's tests).  No instantiation in
the source is unreachable by a legal batch: the `G == 16 && NSB == 16` 16x16 arm, the
candidate, belongs to quant_rdo_packed_wave<16, 16, false>, which quant_rdo_packed4_kernel
takes for class 1 once that list is longer than RDOQ4_LATENCY_BLOCKS (4096) - a legal batch,
only a long one; tests/test_gpu_rdoq_cases.py builds it.  There is no `wave_rdoq4<4,1>`: the
group of class 0 is sixteen lanes (four per sub-block, four sub-blocks).

The sign hiding's saturation branch (`level == 32767 || level == -32768` in front of the
adjustment) is unreachable: a CU's raw QP is clipped to 0 .. 63 where it is looked up
(PictureData::GetQp) and the chroma QP to 0 .. 57 (Qp::ScaleChromaQp), so qp_bitdepth =
qp + 6 (depth - 8) >= 6 (depth - 8); the forward quantiser's shift is 14 + qp_bitdepth / 6 +
(15 - depth - (log2 w + log2 h) / 2) >= 14 + (depth - 8) + 15 - depth - 6 = 15 for every shape
up to 64x64 (the 181 / 128 of the odd shapes is below 2 and comes with a shift one larger), so
a level is at most (32768 * 26214 + 2^14) >> 15 = 26215 and the sign hiding adds one
(test_saturation_is_out_of_reach evaluates it per shape).  xvcgpu_tx_block.qp is that raw QP
(Qp::GetQpRaw): the ABI's int8 could hold a negative one, which at 10 or 12 bits would lower
the shift below 15 and wrap the int16 level, but no Qp the reference builds has one.
EXCLUDED["*"] names the class, test_rdoq_model.py asserts that it never occurs.
"""
import collections

FWD = [26214, 23302, 20560, 18396, 16384, 14564]
INV = [40, 45, 51, 57, 64, 72]
BYPASS = 1 << 15
I64_MAX = (1 << 63) - 1
I32_MAX = (1 << 31) - 1
RICE_RANGE = [6, 5, 6, 3, 3, 3, 3, 3, 3, 3]
MIN_IN_GROUP = [0, 1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 64, 96]
SCAN2 = [[0, 2, 1, 3], [0, 1, 2, 3], [0, 2, 1, 3]]
SCAN4 = [[0, 4, 1, 8, 5, 2, 12, 9, 6, 3, 13, 10, 7, 14, 11, 15], list(range(16)),
         [0, 4, 8, 12, 1, 5, 9, 13, 2, 6, 10, 14, 3, 7, 11, 15]]
INTRA_CU, NO_2X2 = 1, 2

# every decision class, in the order of the census table
KEYS = [
    # the level's price
    "g1_budget_spent",     # a level priced after eight non-zero levels of its sub-block
    "g2_budget_spent",     # a level priced after a level >= 2 of its sub-block
    "rice_k0", "rice_k1", "rice_k2", "rice_k3", "rice_k4", "rice_k5_8",
    "rice_k9_cap",         # the template's parameter at its cap of 9
    "rice_update_cap4",    # UpdateCodeState's min(k + 1, 4) with k >= 4
    "escape_k0", "escape_k1", "escape_k2", "escape_k3", "escape_k4_9",
    # the coefficient
    "src_32767", "src_m32767", "src_m32768", "deq_clip", "iq_shift_left",
    # zero / q - 1 / q
    "q1_to_0", "q1_to_1", "q2_to_0", "q2_to_1", "q2_to_2", "q3up_to_qm1", "q3up_kept",
    "tie_zero_level",      # the zero's cost == the level's: zero wins
    "tie_qm1_q",           # q - 1's cost == q's: q wins
    # sub-blocks in front of the last position
    "sb_empty", "sb_zeroed", "sb_kept", "sig_inferred",
    # the last position
    "last_stop_gt1", "last_reach_dc", "last_moved", "last_stays", "block_zeroed",
    "lastpos_suffix_x", "lastpos_suffix_y", "lastpos_swapped",
    "chroma_last_4", "chroma_last_8", "chroma_last_16", "chroma_last_32",
    # the context states read
    "ctx_state_0", "ctx_state_62_63", "ctx_mps_0", "ctx_mps_1",
    # sign hiding
    "sh_parity_ok", "sh_parity_fix", "sh_dist_3", "sh_dist_4",
    "sh_adj_inc", "sh_adj_dec", "sh_adj_1_to_0", "sh_adj_zero_below_first",
    "sh_adj_zero_above_last", "sh_barred_sign",
    "sh_bar_decides",      # a barred zero below `first` would have been the cheapest
    "sh_first_barred", "sh_last_sb_bonus", "sh_in_last_sb", "sh_in_later_sb",
    "sh_off", "sh_single_level", "sh_saturated",
]
SH_KEYS = [k for k in KEYS if k.startswith("sh_") and k not in ("sh_off", "sh_single_level",
                                                                "sh_saturated")]

# walk instance -> {class: why no legal block of that walk reaches it}; "*": every walk.
# tests/test_rdoq_model.py asserts that an excluded class never occurs there.
_IQ = "only the 2x2 block at 8 bits has a transform shift of 6, where the dequantiser shifts left"
_SWAP = "the coordinates swap under the vertical scan only"
_NO_SH = "QuantRdo hides no sign in 2x2 sub-blocks (SubBlockShift == 1)"
_G1 = "a 2x2 sub-block holds four levels, the greater-than-1 budget is eight"
_C32 = "a chroma block is at most 32x32: more than sixteen sub-blocks need both sides >= 16"
_SCAN16 = "scans 1 and 2 run up to 16x16 (DetermineScanOrder gives them only below that)"
_FWD = ("behind the forward transform |coefficient| <= (2^depth - 1) * 2^(15 - depth) = 32640, "
        "32736, 32760: a row of the 256-scaled matrices sums to at most 256 N in absolute value "
        "and either stage's shift takes exactly that gain out (test_forward_coefficients_...)")
_TWO = dict({k: _NO_SH for k in SH_KEYS + ["sh_off", "sh_single_level"]}, g1_budget_spent=_G1)
_INT16 = {k: _FWD for k in ("src_32767", "src_m32767", "src_m32768")}
EXCLUDED = {
    "*": {"sh_saturated": "a level is at most 26215 for a raw QP >= 0 (module docstring)"},
    "packed4/wave_rdoq4<16,1>": {"iq_shift_left": _IQ, "lastpos_swapped": _SWAP,
                                 "chroma_last_32": "no side of 32 within four sub-blocks"},
    "packed4/wave_rdoq4<64,1>": {"iq_shift_left": _IQ, "lastpos_swapped": _SWAP},
    "packed4/wave_rdoq<16>": {"iq_shift_left": _IQ, "lastpos_swapped": _SWAP},
    "packed/wave_rdoq4<64,4>": {"iq_shift_left": _IQ, "lastpos_swapped": _SWAP,
                                "chroma_last_4": _C32, "chroma_last_8": _C32},
    "packed/wave_rdoq<64>/scan": {"iq_shift_left": _IQ, "chroma_last_32": _SCAN16},
    "packed/wave_rdoq<64>/2x2": _TWO,
}
RESIDUAL_EXCLUDED = {
    "wave/wave_rdoq4<64,1>": dict(_INT16, iq_shift_left=_IQ, lastpos_swapped=_SWAP,
                                  chroma_last_32="sides 4, 8 and 16 only"),
    "wave/wave_rdoq<64>/scan": dict(_INT16, iq_shift_left=_IQ,
                                    chroma_last_32="sides 4, 8 and 16 only"),
    "workgroup/wave_rdoq4<64,1>": dict(_INT16, iq_shift_left=_IQ, lastpos_swapped=_SWAP,
                                       chroma_last_16="its shapes are 32x4, 32x8, 64x4, 64x8"),
    "workgroup/wave_rdoq4<64,4>": dict(_INT16, iq_shift_left=_IQ, lastpos_swapped=_SWAP,
                                       chroma_last_4=_C32, chroma_last_8=_C32),
    "workgroup/wave_rdoq<64>/2x2": dict(_TWO, **_INT16),
}


def log2(v):
    return v.bit_length() - 1


def rq4_takes(g, w, h, scan):
    rw, rh = min(w, 32), min(h, 32)
    return scan == 0 and w >= 4 and h >= 4 and (g == 64 or (rw >> 2) * (rh >> 2) * 4 <= g)


def rq_class_of(w, h, scan):
    if not rq4_takes(64, w, h, scan) or w > 32 or h > 32:
        return 2
    n_sb = (w >> 2) * (h >> 2)
    return 0 if n_sb <= 4 else (1 if n_sb <= 16 else 2)


LATENCY_BLOCKS = 4096   # RDOQ4_LATENCY_BLOCKS (k_rdoq.h)


def device_walk(entry, w, h, scan, flags, long_list=False):
    """The walk instance that quantises a w x h block of this scan and xvcgpu_rdoq_params
    flags on entry "packed" (xvcgpu_quant_rdo_batch; long_list: its class-1 list holds more
    than LATENCY_BLOCKS blocks) or "residual" (xvcgpu_residual_rdoq_batch, a block without
    the 4x4 DST or transform skip).  None: the entry does not take the block."""
    two = w == 2 or h == 2
    if entry == "packed":
        if two:
            return None if flags & NO_2X2 else "packed/wave_rdoq<64>/2x2"
        cls = rq_class_of(w, h, scan)
        if cls == 0:
            return "packed4/wave_rdoq4<16,1>"
        if cls == 1:
            return "packed4/wave_rdoq<16>" if long_list else "packed4/wave_rdoq4<64,1>"
        return "packed/wave_rdoq4<64,4>" if rq4_takes(64, w, h, scan) else \
            "packed/wave_rdoq<64>/scan"
    assert entry == "residual"
    if two:
        return "QuantFast" if flags & NO_2X2 else "workgroup/wave_rdoq<64>/2x2"
    if w in (4, 8, 16) and h in (4, 8, 16):      # tx_small_job: the one-wave kernel, G = 64
        return "wave/wave_rdoq4<64,1>" if rq4_takes(64, w, h, scan) else "wave/wave_rdoq<64>/scan"
    if not rq4_takes(64, w, h, scan):
        return "workgroup/wave_rdoq<64>/scan"
    nr4 = (min(w, 32) >> 2) * (min(h, 32) >> 2) > 16     # rq4_needs_nr4
    return "workgroup/wave_rdoq4<64,4>" if nr4 else "workgroup/wave_rdoq4<64,1>"


def subblock_scan(order, gw, gh):
    """DeriveSubblockScan: scan index -> y * gw + x of the sub-block."""
    tab, px, py = [], 0, 0
    for _ in range(gw * gh):
        tab.append(py * gw + px)
        if order == 0:
            if px == gw - 1 or py == 0:
                py += px + 1
                px = 0
                if py >= gh:
                    px += py - (gh - 1)
                    py = gh - 1
            else:
                px += 1
                py -= 1
        elif order == 1:
            if px == gw - 1:
                px, py = 0, py + 1
            else:
                px += 1
        elif py == gh - 1:
            px, py = px + 1, 0
        else:
            py += 1
    return tab


def scan_positions(w, h, scan):
    """Scan index -> (x, y) of the whole block."""
    sbs = 1 if (w == 2 or h == 2) else 2
    gw, gh = w >> sbs, h >> sbs
    cs = SCAN2[scan] if sbs == 1 else SCAN4[scan]
    out = []
    for sb in subblock_scan(scan, gw, gh):
        sy, sx = divmod(sb, gw)
        out += [((sx << sbs) + (c & ((1 << sbs) - 1)), (sy << sbs) + (c >> sbs)) for c in cs]
    return out


def last_pos_group(pos):
    g = 13
    while MIN_IN_GROUP[g] > pos:
        g -= 1
    return g


def quant_constants(bd, qp, w, h):
    lw, lh = log2(w), log2(h)
    qpb = max(qp + 6 * (bd - 8), 0)
    tshift = 15 - bd - ((lw + lh) >> 1)
    bias = (lw + lh) & 1
    shift = 14 + qpb // 6 + tshift
    return dict(
        qpb=qpb, tshift=tshift, bias=bias, shift=shift,
        scale=FWD[qpb % 6] * (181 if bias else 1), fq_shift=shift + (7 if bias else 0),
        cost_scale=15 - 2 * tshift - 2 * (bd - 8) + 2 * bias,
        iq_shift=6 - tshift + (8 if bias else 0),
        iq_scale=(INV[qpb % 6] << (qpb // 6)) * (181 if bias else 1))


def abs16(v):
    """(int16_t)abs(v) of an int16 v."""
    return -32768 if v == -32768 else abs(v)


def plain_level(k, v):
    """GetFwdQuantFunc on an int16 coefficient, the int16 the walk starts from."""
    q = (abs16(v) * k["scale"] + (1 << (k["fq_shift"] - 1))) >> k["fq_shift"]
    return ((q + 32768) & 0xffff) - 32768


def any_level(bd, qp, w, h, src):
    """rdoq_classify_kernel: does any coefficient (of the 32x32 corner) quantise to a level?"""
    k = quant_constants(bd, qp, w, h)
    return any(plain_level(k, v) != 0 for v in set(src[:32, :32].reshape(-1).tolist()))


def quant_rdo(ent, bd, qp, luma, scan, sign_hide, flags, w, h, src, c, lam, rdf, n):
    """RdoQuant::QuantRdo.  ent: the 128 entropy bits; qp: the component's raw QP; src: h rows
    of w python ints; c: the context snapshot, {field: list}; lam, rdf: xvcgpu_rdoq_params'
    lambda and rd_factor; n: the Counter.  Returns (non-zero levels, h rows of w levels), or
    None for a 2-wide block with NO_2X2 (QuantFast, not modelled)."""
    if (w == 2 or h == 2) and flags & NO_2X2:
        return None
    k_ = quant_constants(bd, qp, w, h)
    sbs = 1 if (w == 2 or h == 2) else 2
    sb_size, sb_mask = 1 << (2 * sbs), (1 << sbs) - 1
    gw, gh = w >> sbs, h >> sbs
    shift, scale, cost_scale = k_["shift"], k_["scale"], k_["cost_scale"]
    fq_shift, iq_shift, iq_scale, bias = k_["fq_shift"], k_["iq_shift"], k_["iq_scale"], k_["bias"]
    fq_offset = 1 << (fq_shift - 1)
    sb_bias_shift, sb_bias_off = (7, 64) if bias else (0, 0)
    cscan = SCAN2[scan] if sbs == 1 else SCAN4[scan]
    sb_scan = subblock_scan(scan, gw, gh)
    size = (log2(w) + log2(h)) >> 1
    sig_tab = c["sig_luma"] if luma else c["sig_chroma"]
    g_tab = c["greater1_luma"] if luma else c["greater1_chroma"]
    seen = [0] * 128

    def bits(state, b):
        seen[state] += 1
        return ent[state ^ b]

    def bit_cost(b):
        return (b * lam) >> 16

    # the levels being decided, two zeros of padding to the right and below: the template
    lv = [[0] * (w + 2) for _ in range(h + 2)]

    def template(x, y):
        r0, r1, r2 = lv[y], lv[y + 1], lv[y + 2]
        return r0[x + 1], r0[x + 2], r1[x + 1], r1[x], r2[x]

    def level_bits(level, c1_ctx, c2_ctx, c1_idx, c2_idx, rice, count=False):
        base = (2 + (c2_idx < 1)) if c1_idx < 8 else 1
        thr = RICE_RANGE[rice]
        b = BYPASS
        if level >= base:
            if count:
                if c1_idx >= 8:
                    n["g1_budget_spent"] += 1
                elif c2_idx >= 1:
                    n["g2_budget_spent"] += 1
            code = level - base
            if code < (thr << rice):
                b += ((code >> rice) + 1 + rice) * BYPASS
            else:
                if count:
                    n["escape_k%d" % rice if rice < 4 else "escape_k4_9"] += 1
                length = rice
                code -= thr << rice
                while code >= (1 << length):
                    code -= 1 << length
                    length += 1
                b += (length + thr + length + 1 - rice) * BYPASS
            if c1_idx < 8:
                b += bits(c1_ctx, 1)
                if c2_idx < 1:
                    b += bits(c2_ctx, 1)
        elif level == 1:
            b += bits(c1_ctx, 0)
        elif level == 2:
            b += bits(c1_ctx, 1) + bits(c2_ctx, 0)
        else:
            return 0
        return b

    def last_pos_bits(lx, ly):
        bw, bh = w, h
        if scan == 2:
            lx, ly, bw, bh = ly, lx, h, w
            n["lastpos_swapped"] += 1
        total = 0
        for is_x, pos, sz in ((True, lx, bw), (False, ly, bh)):
            if luma:
                l2 = log2(sz)
                tab = c["last_x_luma"] if is_x else c["last_y_luma"]
                ctx_of = lambda p: tab[[0, 0, 0, 3, 6, 10, 15, 21][l2] + (p >> ((l2 + 1) >> 2))]
            else:
                tab = c["last_x_chroma"] if is_x else c["last_y_chroma"]
                sh = min(sz >> 3, 2)
                ctx_of = lambda p: tab[p >> sh]
                if sz >= 4:
                    n["chroma_last_%d" % sz] += 1
            g = last_pos_group(pos)
            for p in range(g):
                total += bits(ctx_of(p), 1)
            if g < last_pos_group(sz - 1):
                total += bits(ctx_of(g), 0)
            if g > 3:
                total += ((g - 2) >> 1) * BYPASS
                n["lastpos_suffix_x" if is_x else "lastpos_suffix_y"] += 1
        return total

    n_el = w * h
    sb_csbf = [0] * (gw * gh)
    csbf_bits_to_zero = [0] * (gw * gh)
    cost_to_zero = [0] * n_el
    sig_bits_arr = [0] * n_el
    err_dist = [0] * n_el
    sig_rate = [0] * n_el
    rate_up = [0] * n_el
    rate_down = [0] * n_el
    last_pos_index = -1
    comp_zero_dist = comp_code_cost = 0

    for sbi in range(gw * gh - 1, -1, -1):
        sb_index = sbi << (2 * sbs)
        sb_pos = sb_scan[sbi]
        sb_y, sb_x = divmod(sb_pos, gw)
        c1_idx = c2_idx = 0
        sb_zero_dist = sb_code_cost = 0
        right = sb_csbf[sb_y * gw + sb_x + 1] if sb_x < gw - 1 else 0
        below = sb_csbf[(sb_y + 1) * gw + sb_x] if sb_y < gh - 1 else 0
        csbf_ctx = c["csbf"][0 if luma else 1][right | below]
        num_non_zero = 0
        for k in range(sb_size - 1, -1, -1):
            index = sb_index + k
            x, y = (sb_x << sbs) + (cscan[k] & sb_mask), (sb_y << sbs) + (cscan[k] >> sbs)
            s_ = src[y][x]
            abs_coeff = abs16(s_)
            zero_cost = (abs_coeff * abs_coeff) << cost_scale
            sb_zero_dist += zero_cost
            q = ((((abs_coeff * scale + fq_offset) >> fq_shift) + 32768) & 0xffff) - 32768
            if q and last_pos_index == -1:
                last_pos_index = index
            elif last_pos_index == -1:
                sb_code_cost += zero_cost
                continue
            is_last = index == last_pos_index
            assert not (is_last and abs_coeff < 0), "a last coefficient of -32768: not modelled"
            if s_ == 32767:
                n["src_32767"] += 1
            elif s_ == -32767:
                n["src_m32767"] += 1
            elif s_ == -32768:
                n["src_m32768"] += 1
            t = template(x, y)
            posxy = x + y
            nsig = sum(1 for v in t if v)
            start = (6 if posxy < 2 else 0) + (6 if luma and posxy < 5 else 0) + \
                ((18 << min(1, size - 3)) if size > 2 and luma else 0)
            sig_ctx = sig_tab[start + min(nsig, 5)]
            if is_last:
                c1_ctx = c2_ctx = g_tab[0]
            else:
                gstart = (10 if posxy < 3 else (5 if posxy < 10 else 0)) if luma else 0
                c1_ctx = g_tab[gstart + min(sum(1 for v in t if v > 1), 4) + 1]
                c2_ctx = g_tab[gstart + min(sum(1 for v in t if v > 2), 4) + 1]
            thr = 4 + sum(t) - nsig
            rice = 9
            for kk in range(10):
                if (1 << (kk + 3)) > thr:
                    rice = kk
                    break
            sig0, sig1 = bits(sig_ctx, 0), bits(sig_ctx, 1)
            if is_last:
                sig1 = 0
            elif sb_index > 0 and k == 0 and num_non_zero == 0:
                sig1 = 0
                n["sig_inferred"] += 1
            best_cost, best_sig, best_level = I64_MAX, 0, q
            if q > 0:
                best_sig = sig1
                bc, bl = I64_MAX, q
                for lvl in ((q - 1, q) if q > 1 else (q,)):
                    b = sig1 + level_bits(lvl, c1_ctx, c2_ctx, c1_idx, c2_idx, rice)
                    prod = lvl * iq_scale
                    assert prod <= I32_MAX, "level * inverse scale beyond 31 bits: not modelled"
                    if iq_shift > 0:
                        deq = (prod + (1 << (iq_shift - 1))) >> iq_shift
                    else:
                        deq = prod << -iq_shift
                        n["iq_shift_left"] += 1
                    if deq > 32767:
                        deq = 32767
                        n["deq_clip"] += 1
                    err = abs_coeff - deq
                    cost = ((err * err) << cost_scale) + bit_cost(b)
                    if lvl == q - 1 or cost <= bc:
                        if lvl == q and q > 1 and cost == bc:
                            n["tie_qm1_q"] += 1
                        bc, bl = cost, lvl
                best_cost, best_level = bc, bl
            if not is_last and q < 3:
                cost = zero_cost + bit_cost(sig0)
                if cost <= best_cost:
                    if cost == best_cost:
                        n["tie_zero_level"] += 1
                    best_cost, best_sig, best_level = cost, sig0, 0
            if q == 1:
                n["q1_to_%d" % best_level] += 1
            elif q == 2:
                n["q2_to_%d" % best_level] += 1
            elif q > 2:
                n["q3up_kept" if best_level == q else "q3up_to_qm1"] += 1
            lv[y][x] = best_level
            cost_to_zero[index] = zero_cost - best_cost
            sig_bits_arr[index] = best_sig
            sb_code_cost += best_cost
            orig_scaled = (abs_coeff * scale + sb_bias_off) >> sb_bias_shift
            quant_err = orig_scaled - (best_level << shift)
            err_dist[index] = (((quant_err >> (shift - 8)) + 32768) & 0xffff) - 32768
            sig_rate[index] = (sig1 - sig0) if not is_last else 0
            if best_level:
                sb_csbf[sb_pos] = 1
                num_non_zero += 1
                n["rice_k%d" % rice if rice < 5 else ("rice_k9_cap" if rice == 9 else "rice_k5_8")] += 1
                a = (c1_ctx, c2_ctx, c1_idx, c2_idx, rice)
                lvl_rate = level_bits(best_level, *a, count=True)
                rate_up[index] = -lvl_rate + level_bits(best_level + 1, *a)
                rate_down[index] = -lvl_rate + level_bits(best_level - 1, *a)
            else:
                rate_up[index] = bits(c1_ctx, 0)
            # UpdateCodeState (the rice parameter is the template's at the next coefficient)
            base = (2 + (c2_idx < 1)) if c1_idx < 8 else 1
            if best_level >= 1:
                c1_idx += 1
            if best_level >= 2:
                c2_idx += 1
            if best_level >= base and best_level > 3 * (1 << rice) and rice >= 4:
                n["rice_update_cap4"] += 1

        # EvalZeroSubblock
        zero_sb = False
        if last_pos_index < 0 or sb_index == 0 or sb_index + sb_size > last_pos_index:
            csbf_bits_to_zero[sb_pos] = 0
        else:
            z_bits, c_bits = bits(csbf_ctx, 0), bits(csbf_ctx, 1)
            zero_cost = sb_zero_dist + bit_cost(z_bits)
            if sb_csbf[sb_pos]:
                code_cost = sb_code_cost + bit_cost(c_bits)
                if zero_cost < code_cost:
                    sb_code_cost, zero_sb = zero_cost, True
                    csbf_bits_to_zero[sb_pos] = z_bits
                    n["sb_zeroed"] += 1
                else:
                    sb_code_cost = code_cost
                    csbf_bits_to_zero[sb_pos] = c_bits
                    n["sb_kept"] += 1
            else:
                sb_code_cost = zero_cost
                csbf_bits_to_zero[sb_pos] = z_bits
                n["sb_empty"] += 1
        if zero_sb:
            sb_csbf[sb_pos] = 0
            for k in range(sb_size):
                lv[(sb_y << sbs) + (cscan[k] >> sbs)][(sb_x << sbs) + (cscan[k] & sb_mask)] = 0
                cost_to_zero[sb_index + k] = 0
        comp_code_cost += sb_code_cost
        comp_zero_dist += sb_zero_dist

    def fold_states():
        for s_, cnt in enumerate(seen):
            if cnt:
                n["ctx_mps_%d" % (s_ & 1)] += cnt
                if s_ >> 1 == 0:
                    n["ctx_state_0"] += cnt
                elif s_ >> 1 >= 62:
                    n["ctx_state_62_63"] += cnt

    zeros = [[0] * w for _ in range(h)]
    if last_pos_index < 0:
        fold_states()
        return 0, zeros

    # EvalLastPos
    cbf_ctx = c["cbf_chroma"] if not luma else (c["cbf_luma"] if flags & INTRA_CU else c["root_cbf"])
    comp_code_cost += bit_cost(bits(cbf_ctx, 1))
    first_last = last_pos_index
    start = last_pos_index % sb_size
    best_cost, best_last_plus1, stop = I64_MAX, 0, False
    for sbi in range(gw * gh - 1, -1, -1):
        if stop:
            break
        sb_index = sbi << (2 * sbs)
        if sb_index > last_pos_index:
            continue
        sb_pos = sb_scan[sbi]
        sb_y, sb_x = divmod(sb_pos, gw)
        comp_code_cost -= bit_cost(csbf_bits_to_zero[sb_pos])
        if not sb_csbf[sb_pos]:
            continue
        for k in range(start, -1, -1):
            index = sb_index + k
            x, y = (sb_x << sbs) + (cscan[k] & sb_mask), (sb_y << sbs) + (cscan[k] >> sbs)
            v = lv[y][x]
            if index == 0:
                n["last_reach_dc"] += 1
            if not v:
                comp_code_cost += cost_to_zero[index]
                continue
            cost = comp_code_cost + bit_cost(last_pos_bits(x, y)) - bit_cost(sig_bits_arr[index])
            if cost < best_cost:
                best_cost, best_last_plus1 = cost, index + 1
            if v > 1:
                stop = True
                n["last_stop_gt1"] += 1
                break
            comp_code_cost += cost_to_zero[index]
        start = sb_size - 1
    comp_zero_cost = comp_zero_dist + bit_cost(bits(cbf_ctx, 0))
    fold_states()
    if comp_zero_cost < best_cost:
        n["block_zeroed"] += 1
        return 0, zeros
    last_pos_index = best_last_plus1
    n["last_stays" if best_last_plus1 - 1 == first_last else "last_moved"] += 1

    # what lies beyond the new last position ("plus 1": the coefficient at it is kept)
    last_sb_index = last_pos_index - (last_pos_index & (sb_size - 1))
    for sbi in range(gw * gh - 1, -1, -1):
        sb_index = sbi << (2 * sbs)
        if sb_index < last_sb_index:
            break
        sb_y, sb_x = divmod(sb_scan[sbi], gw)
        end = last_pos_index % sb_size if sb_index == last_sb_index else 0
        for k in range(sb_size - 1, end - 1, -1):
            lv[(sb_y << sbs) + (cscan[k] >> sbs)][(sb_x << sbs) + (cscan[k] & sb_mask)] = 0
    out = [[(-lv[y][x] if src[y][x] < 0 else lv[y][x]) for x in range(w)] for y in range(h)]
    nnz = sum(1 for row in out for v in row if v)
    if sbs == 1:
        return nnz, out
    if not sign_hide:
        if nnz > 1:
            n["sh_off"] += 1
        return nnz, out
    if nnz <= 1:
        n["sh_single_level"] += 1
        return nnz, out

    # CoeffSignHideRdo
    nnz = 0
    is_last_sb = -1
    for sbi in range(gw * gh - 1, -1, -1):
        sb_index = sbi << 4
        sb_y, sb_x = divmod(sb_scan[sbi], gw)
        pos = [((sb_x << 2) + (cscan[k] & 3), (sb_y << 2) + (cscan[k] >> 2)) for k in range(16)]
        first, last, total = 16, -1, 0
        for k in range(15, -1, -1):
            v = out[pos[k][1]][pos[k][0]]
            if v:
                first = min(first, k)
                last = max(last, k)
                total += v
                nnz += 1
        if last >= 0 and is_last_sb == -1:
            is_last_sb = 1
        if last - first < 4:
            if last - first == 3:
                n["sh_dist_3"] += 1
            if is_last_sb == 1:
                is_last_sb = 0
            continue
        if last - first == 4:
            n["sh_dist_4"] += 1
        first_sign = 0 if out[pos[first][1]][pos[first][0]] > 0 else 1
        if first_sign == (total & 1):
            n["sh_parity_ok"] += 1
            if is_last_sb == 1:
                is_last_sb = 0
            continue
        n["sh_parity_fix"] += 1
        n["sh_in_last_sb" if is_last_sb == 1 else "sh_in_later_sb"] += 1
        best_cost, best_delta, best_k, best_kind = I64_MAX, 0, -1, None
        barred_min = I64_MAX
        for k in range(last if is_last_sb == 1 else 15, -1, -1):
            index = sb_index + k
            x, y = pos[k]
            lvl = out[y][x]
            if lvl:
                cost_inc = rdf * -err_dist[index] + rate_up[index]
                cost_dec = rdf * err_dist[index] + rate_down[index] - \
                    (sig_rate[index] if abs(lvl) == 1 else 0)
                if is_last_sb == 1 and k == last and abs(lvl) == 1:
                    cost_dec -= 4 * BYPASS
                    n["sh_last_sb_bonus"] += 1
                if cost_inc < cost_dec:
                    cost, delta, kind = cost_inc, 1, "sh_adj_inc"
                else:
                    delta, cost = -1, cost_dec
                    kind = "sh_adj_1_to_0" if abs(lvl) == 1 else "sh_adj_dec"
                    if k == first and abs(lvl) == 1:
                        n["sh_first_barred"] += 1
                        barred_min = min(barred_min, cost)
                        cost = I32_MAX
            else:
                cost = rdf * -abs(err_dist[index]) + rate_up[index] + sig_rate[index] + BYPASS
                delta = 1
                kind = "sh_adj_zero_below_first" if k < first else "sh_adj_zero_above_last"
                if k < first and (0 if src[y][x] >= 0 else 1) != first_sign:
                    n["sh_barred_sign"] += 1
                    barred_min = min(barred_min, cost)
                    cost = I32_MAX
            if cost < best_cost:
                best_cost, best_delta, best_k, best_kind = cost, delta, k, kind
        if barred_min < best_cost:
            n["sh_bar_decides"] += 1
        n[best_kind] += 1
        x, y = pos[best_k]
        o = out[y][x]
        if o == 32767 or o == -32768:
            best_delta = -1
            n["sh_saturated"] += 1
        if not o:
            nnz += 1
        o = o + best_delta if src[y][x] >= 0 else o - best_delta
        out[y][x] = o
        if not o:
            nnz -= 1
        if is_last_sb == 1:
            is_last_sb = 0
    return nnz, out


def new_census():
    return collections.Counter()
