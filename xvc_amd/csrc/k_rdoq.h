// k_rdoq.h -- Q2 / N2: RdoQuant::QuantRdo with CoeffSignHideRdo
// (xvc_enc_lib/rdo_quant.cc:203-446, :575-687; QuantCoeffRdo :689-720,
// EvalZeroSubblock :722-760, EvalLastPos :762-832, GetAbsLevelBits :834-878,
// UpdateCodeState :880-898, GetLastPosBits :900-947) and the context selection
// it calls (xvc_common_lib/cabac.cc:491-770, extended residual context set) -
// the quantiser the reference's encoder always runs (encoder_settings.h:59).
//
// One WAVE per transform block.  The reference walks the coefficients in
// reverse scan order, one at a time; what that order really constrains is:
//   * a coefficient's contexts read the decided levels of five neighbours to
//     its right / below (cabac.cc:535-552): up to 2 samples away, i.e. inside
//     its own 4x4 sub-block or the sub-blocks right / below / diagonal;
//   * the sub-block's coded flag context reads the flags of the sub-blocks to
//     its right and below (cabac.cc:491-518);
//   * inside a sub-block the greater1 / greater2 flag budget (c1_idx, c2_idx)
//     runs along the scan;
//   * the "last position" is the first non-zero quantised value in reverse
//     scan - a function of the input alone.
// With the extended context set nothing else crosses sub-blocks (ctx_set / c1
// only feed the non-extended contexts).  So: lane = 4x4 sub-block; the
// sub-blocks of one anti-diagonal of the sub-block grid are independent and
// run together, each lane walking its 16 coefficients in scan order - 7 steps
// for a 16x16 block instead of 16 - and every sum the reference accumulates
// along the way (int64) is formed by an order-free reduction afterwards.
// EvalLastPos is a short serial walk (it stops at the first level above 1) on
// lane 0; zero-out, re-signing and the sign-data hiding (independent per
// sub-block) are lane-parallel again.
//
// 64-point transforms only have coefficients in their 32x32 low-frequency
// corner (transform.cc:1458): the other sub-blocks matter only through the
// cost of their (zero) coded flags, which is added in closed form.
#ifndef XVCGPU_K_RDOQ_H_
#define XVCGPU_K_RDOQ_H_

#include "dev_common.h"
#include "k_me.h"
#include "k_me2.h"
#include "k_quant.h"
#include "k_rdoq4.h"
#include "k_rdoq_common.h"
#include "k_scan.h"
#include "xvcgpu_internal.h"

// G lanes quantise one block: G = 64 (one block per wave), or 32 / 16 / 4 (the
// blocks of a wave side by side - `s`, cf, lev, the contexts and parameters
// are then per-lane values of the lane's own group).  cf(x, y) reads a
// transform coefficient, lev(x, y) addresses the level array (both only inside
// the region); `lane` is 0..G-1 and all G lanes must call.  Returns the number
// of non-zero levels (to every lane); levels outside the region are NOT
// written (they are zero: the caller clears what its layout needs).
// S: the scratch - RdoqShared<N> or RdoqView (the same members as pointers).
//
// What is serial and what is not.  A coefficient whose plain quantised value q
// is 0 has no choice to make (rdo_quant.cc:404-411 leaves it at level 0); it
// adds nothing to a neighbour's template nor to the sub-block's c1 / c2 budget,
// it only COSTS (its zero distortion + the bits of a zero significance flag in
// the context its decided neighbours select) and leaves the records the later
// passes read.  So a sub-block is done in three steps:
//   1. its owner lane walks the q > 0 coefficients in scan order and decides
//      them (on real content: one or two per block);
//   2. all G lanes share out the q == 0 coefficients of the sub-blocks of the
//      current anti-diagonal: costs (summed per sub-block by DPP adds) and
//      records, every template now final;
//   3. the owner evaluates the zero-sub-block choice (EvalZeroSubblock).
// The first version walked all 16 coefficients of a sub-block on its owner
// lane, ~450 instructions each at the ~5 clocks per instruction of a lone wave
// with four busy lanes: 0.1 ms for a 16x16 block and the slowest block is the
// kernel's duration.
//
// The sign hiding's rate_up / rate_down of a coefficient with a non-zero level
// (three GetAbsLevelBits evaluations) are formed when - and if - the sign
// hiding asks for them: rate_up[] then holds the coefficient's decision-time
// state (RQ_STATE_*), rate_down[] does not exist.

template <int G = 64, typename S, typename CF, typename LEV>
__device__ __forceinline__ int wave_rdoq(S &s, int lane, const BlockQuant &bq, int w, int h,
                                         bool luma, int scan_order, bool sign_hide,
                                         const xvcgpu_rdoq_contexts &ctx,
                                         const xvcgpu_rdoq_params &prm, CF cf, LEV lev,
                                         bool stage_ctx = true, bool clear_levels = true) {
  const int sbs = (w == 2 || h == 2) ? 1 : 2;
  const int sb_size = 1 << (2 * sbs);
  const int gw = w >> sbs, gh = h >> sbs;                   // the whole grid (scan indices)
  const int rw = w < 32 ? w : 32, rh = h < 32 ? h : 32;     // coefficients exist here
  const int rgw = rw >> sbs, rgh = rh >> sbs;
  const int size_cls = (rq_log2(w) + rq_log2(h)) >> 1;
  const long long lambda = prm.lambda;

  const bool mine = lane < rgw * rgh;
  const int sx = mine ? lane % rgw : 0, sy = mine ? lane / rgw : 0;
  const int my_scan = d_sb_scan_index(scan_order, gw, gh, sx, sy);
  const int sb_index = my_scan << (2 * sbs);
  const int px = sx << sbs, py = sy << sbs;
  auto coeff_xy = [&](int k, int &x, int &y) {
    const int p = rq_scan_pos(sbs, scan_order, k);
    x = px + (p & 3);
    y = py + (p >> 2);
  };
  // where a coefficient's records live (RQ_SB_STRIDE): sub-block major
  auto rec_pos = [&](int x, int y) {
    return sbs == 2 ? ((y >> 2) * rgw + (x >> 2)) * RQ_SB_STRIDE + (((y & 3) << 2) | (x & 3))
                    : y * rw + x;
  };
  // the template of decided neighbours (cabac.cc:535-552): five reads issued
  // together (clamped addresses, masked values) - inside the region; beyond it
  // every level is 0
  auto neighbours = [&](int x, int y, int &n_sig, int &n_g1, int &n_g2, int &sum_abs) {
    const int x1 = x + 1 < rw ? x + 1 : x, x2 = x + 2 < rw ? x + 2 : x;
    const int y1 = y + 1 < rh ? y + 1 : y, y2 = y + 2 < rh ? y + 2 : y;
    const int v0 = *lev(x1, y), v1 = *lev(x2, y), v2 = *lev(x1, y1), v3 = *lev(x, y1),
              v4 = *lev(x, y2);
    const bool m0 = x + 1 < rw, m1 = x + 2 < rw, m2 = m0 && y + 1 < rh, m3 = y + 1 < rh,
               m4 = y + 2 < rh;
    n_sig = n_g1 = n_g2 = sum_abs = 0;
    auto nb = [&](int v, bool m) {
      v = m ? d_abs(v) : 0;
      n_sig += v != 0;
      n_g1 += v > 1;
      n_g2 += v > 2;
      sum_abs += v;
    };
    nb(v0, m0); nb(v1, m1); nb(v2, m2); nb(v3, m3); nb(v4, m4);
  };
  auto sig_ctx_of = [&](int posxy, int n_sig) {
    return rq_sig_ctx_base(luma, posxy, size_cls) + 2 * (n_sig < 5 ? n_sig : 5);
  };
  auto greater_ctx_nn = [&](int posxy, int nn) { return rq_greater_ctx(luma, posxy, nn); };

  // The last position: the first non-zero quantised value in reverse scan; every
  // sub-block's sum of zero costs (what a sub-block beyond the last position
  // contributes - to both totals, rdo_quant.cc:295-307 - and all it needs: its
  // levels are zero and nothing reads its per-coefficient records); and the set
  // of its coefficients that have a decision to make.
  int last = -1;
  unsigned qmask = 0;
  long long my_zero_dist = 0;
  if (mine) {
    // sum of zero_dist(a) = (sum of a * a) << cost_scale: cost_scale = 1 + 2 * (the
    // block's size class) + 2 * bias > 0, a * a < 2^31
    unsigned long long sum_sq = 0;
    for (int k = sb_size - 1; k >= 0; k--) {
      int x, y;
      coeff_xy(k, x, y);
      const int a = (short)d_abs(cf(x, y));
      sum_sq += (unsigned)(a * a);
      if (bq.fwd(a)) {
        qmask |= 1u << k;
        if (last < 0) last = sb_index + k;
      }
      if (clear_levels) *lev(x, y) = 0;   // (a caller that staged zero levels says so)
    }
    my_zero_dist = (long long)(sum_sq << bq.cost_scale);
  }
  const int last_pos_index = rq_wave_max_i32<G>(last);
  RQ_TRACE(4);
  if (last_pos_index < 0) return 0;  // nothing quantises to a level (most blocks)

  // every context's two bin costs into LDS
  if (stage_ctx) {
    const unsigned char *cbytes = reinterpret_cast<const unsigned char *>(&ctx);
    for (int i = lane; i < (int)sizeof(xvcgpu_rdoq_contexts); i += G) {
      const unsigned char st8 = cbytes[i] & 127;
      s.ctx_bits[2 * i] = kEntropyBits[st8];
      s.ctx_bits[2 * i + 1] = kEntropyBits[st8 ^ 1];
    }
  }
  const unsigned *cb = s.ctx_bits;
  // scan index -> sub-block (whole grid), for EvalLastPos
  for (int t = lane; t < gw * gh; t += G)
    s.sb_of_scan[d_sb_scan_index(scan_order, gw, gh, t % gw, t / gw)] = (unsigned char)t;
  // a sub-block is "live" when the walk reaches it at or before the last position
  const bool live = mine && sb_index <= last_pos_index;
  // the two costs of a coefficient's significance flag as the decision used them
  // (sig1 = 0 for the last position and for the k = 0 coefficient of a sub-block
  // that was empty up to it, rdo_quant.cc:343), and its rate sig1 - sig0 (0 at and
  // beyond the last position: :303-307)
  auto sig_pair = [&](unsigned pk, int posxy, int index, int k, bool dcz, unsigned &sig0,
                      unsigned &sig1) {
    const uint2 b2 =
        *reinterpret_cast<const uint2 *>(cb + sig_ctx_of(posxy, (int)((pk >> 12) & 7u)));
    sig0 = b2.x;
    sig1 = (index == last_pos_index || (k == 0 && dcz)) ? 0u : b2.y;
  };
  auto sig_rate_of = [&](unsigned pk, int posxy, int index, int k, bool dcz) {
    if (index >= last_pos_index) return 0;
    unsigned sig0, sig1;
    sig_pair(pk, posxy, index, k, dcz, sig0, sig1);
    return (int)(sig1 - sig0);
  };
  // the greater1 / greater2 flag costs and the budget state of a decided
  // coefficient from its 16-bit record
  auto state_of = [&](unsigned pk, int posxy, RdoqFlagBits &fb, RdoqCoeffState &st) {
    const uint2 c1_b =
        *reinterpret_cast<const uint2 *>(cb + greater_ctx_nn(posxy, (int)(pk & 7u)));
    const uint2 c2_b =
        *reinterpret_cast<const uint2 *>(cb + greater_ctx_nn(posxy, (int)((pk >> 3) & 7u)));
    fb.c1_0 = c1_b.x; fb.c1_1 = c1_b.y; fb.c2_0 = c2_b.x; fb.c2_1 = c2_b.y;
    st.c1_idx = (pk >> 6) & 1u ? 8 : 0;
    st.c2_idx = (int)((pk >> 7) & 1u);
    st.golomb_rice_k = (pk >> 8) & 15u;
  };
  // coeff_cost_to_zero_[index] (rdo_quant.cc:350, :307) of a coefficient whose
  // sub-block is coded, recomputed: zero_cost - best_cost of the decision that
  // left it at level v.  A level of 0 - chosen, or without a choice - cost a zero
  // significance flag: -sig0.  A non-zero level cost its distortion + sig1 + the
  // level's bits in the state the decision saw.  (v < 0: a magnitude of 32768
  // wrapped, no candidate was priced and best_cost stayed at its initial value.)
  auto ctz_of = [&](unsigned pk, int posxy, int index, int k, bool dcz, int abs_coeff,
                    int v) -> long long {
    unsigned sig0, sig1;
    sig_pair(pk, posxy, index, k, dcz, sig0, sig1);
    if (v == 0) return -rq_bit_cost(sig0, lambda);
    const long long zero_cost = bq.zero_dist(abs_coeff);
    if (v < 0) return zero_cost - 0x7fffffffffffffffll;
    RdoqFlagBits fb;
    RdoqCoeffState st;
    state_of(pk, posxy, fb, st);
    const unsigned bits = sig1 + rq_abs_level_bits(fb, v, st);
    const int err = abs_coeff - bq.dequant(v);
    return zero_cost - (bq.dist(err) + rq_bit_cost(bits, lambda));
  };
  if (mine) {
    s.csbf[lane] = 0;
    s.sb_dcz[lane] = 0;
    s.sb_live[lane] = live ? 1 : 0;
    if (!live) {
      s.csbf_bits[lane] = 0;
      s.sb_code_cost[lane] = my_zero_dist;
    }
  }
  // the sub-block (region index) and offset of the last position
  const int last_k = last_pos_index & (sb_size - 1);
  const int last_l = rq_wave_max_i32<G>(mine && (last_pos_index >> (2 * sbs)) == my_scan ? lane
                                                                                          : -1);
  // the wavefront starts at the highest anti-diagonal that holds a live sub-block
  const int d_first = rq_wave_max_i32<G>(live ? sx + sy : -1);
  wave_sync();
  RQ_TRACE(5);

  // ---- one anti-diagonal of sub-blocks at a time
  RQ_STEP_BEGIN();
  for (int d = d_first; d >= 0; d--) {
    const bool act = live && sx + sy == d;
    bool any = false;
    RQ_STEP(3);
    // step 1: the owner decides the coefficients that have a choice
    if (act) {
      RdoqCoeffState st = {0, 0, 0};
      long long code_cost = 0;
      int num_non_zero = 0;
      unsigned m = qmask;
      while (m) {
        const int k = 31 - __clz((int)m);
        m ^= 1u << k;
        const int index = sb_index + k;
        int x, y;
        coeff_xy(k, x, y);
        const int pos = rec_pos(x, y);
        const int abs_coeff = (short)d_abs(cf(x, y));
        const long long zero_cost = bq.zero_dist(abs_coeff);
        const int q = bq.fwd(abs_coeff);
        const bool is_last = index == last_pos_index;
        int n_sig, n_g1, n_g2, sum_abs;
        neighbours(x, y, n_sig, n_g1, n_g2, sum_abs);
        const int posxy = x + y;
        const int sig_ctx = sig_ctx_of(posxy, n_sig);
        const int nn1 = rq_greater_nn(n_g1, is_last), nn2 = rq_greater_nn(n_g2, is_last);
        const int c1_ctx = greater_ctx_nn(posxy, nn1);
        const int c2_ctx = greater_ctx_nn(posxy, nn2);
        {  // GetCoeffGolombRiceK (cabac.cc:686-725): smallest k with 2^(k+3) > threshold
          const unsigned threshold = 4u + (unsigned)(sum_abs - n_sig);
          const int kk = 29 - __clz((int)threshold);  // floor(log2) - 2
          st.golomb_rice_k = (unsigned)(kk < 0 ? 0 : (kk > 9 ? 9 : kk));
        }
        // the six context costs of this coefficient: three 8-byte reads, together
        const uint2 sig_b = *reinterpret_cast<const uint2 *>(cb + sig_ctx);
        const uint2 c1_b = *reinterpret_cast<const uint2 *>(cb + c1_ctx);
        const uint2 c2_b = *reinterpret_cast<const uint2 *>(cb + c2_ctx);
        const RdoqFlagBits fb = {c1_b.x, c1_b.y, c2_b.x, c2_b.y};
        const unsigned sig0 = sig_b.x;
        unsigned sig1 = sig_b.y;
        const bool dc_sig_zero = sb_index > 0 && k == 0 && num_non_zero == 0;
        if (is_last || dc_sig_zero) sig1 = 0;

        // QuantCoeffRdo (rdo_quant.cc:689-720)
        // (a magnitude of 32768 wraps to a negative q, as in the reference: no
        // candidate but zero)
        long long best_cost = 0x7fffffffffffffffll;
        int best_level = q;
        if (q > 0) {
          for (int lvl = q > 1 ? q - 1 : q; lvl <= q; lvl++) {
            const unsigned bits = sig1 + rq_abs_level_bits(fb, lvl, st);
            const int err = abs_coeff - bq.dequant(lvl);
            const long long cost =
                bq.dist(err) + rq_bit_cost(bits, lambda);
            if (lvl == q - 1 || cost <= best_cost) {
              best_cost = cost;
              best_level = lvl;
            }
          }
        }
        if (!is_last && q < 3) {
          const long long cost = zero_cost + rq_bit_cost(sig0, lambda);
          if (cost <= best_cost) {
            best_cost = cost;
            best_level = 0;
          }
        }
        *lev(x, y) = (short)best_level;
        if (dc_sig_zero) s.sb_dcz[lane] = 1;
        code_cost += best_cost;
        if (best_level) {
          any = true;
          num_non_zero++;
        }
        s.rate_up[pos] = RQ_STATE_PACK(nn1, nn2, st.c1_idx, st.c2_idx, st.golomb_rice_k,
                                       n_sig < 5 ? n_sig : 5);
        // UpdateCodeState (rdo_quant.cc:880-898); golomb_rice_k is re-derived
        if (best_level >= 1) st.c1_idx++;
        if (best_level >= 2) st.c2_idx++;
      }
      s.sb_code_cost[lane] = code_cost;
      // EvalZeroSubblock replaces the code cost of a sub-block without a level by
      // its zero cost (:745-749; not for the first and the last sub-block, :729),
      // and nothing reads the records of such a sub-block afterwards (it is not
      // coded): its coefficients without a choice need not be priced at all.  On
      // real content that is most live sub-blocks.
      if (!any && !(sb_index == 0 || sb_index + sb_size > last_pos_index)) s.sb_live[lane] = 4;
    }
    wave_sync();
    RQ_STEP(0);
    // step 2: the coefficients without a choice, dealt over the group's lanes:
    // SEG lanes share a sub-block in every round; their costs are summed by
    // shuffles and added by the segment's first lane (16 lanes adding to one LDS
    // word with 64-bit atomics serialised)
    {
      const int ax0 = d > rgh - 1 ? d - (rgh - 1) : 0;
      const int ax1 = d < rgw - 1 ? d : rgw - 1;
      const int pairs = (ax1 - ax0 + 1) << (2 * sbs);
      constexpr int SEG = G < 16 ? G : 16;
      for (int t0 = 0; t0 < pairs; t0 += G) {
        const int t = t0 + lane;
        const bool in = t < pairs;
        const int ax = ax0 + ((in ? t : 0) >> (2 * sbs)), ay = d - ax, k = t & (sb_size - 1);
        const int l2 = ay * rgw + ax;
        long long cost = 0;
        if (in && s.sb_live[l2] == 1) {
          const int p = rq_scan_pos(sbs, scan_order, k);
          const int x = (ax << sbs) + (p & 3), y = (ay << sbs) + (p >> 2);
          const int pos = rec_pos(x, y);
          const int abs_coeff = (short)d_abs(cf(x, y));
          if (!bq.codes(abs_coeff)) {  // (else: decided in step 1)
            cost = bq.zero_dist(abs_coeff);
            if (l2 == last_l && k > last_k) {  // rdo_quant.cc:303-307 (+ the memsets :262-265)
              s.rate_up[pos] = (unsigned short)RQ_STATE_NO_RATE;
            } else {
              int n_sig, n_g1, n_g2, sum_abs;
              neighbours(x, y, n_sig, n_g1, n_g2, sum_abs);
              const int sig_ctx2 = sig_ctx_of(x + y, n_sig);
              cost += rq_bit_cost(cb[sig_ctx2], lambda);
              // (the k == 0 coefficient of an otherwise empty sub-block codes no flag,
              // sig1 = 0 at rdo_quant.cc:343; nothing reads the rate of such a sub-block)
              s.rate_up[pos] = RQ_STATE_PACK(rq_greater_nn(n_g1, false), 0, 0, 0, 0,
                                             n_sig < 5 ? n_sig : 5);
            }
          }
        }
        // (sb_size < SEG only for 2x2 sub-blocks: then a segment is one sub-block too)
        if (sbs == 2) {
          cost = rq_group_sum_i64<SEG>(cost);
          if ((lane & (SEG - 1)) == 0 && in && cost) s.sb_code_cost[l2] += cost;
        } else {
          cost = rq_group_sum_i64<4>(cost);
          if ((lane & 3) == 0 && in && cost) s.sb_code_cost[l2] += cost;
        }
      }
    }
    wave_sync();
    RQ_STEP(1);
    // step 3: EvalZeroSubblock (rdo_quant.cc:722-760)
    bool zeroed = false;
    if (act) {
      long long sb_code_cost = s.sb_code_cost[lane];
      const long long sb_zero_dist = my_zero_dist;
      // GetSubblockCsbfCtx (cabac.cc:491-518); sub-blocks beyond the region are zero
      const bool right = sx < rgw - 1 ? s.csbf[lane + 1] != 0 : false;
      const bool below = sy < rgh - 1 ? s.csbf[lane + rgw] != 0 : false;
      const int csbf_ctx = 2 * (RQ_OFF(csbf) + (luma ? 0 : 2) + ((right || below) ? 1 : 0));
      unsigned bits_to_zero = 0;
      bool zero_sb = false;
      if (!(sb_index == 0 || sb_index + sb_size > last_pos_index)) {
        const unsigned z_bits = cb[csbf_ctx], c_bits = cb[csbf_ctx + 1];
        const long long zero_cost = sb_zero_dist + rq_bit_cost(z_bits, lambda);
        if (any) {
          const long long code_cost = sb_code_cost + rq_bit_cost(c_bits, lambda);
          if (zero_cost < code_cost) {
            sb_code_cost = zero_cost;
            bits_to_zero = z_bits;
            zero_sb = true;
          } else {
            sb_code_cost = code_cost;
            bits_to_zero = c_bits;
          }
        } else {
          sb_code_cost = zero_cost;
          bits_to_zero = z_bits;
        }
      }
      if (zero_sb) {
        any = false;
        zeroed = true;
        s.sb_live[lane] = 2;   // its levels and zero costs are cleared by all lanes below
      }
      s.csbf[lane] = any ? 1 : 0;
      s.csbf_bits[lane] = bits_to_zero;
      s.sb_code_cost[lane] = sb_code_cost;
    }
    wave_sync();
    // the sub-blocks of this diagonal that were just zeroed: their 16 levels and
    // zero costs, one coefficient per lane and step (the owner alone took 16
    // steps of two writes) - when a lane of the wave zeroed one at all
    if (__ballot(zeroed)) {
      const int ax0 = d > rgh - 1 ? d - (rgh - 1) : 0;
      const int ax1 = d < rgw - 1 ? d : rgw - 1;
      const int pairs = (ax1 - ax0 + 1) << (2 * sbs);
      for (int t = lane; t < pairs; t += G) {
        const int ax = ax0 + (t >> (2 * sbs)), ay = d - ax, k = t & (sb_size - 1);
        if (s.sb_live[ay * rgw + ax] != 2) continue;
        const int p = rq_scan_pos(sbs, scan_order, k);
        const int x = (ax << sbs) + (p & 3), y = (ay << sbs) + (p >> 2);
        *lev(x, y) = 0;
      }
      wave_sync();
    }
    RQ_STEP(2);
  }
  RQ_STEP_END();
  long long comp_code_cost = rq_wave_sum_i64<G>(mine ? s.sb_code_cost[lane] : 0ll);
  const long long comp_zero_dist = rq_wave_sum_i64<G>(mine ? my_zero_dist : 0ll);
  // sub-blocks outside the region (64-point transforms): all zero, never the
  // last one, no coded neighbour to the right / below: the cost of a zero flag
  // each (EvalZeroSubblock's csbf == 0 branch)
  const unsigned outside_bits = cb[2 * (RQ_OFF(csbf) + (luma ? 0 : 2))];
  if (gw * gh > rgw * rgh) {
    int n_out = 0;
    for (int t = lane; t < gw * gh; t += G) {
      const int tx = t % gw, ty = t / gw;
      if (tx < rgw && ty < rgh) continue;
      const int idx = d_sb_scan_index(scan_order, gw, gh, tx, ty) << (2 * sbs);
      n_out += idx > 0 && idx + sb_size <= last_pos_index;
    }
    comp_code_cost += (long long)rq_wave_sum_i32<G>(n_out) * rq_bit_cost(outside_bits, lambda);
  }

  RQ_TRACE(6);
  // ---- EvalLastPos (rdo_quant.cc:762-832).  The reference walks back from the
  // last position carrying a running cost: minus every visited sub-block's flag
  // cost, plus cost_to_zero of every visited coefficient; a non-zero level is a
  // candidate (running cost + last-position bits - its implicit sig bits), the
  // first level above 1 ends the walk.  The running cost in front of a
  // coefficient is a prefix sum in scan order: every lane sums its own
  // sub-block, takes the sum of the sub-blocks behind it (64-bit integer adds:
  // any order), evaluates its own candidates down to the stop position and the
  // group keeps the cheapest - on equal cost the one met first, i.e. the
  // highest index.  (One lane doing the walk alone cost 36 of a wave's 93 us.)
  int new_last = 0;
  const int cbf_ctx = 2 * (!luma ? RQ_OFF(cbf_chroma)
                                 : ((prm.flags & XVC_RDOQ_INTRA_CU) ? RQ_OFF(cbf_luma)
                                                                    : RQ_OFF(root_cbf)));
  const long long comp_zero_cost = comp_zero_dist + rq_bit_cost(cb[cbf_ctx], lambda);
  if (gw * gh == rgw * rgh) {
    RQ_STEP2_BEGIN();
    const int last_sb = last_pos_index >> (2 * sbs);
    const bool visited = mine && my_scan <= last_sb;
    const bool coded = visited && s.csbf[lane] != 0;
    const int start_k = my_scan == last_sb ? last_k : sb_size - 1;
    const long long flag_cost = visited ? rq_bit_cost(s.csbf_bits[lane], lambda) : 0ll;
    // the last-position bits of every position group of the two axes, once per
    // block: entries [g] for the (scan-swapped) x, [16 + g] for y - a candidate
    // then costs two reads instead of up to eighteen
    const bool lp_swap = scan_order == 2;
    constexpr int LPY = G == 4 ? 8 : 16;   // where the y groups' entries start
    {
      const int tw = lp_swap ? h : w, th = lp_swap ? w : h;
      const int nx = rq_last_pos_group(tw - 1) + 1, ny = rq_last_pos_group(th - 1) + 1;
      for (int i = lane; i < nx + ny; i += G) {
        const bool is_x = i < nx;
        const int g = is_x ? i : i - nx;
        s.lp_bits[is_x ? g : LPY + g] = rq_last_pos_group_bits(cb, luma, tw, th, g, is_x);
      }
    }
    // own sub-block, back from start_k, in ONE pass: the running sum of the
    // coefficients' cost_to_zero (recomputed, ctz_of) and, at every non-zero
    // level, the candidate's part that belongs to this sub-block (running sum +
    // last-position bits - its implicit significance bits); the cheapest is kept,
    // on equal cost the one met first.  The walk ends at the first level above 1:
    // candidates behind it - in this sub-block or in the sub-blocks below the one
    // that holds the highest such level - do not count.
    long long best_cost = 0x7fffffffffffffffll;
    int best_last_plus1 = 0;
    if (sbs == 2 && G >= 16) {
      // Sixteen lanes take the sixteen coefficients of ONE sub-block per round, from
      // the last position's sub-block down to the one that holds the highest level
      // above 1 (where the walk ends): on real content the walk passes one or two
      // coded sub-blocks, while every owner lane walking its own sixteen
      // coefficients cost sixteen serial steps whatever the content.  The running
      // cost in front of a coefficient is an exclusive prefix sum over the lanes.
      int stop_local = -1;
      if (coded) {
        // sixteen independent reads, then the highest offset with a level above 1
        // (a loop that stops at the first one waits for every read in turn)
        unsigned gt1 = 0;
#pragma unroll
        for (int k = 0; k < 16; k++) {
          int x, y;
          coeff_xy(k, x, y);
          gt1 |= (unsigned)((int)*lev(x, y) > 1) << k;
        }
        gt1 &= (2u << start_k) - 1u;
        if (gt1) stop_local = sb_index + 31 - __clz((int)gt1);
      }
      const int stop_idx = rq_wave_max_i32<G>(stop_local);
      const int stop_sb = stop_idx >= 0 ? stop_idx >> 4 : 0;
      RQ_STEP(0);
      const int kk = lane & 15;
      const bool worker = lane < 16;     // (G = 64: the first sixteen lanes of the wave)
      const int p = rq_scan_pos(sbs, scan_order, kk);
      const long long base = comp_code_cost + rq_bit_cost(cb[cbf_ctx + 1], lambda);
      long long acc = 0;                 // sum of (run - flag cost) of the sub-blocks behind
      for (int j = last_sb; j >= stop_sb; j--) {
        const int t = (int)s.sb_of_scan[j];
        const long long fcost = rq_bit_cost(s.csbf_bits[t], lambda);
        if (!s.csbf[t]) {                // not coded: only its flag's cost leaves the total
          acc -= fcost;
          continue;
        }
        const bool dcz = s.sb_dcz[t] != 0;
        const int x = ((t % rgw) << 2) + (p & 3), y = ((t / rgw) << 2) + (p >> 2);
        const int index = (j << 4) + kk;
        const int first_k = j == last_sb ? last_k : 15;
        const bool in = worker && kk <= first_k && index >= stop_idx;
        const unsigned pk = (unsigned)s.rate_up[rec_pos(x, y)];
        const int v = (int)*lev(x, y);
        const int ac = (short)d_abs(cf(x, y));
        unsigned sig0, sig1;
        sig_pair(pk, x + y, index, kk, dcz, sig0, sig1);
        long long ctz = 0;
        if (in && index != stop_idx) {   // (the level that ends the walk adds nothing)
          ctz = -rq_bit_cost(sig0, lambda);
          if (v == 1) {
            // GetAbsLevelBits (rdo_quant.cc:844-878) for quant_level = 1
            const unsigned c1_0 = cb[greater_ctx_nn(x + y, (int)(pk & 7u))];
            const unsigned bits1 = sig1 + (((pk >> 6) & 1u) ? (2u + ((pk >> 8) & 15u)) * RQ_BYPASS
                                                           : RQ_BYPASS + c1_0);
            const int err = ac - bq.dequant(1);
            ctz = bq.zero_dist(ac) -
                  (bq.dist(err) + rq_bit_cost(bits1, lambda));
          } else if (v != 0) {
            ctz = ctz_of(pk, x + y, index, kk, dcz, ac, v);
          }
        }
        // inclusive prefix over the segment's lanes (scan offsets ascending), then
        // the sum of the coefficients BEHIND this one = total - inclusive
        const long long inc = rq_row_scan_i64(ctz);
        const long long total = rq_group_sum_i64<16>(ctz);
        if (in && v != 0) {
          const unsigned lp_bits = s.lp_bits[rq_last_pos_group(lp_swap ? y : x)] +
                                   s.lp_bits[LPY + rq_last_pos_group(lp_swap ? x : y)];
          const long long cost = base - fcost + acc + (total - inc) +
                                 rq_bit_cost(lp_bits, lambda) - rq_bit_cost(sig1, lambda);
          if (cost < best_cost) {        // (equal cost: the one met first, the higher index)
            best_cost = cost;
            best_last_plus1 = index + 1;
          }
        }
        acc += total - fcost;
      }
      RQ_STEP(1);
    } else {
      long long run = 0, part_best = 0x7fffffffffffffffll;
      int part_k = -1, stop_local = -1;
      if (coded) {
        const bool dcz = s.sb_dcz[lane] != 0;
        // four coefficients' reads in flight at a time (the walk itself is serial:
        // the running sum, and it ends at the first level above 1)
        for (int kb = (sb_size - 1) & ~3; kb >= 0 && stop_local < 0; kb -= 4) {
          int v[4], ac[4], xs[4], ys[4];
          unsigned pk[4], sig0[4], sig1[4];
  #pragma unroll
          for (int i = 0; i < 4; i++) {
            const int k = kb + 3 - i;
            int x, y;
            coeff_xy(k < sb_size ? k : 0, x, y);
            xs[i] = x;
            ys[i] = y;
            pk[i] = (unsigned)s.rate_up[rec_pos(x, y)];
            v[i] = (int)*lev(x, y);
            ac[i] = (short)d_abs(cf(x, y));
            sig_pair(pk[i], x + y, sb_index + k, k, dcz, sig0[i], sig1[i]);
          }
  #pragma unroll
          for (int i = 0; i < 4; i++) {
            const int k = kb + 3 - i;
            if (k >= sb_size || k > start_k || stop_local >= 0) continue;
            long long ctz = -rq_bit_cost(sig0[i], lambda);
            if (v[i]) {
              const unsigned lp_bits = s.lp_bits[rq_last_pos_group(lp_swap ? ys[i] : xs[i])] +
                                       s.lp_bits[LPY + rq_last_pos_group(lp_swap ? xs[i] : ys[i])];
              const long long part =
                  run + rq_bit_cost(lp_bits, lambda) - rq_bit_cost(sig1[i], lambda);
              if (part < part_best) {
                part_best = part;
                part_k = k;
              }
              // the walk ends at a level above 1: nothing behind it counts, its own
              // cost_to_zero included.  What it passes on its way are levels of 1 (and
              // zeros): a level of 1 costs its sign and either the zero bin of its
              // greater-1 flag or, with the flag budget spent, a Golomb-Rice code of 0
              // (GetAbsLevelBits, rdo_quant.cc:844-878, for quant_level = 1)
              if (v[i] > 1) {
                stop_local = sb_index + k;
              } else if (v[i] == 1) {
                const unsigned c1_0 = cb[greater_ctx_nn(xs[i] + ys[i], (int)(pk[i] & 7u))];
                const unsigned bits1 =
                    sig1[i] + (((pk[i] >> 6) & 1u) ? (2u + ((pk[i] >> 8) & 15u)) * RQ_BYPASS
                                                   : RQ_BYPASS + c1_0);
                const int err = ac[i] - bq.dequant(1);
                ctz = bq.zero_dist(ac[i]) -
                      (bq.dist(err) + rq_bit_cost(bits1, lambda));
              } else {
                ctz = ctz_of(pk[i], xs[i] + ys[i], sb_index + k, k, dcz, ac[i], v[i]);
              }
            }
            run += ctz;
          }
        }
        // (the sum is only needed in full by the sub-blocks in FRONT of this one, and
        // they only count when no level above 1 lies here: then the loop ran to k = 0)
      }
      const long long t = run - flag_cost;
      RQ_STEP(0);
      wave_sync();   // every lane has read its sb_code_cost entry (the sums above)
      if (mine) s.sb_code_cost[my_scan] = visited ? t : 0ll;   // now indexed by scan position
      wave_sync();
      const int stop_idx = rq_wave_max_i32<G>(stop_local);
      RQ_STEP(1);
      if (part_k >= 0 && sb_index + start_k >= stop_idx && (stop_local < 0 || stop_local == stop_idx)) {
        long long c = comp_code_cost + rq_bit_cost(cb[cbf_ctx + 1], lambda) - flag_cost;
        for (int j = my_scan + 1; j <= last_sb; j++) c += s.sb_code_cost[j];
        best_cost = c + part_best;
        best_last_plus1 = sb_index + part_k + 1;
      }
    }
    RQ_STEP(2);
#pragma unroll
    for (int sh = 1; sh < G; sh <<= 1) {
      const long long oc = __shfl_xor(best_cost, sh, 64);
      const int oi = __shfl_xor(best_last_plus1, sh, 64);
      if (oc < best_cost || (oc == best_cost && oi > best_last_plus1)) {
        best_cost = oc;
        best_last_plus1 = oi;
      }
    }
    new_last = comp_zero_cost < best_cost ? -1 : best_last_plus1;
    RQ_STEP(3);
    RQ_STEP2_END();
  } else {
    // 64-point transforms (sub-blocks beyond the coefficient region take part in
    // the walk): lane 0, result broadcast
    if (lane == 0) {
      long long code_cost = comp_code_cost + rq_bit_cost(cb[cbf_ctx + 1], lambda);
      int start = last_k;
      long long best_cost = 0x7fffffffffffffffll;
      int best_last_plus1 = 0;
      bool stop = false;
      for (int sbi = last_pos_index >> (2 * sbs); sbi >= 0 && !stop; sbi--) {
        const int t = s.sb_of_scan[sbi];
        const int tx = t % gw, ty = t / gw;
        const int idx = sbi << (2 * sbs);
        if (tx >= rgw || ty >= rgh) {
          if (idx > 0 && idx + sb_size <= last_pos_index)
            code_cost -= rq_bit_cost(outside_bits, lambda);
          continue;
        }
        const int l = ty * rgw + tx;
        code_cost -= rq_bit_cost(s.csbf_bits[l], lambda);
        if (!s.csbf[l]) continue;
        for (int k = start; k >= 0; k--) {
          const int p = rq_scan_pos(sbs, scan_order, k);
          const int x = (tx << sbs) + (p & 3), y = (ty << sbs) + (p >> 2);
          const int pos = rec_pos(x, y);
          const int v = *lev(x, y);
          const unsigned pk = (unsigned)s.rate_up[pos];
          const long long ctz =
              ctz_of(pk, x + y, idx + k, k, s.sb_dcz[l] != 0, (int)(short)d_abs(cf(x, y)), v);
          if (!v) {
            code_cost += ctz;
            continue;
          }
          const unsigned lp_bits = rq_last_pos_bits(cb, luma, w, h, scan_order, x, y);
          unsigned sg0, sg1;
          sig_pair(pk, x + y, idx + k, k, s.sb_dcz[l] != 0, sg0, sg1);
          const long long cost =
              code_cost + rq_bit_cost(lp_bits, lambda) - rq_bit_cost(sg1, lambda);
          if (cost < best_cost) {
            best_cost = cost;
            best_last_plus1 = idx + k + 1;
          }
          if (v > 1) {
            stop = true;
            break;
          }
          code_cost += ctz;
        }
        start = sb_size - 1;
      }
      new_last = comp_zero_cost < best_cost ? -1 : best_last_plus1;
    }
    new_last = __shfl(new_last, (int)(ME2_LANE & ~(G - 1)), 64);
  }

  RQ_TRACE(7);
  // ---- zero what lies at / beyond the new last position, re-apply the signs
  int nnz = 0;
  bool has = false;
  if (mine)
    for (int k = 0; k < sb_size; k++) {
      int x, y;
      coeff_xy(k, x, y);
      short *out = lev(x, y);
      int level = *out;
      if (new_last < 0 || sb_index + k >= new_last) level = 0;
      nnz += level != 0;
      has |= level != 0;
      *out = (short)(cf(x, y) < 0 ? -level : level);
    }
  nnz = rq_wave_sum_i32<G>(nnz);
  if (new_last < 0) return 0;
  if (!(sign_hide && nnz > 1 && sbs > 1)) return nnz;

  RQ_TRACE(8);
  // ---- CoeffSignHideRdo (rdo_quant.cc:575-687): lane = sub-block
  const int last_sb_scan = rq_wave_max_i32<G>(has ? my_scan : -1);
  int dn = 0;
  if (mine && has) {
    const bool is_last_sb = my_scan == last_sb_scan;
    int first = 16, lastk = -1, sum = 0;
    for (int k = 15; k >= 0; k--) {
      int x, y;
      coeff_xy(k, x, y);
      const int v = *lev(x, y);
      if (v) {
        first = k < first ? k : first;
        lastk = lastk > k ? lastk : k;
        sum += v;
      }
    }
    int fx, fy;
    coeff_xy(first, fx, fy);
    const int first_sign = *lev(fx, fy) > 0 ? 0 : 1;
    if (lastk - first >= 4 && first_sign != (sum & 1)) {
      const long long rd_factor = prm.rd_factor;
      long long best_cost = 0x7fffffffffffffffll;
      int best_delta = 0, best_k = 0;
      for (int k = is_last_sb ? lastk : 15; k >= 0; k--) {
        int x, y;
        coeff_xy(k, x, y);
        const unsigned pk = (unsigned)s.rate_up[rec_pos(x, y)];
        const int lvl = *lev(x, y);
        // delta_u (rdo_quant.cc:360-365) of the level as it was decided (the sign
        // was re-applied above: undo it - a magnitude of 32768 keeps its wrapped value)
        const int coeff = cf(x, y);
        const int err_dist = bq.err_of((short)d_abs(coeff), coeff < 0 ? -lvl : lvl);
        long long cost;
        int delta;
        if (lvl != 0) {
          // rate_up / rate_down (rdo_quant.cc:367-374) from the decision-time state
          RdoqFlagBits fb;
          RdoqCoeffState st;
          state_of(pk, x + y, fb, st);
          const int al = d_abs(lvl);
          const int lvl_rate = (int)rq_abs_level_bits(fb, al, st);
          const int rate_up = -lvl_rate + (int)rq_abs_level_bits(fb, al + 1, st);
          const int rate_down = -lvl_rate + (int)rq_abs_level_bits(fb, al - 1, st);
          const long long cost_inc = rd_factor * (-err_dist) + rate_up;
          long long cost_dec = rd_factor * err_dist + rate_down -
                               (al == 1 ? sig_rate_of(pk, x + y, sb_index + k, k, s.sb_dcz[lane] != 0) : 0);
          if (is_last_sb && k == lastk && al == 1) cost_dec -= 4ll * RQ_BYPASS;
          if (cost_inc < cost_dec) {
            cost = cost_inc;
            delta = 1;
          } else {
            delta = -1;
            cost = (k == first && al == 1) ? 0x7fffffffll : cost_dec;
          }
        } else {
          // the rate of a level that was left at 0: the zero bin of its greater1 flag
          const int rate0 =
              (pk & RQ_STATE_NO_RATE) ? 0 : (int)cb[greater_ctx_nn(x + y, (int)(pk & 7u))];
          cost = rd_factor * -(long long)d_abs(err_dist) + rate0 +
                 sig_rate_of(pk, x + y, sb_index + k, k, s.sb_dcz[lane] != 0) + (long long)RQ_BYPASS;
          delta = 1;
          if (k < first && (coeff >= 0 ? 0 : 1) != first_sign) cost = 0x7fffffffll;
        }
        if (cost < best_cost) {
          best_cost = cost;
          best_delta = delta;
          best_k = k;
        }
      }
      int x, y;
      coeff_xy(best_k, x, y);
      short *o = lev(x, y);
      const int before = *o;
      if (before == 32767 || before == -32768) best_delta = -1;
      const int after = (short)(cf(x, y) >= 0 ? before + best_delta : before - best_delta);
      *o = (short)after;
      dn = (after != 0) - (before != 0);
    }
  }
  return nnz + rq_wave_sum_i32<G>(dn);
}

// ---- the quantiser alone, packed ------------------------------------------------
// For flows that hold the transform coefficients (xvcgpu_fwd_transform_batch ->
// here -> xvcgpu_inv_transform_batch).  A block keeps <= 4 lanes of a wave busy
// per wavefront step, so one block per wave wastes the machine: 0.86 ms per
// 1080p picture.  Here G lanes take a block, G = its sub-block count rounded up
// to 4 / 16 / 64: a wave runs 16 blocks of up to 8x8, 4 blocks of up to 16x16 or
// one larger block, every block on its own wavefront.  A classification pass
// sorts the block indices into the three lists; everything the walk keeps per
// coefficient - the coefficient, its level and a 16-bit decision record - and the
// context costs live in LDS (9.9 KB per wave).
struct RdoqLists {
  int *list[3];       // block indices per class (4 / 16 / 64 lanes)
  int *count;         // [3]
  signed char *cls;   // per block: class, -1 = nothing to code
  int *part;          // [chunks][4]: class counts per chunk of RDOQ_CHUNK blocks (compaction)
};
#define RDOQ_CHUNK 4096   // blocks per workgroup of the compaction kernels (4 per thread)

// The context's scratch behind the lists, for a capacity of `cap` blocks: count[4],
// the three lists (cap ints each), the classes (cap bytes = cap / 4 ints), then the
// compaction's per-chunk counts.  cap is a multiple of four (rdoq_scratch_cap): the
// classes then start 16 bytes aligned behind count[4] and the three lists, which
// rdoq_lists_kernel's 16-byte reads rely on.
inline int rdoq_scratch_cap(int n) { return (n + n / 4 + 3) & ~3; }
inline size_t rdoq_scratch_bytes(int cap) {
  return sizeof(int) * (4 + 4 * (size_t)cap + 4 * ((size_t)cap / RDOQ_CHUNK + 2));
}
inline RdoqLists rdoq_scratch_lists(int *base, int cap) {
  RdoqLists l;
  l.count = base;
  for (int c = 0; c < 3; c++) l.list[c] = base + 4 + (size_t)c * cap;
  l.cls = reinterpret_cast<signed char *>(base + 4 + 3 * (size_t)cap);
  l.part = base + 4 + 4 * (size_t)cap;
  return l;
}

// ---- the pieces the list builders below are made of ----
// the classes 0 / 1 / 2 among the four class bytes of word v (blocks i .. i + 3),
// as far as they lie below `end`, added to cnt[]
__device__ __forceinline__ void rq_count_word(uint32_t v, int i, int end, int cnt[3]) {
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const int c = (int)(signed char)(v >> (8 * k));
    const bool in = i + k < end;
    cnt[0] += in && c == 0;
    cnt[1] += in && c == 1;
    cnt[2] += in && c == 2;
  }
}
// inclusive scan of a counter over the 64 lanes of a wave (the builders run it on
// their three counters in turn)
__device__ __forceinline__ int rq_wave_scan(int v) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int o = __shfl_up(v, d, 64);
    if (lane >= d) v += o;
  }
  return v;
}
// the sixteen wave totals of a 1024-thread workgroup, tot[k][0..15], scanned by the
// first wave: tot[k][16 + w] = inclusive total of waves 0..w.  The caller's barriers
// stand before and behind it.
template <int ROW>
__device__ __forceinline__ void rq_wave_totals_scan(int (&tot)[3][ROW]) {
  const int t = threadIdx.x;
  if (t < 64) {
#pragma unroll
    for (int k = 0; k < 3; k++) {
      int v = t < 16 ? tot[k][t] : 0;
#pragma unroll
      for (int d = 1; d < 16; d <<= 1) {
        const int o = __shfl_up(v, d, 64);
        if (t >= d) v += o;
      }
      if (t < 16) tot[k][16 + t] = v;
    }
  }
}
// the listed blocks among i .. i + 3 (class bytes in word v, below `end`) appended to
// their lists at pos[]
__device__ __forceinline__ void rq_scatter_word(uint32_t v, int i, int end, const RdoqLists &l,
                                                int pos[3]) {
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const int c = (int)(signed char)(v >> (8 * k));
    if (i + k < end && c >= 0) l.list[c][pos[c]++] = i + k;
  }
}

// 0 / 1: diagonal scan, 4x4 sub-blocks, at most four / sixteen of them - four lanes
// per sub-block (wave_rdoq4); 2: everything else (the other scans, 2-wide blocks,
// more than sixteen sub-blocks, 64-point sides) - a lane per sub-block (wave_rdoq)
__device__ __forceinline__ int rq_class_of(const xvcgpu_tx_block &b) {
  if (!rq4_takes(64, b.w, b.h, tx_block_flags(b.intra_pic).scan_order) || b.w > 32 || b.h > 32)
    return 2;
  const int n_sb = (b.w >> 2) * (b.h >> 2);
  return n_sb <= 4 ? 0 : (n_sb <= 16 ? 1 : 2);
}

// Classification + the trivial case.  One wave per block: does any coefficient
// quantise to a non-zero value at all (GetFwdQuantFunc, rdo_quant.cc:949-964)?
// If not, QuantRdo returns 0 right after its scan (:387-390) - on real content
// that is most blocks (1080p QP 32: 3 of 4 luma blocks, nearly every chroma
// block): they get their zero levels and count here and never reach the serial
// walk; the others are appended to their class list.  counts must be zero on
// entry.  grid: ceil(n / 4); block: 256.
__device__ __forceinline__ void rdoq_classify_kernel_body(int bd, const xvcgpu_tx_block *blocks, int n, const int16_t *coeffs, const uint32_t *d_off, int16_t *levels, int32_t *nnz_out, RdoqLists l) {
  const int bi = blockIdx.x * 4 + (int)(threadIdx.x >> 6);
  if (bi >= n) return;
  const int lane = threadIdx.x & 63;
  const xvcgpu_tx_block b = blocks[bi];
  const int w = b.w, h = b.h;
  const BlockQuant q = block_quant(b, bd);
  const int16_t *src = coeffs + d_off[bi];
  int16_t *dst = levels + d_off[bi];
  bool any = false;
  for (int i = lane; i < w * h; i += 64) any |= q.codes((short)d_abs((int)src[i]));
  if (__ballot(any)) {
    if (lane == 0) l.cls[bi] = (signed char)rq_class_of(b);
    return;
  }
  if (lane == 0) l.cls[bi] = -1;
  for (int i = lane; i < w * h; i += 64) dst[i] = 0;
  if (lane == 0 && nnz_out) nnz_out[bi] = 0;
}

__global__ void __launch_bounds__(256)
rdoq_classify_kernel(int bd, const xvcgpu_tx_block *blocks, int n, const int16_t *coeffs, const uint32_t *d_off, int16_t *levels, int32_t *nnz_out, RdoqLists l) {
  rdoq_classify_kernel_body(bd, blocks, n, coeffs, d_off, levels, nnz_out, l);
}

// Blocks whose walk is bound to end in "all zero" (rdo_quant.cc:432-446: the
// coded alternative loses against cbf = 0), proved from the first pass alone and
// taken off the class lists.  With q = the plain quantised magnitude, the
// candidates for a coded level are the coefficients with q > 0 (rdo_quant.cc:
// 314-336: a coefficient with q = 0 keeps level 0).  For a last position L (a
// candidate in scan order) the coded alternative costs at least
//   cbf(1) + lastpos(L) + sum over i < L of min(zd_i, code_i) + code_last_L
//   + zd of everything else,
// where code_i >= d_best_i + lambda * (cheapest significance "1" the position can
// meet - any template count up to the number of q > 0 neighbours; none for a
// sub-block's DC behind the first sub-block, whose flag may be inferred - + sign
// + cheapest continuation: the smaller bin of a greater-1 context the position can
// meet, or a bypass bin once the budget is spent), d_best_i = the smaller of the
// distortions of q and q - 1 (the two levels the walk tries), and code_last the
// same without the significance flag.  The all-zero alternative costs cbf(0) +
// sum of zd.  So if for EVERY candidate L
//   sum_{i < L} (zd_i - min(zd_i, code_i)) + (zd_L - code_last_L)
//     < cbf(1) - cbf(0) + lastpos(L)
// then QuantRdo returns 0 for the block.  Every term is a lower bound of what the
// walk would charge, so the proof never zeroes a block the walk would code; blocks
// it cannot decide stay on the lists.  1080p QP 32, settled chain: 84 % of the luma
// blocks and nearly all chroma blocks the walk zeroes are proved here
// (tools/dbg/rdoq_zero_bound.py is the offline form of the bound).
// Blocks with 2-wide sub-blocks, a 64-point side, a magnitude of 32768, more than
// 16 candidates, coefficients that do not start on 8 bytes or another context
// snapshot than the workgroup's are left to the walk.  Sixteen lanes per block,
// RQ_PROVE_BLOCKS blocks per workgroup in rounds of sixteen (one table of context
// costs for all of them); grid: ceil(n / RQ_PROVE_BLOCKS); block: 256.
#define RQ_PROVE_BLOCKS 16
#define RQ_PROVE_MAX_CANDS 16

// What the context costs of a candidate with magnitude a come to: sig1 = the cheapest
// significance "1" it can meet (0 where the flag may be inferred), flag_min = the cheapest
// greater-1 bin, lp = the bits of a last position there, cbf0 / cbf1 = the bins of the
// block's cbf.
template <bool NARROW>
__device__ __forceinline__ void rq_prove_price(const BlockQuant &bq, long long lambda, int a,
                                               unsigned sig1, unsigned flag_min, unsigned lp,
                                               unsigned cbf0, unsigned cbf1, long long &gain,
                                               long long &gain_last, long long &rhs) {
  auto price = [&](unsigned bits) -> long long {
    if (NARROW)
      return (long long)(((unsigned long long)bits * (unsigned long long)(unsigned)lambda) >> 16);
    return rq_bit_cost(bits, lambda);
  };
  // a squared error |e| <= 65535 fits 32 bits (BlockQuant::dist's value)
  auto dist = [&](int e) -> long long {
    return (long long)((unsigned long long)((unsigned)e * (unsigned)e)) << bq.cost_scale;
  };
  const int q = bq.fwd(a);
  const unsigned lvl_min = RQ_BYPASS + flag_min;   // sign + the cheapest continuation
  long long d_best = dist(a - bq.dequant(q));
  if (q > 1) {
    const long long d1 = dist(a - bq.dequant(q - 1));
    d_best = d1 < d_best ? d1 : d_best;
  }
  const long long zd = bq.zero_dist(a);
  const long long coded = d_best + price(sig1 + lvl_min);
  const long long coded_last = d_best + price(lvl_min);
  gain = zd - (coded < zd ? coded : zd);
  gain_last = zd - coded_last;
  rhs = price(cbf1) - price(cbf0) + price(lp);
}

// A position's place in the scan: sub-block in the grid's scan, offset in the sub-block's
// (the inverse of the 4x4 scan: position y * 4 + x -> scan offset, 16 nibbles).  W, H >
// 0: the block is exactly that.
template <int W, int H>
__device__ __forceinline__ int rq_prove_scan_index(int scan_order, int w, int h, int x, int y) {
  constexpr unsigned long long inv0 = rq_pack_scan4_inv(0), inv1 = rq_pack_scan4_inv(1),
                               inv2 = rq_pack_scan4_inv(2);
  const unsigned long long inv = scan_order == 0 ? inv0 : (scan_order == 1 ? inv1 : inv2);
  const int kk = (int)((inv >> (4 * (((y & 3) << 2) | (x & 3)))) & 15ull);
  int sb;
  if constexpr (W >= 4 && H >= 4 && (W >> 2) * (H >> 2) <= 16) {
    // the diagonal scan of this grid as a constant
    constexpr int GW = W >> 2, GH = H >> 2;
    constexpr unsigned long long kSb = rq_pack_sb_scan(GW, GH);
    const int sx = x >> 2, sy = y >> 2;
    sb = scan_order == 0 ? (int)((kSb >> (4 * (sy * GW + sx))) & 15ull)
                         : (scan_order == 1 ? sy * GW + sx : sx * GH + sy);
  } else {
    sb = d_sb_scan_index(scan_order, w >> 2, h >> 2, x >> 2, y >> 2);
  }
  return (sb << 4) + kk;
}

// the smallest magnitude that quantises to a level: a * scale >= 2^(shift - 1)
__device__ __forceinline__ int rq_prove_threshold(const BlockQuant &bq) {
  long long t = (long long)((double)bq.fq_offset / (double)bq.scale);
  while (t * bq.scale < bq.fq_offset) t++;
  while (t > 0 && (t - 1) * bq.scale >= bq.fq_offset) t--;
  return t > 32768 ? 32768 : (int)t;
}

// One candidate (x, y) of block b (quantiser bq) with magnitude a: what coding it
// can save at most as an inner coefficient (gain) and as the last one (gain_last),
// what a last position there costs on top (rhs), and its place in the scan (idx).
// qat(x, y) = the plain quantised magnitude at a position, 0 outside the block; cb
// = the snapshot's bit costs (entry 2 * ctx + bin).
template <class QAt>
__device__ __forceinline__ void rq_prove_candidate(const BlockQuant &bq, const xvcgpu_tx_block &b,
                                                   const xvcgpu_rdoq_params &prm,
                                                   const unsigned *cb, int x, int y, int a,
                                                   QAt qat, long long &gain, long long &gain_last,
                                                   long long &rhs, int &idx) {
  const int w = b.w, h = b.h, scan_order = tx_block_flags(b.intra_pic).scan_order;
  const bool luma = b.comp == 0;
  const long long lambda = prm.lambda;
  const int q = bq.fwd(a);
  int cnt, cnt1;
  {
    const int q0 = qat(x + 1, y), q1 = qat(x + 2, y), q2 = qat(x + 1, y + 1), q3 = qat(x, y + 1),
              q4 = qat(x, y + 2);
    cnt = (q0 > 0) + (q1 > 0) + (q2 > 0) + (q3 > 0) + (q4 > 0);
    cnt1 = (q0 > 1) + (q1 > 1) + (q2 > 1) + (q3 > 1) + (q4 > 1);
  }
  const int posxy = x + y;
  // the cheapest "1" bin the significance flag can meet
  const int sig_base = rq_sig_ctx_base(luma, posxy, (rq_log2(w) + rq_log2(h)) >> 1);
  unsigned sig1 = 0xffffffffu;
  for (int nn = 0; nn <= cnt; nn++) {
    const unsigned v = cb[sig_base + 2 * nn + 1];
    sig1 = v < sig1 ? v : sig1;
  }
  const bool sub_dc = ((x | y) & 3) == 0 && (x | y) != 0;   // k = 0 behind the first sub-block
  if (sub_dc) sig1 = 0;
  // the greater-1 contexts: the last position's, or by the count
  unsigned flag_min = RQ_BYPASS;   // (budget spent: a Golomb-Rice code of at least one bin)
  auto meet = [&](int nn) {
    const int c = rq_greater_ctx(luma, posxy, nn);
    const unsigned v0 = cb[c], v1 = cb[c + 1];
    flag_min = v0 < flag_min ? v0 : flag_min;
    flag_min = v1 < flag_min ? v1 : flag_min;
  };
  meet(0);
  for (int n = 0; n <= cnt1; n++) meet(rq_greater_nn(n, false));
  const unsigned lvl_min = RQ_BYPASS + flag_min;   // sign + the cheapest continuation
  long long d_best = bq.dist(a - bq.dequant(q));
  if (q > 1) {
    const long long d1 = bq.dist(a - bq.dequant(q - 1));
    d_best = d1 < d_best ? d1 : d_best;
  }
  const long long zd = bq.zero_dist(a);
  const long long coded = d_best + rq_bit_cost(sig1 + lvl_min, lambda);
  const long long coded_last = d_best + rq_bit_cost(lvl_min, lambda);
  gain = zd - (coded < zd ? coded : zd);
  gain_last = zd - coded_last;
  const unsigned lp = rq_last_pos_bits(cb, luma, w, h, scan_order, x, y);
  const int cbf_ctx = 2 * (!luma ? RQ_OFF(cbf_chroma)
                                 : ((prm.flags & XVC_RDOQ_INTRA_CU) ? RQ_OFF(cbf_luma)
                                                                    : RQ_OFF(root_cbf)));
  rhs = rq_bit_cost(cb[cbf_ctx + 1], lambda) - rq_bit_cost(cb[cbf_ctx], lambda) +
        rq_bit_cost(lp, lambda);
  // scan index: sub-block in the grid's scan, offset in the sub-block's (the
  // inverse of the 4x4 scan: position y * 4 + x -> scan offset, 16 nibbles)
  constexpr unsigned long long inv0 = rq_pack_scan4_inv(0), inv1 = rq_pack_scan4_inv(1),
                               inv2 = rq_pack_scan4_inv(2);
  const unsigned long long inv = scan_order == 0 ? inv0 : (scan_order == 1 ? inv1 : inv2);
  const int kk = (int)((inv >> (4 * (((y & 3) << 2) | (x & 3)))) & 15ull);
  idx = (d_sb_scan_index(scan_order, w >> 2, h >> 2, x >> 2, y >> 2) << 4) + kk;
}

__global__ void __launch_bounds__(256)
rdoq_prove_zero_kernel(int bd, const xvcgpu_tx_block *blocks, int n, const int16_t *coeffs,
                       const uint32_t *d_off, int16_t *levels, int32_t *nnz_out,
                       const xvcgpu_rdoq_contexts *rq_ctx, const xvcgpu_rdoq_params *rq_prm,
                       RdoqLists l) {
  __shared__ __attribute__((aligned(16))) unsigned s_cb[2 * sizeof(xvcgpu_rdoq_contexts)];
  __shared__ unsigned short s_xy[16][RQ_PROVE_MAX_CANDS];
  __shared__ int s_idx[16][RQ_PROVE_MAX_CANDS];
  __shared__ long long s_gain[16][RQ_PROVE_MAX_CANDS];
  __shared__ int s_n[16];
  __shared__ int s_fail[16];
  __shared__ int s_ctx;
  const int g = threadIdx.x >> 4, gl = threadIdx.x & 15;
  const int base = blockIdx.x * RQ_PROVE_BLOCKS;
  // the workgroup's snapshot: the largest index among its live blocks
  if (threadIdx.x == 0) s_ctx = -1;
  __syncthreads();
  if ((int)threadIdx.x < RQ_PROVE_BLOCKS) {
    const int b2 = base + (int)threadIdx.x;
    if (b2 < n && l.cls[b2] >= 0) atomicMax(&s_ctx, (int)rq_prm[b2].ctx_index);
  }
  __syncthreads();
  const int wg_ctx = s_ctx;
  if (wg_ctx < 0) return;   // no live block (uniform)
  rq_stage_costs(gEntropyBits, &rq_ctx[wg_ctx], s_cb, (int)threadIdx.x, 256);
  __syncthreads();   // the context costs are in place
  // From here on a group of sixteen lanes works on its own block and its own rows
  // of the shared arrays: groups never share data, a wave holds four of them, so
  // ordering LDS traffic inside the wave is all that is needed.
  for (int sub = 0; sub < RQ_PROVE_BLOCKS / 16; sub++) {
    const int bi = base + sub * 16 + g;
    const bool live = bi < n && l.cls[bi < n ? bi : 0] >= 0;
    const xvcgpu_tx_block b = blocks[live ? bi : 0];
    const xvcgpu_rdoq_params prm = rq_prm[live ? bi : 0];
    if (gl == 0) {
      s_n[g] = 0;
      s_fail[g] = 0;
    }
    wave_sync();
    const BlockQuant bq = block_quant(b, bd);
    const int w = b.w, h = b.h;
    const int16_t *src = coeffs + d_off[live ? bi : 0];
    // (coefficients are read four at a time: a block that does not start on 8 bytes
    // is left to the walk)
    const bool tried = live && (int)prm.ctx_index == wg_ctx && w >= 4 && h >= 4 && w <= 32 &&
                       h <= 32 && (reinterpret_cast<uintptr_t>(src) & 7) == 0;
    auto qat = [&](int x, int y) {
      if (x >= w || y >= h) return 0;
      return bq.fwd((short)d_abs((int)src[y * w + x]));
    };
    // the candidates: coefficients with q > 0 - one compare against the smallest
    // such magnitude, four coefficients per load (a magnitude of 32768: no proof)
    if (tried) {
      const int thr = rq_prove_threshold(bq);
      bool wrap = false;
      for (int i = 4 * gl; i < w * h; i += 64) {
        const uint2 v = *reinterpret_cast<const uint2 *>(src + i);
        const int a4[4] = {d_abs((int)(short)(v.x & 0xffff)), d_abs((int)(short)(v.x >> 16)),
                           d_abs((int)(short)(v.y & 0xffff)), d_abs((int)(short)(v.y >> 16))};
#pragma unroll
        for (int t = 0; t < 4; t++) {
          wrap |= a4[t] == 32768;
          if (a4[t] >= thr) {
            const int slot = atomicAdd(&s_n[g], 1);
            const int ii = i + t;
            if (slot < RQ_PROVE_MAX_CANDS)
              s_xy[g][slot] = (unsigned short)(((ii >> rq_log2(w)) << 8) | (ii & (w - 1)));
          }
        }
      }
      if (wrap) s_fail[g] = 1;
    }
    wave_sync();   // the group's candidate list is complete
    const int nq = s_n[g];
    long long gain_last = 0, rhs = 0;
    int my_idx = 0;
    const bool cand = tried && nq <= RQ_PROVE_MAX_CANDS && gl < nq && !s_fail[g];
    if (tried && gl == 0 && (nq > RQ_PROVE_MAX_CANDS || nq == 0)) s_fail[g] = 1;
    if (cand) {
      const int x = s_xy[g][gl] & 255, y = s_xy[g][gl] >> 8;
      const int a = (short)d_abs((int)src[y * w + x]);
      long long gain;
      rq_prove_candidate(bq, b, prm, s_cb, x, y, a, qat, gain, gain_last, rhs, my_idx);
      s_idx[g][gl] = my_idx;
      s_gain[g][gl] = gain;
    }
    wave_sync();
    if (cand) {
      long long before = 0;
      for (int j = 0; j < nq; j++)
        if (s_idx[g][j] < my_idx) before += s_gain[g][j];
      if (before + gain_last >= rhs) s_fail[g] = 1;
    }
    wave_sync();
    if (tried && !s_fail[g]) {
      // QuantRdo would return 0: zero levels, no class
      int16_t *dst = levels + d_off[bi];
      for (int i = gl; i < w * h; i += 16) dst[i] = 0;
      if (gl == 0) {
        if (nnz_out) nnz_out[bi] = 0;
        l.cls[bi] = -1;
      }
    }
    wave_sync();   // the group's rows are free for its next block
  }
}

// The same proof where the coefficients of a block lie in LDS (the forward
// transform of the frame pass, k_tx2.h: C[x][y] at c[x * h + y]): G lanes per
// block, 64 / G blocks per wave; the block's q > 0 coefficients are collected by the
// caller through rq_prove_collect (count nq, positions (y << 8) | x in xy).  Returns
// true (to every lane of the group) when QuantRdo is bound to return 0.  The wave's LDS:
// the candidates' positions, scan indices and gains, and - for the shapes without a
// table of their own (rq_prove_tables) - the snapshot's costs, staged on first use.
struct RqProveLds {
  __attribute__((aligned(16))) unsigned cb[2 * sizeof(xvcgpu_rdoq_contexts)];
  __attribute__((aligned(16))) long long gain[2][RQ_PROVE_MAX_CANDS];
  __attribute__((aligned(16))) int idx[2][RQ_PROVE_MAX_CANDS];
  unsigned short xy[2][RQ_PROVE_MAX_CANDS];
  int staged_ctx;   // snapshot whose costs cb holds (-1: none yet)
};

// The candidates of the block at c: position i (C[x][y] at i = x * h + y) is entered by
// the lane that holds a magnitude of at least thr.t1 there - its slot is the group's
// count so far plus the hits in the lanes below it, from the ballot: no atomic, no
// count in LDS.  `hit`: this lane's coefficient codes; nq: the group's running count
// (the same in all its lanes).  Only the first RQ_PROVE_MAX_CANDS are kept; a trip
// without a hit in the wave costs a ballot and a branch.
template <int G>
__device__ __forceinline__ void rq_prove_collect(RqProveLds *pv, bool hit, int i, int h, int lgh,
                                                 int &nq) {
  static_assert(G == 64 || G == 32, "a wave or half a wave per block");
  const unsigned long long hits = __ballot(hit);
  if (!hits) return;   // (wave-uniform)
  const unsigned lo = (unsigned)hits, hi = (unsigned)(hits >> 32);
  int below, total;
  if (G == 64) {
    below = (int)__builtin_amdgcn_mbcnt_hi(hi, __builtin_amdgcn_mbcnt_lo(lo, 0u));
    total = __popc(lo) + __popc(hi);
  } else {
    const bool up = (threadIdx.x & 32) != 0;
    below = up ? (int)__builtin_amdgcn_mbcnt_hi(hi, 0u) : (int)__builtin_amdgcn_mbcnt_lo(lo, 0u);
    total = up ? __popc(hi) : __popc(lo);
  }
  const int slot = nq + below;
  if (pv && hit && slot < RQ_PROVE_MAX_CANDS)
    pv->xy[(threadIdx.x & 63) / G][slot] = (unsigned short)(((i & (h - 1)) << 8) | (i >> lgh));
  nq += total;
}

// The context costs any candidate of a wave of S x S blocks (S = 16 or 8; all luma or all
// chroma) can ask for, one entry per lane, in rows of eight lanes:
//   rows 0, 1  lane t: the bits of a last position in group t of the x / y axis
//   rows 2-4   lane t: the cheapest significance "1" over the counts 0 .. t, for the sets
//              of x + y < 2, < 5 and beyond (rq_sig_ctx_base); lane 6 of row 2 holds the
//              cbf context instead (its bins in zero / one)
//   rows 5-7   lane t: the cheapest greater-1 bin (or a bypass bin) over the last
//              position's context and those of the counts 1 .. t, for x + y < 3, < 10 and
//              beyond (rq_greater_start)
// A lane reads the state of its ONE context from the snapshot and its two costs from the
// table of bit costs - no snapshot staged in LDS -, the prefix sums (rows 0, 1) and minima
// run along the rows by DPP; a candidate then fetches four entries by lane index.
struct RqProveRow {
  unsigned t, zero, one;
};
template <int S>
__device__ __forceinline__ RqProveRow rq_prove_tables(const xvcgpu_rdoq_contexts *snap, bool luma,
                                                      bool intra_cu) {
  static_assert(S == 16 || S == 8, "last-position groups 0 .. 7 fit a row");
  constexpr int LS = S == 16 ? 4 : 3;
  const int wl = (int)(threadIdx.x & 63), t = wl & 7, row = wl >> 3;
  const int gmax = rq_last_pos_group(S - 1), gc = gmax - 1;
  const int tc = t < 5 ? t : 5;
  int ctx;   // this lane's context: its byte in the snapshot
  if (row < 2) {
    ctx = rq_last_pos_ctx(luma, S, S, t < gc ? t : gc, row == 0) >> 1;
  } else if (row < 5) {
    ctx = (rq_sig_ctx_base(luma, row == 2 ? 0 : (row == 3 ? 2 : 5), LS) >> 1) + tc;
    if (wl == 22)
      ctx = !luma ? RQ_OFF(cbf_chroma) : (intra_cu ? RQ_OFF(cbf_luma) : RQ_OFF(root_cbf));
  } else {
    const int g1 = rq_greater1_off(luma);
    ctx = t == 0 ? g1 : g1 + rq_greater_start(luma, row == 5 ? 0 : (row == 6 ? 3 : 10)) + tc;
  }
  const unsigned st = reinterpret_cast<const unsigned char *>(snap)[ctx] & 127u;
  const unsigned zero = gEntropyBits[st], one = gEntropyBits[st ^ 1u];
  const bool sum = row < 2;
  const unsigned own = row < 5 ? one : (zero < one ? zero : one);
  unsigned v = own;
  // inclusive scan along the row's eight lanes (row_shr: the lane 1, 2, 4 below)
  auto step = [&](unsigned got, int s) {
    if (t >= s) v = sum ? v + got : (got < v ? got : v);
  };
  step((unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xF, 0xF, false), 1);
  step((unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xF, 0xF, false), 2);
  step((unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xF, 0xF, false), 4);
  unsigned tv;
  if (sum)   // GetLastPosBits: the ones below the group, its zero unless it is the last, the suffix
    tv = v - own + (t < gmax ? zero : 0u) + (t > 3 ? (unsigned)((t - 2) >> 1) * RQ_BYPASS : 0u);
  else if (row < 5)
    tv = v;
  else
    tv = v < RQ_BYPASS ? v : RQ_BYPASS;
  return {tv, zero, one};
}

// nq: the group's candidates as rq_prove_collect counted them (0: the block is not
// live), thr: rq_level_thresholds(bq); w, h: the block's size (W, H > 0: exactly that, a
// constant).  The exact 16x16 and 8x8 instances (the forward kernel's: a wave holds luma
// blocks or chroma blocks, never both) take their context costs from rq_prove_tables and
// every lane runs the candidate's arithmetic, masked at the end; any other shape stages the
// snapshot in pv.cb and runs rq_prove_candidate in the candidates' lanes.  A candidate
// with a magnitude of 32768 fails its block (such a magnitude is a candidate wherever
// anything is).
template <int G, int W, int H>
__device__ __forceinline__ bool rq_prove_zero_lds(RqProveLds &pv, const xvcgpu_tx_block &b,
                                                  int w, int h, const BlockQuant &bq,
                                                  const RqLevelThr &thr,
                                                  const xvcgpu_rdoq_contexts *rq_ctx,
                                                  const xvcgpu_rdoq_params *rq_prm, int bi,
                                                  const int16_t *c, int nq) {
  const int wl = (int)(threadIdx.x & 63), lane = wl & (G - 1), grp = wl / G;
  const unsigned long long group = G == 64 ? ~0ull : (((1ull << G) - 1) << (wl & ~(G - 1)));
  bool tried = nq >= 1 && nq <= RQ_PROVE_MAX_CANDS && w >= 4 && h >= 4 && w <= 32 && h <= 32;
  // the wave's snapshot: the first trying group's
  const unsigned long long tm = __ballot(tried);
  if (!tm) return false;
  const xvcgpu_rdoq_params prm = rq_prm[bi];
  const int wave_ctx = __shfl((int)prm.ctx_index, __ffsll((long long)tm) - 1, 64);
  tried = tried && (int)prm.ctx_index == wave_ctx;
  wave_sync();   // the candidates' positions are in place
  long long gain = 0, gain_last = 0, rhs = 0;
  int my_idx = 0x7fffffff;   // (a lane without a candidate: in front of nobody)
  bool over = false;         // the magnitude that wraps
  const bool cand = tried && lane < nq;
  if constexpr (W == H && (W == 16 || W == 8)) {
    // the magnitude at a position, 0 outside the block: a neighbour quantises to a level /
    // to more than 1 from thr.t1 / thr.t2 on
    auto mag = [&](int x, int y) {
      if (x >= W || y >= H) return 0;
      return d_abs((int)c[x * H + y]);
    };
    // lambda fits 32 bits (every real one does): a price is a 32 x 32 -> 64 bit product; one
    // of more than 32 bits anywhere in the wave: the 64-bit prices for all of it
    const bool narrow = __ballot(cand && (unsigned long long)prm.lambda > 0xffffffffull) == 0;
    const int scan_order = tx_block_flags(b.intra_pic).scan_order;
    const bool luma = __builtin_amdgcn_readfirstlane((int)(b.comp == 0)) != 0;
    const RqProveRow row =
        rq_prove_tables<W>(&rq_ctx[wave_ctx], luma, (prm.flags & XVC_RDOQ_INTRA_CU) != 0);
    const unsigned xy = cand ? pv.xy[grp][lane] : 0u;   // (the others: position (0, 0))
    const int x = (int)(xy & 255u), y = (int)(xy >> 8);
    const int a = d_abs((int)c[x * H + y]);
    over = a == 32768;
    const int m0 = mag(x + 1, y), m1 = mag(x + 2, y), m2 = mag(x + 1, y + 1), m3 = mag(x, y + 1),
              m4 = mag(x, y + 2);
    const int cnt =
        (m0 >= thr.t1) + (m1 >= thr.t1) + (m2 >= thr.t1) + (m3 >= thr.t1) + (m4 >= thr.t1);
    const int cnt1 =
        (m0 >= thr.t2) + (m1 >= thr.t2) + (m2 >= thr.t2) + (m3 >= thr.t2) + (m4 >= thr.t2);
    const int posxy = x + y;
    const int scls = (posxy >= 2) + (posxy >= 5), gcls = (posxy >= 3) + (posxy >= 10);
    unsigned sig1 = __shfl(row.t, 16 + 8 * scls + cnt, 64);
    const unsigned flag_min = __shfl(row.t, 40 + 8 * gcls + rq_greater_nn(cnt1, false), 64);
    const unsigned lp = __shfl(row.t, rq_last_pos_group(scan_order == 2 ? y : x), 64) +
                        __shfl(row.t, 8 + rq_last_pos_group(scan_order == 2 ? x : y), 64);
    const unsigned cbf0 = __shfl(row.zero, 22, 64), cbf1 = __shfl(row.one, 22, 64);
    if (((x | y) & 3) == 0 && (x | y) != 0) sig1 = 0;   // k = 0 behind the first sub-block
    if (narrow)
      rq_prove_price<true>(bq, prm.lambda, a, sig1, flag_min, lp, cbf0, cbf1, gain, gain_last, rhs);
    else
      rq_prove_price<false>(bq, prm.lambda, a, sig1, flag_min, lp, cbf0, cbf1, gain, gain_last,
                            rhs);
    if (cand) my_idx = rq_prove_scan_index<W, H>(scan_order, W, H, x, y);
  } else {
    if (pv.staged_ctx != wave_ctx) {
      rq_stage_costs(gEntropyBits, &rq_ctx[wave_ctx], pv.cb, wl, 64);
      if (wl == 0) pv.staged_ctx = wave_ctx;
      wave_sync();
    }
    auto qat = [&](int x, int y) {
      if (x >= w || y >= h) return 0;
      return bq.fwd((short)d_abs((int)c[x * h + y]));
    };
    if (cand) {
      const int x = pv.xy[grp][lane] & 255, y = pv.xy[grp][lane] >> 8;
      const int a = d_abs((int)c[x * h + y]);
      over = a == 32768;
      rq_prove_candidate(bq, b, prm, pv.cb, x, y, a, qat, gain, gain_last, rhs, my_idx);
    }
  }
  // all sixteen rows of a trying group are written, so the sum below reads them four at
  // a time and asks only for the scan index
  if (tried && lane < RQ_PROVE_MAX_CANDS) {
    pv.idx[grp][lane] = my_idx;
    pv.gain[grp][lane] = gain;
  }
  wave_sync();
  bool bad = false;
  if (cand) {
    long long before = 0;
    for (int j = 0; j < nq; j += 4) {
      const int4 id = *reinterpret_cast<const int4 *>(&pv.idx[grp][j]);
      const longlong2 g01 = *reinterpret_cast<const longlong2 *>(&pv.gain[grp][j]);
      const longlong2 g23 = *reinterpret_cast<const longlong2 *>(&pv.gain[grp][j + 2]);
      before += id.x < my_idx ? g01.x : 0ll;
      before += id.y < my_idx ? g01.y : 0ll;
      before += id.z < my_idx ? g23.x : 0ll;
      before += id.w < my_idx ? g23.y : 0ll;
    }
    bad = over || before + gain_last >= rhs;
  }
  return tried && (__ballot(bad) & group) == 0;
}

// The class lists from the per-block classes, without atomics (a few thousand
// atomicAdds on three addresses took 150 us): one workgroup, every thread
// counts its contiguous chunk, an LDS scan gives the chunk's place in each list.
// The builder of xvcgpu_frame_pass_multi (rdoq_compact_multi_kernel, k_multi.h).
// grid: 1; block: 1024.
__device__ __forceinline__ void rdoq_compact_kernel_body(int n, RdoqLists l) {
  __shared__ int part[3][1024];
  const int t = threadIdx.x;
  // a multiple of 4 blocks per thread: the classes are read four at a time
  const int per = ((n + 1023) / 1024 + 3) & ~3;
  const int a = t * per, e = a + per < n ? a + per : n;
  const uint32_t *cw = reinterpret_cast<const uint32_t *>(l.cls);
  int cnt[3] = {0, 0, 0};
  for (int i = a; i < e; i += 4) rq_count_word(cw[i >> 2], i, e, cnt);
#pragma unroll
  for (int k = 0; k < 3; k++) part[k][t] = cnt[k];
  __syncthreads();
  // inclusive scan over the 1024 partial counts, three at once: inside each
  // wave by shuffles, then the 16 wave totals by the first wave
  int inc[3];
#pragma unroll
  for (int k = 0; k < 3; k++) {
    inc[k] = rq_wave_scan(cnt[k]);
    if ((t & 63) == 63) part[k][t >> 6] = inc[k];  // wave totals (slots 0..15 reused after the sync)
  }
  __syncthreads();
  rq_wave_totals_scan(part);
  __syncthreads();
  int pos[3];
#pragma unroll
  for (int k = 0; k < 3; k++)
    pos[k] = inc[k] - cnt[k] + ((t >> 6) ? part[k][16 + (t >> 6) - 1] : 0);
  for (int i = a; i < e; i += 4) rq_scatter_word(cw[i >> 2], i, e, l, pos);
  if (t == 1023)
    for (int k = 0; k < 3; k++) l.count[k] = part[k][16 + 15];
}

// The same lists from many workgroups, still without atomics and in block order
// (the single workgroup above takes 13 us for a 1080p picture but 90 / 300 us for
// 2160p / 4320p - on every picture's critical path): a workgroup owns a chunk of
// RDOQ_CHUNK blocks, four per thread.  Launch 1 counts the chunk's classes; launch
// 2 sums the counts of the chunks in front of it (at most a few hundred), scans
// its own threads' counts and scatters.  grid: ceil(n / RDOQ_CHUNK); block: 1024.
__global__ void __launch_bounds__(1024)
rdoq_count_kernel(int n, RdoqLists l) {
  __shared__ int wsum[3][16];
  const int t = threadIdx.x, i = (int)blockIdx.x * RDOQ_CHUNK + 4 * t;
  int cnt[3] = {0, 0, 0};
  if (i < n) rq_count_word(reinterpret_cast<const uint32_t *>(l.cls)[i >> 2], i, n, cnt);
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const int v = wave_reduce_add_i32(cnt[k]);
    if ((t & 63) == 0) wsum[k][t >> 6] = v;
  }
  __syncthreads();
  if (t < 3) {
    int v = 0;
    for (int w = 0; w < 16; w++) v += wsum[t][w];
    l.part[4 * blockIdx.x + t] = v;
  }
}

__global__ void __launch_bounds__(1024)
rdoq_scatter_kernel(int n, RdoqLists l) {
  __shared__ int part[3][1024];
  __shared__ int base[3];
  const int t = threadIdx.x, b = blockIdx.x;
  // the chunks in front of this one
  {
    int v[3] = {0, 0, 0};
    for (int j = t; j < b; j += 1024) {
      v[0] += l.part[4 * j];
      v[1] += l.part[4 * j + 1];
      v[2] += l.part[4 * j + 2];
    }
#pragma unroll
    for (int k = 0; k < 3; k++) {
      const int w = wave_reduce_add_i32(v[k]);
      if ((t & 63) == 0) part[k][t >> 6] = w;
    }
    __syncthreads();
    if (t < 3) {
      int sum = 0;
      for (int w = 0; w < 16; w++) sum += part[t][w];
      base[t] = sum;
    }
    __syncthreads();
  }
  const int i = b * RDOQ_CHUNK + 4 * t;
  const uint32_t *cw = reinterpret_cast<const uint32_t *>(l.cls);
  int cnt[3] = {0, 0, 0};
  if (i < n) rq_count_word(cw[i >> 2], i, n, cnt);
  int inc[3];
#pragma unroll
  for (int k = 0; k < 3; k++) inc[k] = rq_wave_scan(cnt[k]);
  __syncthreads();   // base[] read by everybody before part[] is reused
  const int bs[3] = {base[0], base[1], base[2]};
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 3; k++)
    if ((t & 63) == 63) part[k][t >> 6] = inc[k];
  __syncthreads();
  rq_wave_totals_scan(part);
  __syncthreads();
  int pos[3];
#pragma unroll
  for (int k = 0; k < 3; k++)
    pos[k] = bs[k] + inc[k] - cnt[k] + ((t >> 6) ? part[k][16 + (t >> 6) - 1] : 0);
  if (i < n) rq_scatter_word(cw[i >> 2], i, n, l, pos);
  if (b == (int)gridDim.x - 1 && t == 1023)
    for (int k = 0; k < 3; k++) l.count[k] = bs[k] + part[k][16 + 15];
}

// The same lists in ONE launch, for batches small enough that a redundant read of
// the classes costs less than a second launch and the hand-over through l.part: a
// workgroup owns RDOQ_LISTS_CHUNK blocks (four per thread, the per-thread shape of the
// two kernels above) and counts the classes of all the chunks in front of it itself - a
// byte per block, sixteen at a time, resident in L2.  That read grows with the square of
// n: the caller keeps the two launches above for large batches.  Small workgroups place
// beside other streams' kernels where sixteen waves have to wait for a CU with four free
// slots on every SIMD.  RDOQ_LISTS_WAVES (1, 2 or 4) sets the workgroup.  Measured with
// three picture chains in flight ("Waves per workgroup"): two waves (chunks
// of 512 blocks; 1080p: 48 workgroups, the last one reads 24 KB, 0.6 MB in all) gain
// 1.8 % of the pass over four; one wave (96 workgroups, 1.2 MB, the last one's read 24
// trips long) gains nothing.  grid: ceil(n / RDOQ_LISTS_CHUNK); block: RDOQ_LISTS_THREADS.
#ifndef RDOQ_LISTS_WAVES
#define RDOQ_LISTS_WAVES 2
#endif
#define RDOQ_LISTS_THREADS (64 * RDOQ_LISTS_WAVES)
#define RDOQ_LISTS_CHUNK (4 * RDOQ_LISTS_THREADS)

// the bytes of v that equal c (0..127), exactly: no carry crosses a byte
__device__ __forceinline__ int rq_bytes_equal(uint32_t v, uint32_t c) {
  const uint32_t x = v ^ (c * 0x01010101u);
  return __popc(~(((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x | 0x7f7f7f7fu));
}

__global__ void __launch_bounds__(RDOQ_LISTS_THREADS)
rdoq_lists_kernel(int n, RdoqLists l) {
  constexpr int WAVES = RDOQ_LISTS_WAVES;
  __shared__ int wsum[3][WAVES];    // the prefix read's wave sums
  __shared__ int wtot[3][WAVES];    // the chunk's own wave totals
  const int t = threadIdx.x, b = blockIdx.x, wv = t >> 6;
  const uint32_t *cw = reinterpret_cast<const uint32_t *>(l.cls);
  // the chunks in front of this one: 64 * b 16-byte words of classes, all of them
  // inside n.  l.cls is 16-byte aligned (rdoq_scratch_cap), so the reads cover the
  // prefix and nothing else
  int v[3] = {0, 0, 0};
  {
    const uint4 *q = reinterpret_cast<const uint4 *>(cw);
    const int quads = (RDOQ_LISTS_CHUNK / 16) * b;
    for (int j = t; j < quads; j += RDOQ_LISTS_THREADS) {
      const uint4 u = q[j];
      const uint32_t a[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
      for (int k = 0; k < 4; k++) {
        v[0] += rq_bytes_equal(a[k], 0);
        v[1] += rq_bytes_equal(a[k], 1);
        v[2] += rq_bytes_equal(a[k], 2);
      }
    }
  }
  // this chunk: four blocks per thread
  const int i = b * RDOQ_LISTS_CHUNK + 4 * t;
  uint32_t mine = 0;
  int cnt[3] = {0, 0, 0};
  if (i < n) {
    mine = cw[i >> 2];
    rq_count_word(mine, i, n, cnt);
  }
  int inc[3];
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const int w = wave_reduce_add_i32(v[k]);
    inc[k] = rq_wave_scan(cnt[k]);
    if ((t & 63) == 0) wsum[k][wv] = w;
    if ((t & 63) == 63) wtot[k][wv] = inc[k];
  }
  __syncthreads();
  int pos[3];
#pragma unroll
  for (int k = 0; k < 3; k++) {
    int base = 0, before = 0;
#pragma unroll
    for (int w = 0; w < WAVES; w++) base += wsum[k][w];
#pragma unroll
    for (int w = 0; w < WAVES - 1; w++) before += w < wv ? wtot[k][w] : 0;
    pos[k] = base + before + inc[k] - cnt[k];
  }
  if (i < n) rq_scatter_word(mine, i, n, l, pos);
  if (b == (int)gridDim.x - 1 && t == RDOQ_LISTS_THREADS - 1)
    for (int k = 0; k < 3; k++) l.count[k] = pos[k];   // base + the chunk's total
}

// LDS of one wave: G lanes per block (64 / G blocks per wave), blocks of at most NSB
// region sub-blocks.  One table of context costs per wave: the groups of a wave
// nearly always name the same snapshot; when they do not, the wave serves one
// snapshot after the other (a table per group cost 19 KB of LDS per wave in the
// 4-lane class - enough, with the walk's long-lived waves, to keep other kernels
// off the CUs).
template <int G, int NSB>
struct RdoqPackedLds {
  static constexpr int GROUPS = 64 / G;
  static constexpr int MAXC = 16 * NSB;                                // region coefficients
  static constexpr int MAXSB = NSB;                                    // region sub-blocks
  static constexpr int MAXR = RQ_PADDED(MAXC);     // records: RQ_SB_STRIDE per sub-block
  static constexpr int MAXT = RQ_CF_PADDED(MAXC);  // coefficient / level tiles: RQ_CF_STRIDE
  // the per-coefficient records: 5 bytes each (+ 4 of coefficient and level)
  alignas(8) long long sb_code_cost[GROUPS][MAXSB];
  alignas(8) int16_t cf[GROUPS][MAXT], lv[GROUPS][MAXT];
  alignas(8) int16_t wl[GROUPS][RQ_WL(MAXC)];          // wave_rdoq4's working levels
  long long fcs[NSB == 64 ? 256 : 1];                  // (64-point sides; else sb_code_cost)
  unsigned short rate_up[GROUPS][MAXR];
  alignas(8) unsigned ctx_bits[2 * sizeof(xvcgpu_rdoq_contexts)];
  unsigned csbf_bits[GROUPS][MAXSB];
  unsigned char csbf[GROUPS][MAXSB], sb_live[GROUPS][MAXSB], sb_dcz[GROUPS][MAXSB];
  // the whole grid's scan (64-point sides: up to four times the region; NSB = 4: grid = region)
  unsigned char sb_of_scan[GROUPS][NSB == 4 ? MAXSB : MAXSB * 4];
  // one table per wave: the groups of a round share shape, scan and snapshot
  unsigned lp_bits[32];
};

// G lanes per block; grid: an upper bound on ceil(count / (64 / G)) waves (the
// list's count is read on the device); block: 64.
// wave_rdoq4's accessors in the packed kernel: the coefficient tile (sub-block major,
// RQ_CF_STRIDE: a sub-block's row is 8 contiguous bytes) and the block's levels in
// global memory (row-major, the block's own width): a unit's row is one access.
struct RqTileCf {
  const int16_t *p;
  int rgw;
  __device__ __forceinline__ int pos(int x, int y) const {
    return ((y >> 2) * rgw + (x >> 2)) * RQ_CF_STRIDE + (((y & 3) << 2) | (x & 3));
  }
  __device__ __forceinline__ int operator()(int x, int y) const { return (int)p[pos(x, y)]; }
  __device__ __forceinline__ void row4(int px, int y, int c[4]) const {
    const uint2 v = *reinterpret_cast<const uint2 *>(p + pos(px, y));
    c[0] = (int)(short)(v.x & 0xffffu);
    c[1] = (int)(short)(v.x >> 16);
    c[2] = (int)(short)(v.y & 0xffffu);
    c[3] = (int)(short)(v.y >> 16);
  }
};
struct RqGlobalLev {
  int16_t *p;
  int w;
  __device__ __forceinline__ int16_t *operator()(int x, int y) const { return p + y * w + x; }
  __device__ __forceinline__ void store4(int px, int y, const int v[4]) const {
    int16_t *o = p + y * w + px;
    if ((reinterpret_cast<uintptr_t>(o) & 7) == 0) {
      *reinterpret_cast<uint2 *>(o) =
          make_uint2((unsigned)(v[0] & 0xffff) | ((unsigned)v[1] << 16),
                     (unsigned)(v[2] & 0xffff) | ((unsigned)v[3] << 16));
    } else {
      o[0] = (int16_t)v[0]; o[1] = (int16_t)v[1]; o[2] = (int16_t)v[2]; o[3] = (int16_t)v[3];
    }
  }
};

template <int G, int NSB, bool FOUR>
__device__ __forceinline__ void quant_rdo_packed_wave(
    RdoqPackedLds<G, NSB> &sm, int wave, int bd, const xvcgpu_tx_block *blocks, const int *list,
    const int *count, const int16_t *coeffs, const uint32_t *d_off, int16_t *levels,
    int32_t *nnz_out, const xvcgpu_rdoq_contexts *rq_ctx, const xvcgpu_rdoq_params *rq_prm,
    xvcgpu_cu_info *cu_patch = nullptr) {
  constexpr int GROUPS = 64 / G;
  const int g = threadIdx.x / G, lane = threadIdx.x % G;
  const int slot = wave * GROUPS + g;
  RQ_TRACE(0);
  RQ_TRACE_RT(0);
  const int n_list = *count;
  if (wave * GROUPS >= n_list) return;  // the launch is an upper bound
  const bool active = slot < n_list;
  const int bi = active ? list[slot] : 0;
  const xvcgpu_tx_block b = blocks[bi];
  const xvcgpu_rdoq_params prm = rq_prm[bi];
  const int w = b.w, h = b.h;
  const int rw = w < 32 ? w : 32, rh = h < 32 ? h : 32;
  const uint32_t off = d_off[bi];
  const int16_t *src = coeffs + off;
  int16_t *cf = sm.cf[g], *lv = sm.lv[g];
  // this lane's word of its own block's snapshot, fetched beside the coefficients (the
  // round below nearly always serves that snapshot: one global round trip less)
  constexpr int kCtxWords = (int)sizeof(xvcgpu_rdoq_contexts) / 4;
  const int ctx_wi = (int)threadIdx.x < kCtxWords ? (int)threadIdx.x : kCtxWords - 1;
  const uint32_t word_own = reinterpret_cast<const uint32_t *>(&rq_ctx[prm.ctx_index])[ctx_wi];
  RQ_TRACE(1);
  // blocks that are their own region (no 64-point side), a multiple of 8
  // coefficients, 16-byte aligned in both arrays: 16-byte copies in and out
  int16_t *dst = levels + off;
  const bool wide = w == rw && h == rh && ((w * h) & 7) == 0 &&
                    ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15) == 0;
  // the tiles are stored sub-block by sub-block (stride RQ_CF_STRIDE: the lanes
  // of a group read the same offset of different sub-blocks - RQ_SB_STRIDE above);
  // blocks with 2x2 sub-blocks (a side of 2) stay raster
  const bool sb4 = !(w == 2 || h == 2);
  const int rgw4 = rw >> 2;
  auto tile_pos = [sb4, rgw4, rw](int x, int y) {
    return sb4 ? ((y >> 2) * rgw4 + (x >> 2)) * RQ_CF_STRIDE + (((y & 3) << 2) | (x & 3))
               : y * rw + x;
  };
  if (active) {
    if (wide && sb4) {
      // 8 coefficients = two sub-blocks' rows of 4 (a 4-wide block: two rows of one)
      for (int i = lane; i < (w * h) >> 3; i += G) {
        const uint4 v8 = reinterpret_cast<const uint4 *>(src)[i];
        const int y = (8 * i) / rw, x = 8 * i - y * rw;
        const int p0 = tile_pos(x, y), p1 = rw == 4 ? tile_pos(0, y + 1) : tile_pos(x + 4, y);
        *reinterpret_cast<uint2 *>(cf + p0) = make_uint2(v8.x, v8.y);
        *reinterpret_cast<uint2 *>(cf + p1) = make_uint2(v8.z, v8.w);
        if (!FOUR) {   // (wave_rdoq4 writes its levels to global memory itself)
          *reinterpret_cast<uint2 *>(lv + p0) = make_uint2(0, 0);
          *reinterpret_cast<uint2 *>(lv + p1) = make_uint2(0, 0);
        }
      }
    } else {
      for (int i = lane; i < rw * rh; i += G) {
        const int y = i / rw, x = i - y * rw;
        cf[tile_pos(x, y)] = src[y * w + x];
        if (!FOUR) lv[tile_pos(x, y)] = 0;
      }
    }
  }
  RdoqView v;
  v.wl = sm.wl[g];
  v.fcs = NSB == 64 ? sm.fcs : sm.sb_code_cost[g];
  v.sb_dcz = sm.sb_dcz[g];
  v.rate_up = sm.rate_up[g];
  v.sb_live = sm.sb_live[g];
  v.sb_code_cost = sm.sb_code_cost[g];
  v.csbf_bits = sm.csbf_bits[g];
  v.csbf = sm.csbf[g];
  v.sb_of_scan = sm.sb_of_scan[g];
  v.lp_bits = sm.lp_bits;
  v.ctx_bits = sm.ctx_bits;
  RQ_TRACE(2);
  // One (context snapshot, block shape, qp, component kind, flags, lambda) at a
  // time - normally one round: a picture's blocks of one class share them.  What
  // the walk derives from them (quantiser scales and shifts, grid sizes, context
  // bases, the lambda it multiplies every rate with) then lives in SCALAR
  // registers; as per-lane values - every group of a wave its own block - they
  // cost the walk 70 of its 200 vector registers, i.e. a wave per SIMD.
  bool pending = active;
  int nnz = 0;
  for (;;) {
    const unsigned long long todo = __ballot(pending);
    if (!todo) break;
    const int leader = __ffsll((long long)todo) - 1;
    const int cur = __shfl((int)prm.ctx_index, leader, 64);
    // the leader's key, as per-lane copies for the comparison
    const int kw = __shfl(w, leader, 64), kh = __shfl(h, leader, 64);
    const int kqp = __shfl((int)b.qp, leader, 64);
    const int kluma = __shfl((int)(b.comp == 0), leader, 64);
    const int kflags = __shfl((int)b.intra_pic, leader, 64);
    const int kpf = __shfl((int)prm.flags, leader, 64);
    const long long klambda = __shfl(prm.lambda, leader, 64);
    wave_sync();  // the previous round's readers are done with the table
    {
      // rq_stage_costs with a word per lane, the lane's own word already at hand
      static_assert(RQ_CTX_WORDS <= 64, "one word of contexts per lane");
      const uint32_t *cw = reinterpret_cast<const uint32_t *>(&rq_ctx[cur]);
      const uint32_t word = (int)prm.ctx_index == cur ? word_own : cw[ctx_wi];
      if ((int)threadIdx.x < RQ_CTX_WORDS)
        rq_stage_word(kEntropyBits, word, sm.ctx_bits + 8 * threadIdx.x);
    }
    wave_sync();
    RQ_TRACE(3);
    const bool take = pending && (int)prm.ctx_index == cur && w == kw && h == kh &&
                      (int)b.qp == kqp && (int)(b.comp == 0) == kluma &&
                      (int)b.intra_pic == kflags && (int)prm.flags == kpf &&
                      prm.lambda == klambda;
    if (take) {
      // every lane in here holds the same key: read it into scalar registers
      const int uw = __builtin_amdgcn_readfirstlane(w), uh = __builtin_amdgcn_readfirstlane(h);
      const int uqp = __builtin_amdgcn_readfirstlane((int)b.qp);
      const int uluma = __builtin_amdgcn_readfirstlane((int)(b.comp == 0));
      const int uflags = __builtin_amdgcn_readfirstlane((int)b.intra_pic);
      const int upf = __builtin_amdgcn_readfirstlane((int)prm.flags);
      const unsigned ulam_lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)prm.lambda);
      const unsigned ulam_hi = (unsigned)__builtin_amdgcn_readfirstlane(
          (int)(unsigned)((unsigned long long)prm.lambda >> 32));
      const long long ulambda = (long long)(((unsigned long long)ulam_hi << 32) | ulam_lo);
      // the groups walk independently (their shuffles stay inside the group)
      const bool usb4 = !(uw == 2 || uh == 2);
      const int urw = uw < 32 ? uw : 32, urgw4 = urw >> 2;
      auto utile = [usb4, urgw4, urw](int x, int y) {
        return usb4 ? ((y >> 2) * urgw4 + (x >> 2)) * RQ_CF_STRIDE + (((y & 3) << 2) | (x & 3))
                    : y * urw + x;
      };
      xvcgpu_rdoq_params uprm = prm;   // rd_factor stays the lane's own
      uprm.lambda = ulambda;
      uprm.flags = (uint8_t)upf;
      const TxBlockFlags ufl = tx_block_flags(uflags);
      const int uscan = ufl.scan_order;
      const bool ush = ufl.sign_hide;
      // (k_quant.h; derived in the arm that walks, in front of the walk)
      auto ubq = [&](int bw, int bh) { return block_quant(bw, bh, uqp, bd, ufl.intra_pic); };
      auto cf_at = [cf, utile](int x, int y) { return (int)cf[utile(x, y)]; };
      auto lv_at = [lv, utile](int x, int y) { return lv + utile(x, y); };
      if (FOUR) {
        // four lanes per sub-block (k_rdoq4.h): the class lists hold what it takes; the
        // levels go straight to the block's place in global memory
        const RqTileCf cf4 = {cf, urgw4};
        const RqGlobalLev lv4 = {dst, uw};
        nnz = wave_rdoq4<G, 1>(v, lane, ubq(uw, uh), uw, uh, uluma != 0, ush, uprm, cf4, lv4);
      } else if (NSB == 64) {
        // the general class: more than sixteen sub-blocks or a 64-point side in the diagonal
        // scan (four units per lane), or a lane per sub-block
        const BlockQuant q = ubq(uw, uh);
        if (rq4_takes(64, uw, uh, uscan))
          nnz = wave_rdoq4<64, 4>(v, lane, q, uw, uh, uluma != 0, ush, uprm, cf_at, lv_at);
        else
          nnz = wave_rdoq<G>(v, lane, q, uw, uh, uluma != 0, uscan, ush, rq_ctx[cur], uprm, cf_at,
                             lv_at, false, false);
      } else if (G == 16 && NSB == 16 && uw == 16 && uh == 16) {
        // (the instance for the exact 16x16 block beside the any-size one: the long lists of
        // a large picture - RDOQ4_LATENCY_BLOCKS - are almost only these)
        auto cf16 = [cf](int x, int y) {
          return (int)cf[((y >> 2) * 4 + (x >> 2)) * RQ_CF_STRIDE + (((y & 3) << 2) | (x & 3))];
        };
        auto lv16 = [lv](int x, int y) {
          return lv + ((y >> 2) * 4 + (x >> 2)) * RQ_CF_STRIDE + (((y & 3) << 2) | (x & 3));
        };
        nnz = wave_rdoq<G>(v, lane, ubq(16, 16), 16, 16, uluma != 0, uscan, ush, rq_ctx[cur], uprm,
                           cf16, lv16, false, false);
      } else {
        nnz = wave_rdoq<G>(v, lane, ubq(uw, uh), uw, uh, uluma != 0, uscan, ush, rq_ctx[cur], uprm,
                           cf_at, lv_at, false, false);
      }
      pending = false;
    }
  }
  wave_sync();
  RQ_TRACE(9);
  if (!active) return;
  if (FOUR) {
    // (the walk wrote the levels)
  } else if (wide && sb4) {
    for (int i = lane; i < (w * h) >> 3; i += G) {
      const int y = (8 * i) / rw, x = 8 * i - y * rw;
      const uint2 a = *reinterpret_cast<const uint2 *>(lv + tile_pos(x, y));
      const uint2 b2 = *reinterpret_cast<const uint2 *>(
          lv + (rw == 4 ? tile_pos(0, y + 1) : tile_pos(x + 4, y)));
      reinterpret_cast<uint4 *>(dst)[i] = make_uint4(a.x, a.y, b2.x, b2.y);
    }
  } else {
    for (int i = lane; i < w * h; i += G) {
      const int y = i / w, x = i - y * w;
      dst[i] = (x < rw && y < rh) ? lv[tile_pos(x, y)] : (int16_t)0;
    }
  }
  if (lane == 0 && nnz_out) nnz_out[bi] = nnz;
  // blocks 3 * cu + comp (xvcgpu_fwd_from_me_classify wrote the CU's record with cbf_luma = 0)
  if (lane == 0 && cu_patch && b.comp == 0 && nnz) cu_patch[bi / 3].cbf_luma = 1;
  RQ_TRACE(10);
  RQ_TRACE_RT(1);
}

// The classes' walks are independent and each is bounded by its own slowest block.
// Two launches: the two classes of wave_rdoq4 together (quant_rdo_packed4_kernel:
// workgroups [0, g16) take the blocks of up to sixteen sub-blocks, a block per wave,
// the rest the blocks of up to four, four per wave), and the general class
// (quant_rdo_packed_kernel, a lane per sub-block) - in one kernel the general walk's
// 198 vector registers were every wave's: two waves per SIMD, 2048 wave slots on the
// chip for the 2300 - 7600 blocks of a 1080p picture, i.e. a second round of waves
// behind the first (66 us for walks of at most 45).  The lists' counts are only known
// on the device, and one workgroup per possible block made the launch last as long as
// the churn of workgroups retiring after a look at the count: each class gets a bounded
// number of workgroups instead, which walk their list with that stride.
// grid: g16 + g4 (packed4) / g64 (general); block: 64.
#ifndef RDOQ4_LATENCY_BLOCKS
#define RDOQ4_LATENCY_BLOCKS 4096   // a block per wave up to this many blocks of the class
#endif
__device__ __forceinline__ void quant_rdo_packed4_kernel_body(int bd, const xvcgpu_tx_block *blocks, RdoqLists l, int g16, const int16_t *coeffs, const uint32_t *d_off, int16_t *levels, int32_t *nnz_out, const xvcgpu_rdoq_contexts *rq_ctx, const xvcgpu_rdoq_params *rq_prm, xvcgpu_cu_info *cu_patch) {
  union Lds {
    RdoqPackedLds<64, 16> a;
    RdoqPackedLds<16, 4> b;
    RdoqPackedLds<16, 16> t;
  };
  __shared__ Lds sm;
  const int wg = blockIdx.x, g4 = (int)gridDim.x - g16;
  if (wg < g16) {
    const int n1 = l.count[1];
    if (n1 > RDOQ4_LATENCY_BLOCKS) {
      // More blocks than the chip has wave slots: waves queue behind each other whatever
      // their shape, and what the launch costs - alone and beside the other pictures'
      // kernels - is its total instruction count.  A block per wave spends about twice
      // the wave instructions per block of the lane-per-sub-block walk with four blocks
      // side by side (2160p QP 27, 25 000 blocks, three chains: 1290 against 1550 frame
      // passes/s): the long lists take that walk.
      const int waves = (n1 + 3) >> 2;
      for (int wv = wg; wv < waves; wv += g16) {
        quant_rdo_packed_wave<16, 16, false>(sm.t, wv, bd, blocks, l.list[1], l.count + 1, coeffs,
                                             d_off, levels, nnz_out, rq_ctx, rq_prm, cu_patch);
        wave_sync();
      }
      return;
    }
    for (int wv = wg; wv < n1; wv += g16) {
      quant_rdo_packed_wave<64, 16, true>(sm.a, wv, bd, blocks, l.list[1], l.count + 1, coeffs,
                                          d_off, levels, nnz_out, rq_ctx, rq_prm, cu_patch);
      wave_sync();
    }
  } else {
    const int waves = (l.count[0] + 3) >> 2;
    for (int wv = wg - g16; wv < waves; wv += g4) {
      quant_rdo_packed_wave<16, 4, true>(sm.b, wv, bd, blocks, l.list[0], l.count + 0, coeffs,
                                         d_off, levels, nnz_out, rq_ctx, rq_prm, cu_patch);
      wave_sync();
    }
  }
}

__device__ __forceinline__ void quant_rdo_packed_kernel_body(int bd, const xvcgpu_tx_block *blocks, RdoqLists l, const int16_t *coeffs, const uint32_t *d_off, int16_t *levels, int32_t *nnz_out, const xvcgpu_rdoq_contexts *rq_ctx, const xvcgpu_rdoq_params *rq_prm, xvcgpu_cu_info *cu_patch) {
  __shared__ RdoqPackedLds<64, 64> sm;
  const int waves = l.count[2];
  for (int wv = blockIdx.x; wv < waves; wv += (int)gridDim.x) {
    quant_rdo_packed_wave<64, 64, false>(sm, wv, bd, blocks, l.list[2], l.count + 2, coeffs, d_off,
                                         levels, nnz_out, rq_ctx, rq_prm, cu_patch);
    wave_sync();
  }
}

#ifndef RDOQ4_MIN_WAVES
#define RDOQ4_MIN_WAVES 3   // per SIMD: 168 vector registers (the walk holds 156 - 167)
#endif
__global__ void __launch_bounds__(64, RDOQ4_MIN_WAVES)
quant_rdo_packed4_kernel(int bd, const xvcgpu_tx_block *blocks, RdoqLists l, int g16, const int16_t *coeffs, const uint32_t *d_off, int16_t *levels, int32_t *nnz_out, const xvcgpu_rdoq_contexts *rq_ctx, const xvcgpu_rdoq_params *rq_prm, xvcgpu_cu_info *cu_patch = nullptr, int *misuse = nullptr) {
  // misuse: the general class's launch was left out on the caller's word
  // (xvcgpu_quant_rdo_set_four_lane_only); a block on its list is reported, not dropped
  if (misuse && blockIdx.x == 0 && threadIdx.x == 0 && l.count[2] != 0) *misuse = 1;
  quant_rdo_packed4_kernel_body(bd, blocks, l, g16, coeffs, d_off, levels, nnz_out, rq_ctx, rq_prm, cu_patch);
}

#ifndef RDOQ_MIN_WAVES
#define RDOQ_MIN_WAVES 2   // per SIMD: 256 vector registers
#endif
__global__ void __launch_bounds__(64, RDOQ_MIN_WAVES)
quant_rdo_packed_kernel(int bd, const xvcgpu_tx_block *blocks, RdoqLists l, const int16_t *coeffs, const uint32_t *d_off, int16_t *levels, int32_t *nnz_out, const xvcgpu_rdoq_contexts *rq_ctx, const xvcgpu_rdoq_params *rq_prm, xvcgpu_cu_info *cu_patch = nullptr) {
  quant_rdo_packed_kernel_body(bd, blocks, l, coeffs, d_off, levels, nnz_out, rq_ctx, rq_prm, cu_patch);
}

#endif  // XVCGPU_K_RDOQ_H_
