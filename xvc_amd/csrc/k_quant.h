// k_quant.h -- what a transform block's width, height, QP and bit depth decide,
// said once: the block's flags, the quantiser's constants and element steps
// (Quantize, quantize.cc:48-72, :94-131; RdoQuant::QuantFast / QuantRdo,
// rdo_quant.cc:156-195, :223-300, :360-365, :949-964), the shifts of the
// transform stages (transform.cc:83-182, :869-961), the context selection the
// RDO quantiser's walks and its all-zero proof share (cabac.cc:520-560,
// :594-684) and the table of context bit costs they read.  Every kernel that
// transforms or quantises takes these from here (k_tx.h, k_tx2.h, k_rdoq.h,
// k_rdoq4.h); width and height come in as values, so an instance for an exact
// block shape folds every shift to a constant, and what a caller does not read
// is never computed.
#ifndef XVCGPU_K_QUANT_H_
#define XVCGPU_K_QUANT_H_

#include "dev_common.h"
#include "dev_tables.h"
#include "xvcgpu_internal.h"

// ---- the XVC_TXF_* bits of xvcgpu_tx_block::intra_pic ---------------------------
struct TxBlockFlags {
  bool intra_pic;   // pic_type == kIntra: QuantFast rounds with 171/512, else 85/512
  bool sign_hide;
  bool rdoq;        // the block asks for RdoQuant::QuantRdo
  int scan_order;   // 0 diagonal, 1 horizontal, 2 vertical
};
__device__ __forceinline__ TxBlockFlags tx_block_flags(int f) {
  return {(f & XVC_TXF_INTRA_PIC) != 0, !(f & XVC_TXF_NO_SIGN_HIDING), (f & XVC_TXF_RDOQ) != 0,
          (f >> XVC_TXF_SCAN_SHIFT) & 3};
}

__device__ __forceinline__ int rq_log2(int size) {  // util::SizeToLog2, powers of two
  return 31 - __clz(size);
}

// ---- the quantiser of one block --------------------------------------------------
// A block whose log2 sizes sum to an odd number carries a factor of sqrt(2): 181 /
// 128 in the forward scale (7 more bits of shift), 181 / 256 in the inverse.
struct BlockQuant {
  bool bias;               // the odd log-size sum
  int tshift;              // the transform's scaling left to the quantiser
  int scale;               // forward: kFwdQuantScales[qp % 6] (x 181)
  int scale_idx;           // which of the twelve forward scales: qp % 6, + 6 with the bias
  int shift;               // 14 + qp / 6 + tshift
  int size_bias_shift, size_bias_offset;
  int fq_shift;            // shift + size_bias_shift: what a magnitude * scale is shifted by
  long long fq_offset;     // GetFwdQuantFunc rounds to nearest
  long long fast_offset;   // QuantFast rounds with 171/512 (intra picture) or 85/512
  int iq_scale, iq_shift;  // Quantize::Inverse
  int cost_scale;          // a squared coefficient error in the units of lambda * bits

  // GetFwdQuantFunc on a magnitude (rdo_quant.cc:949-964); 32768 wraps as there
  __device__ __forceinline__ int fwd(int a) const {
    return (int)(short)(int)((((long long)a * scale) + fq_offset) >> fq_shift);
  }
  // does the magnitude quantise to a level at all?  (what the RDO quantiser's
  // classification asks of every coefficient of a block)
  __device__ __forceinline__ bool codes(int a) const { return fwd(a) != 0; }
  // QuantFast of one coefficient (rdo_quant.cc:171-190): the signed level and its
  // rounding remainder in 1/256 of a step, what the sign hiding prices.  (Both by value:
  // with the remainder stored through a reference into LDS the one-wave QuantFast
  // kernels took twice the vector registers.)
  struct Fast {
    int16_t level, rem;
  };
  __device__ __forceinline__ Fast fast(int coeff) const {
    const int sign = coeff < 0 ? -1 : 1;
    const long long abs_coeff = d_abs(coeff);
    const int level = (int)(((abs_coeff * scale) + fast_offset) >> fq_shift);
    return {(int16_t)d_clip3(level * sign, -32768, 32767),
            (int16_t)(((abs_coeff * scale) - ((long long)level << fq_shift)) >> (fq_shift - 8))};
  }
  // Quantize::Inverse of one level (quantize.cc:94-125), clipped to 16 bits
  __device__ __forceinline__ int dequant(int level) const {
    const int prod = level * iq_scale;
    int cf;
    if (iq_shift > 0) cf = (prod + (1 << (iq_shift - 1))) >> iq_shift;
    else cf = (int)((unsigned)prod << -iq_shift);
    return (int)(short)d_clip3(cf, -32768, 32767);
  }
  // delta_u (rdo_quant.cc:360-365): the quantisation error of `level` in 1/256 of a step
  __device__ __forceinline__ int err_of(int abs_coeff, int level) const {
    const long long orig_scaled =
        (((long long)abs_coeff * scale) + size_bias_offset) >> size_bias_shift;
    const long long quant_err = orig_scaled - ((long long)level << shift);
    return (int)(short)(quant_err >> (shift - 8));
  }
  // the distortion of an error e = coefficient - dequantised level (e = the
  // magnitude itself: the coefficient left at zero); |e| <= 65535
  __device__ __forceinline__ long long dist(int e) const {
    return ((long long)e * e) << cost_scale;
  }
  __device__ __forceinline__ long long zero_dist(int a) const {
    return ((long long)(a * a)) << cost_scale;
  }
};

__device__ __forceinline__ BlockQuant block_quant(int w, int h, int qp, int bd, bool intra_pic) {
  const int lsum = rq_log2(w) + rq_log2(h);
  int qpb = qp + 6 * (bd - 8);
  qpb = qpb > 0 ? qpb : 0;
  BlockQuant q;
  q.bias = (lsum & 1) != 0;
  q.tshift = 15 - bd - (lsum >> 1);
  q.scale = kFwdQuantScales[qpb % 6] * (q.bias ? 181 : 1);
  q.scale_idx = qpb % 6 + (q.bias ? 6 : 0);
  q.shift = 14 + qpb / 6 + q.tshift;
  q.size_bias_shift = q.bias ? 7 : 0;
  q.size_bias_offset = q.bias ? 64 : 0;
  q.fq_shift = q.shift + q.size_bias_shift;
  q.fq_offset = 1ll << (q.fq_shift - 1);
  q.fast_offset = (long long)((intra_pic ? 171ull : 85ull) << (q.fq_shift - 9));
  q.iq_scale = (kInvQuantScales[qpb % 6] << (qpb / 6)) * (q.bias ? 181 : 1);
  q.iq_shift = 6 - q.tshift + (q.bias ? 8 : 0);
  q.cost_scale = 15 - 2 * q.tshift - 2 * (bd - 8) + 2 * (q.bias ? 1 : 0);
  return q;
}
__device__ __forceinline__ BlockQuant block_quant(const xvcgpu_tx_block &b, int bd) {
  return block_quant(b.w, b.h, b.qp, bd, tx_block_flags(b.intra_pic).intra_pic);
}

// ---- the magnitudes at which the plain quantiser's level steps -------------------
// fwd(a) >= 1 <=> a >= t1 and fwd(a) >= 2 <=> a >= t2 for magnitudes up to 32767 (fwd is
// monotonic there: scale < 2^fq_shift): t_m = ceil(m * fq_offset / scale), m = 1 and 3.
// They depend on the scale (twelve of them) and on fq_shift alone, so they are a table
// made at compile time: one scalar load where the QP is the wave's.  A magnitude of 32768
// reaches fwd as -32768 (the classification's `codes` and the proofs' callers cast to
// short): it codes <=> 32768 * scale > fq_offset, which t1 answers too - t1 is 32769 where
// 32768 * scale == fq_offset.  Thresholds above 65535 are entered as 65535 (no magnitude
// gets there), as are those of an fq_shift outside the table.
#define RQ_THR_SHIFTS 48
struct RqLevelThrTable {
  unsigned short t[12][RQ_THR_SHIFTS][2];
};
constexpr RqLevelThrTable rq_make_level_thr_table() {
  constexpr int fwd[6] = {26214, 23302, 20560, 18396, 16384, 14564};   // kFwdQuantScales
  RqLevelThrTable r{};
  for (int i = 0; i < 12; i++) {
    const unsigned long long scale = (unsigned long long)(fwd[i % 6] * (i < 6 ? 1 : 181));
    for (int s = 0; s < RQ_THR_SHIFTS; s++) {
      for (int m = 0; m < 2; m++) {
        unsigned long long t = 65535;
        if (s >= 1) {
          const unsigned long long target = (m ? 3ull : 1ull) << (s - 1);   // m * fq_offset
          t = (target + scale - 1) / scale;
          if (m == 0 && t == 32768 && t * scale == target) t = 32769;
          if (t > 65535) t = 65535;
        }
        r.t[i][s][m] = (unsigned short)t;
      }
    }
  }
  return r;
}
__constant__ RqLevelThrTable kRqLevelThr = rq_make_level_thr_table();
struct RqLevelThr {
  int t1, t2;
};
__device__ __forceinline__ RqLevelThr rq_level_thresholds(const BlockQuant &bq) {
  if (bq.fq_shift < 0 || bq.fq_shift >= RQ_THR_SHIFTS) return {65535, 65535};
  const uint32_t v =
      *reinterpret_cast<const uint32_t *>(kRqLevelThr.t[bq.scale_idx][bq.fq_shift]);
  return {(int)(v & 0xffff), (int)(v >> 16)};
}

// ---- the shifts of the four 1-D transform stages ---------------------------------
// A stage of XVC_TX_DCT2_LOW has the 6-bit matrix and no high-precision shift
// (transform.cc:876-884).  Forward: horizontal then vertical; inverse: vertical then
// horizontal.  dct2_both: the DC-only inverse applies (InvDct2Dc, transform.cc:279-291).
struct TxStageShifts {
  int fwd1, fwd2, inv1, inv2;
  bool dct2_both;
};
__device__ __forceinline__ TxStageShifts tx_stage_shifts(int tx_hor, int tx_ver, int lgw, int lgh,
                                                         int bd) {
  const int hp_hor = tx_hor == XVC_TX_DCT2_LOW ? 0 : 2, hp_ver = tx_ver == XVC_TX_DCT2_LOW ? 0 : 2;
  auto dct2 = [](int t) { return t == XVC_TX_DEFAULT || t == XVC_TX_DCT2 || t == XVC_TX_DCT2_LOW; };
  return {lgw + bd - 9 + hp_hor, lgh + 6 + hp_ver, 7 + hp_ver, 20 - bd + hp_hor,
          dct2(tx_ver) && dct2(tx_hor)};
}
// the 4x4 DST of intra luma (FwdPartialDst4 / InvPartialDst4, transform.cc:997-1017,
// :217-242): no high-precision shift in either stage, no DC-only inverse
__device__ __forceinline__ TxStageShifts tx_stage_shifts_dst4(int bd) {
  TxStageShifts s = tx_stage_shifts(XVC_TX_DCT2_LOW, XVC_TX_DCT2_LOW, 2, 2, bd);
  s.dct2_both = false;
  return s;
}

// ---- context bit costs -------------------------------------------------------------
// ContextModel::kEntropyBits_ (context_model.cc:75-93): bits = table[state ^ bin]
__constant__ uint32_t kEntropyBits[128] = {
#include "entropy_bits.inc"
};
#define RQ_BYPASS 32768u  // ContextModel::kEntropyBypassBits
// the same table in global memory (filled by xvcgpu_create): a lookup by lane from
// __constant__ memory is one scalar load per distinct index
__device__ uint32_t gEntropyBits[128];

// byte offsets of the context groups inside xvcgpu_rdoq_contexts
#define RQ_OFF(field) ((int)__builtin_offsetof(xvcgpu_rdoq_contexts, field))

__device__ __forceinline__ unsigned rq_bits(unsigned char state, int bin) {
  return kEntropyBits[state ^ bin];
}
__device__ __forceinline__ long long rq_bit_cost(unsigned bits, long long lambda) {
  return ((long long)bits * lambda) >> 16;
}

// GetEntropyBits(bin) of every context of a snapshot: cb[2 * i + bin] for the
// context at byte offset i of xvcgpu_rdoq_contexts; `table` = kEntropyBits or
// gEntropyBits.  A word of four contexts becomes its eight entries...
static_assert(sizeof(xvcgpu_rdoq_contexts) % 4 == 0, "whole words of contexts");
#define RQ_CTX_WORDS ((int)sizeof(xvcgpu_rdoq_contexts) / 4)
__device__ __forceinline__ void rq_stage_word(const uint32_t *table, uint32_t word, unsigned *cb8) {
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const unsigned st8 = (word >> (8 * k)) & 127;
    *reinterpret_cast<uint2 *>(cb8 + 2 * k) = make_uint2(table[st8], table[st8 ^ 1]);
  }
}
// ... and `lanes` lanes (lane = 0 .. lanes - 1) stage the snapshot a word per lane and
// round: two round trips (byte by byte: three dependent pairs).
__device__ __forceinline__ void rq_stage_costs(const uint32_t *table,
                                               const xvcgpu_rdoq_contexts *snap, unsigned *cb,
                                               int lane, int lanes) {
  const uint32_t *cw = reinterpret_cast<const uint32_t *>(snap);
  for (int wi = lane; wi < RQ_CTX_WORDS; wi += lanes) rq_stage_word(table, cw[wi], cb + 8 * wi);
}

// ---- context selection of a coefficient at position class posxy = x + y ----------
// (table indices: 2 * context, + bin)
// GetCoeffSigCtx (cabac.cc:520-560) without the template's count; size_cls = (log2 w +
// log2 h) / 2.  The context of a count n is 2 * min(n, 5) further on.
__device__ __forceinline__ int rq_sig_ctx_base(bool luma, int posxy, int size_cls) {
  int start = posxy < 2 ? 6 : 0;
  start += luma && posxy < 5 ? 6 : 0;
  start += size_cls > 2 && luma ? 18 << (size_cls - 3 < 1 ? size_cls - 3 : 1) : 0;
  return 2 * ((luma ? RQ_OFF(sig_luma) : RQ_OFF(sig_chroma)) + start);
}
// the greater-1 / greater-2 contexts (cabac.cc:594-684): the set's first context serves
// the last position; the others are chosen by the count field nn of a decision record:
// 0 for the last position, else min(greater-1 / greater-2 neighbours, 4) + 1
__device__ __forceinline__ int rq_greater1_off(bool luma) {
  return luma ? RQ_OFF(greater1_luma) : RQ_OFF(greater1_chroma);
}
__device__ __forceinline__ int rq_greater_start(bool luma, int posxy) {
  return luma ? (posxy < 3 ? 10 : (posxy < 10 ? 5 : 0)) : 0;
}
__device__ __forceinline__ int rq_greater_nn(int n, bool is_last) {
  return is_last ? 0 : (n < 4 ? n : 4) + 1;
}
__device__ __forceinline__ int rq_greater_ctx(bool luma, int posxy, int nn) {
  const int g1 = rq_greater1_off(luma);
  return nn == 0 ? 2 * g1 : 2 * (g1 + rq_greater_start(luma, posxy) + nn);
}

#endif  // XVCGPU_K_QUANT_H_
