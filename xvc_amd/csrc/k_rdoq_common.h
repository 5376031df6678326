// k_rdoq_common.h -- what the two walks of RdoQuant::QuantRdo (wave_rdoq, k_rdoq.h:
// a lane per sub-block; wave_rdoq4, k_rdoq4.h: four lanes per sub-block) share: the
// per-block scratch and its layout, the lane-group reductions, GetAbsLevelBits, the
// last-position bits and the 16-bit decision record.
#ifndef XVCGPU_K_RDOQ_COMMON_H_
#define XVCGPU_K_RDOQ_COMMON_H_

#include "dev_common.h"
#include "k_me.h"
#include "k_me2.h"
#include "k_quant.h"
#include "k_scan.h"
#include "xvcgpu_internal.h"

// Per-block scratch: N = coefficients of the (at most 32x32) low-frequency
// region; arrays indexed by rec_pos(x, y) (sub-block major, RQ_SB_STRIDE).
// Developer build (-DXVCGPU_TRACE): clock readings of the walk's sections, one
// row per workgroup of quant_rdo_packed_kernel (tools/trace_rdoq.py).
#ifdef XVCGPU_TRACE
__device__ unsigned long long g_rq_trace[4096][16];
#define RQ_TRACE(k)                                                          \
  do {                                                                       \
    if (threadIdx.x == 0 && blockIdx.x < 4096)                               \
      g_rq_trace[blockIdx.x][k] = __builtin_amdgcn_s_memtime();              \
  } while (0)
// the 100 MHz wall clock beside it (rows 2048 + workgroup, columns 0 / 1): what a
// tick of s_memtime is worth at the clock the chip runs this kernel at
#define RQ_TRACE_RT(k)                                                       \
  do {                                                                       \
    if (threadIdx.x == 0 && blockIdx.x < 2048)                               \
      g_rq_trace[2048 + blockIdx.x][k] = __builtin_amdgcn_s_memrealtime();   \
  } while (0)
#else
#define RQ_TRACE(k) do {} while (0)
#define RQ_TRACE_RT(k) do {} while (0)
#endif
// step times inside the diagonal loop, summed (rows' columns 11-13, 14 = diagonals)
#ifdef XVCGPU_TRACE
#define RQ_STEP_BEGIN() unsigned long long rq_t_ = __builtin_amdgcn_s_memtime(), rq_a_[4] = {0, 0, 0, 0}
#define RQ_STEP(i)                                              \
  do {                                                          \
    const unsigned long long n_ = __builtin_amdgcn_s_memtime(); \
    rq_a_[i] += n_ - rq_t_;                                     \
    rq_t_ = n_;                                                 \
  } while (0)
#define RQ_STEP_END()                                                           \
  do {                                                                          \
    if (threadIdx.x == 0 && blockIdx.x < 2048)                                  \
      for (int i_ = 0; i_ < 4; i_++) g_rq_trace[blockIdx.x][11 + i_] = rq_a_[i_]; \
  } while (0)
// a second set of four (EvalLastPos' parts): rows 2048 + workgroup
#define RQ_STEP2_BEGIN() rq_t_ = __builtin_amdgcn_s_memtime(); rq_a_[0] = rq_a_[1] = rq_a_[2] = rq_a_[3] = 0
#define RQ_STEP2_END()                                                          \
  do {                                                                          \
    if (threadIdx.x == 0 && blockIdx.x < 2048)                                  \
      for (int i_ = 0; i_ < 4; i_++) g_rq_trace[2048 + blockIdx.x][11 + i_] = rq_a_[i_]; \
  } while (0)
#else
#define RQ_STEP_BEGIN() do {} while (0)
#define RQ_STEP(i) do {} while (0)
#define RQ_STEP_END() do {} while (0)
#define RQ_STEP2_BEGIN() do {} while (0)
#define RQ_STEP2_END() do {} while (0)
#endif

// Per-coefficient records are laid out sub-block by sub-block with a stride of 17
// entries (rq_pos): the lanes of a group address the SAME offset of DIFFERENT
// sub-blocks together, and with the raster layout (stride 4 in x, 64 in y) the
// 16 lanes of a 16x16 block - and the four blocks of a wave - fell onto the same
// LDS banks (SQ_LDS_BANK_CONFLICT was 52 % of the LDS cycles).  17 is odd: any 16
// consecutive sub-blocks land on distinct banks for 1-, 2-, 4- and 8-byte entries.
#define RQ_SB_STRIDE 17
#define RQ_PADDED(n) ((n) + (n) / 16)
// the coefficient / level tiles of the packed kernel are copied 8 bytes at a
// time: stride 20 keeps every sub-block row 8-byte aligned
#define RQ_CF_STRIDE 20
#define RQ_CF_PADDED(n) ((n) + (n) / 4)

// wave_rdoq4's working levels (k_rdoq4.h): the corner's raster with two zero columns /
// rows to the right / below; its largest shape per coefficient budget: 4x16 / 8x32 /
// 32x32 ((w + 2) x (h + 2))
#define RQ_WL(n) ((n) + 2 * ((n) >= 1024 ? 64 : ((n) >= 256 ? 40 : 20)) + 4)

template <int N0>
struct RdoqShared {
  static constexpr int N = RQ_PADDED(N0);
  // coeff_cost_to_zero_ is not kept (8 bytes per coefficient: the records' size is
  // what limits the waves per CU): EvalLastPos recomputes a coefficient's entry
  // from what is kept - its level and its 16-bit decision record (rq ctz_of).
  // coeff_sig_bits_ / the sig-flag rate as what they are made of: the count that
  // selects the coefficient's significance context, 3 bits of its record - with
  // the records in LDS their size is what limits the waves per CU
  unsigned short rate_up[N];   // the decision-time state, 16 bits (RQ_STATE_PACK)
  // (delta_u - the quantisation error the sign hiding prices, rdo_quant.cc:360-365 - is
  // a function of the coefficient and its level: re-derived there, BlockQuant::err_of;
  // a sub-block's zero distortion stays in its owner lane's register)
  long long sb_code_cost[64];
  unsigned csbf_bits[64];      // csbf_bits_to_zero
  unsigned char csbf[64];
  unsigned char sb_live[64];   // the walk reaches the sub-block
  unsigned char sb_dcz[64];    // its k = 0 coefficient was decided with sig1 = 0 (rdo_quant.cc:343)
  unsigned char sb_of_scan[256];  // sub-block scan index -> sy * gw + sx
  unsigned lp_bits[32];        // EvalLastPos: last-position bits by group of x [0..15], of y [16..31]
  // GetEntropyBits(bin) of every context of the snapshot: [2 * i + bin] for the
  // context at byte offset i of xvcgpu_rdoq_contexts.  The walk looks a dozen
  // of these up per coefficient, each depending on the previous decision: from
  // global / constant memory that is a dozen dependent ~1 us round trips per
  // coefficient (the first version ran 0.86 ms per 1080p picture that way).
  alignas(8) unsigned ctx_bits[2 * sizeof(xvcgpu_rdoq_contexts)];
  alignas(8) int16_t wl[RQ_WL(N0)];
  // wave_rdoq4: the flag costs at / behind a scan position (blocks with a 64-point
  // side: up to 256 positions; the others re-use sb_code_cost)
  long long fcs_store[N0 >= 1024 ? 256 : 1];
};
template <int N0>
__device__ __forceinline__ long long *rq_fcs(RdoqShared<N0> &s) {
  return N0 >= 1024 ? s.fcs_store : s.sb_code_cost;
}

// The same members as pointers (packed kernel: per-coefficient arrays in
// global memory, the rest in LDS).
struct RdoqView {
  int16_t *wl;
  long long *fcs;
  unsigned short *rate_up;
  long long *sb_code_cost;
  unsigned *csbf_bits;
  unsigned char *csbf, *sb_live, *sb_dcz;
  unsigned char *sb_of_scan;
  unsigned *lp_bits;
  unsigned *ctx_bits;
};

__device__ __forceinline__ int rq_last_pos_group(int pos) {  // kLastPosGroupIdx
  if (pos < 4) return pos;
  const int l = 31 - __clz(pos);                // 4..7 -> 2, 8..15 -> 3, ...
  return 2 * l + ((pos >> (l - 1)) & 1);
}
// reductions over the G (64 or 32) lanes that share a block
template <int G>
__device__ __forceinline__ int rq_wave_max_i32(int v) {
#pragma unroll
  for (int s = 1; s < G; s <<= 1) {
    const int o = __shfl_xor(v, s, 64);
    v = o > v ? o : v;
  }
  return v;
}
template <int G>
__device__ __forceinline__ long long rq_wave_sum_i64(long long v) {
#pragma unroll
  for (int s = 1; s < G; s <<= 1) v += __shfl_xor(v, s, 64);
  return v;
}
template <int G>
__device__ __forceinline__ int rq_wave_sum_i32(int v) {
#pragma unroll
  for (int s = 1; s < G; s <<= 1) v += __shfl_xor(v, s, 64);
  return v;
}

// 64-bit sum over each aligned group of SEG (4 or 16) lanes without LDS traffic:
// three 32-bit DPP sums (the high word, and the low word as two 16-bit halves so
// that no partial sum can overflow); every lane of the group gets the total.
template <int SEG>
__device__ __forceinline__ long long rq_group_sum_i64(long long v) {
  const unsigned lo = (unsigned)v;
  const int hi = dpp_group_sum<SEG>((int)(v >> 32));
  const int l0 = dpp_group_sum<SEG>((int)(lo & 0xffffu));
  const int l1 = dpp_group_sum<SEG>((int)(lo >> 16));
  return (long long)(((unsigned long long)(unsigned)hi << 32) +
                     ((unsigned long long)(unsigned)l1 << 16) + (unsigned long long)(unsigned)l0);
}

// Inclusive prefix sum of a 64-bit value over each aligned row of 16 lanes (lane
// offsets ascending), by DPP row shifts - no LDS crossbar trips: four steps, both
// halves moved with the same control, lanes in front of the row's start read 0.
template <int N>
__device__ __forceinline__ long long rq_row_shr_add_i64(long long v) {
  const int lo = __builtin_amdgcn_update_dpp(0, (int)(unsigned)v, 0x110 + N, 0xF, 0xF, true);
  const int hi = __builtin_amdgcn_update_dpp(0, (int)(v >> 32), 0x110 + N, 0xF, 0xF, true);
  return v + (long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo);
}
__device__ __forceinline__ long long rq_row_scan_i64(long long v) {
  v = rq_row_shr_add_i64<1>(v);
  v = rq_row_shr_add_i64<2>(v);
  v = rq_row_shr_add_i64<4>(v);
  v = rq_row_shr_add_i64<8>(v);
  return v;
}

__device__ __forceinline__ long long *rq_fcs(RdoqView &v) { return v.fcs; }

struct RdoqCoeffState {  // RdoQuant::CoeffCodingState, the part the extended set reads
  int c1_idx, c2_idx;
  unsigned golomb_rice_k;
};

// The greater1 / greater2 flag costs of the coefficient's two contexts, loaded
// once per coefficient (c1[bin], c2[bin]); the function itself touches no memory.
struct RdoqFlagBits {
  unsigned c1_0, c1_1, c2_0, c2_1;
};
__device__ __forceinline__ unsigned rq_abs_level_bits(const RdoqFlagBits &f, int level,
                                                      const RdoqCoeffState &s) {
  const int base_level = s.c1_idx < 8 ? (2 + (s.c2_idx < 1)) : 1;
  // TransformHelper::kGolombRiceRangeExt = {6, 5, 6, 3, 3, ...} (transform.cc:61-63), as
  // arithmetic: a divergent lookup in constant memory costs a ~1 us round trip
  const unsigned threshold =
      s.golomb_rice_k < 3 ? (s.golomb_rice_k == 1 ? 5u : 6u) : 3u;
  unsigned bits = RQ_BYPASS;
  if (level >= base_level) {
    unsigned code = (unsigned)(level - base_level);
    if (code < (threshold << s.golomb_rice_k)) {
      bits += ((code >> s.golomb_rice_k) + 1 + s.golomb_rice_k) * RQ_BYPASS;
    } else {
      // the escape's prefix: the reference subtracts 2^k, 2^(k+1), ... while the
      // rest is not smaller (rdo_quant.cc:862-866); the sum of those powers is
      // 2^length - 2^k, so length = floor(log2(rest + 2^k))
      code -= threshold << s.golomb_rice_k;
      const int length = 31 - __clz((int)(code + (1u << s.golomb_rice_k)));
      bits += (unsigned)(length + (int)threshold + length + 1 - (int)s.golomb_rice_k) * RQ_BYPASS;
    }
    if (s.c1_idx < 8) {
      bits += f.c1_1;
      if (s.c2_idx < 1) bits += f.c2_1;
    }
  } else if (level == 1) {
    bits += f.c1_0;
  } else if (level == 2) {
    bits += f.c1_1 + f.c2_0;
  } else {
    return 0;
  }
  return bits;
}

// GetCoeffLastPosCtx (cabac.cc:727-770) + GetLastPosBits (rdo_quant.cc:900-947);
// returns the table index of the context
__device__ __forceinline__ int rq_last_pos_ctx(bool luma, int w, int h, int pos, bool is_x) {
  const int size = is_x ? w : h;
  if (luma) {
    const int l2 = rq_log2(size);
    const int off = l2 < 3 ? 0 : (l2 == 3 ? 3 : (l2 == 4 ? 6 : (l2 == 5 ? 10 : (l2 == 6 ? 15 : 21))));
    const int idx = off + (pos >> ((l2 + 1) >> 2));
    return 2 * ((is_x ? RQ_OFF(last_x_luma) : RQ_OFF(last_y_luma)) + idx);
  }
  const int shift = d_clip3(size >> 3, 0, 2);
  return 2 * ((is_x ? RQ_OFF(last_x_chroma) : RQ_OFF(last_y_chroma)) + (pos >> shift));
}
__device__ __forceinline__ unsigned rq_last_pos_bits(const unsigned *cb, bool luma, int w, int h,
                                                     int scan_order, int lx, int ly) {
  if (scan_order == 2) {
    int t = lx; lx = ly; ly = t;
    t = w; w = h; h = t;
  }
  const int gx = rq_last_pos_group(lx), gy = rq_last_pos_group(ly);
  unsigned bits = 0;
  int k;
  for (k = 0; k < gx; k++) bits += cb[rq_last_pos_ctx(luma, w, h, k, true) + 1];
  if (gx < rq_last_pos_group(w - 1)) bits += cb[rq_last_pos_ctx(luma, w, h, k, true)];
  for (k = 0; k < gy; k++) bits += cb[rq_last_pos_ctx(luma, w, h, k, false) + 1];
  if (gy < rq_last_pos_group(h - 1)) bits += cb[rq_last_pos_ctx(luma, w, h, k, false)];
  if (gx > 3) bits += (unsigned)((gx - 2) >> 1) * RQ_BYPASS;
  if (gy > 3) bits += (unsigned)((gy - 2) >> 1) * RQ_BYPASS;
  return bits;
}

// One axis of GetLastPosBits for a whole position GROUP g (every position of a
// group costs the same): the bits of the x (is_x) or y part in a block of
// (already scan-swapped) size w x h - rq_last_pos_bits = axis(group(x)) +
// axis(group(y)).  The context costs of all possible prefix bins are read
// together.
__device__ __forceinline__ unsigned rq_last_pos_group_bits(const unsigned *cb, bool luma, int w,
                                                           int h, int g, bool is_x) {
  const int gmax = rq_last_pos_group((is_x ? w : h) - 1);
  const int gc = gmax > 0 ? gmax - 1 : 0;
  unsigned one[10];
#pragma unroll
  for (int k = 0; k < 10; k++) one[k] = cb[rq_last_pos_ctx(luma, w, h, k < gc ? k : gc, is_x) + 1];
  const unsigned zero_bits = cb[rq_last_pos_ctx(luma, w, h, g < gc ? g : gc, is_x)];
  unsigned bits = 0;
#pragma unroll
  for (int k = 0; k < 10; k++) bits += k < g ? one[k] : 0u;
  if (g < gmax) bits += zero_bits;
  if (g > 3) bits += (unsigned)((g - 2) >> 1) * RQ_BYPASS;
  return bits;
}

// Position of scan offset k inside a sub-block: (x, y) packed as y << 2 | x.
__device__ __forceinline__ int rq_scan_pos(int sbs, int order, int k) {
  if (sbs == 2) return (int)((d_scan4_table(order) >> (4 * k)) & 15ull);
  // TransformHelper::kScanCoeff2x2 (transform.cc:65-69): {0,2,1,3} / raster / {0,2,1,3}
  const int p = order == 1 ? k : (((k & 1) << 1) | (k >> 1));
  return ((p >> 1) << 2) | (p & 1);
}

// 16 bits per coefficient, ALL that is kept of a decision: the template counts
// that select its three contexts - n1 / n2 = 0 for the last position, else
// min(greater-1 / greater-2 neighbours, 4) + 1 (cabac.cc:594-684), nsig =
// min(significant neighbours, 5) (cabac.cc:520-560); the contexts' position
// class is a function of x + y and is re-derived by the readers -, what
// GetAbsLevelBits reads of the budget (c1_idx < 8, c2_idx < 1) and the
// Golomb-Rice parameter (0..9).  A coefficient left at level 0 only needs n1 (the
// cost of its greater1 flag's zero bin) and nsig; RQ_STATE_NO_RATE marks the tail
// of the last sub-block, whose rate is 0.
#define RQ_STATE_PACK(n1, n2, c1_idx, c2_idx, k, nsig)                                   \
  ((unsigned short)((unsigned)(n1) | ((unsigned)(n2) << 3) |                              \
                    ((unsigned)((c1_idx) >= 8) << 6) | ((unsigned)((c2_idx) > 0) << 7) | \
                    ((unsigned)(k) << 8) | ((unsigned)(nsig) << 12)))
#define RQ_STATE_NO_RATE 0x8000u

#endif  // XVCGPU_K_RDOQ_COMMON_H_
