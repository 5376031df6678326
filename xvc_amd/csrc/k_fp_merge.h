// k_fp_merge.h -- merge mode for a whole P picture, between launches that exist
// (xvcgpu_frame_pass_merge): the plain search -> fp_merge_rank_kernel ->
// fp_merge_choice_kernel -> the flat pass's launches behind the search, reading the chosen
// results -> fp_merge_skip_kernel -> the flat pass's tail.
//
// fp_merge_rank_kernel is InterSearch::SearchMergeCandidates (inter_search.cc:165-197) for a
// CU: one wave per listed CU, two waves a workgroup, each with mc_metric_body's LDS (tmp 64 x
// 71, pred 64 x 64 16-bit entries: 34560 B a workgroup).  The wave reads its plain job for
// the geometry and takes the five candidates one after the other: MotionCompensationMv of
// the luma block into LDS (bi_mc_luma clips the vector as ClipMv does), SATD against the
// original (wave_compare).  No prediction goes to memory and there is no candidate-job
// array.  Lane 0 folds the ranking with merge_rank_fold (k_bipred.h), the arithmetic the
// CU-state walk's fold uses.  Shapes as fp_bi_back_mvp_cost_kernel: every w, h in {4, 8, 16,
// 32, 64}; any other shape, and a candidate that is not {0, -1}, gets UINT32_MAX.  The B
// pass's kernel (k_fp_bi_merge.h) takes candidates of either list, of both and of ref_idx > 0
// and shares fp_merge_uni_dist, fp_merge_write_ranking and fp_merge_skip_body with this file.
//
// The choice is the pass's own rule in closed-form bits - not the reference's RD comparison,
// which needs the entropy coder: cost_merge = dist[m0] + (((merge_side_bits + bits(m0)) *
// lambda16) >> 16) against fp_plain_cost (k_fp_affine.h), merge on <= (the reference
// evaluates merge first and a later mode replaces it only on strict <, cu_encoder.cc:449-481).
//
// The small kernels: one thread per CU, 256-thread workgroups, plain loads and stores, no
// LDS, no atomics.  nnz layouts the skip kernel reads: every form keeps a CU's Y, U, V
// counts at d_nnz[t], d_nnz[t + 1], d_nnz[t + 2] with t = d_luma_tx_index[i]
// (FrameDescriptors: 3 i) for the forms with a prediction picture, and t = 3 i for the
// _from_me forms (k_recon.h: tx2_job writes nnz_out[3 * ci + comp]).
//
// hipcc -Rpass-analysis=kernel-resource-usage, gfx950:
//   fp_merge_rank_kernel    56 VGPRs, 106 SGPRs (18 of them spilled to VGPR lanes), no
//                           scratch, LDS 34560 B, 2 waves / SIMD (LDS allows four workgroups
//                           = eight waves a CU = two a SIMD, so the registers cost nothing;
//                           the candidate loop is unrolled: rolled it takes 82 VGPRs and
//                           spills 46 SGPRs)
//   fp_merge_choice_kernel  26 VGPRs, 26 SGPRs, no scratch, no LDS, 8 waves / SIMD
//   fp_merge_skip_kernel     8 VGPRs, 12 SGPRs, no scratch, no LDS, 8 waves / SIMD
#ifndef XVCGPU_K_FP_MERGE_H_
#define XVCGPU_K_FP_MERGE_H_

#include "k_bipred.h"
#include "k_fp_affine.h"

static_assert(XVC_FP_MERGE_CANDS == XVC_CS_MERGE_CANDS, "one ranking arithmetic");

// bits(m) of SearchMergeCandidates (:176): the merge index's truncated unary length
__device__ __forceinline__ uint32_t fp_merge_idx_bits(int m) {
  return (uint32_t)(m + 1 - (m == XVC_FP_MERGE_CANDS - 1 ? 1 : 0));
}

// Is CU i one the list names?  order: strictly ascending, or null = 0 .. n_listed - 1
__device__ __forceinline__ bool fp_merge_listed(const int32_t *order, int n_listed, int i) {
  if (!order) return i < n_listed;
  int lo = 0, hi = n_listed;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (order[mid] < i) lo = mid + 1;
    else hi = mid;
  }
  return lo < n_listed && order[lo] == i;
}

// One candidate that uses one list, by one wave: the luma block at ClipMv(mx, my) of `ref`
// into pred, SATD against the original at src.  pred is free again on return.  Shared with
// the B pass's rank kernel (k_fp_bi_merge.h).
__device__ __forceinline__ uint32_t fp_merge_uni_dist(int bd, const xvcgpu_me_block &b,
                                                      const PlaneView &ref, int mx, int my,
                                                      const uint16_t *src, int src_stride,
                                                      int16_t *tmp, uint16_t *pred) {
  bi_mc_luma(bd, b, ref, mx, my, tmp, pred);
  wave_sync();
  const uint32_t dist =
      (uint32_t)wave_compare(XVC_METRIC_SATD, bd, 0, 0, b.w, b.h, src, src_stride, pred, b.w);
  wave_sync();   // pred is the next candidate's
  return dist;
}

// Lane 0's end of a rank kernel: the fold and the record
__device__ __forceinline__ void fp_merge_write_ranking(const uint32_t (&dist)[XVC_FP_MERGE_CANDS],
                                                       double lambda_sqrt,
                                                       xvcgpu_fp_merge_ranking *out) {
  double cost[XVC_FP_MERGE_CANDS];
  int rank[XVC_FP_MERGE_CANDS];
  xvcgpu_fp_merge_ranking r;
  r.num = merge_rank_fold(dist, lambda_sqrt, cost, rank);
  r.reserved = 0;
#pragma unroll
  for (int k = 0; k < XVC_FP_MERGE_CANDS; k++) {
    r.dist[k] = dist[k];
    r.order[k] = rank[k];
    r.cost[k] = cost[k];
  }
  *out = r;
}

// grid: ceil(n_listed / 2); block: 128.  n_cus bounds the indices of `order`.
__global__ void __launch_bounds__(128)
fp_merge_rank_kernel(PlaneView orig, PlaneView ref, int bd, const xvcgpu_me_block *me,
                     const xvcgpu_fp_merge_cand *cands, const int32_t *order, int n_listed,
                     int n_cus, double lambda_sqrt, xvcgpu_fp_merge_ranking *out) {
  __shared__ struct {
    int16_t tmp[64 * 71];
    uint16_t pred[64 * 64];
  } sh[2];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int g = __builtin_amdgcn_readfirstlane((int)blockIdx.x * 2 + wave);
  if (g >= n_listed) return;
  const int i = order ? __builtin_amdgcn_readfirstlane(order[g]) : g;
  if (i < 0 || i >= n_cus) return;
  const xvcgpu_me_block b = me[i];
  const bool pow2 = (b.w & (b.w - 1)) == 0 && (b.h & (b.h - 1)) == 0;
  const bool shape = pow2 && b.w >= 4 && b.h >= 4 && b.w <= 64 && b.h <= 64;
  const uint16_t *src = orig.p + (ptrdiff_t)b.y * orig.stride + b.x;
  uint32_t dist[XVC_FP_MERGE_CANDS];
#pragma unroll
  for (int m = 0; m < XVC_FP_MERGE_CANDS; m++) {
    const xvcgpu_fp_merge_cand c = cands[(size_t)i * XVC_FP_MERGE_CANDS + m];
    dist[m] = 0xffffffffu;
    // (one candidate per wave: the branch is scalar)
    if (!__builtin_amdgcn_readfirstlane((int)(shape && c.ref_idx[0] == 0 && c.ref_idx[1] == -1)))
      continue;
    dist[m] = fp_merge_uni_dist(bd, b, ref, c.mv[0][0], c.mv[0][1], src, orig.stride,
                                sh[wave].tmp, sh[wave].pred);
  }
  if (lane != 0) return;
  fp_merge_write_ranking(dist, lambda_sqrt, &out[i]);
}

// grid: ceil(n / 256); block: 256
__global__ void __launch_bounds__(256)
fp_merge_choice_kernel(const xvcgpu_me_block *me, const xvcgpu_me_result *res, int n,
                       const xvcgpu_fp_merge_cand *cands, const int32_t *order, int n_listed,
                       const xvcgpu_fp_merge_ranking *rank, uint32_t side_bits,
                       uint32_t merge_side_bits, xvcgpu_fp_merge_result *choice,
                       xvcgpu_me_result *chosen) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const xvcgpu_me_block b = me[i];
  xvcgpu_me_result q = res[i];
  xvcgpu_fp_merge_result c;
  if (q.subpel_dist == XVCGPU_ME_UNSUPPORTED) {
    memset(&c, 0xff, sizeof(c));
  } else {
    memset(&c, 0, sizeof(c));
    c.merge_idx = -1;
    c.cost_plain = fp_plain_cost(b, q, side_bits);
    c.cost_merge = 0xffffffffu;
    if (!(b.fullpel_mv & XVC_ME_USE_LIC) && fp_merge_listed(order, n_listed, i)) {
      const xvcgpu_fp_merge_ranking r = rank[i];
      const int m0 = r.order[0];
      c.num = r.num;
      if (m0 >= 0 && m0 < XVC_FP_MERGE_CANDS) {
        uint32_t d0 = 0xffffffffu;
#pragma unroll
        for (int m = 0; m < XVC_FP_MERGE_CANDS; m++)
          if (m == m0) d0 = r.dist[m];
        if (d0 != 0xffffffffu) {
          c.cost_merge = fp_bi_cost(d0, merge_side_bits + fp_merge_idx_bits(m0), b.lambda16);
          if (c.cost_merge <= c.cost_plain) {   // (merge is evaluated first: it stays on a tie)
            const xvcgpu_fp_merge_cand cd = cands[(size_t)i * XVC_FP_MERGE_CANDS + m0];
            c.use_merge = 1;
            c.merge_idx = m0;
            q.mv_x = cd.mv[0][0];
            q.mv_y = cd.mv[0][1];
            q.subpel_dist = d0;
          }
        }
      }
    }
    c.mv[0] = q.mv_x;
    c.mv[1] = q.mv_y;
    c.cost = c.use_merge ? c.cost_merge : c.cost_plain;
  }
  choice[i] = c;
  chosen[i] = q;
}

// skip = use_merge && no transform block of the CU has a level.  A record whose use_merge
// is neither 0 nor 1 (all ones: no search result) is left alone.  luma_tx_index: null = 3 i.
// Record: xvcgpu_fp_merge_result, or the B pass's xvcgpu_fp_bi_merge_result (k_fp_bi_merge.h)
template <class Record>
__device__ __forceinline__ void fp_merge_skip_body(const int32_t *nnz,
                                                   const int32_t *luma_tx_index, int n,
                                                   Record *choice) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int32_t use = choice[i].use_merge;
  if (use != 0 && use != 1) return;
  const int t = luma_tx_index ? luma_tx_index[i] : 3 * i;
  choice[i].skip = use == 1 && nnz[t] == 0 && nnz[t + 1] == 0 && nnz[t + 2] == 0;
}

// grid: ceil(n / 256); block: 256
__global__ void __launch_bounds__(256)
fp_merge_skip_kernel(const int32_t *nnz, const int32_t *luma_tx_index, int n,
                     xvcgpu_fp_merge_result *choice) {
  fp_merge_skip_body(nnz, luma_tx_index, n, choice);
}

#endif  // XVCGPU_K_FP_MERGE_H_
