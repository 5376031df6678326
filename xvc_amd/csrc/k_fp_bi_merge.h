// k_fp_bi_merge.h -- merge mode for a whole B picture, between launches that exist
// (xvcgpu_frame_pass_bi_refs_merge): the plain run of xvcgpu_frame_pass_bi_refs up to its
// choice -> fp_bi_merge_rank_kernel -> fp_bi_merge_choice_kernel -> the prediction, the
// residual pipeline and the CU records, reading the chosen records -> fp_bi_merge_skip_kernel
// -> the B tail.
//
// fp_bi_merge_rank_kernel is InterSearch::SearchMergeCandidates (inter_search.cc:165-197)
// with MotionCompensation's two branches (inter_prediction.cc:710-738) for a CU: one wave
// per listed CU, two waves a workgroup, each with the P kernel's LDS (tmp 64 x 71, pred
// 64 x 64 16-bit entries: 34560 B a workgroup).  A candidate names a picture per list through
// the pass's own tables: refs[slot[l][ref_idx[l]]].  One list used: fp_merge_uni_dist, the P
// kernel's body.  Both lists used: list 0's luma block at ClipMv of its own vector in the
// 14-bit intermediate form (MotionCompRefList with post_filter = false) goes into pred as
// int16; list 1's pass then reads each entry back in its output functor (McBiAvgInPlace) and
// stores AddAvgBi's sample (:1545-1547, wg_add_avg_bi's arithmetic) in its place.  Every path
// of mc_filter_block gives sample i to lane i % 64, so an entry is read and written by the
// lane that wrote it; the wave_sync between the passes is for tmp, which list 1's horizontal
// pass overwrites.  Then SATD against the original (wave_compare).  So the bi-directional
// branch needs no LDS beyond the P kernel's, no prediction goes to memory and there is no
// candidate-job array.  Lane 0 folds with merge_rank_fold (k_bipred.h).  A candidate that is
// not valid - an index outside -1 .. num_ref[l] - 1, no list used, a slot outside the
// reference table - and any CU shape outside w, h in {4, 8, 16, 32, 64} gets UINT32_MAX.
//
// The choice is the pass's own rule in closed-form bits, as k_fp_merge.h's: cost_merge =
// dist[m0] + (((merge_side_bits + bits(m0)) * lambda16) >> 16) against the plain choice's
// cost, merge on <=.  It also takes a candidate that is not valid as no merge, whatever the
// ranking record says: its pictures become slots of the prediction's jobs.
//
// The small kernels: one thread per CU, 256-thread workgroups, plain loads and stores, no
// atomics.  The tables are read with constant indices under a comparison.
//
// hipcc -Rpass-analysis=kernel-resource-usage, gfx950:
//   fp_bi_merge_rank_kernel    92 VGPRs, 106 SGPRs and 113 scalar values spilled to VGPR lanes,
//                              no scratch, LDS 34560 B, 2 waves / SIMD.  LDS allows four
//                              workgroups = eight waves a CU = two a SIMD, as for the P
//                              kernel; 92 VGPRs would allow five, so the registers and the
//                              lane spills of the two plane views cost no residency.  The
//                              candidate loop is left to the compiler, which keeps it
//                              rolled.
//   fp_bi_merge_choice_kernel  54 VGPRs, 42 SGPRs, no scratch, no LDS, 8 waves / SIMD.  The
//                              plain record is copied from array to array and a winner's
//                              fields are stored behind it, which keeps the fields the
//                              stage never reads out of private memory.
//   fp_bi_merge_skip_kernel    8 VGPRs, 12 SGPRs, no scratch, no LDS, 8 waves / SIMD
//   fp_merge_rank_kernel (k_fp_merge.h), whose per-candidate body and record write moved
//   into functions this file shares: 56 VGPRs, 106 SGPRs, 18 values spilled to VGPR lanes, no
//   scratch, LDS 34560 B, 2 waves / SIMD before and after; fp_merge_skip_kernel 8 VGPRs, 12
//   SGPRs before and after.
#ifndef XVCGPU_K_FP_BI_MERGE_H_
#define XVCGPU_K_FP_BI_MERGE_H_

#include "k_fp_bi_refs.h"
#include "k_fp_merge.h"

// List 1's output of a bi-directional candidate: pred[i] holds list 0's 14-bit sample;
// AddAvgBi of the two takes its place.
struct McBiAvgInPlace {
  static constexpr bool kInt14 = true;
  uint16_t *pred;
  int sh, off, smax;
  __device__ __forceinline__ McBiAvgInPlace(uint16_t *p, int bd) : pred(p) {
    const int head = 14 - bd;
    sh = (head > 2 ? head : 2) + 1;
    off = (1 << (sh - 1)) + 2 * 8192;
    smax = (1 << bd) - 1;
  }
  __device__ __forceinline__ void put(int i, int, int, int v) const {
    pred[i] = d_clip_bd(((int)(int16_t)pred[i] + v + off) >> sh, smax);
  }
};

// One bi-directional candidate by one wave: MotionCompensation's bi branch of the luma
// block into pred, SATD against the original at src.  pred is free again on return.
__device__ __forceinline__ uint32_t fp_merge_bi_dist(int bd, const xvcgpu_me_block &b,
                                                     const PlaneView &ref0, int mx0, int my0,
                                                     const PlaneView &ref1, int mx1, int my1,
                                                     const uint16_t *src, int src_stride,
                                                     int16_t *tmp, uint16_t *pred) {
  const McBlock m0(b.x, b.y, b.w, b.h, 0, mx0, my0, ref0, ref0.w, ref0.h);
  mc_filter_block<false, McWave>(bd, m0.cw, m0.ch, m0.fx, m0.fy, m0.ref, m0.rs, tmp,
                                 McInt14Dense{reinterpret_cast<int16_t *>(pred)});
  wave_sync();   // tmp is list 1's
  const McBlock m1(b.x, b.y, b.w, b.h, 0, mx1, my1, ref1, ref1.w, ref1.h);
  mc_filter_block<false, McWave>(bd, m1.cw, m1.ch, m1.fx, m1.fy, m1.ref, m1.rs, tmp,
                                 McBiAvgInPlace(pred, bd));
  wave_sync();
  const uint32_t dist =
      (uint32_t)wave_compare(XVC_METRIC_SATD, bd, 0, 0, b.w, b.h, src, src_stride, pred, b.w);
  wave_sync();   // pred is the next candidate's
  return dist;
}

// The table slot of picture r of list l; -1: the list is unused (r == -1) or r names none
__device__ __forceinline__ int fp_bi_merge_slot(const FpBiRefsDev &t, int l, int r) {
  int slot = -1;
#pragma unroll
  for (int ll = 0; ll < 2; ll++)
#pragma unroll
    for (int rr = 0; rr < XVC_CS_MAX_REFS; rr++)
      if (ll == l && rr == r && rr < t.num_ref[ll]) slot = t.slot[ll][rr];
  return slot;
}

// A candidate's validity and its slots (slot[l] = -1: list unused)
__device__ __forceinline__ bool fp_bi_merge_cand_slots(const FpBiRefsDev &t,
                                                       const xvcgpu_fp_merge_cand &c, int n_refs,
                                                       int slot[2]) {
  bool ok = c.ref_idx[0] >= 0 || c.ref_idx[1] >= 0;
#pragma unroll
  for (int l = 0; l < 2; l++) {
    slot[l] = fp_bi_merge_slot(t, l, c.ref_idx[l]);
    ok = ok && c.ref_idx[l] >= -1 && (c.ref_idx[l] == -1 || (slot[l] >= 0 && slot[l] < n_refs));
  }
  return ok;
}

// grid: ceil(n_listed / 2); block: 128.  n_cus bounds the indices of `order`.
__global__ void __launch_bounds__(128)
fp_bi_merge_rank_kernel(PlaneView orig, RefTable refs, FpBiRefsDev t, int bd,
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
  const xvcgpu_me_block b = t.me[0][0][i];
  const bool pow2 = (b.w & (b.w - 1)) == 0 && (b.h & (b.h - 1)) == 0;
  const bool shape = pow2 && b.w >= 4 && b.h >= 4 && b.w <= 64 && b.h <= 64;
  const uint16_t *src = orig.p + (ptrdiff_t)b.y * orig.stride + b.x;
  uint32_t dist[XVC_FP_MERGE_CANDS];
  for (int m = 0; m < XVC_FP_MERGE_CANDS; m++) {
    const xvcgpu_fp_merge_cand c = cands[(size_t)i * XVC_FP_MERGE_CANDS + m];
    dist[m] = 0xffffffffu;
    int slot[2];
    const bool ok = fp_bi_merge_cand_slots(t, c, refs.n, slot);
    // (one candidate per wave: the branches are scalar)
    if (!__builtin_amdgcn_readfirstlane((int)(shape && ok))) continue;
    const int s0 = __builtin_amdgcn_readfirstlane(slot[0]);
    const int s1 = __builtin_amdgcn_readfirstlane(slot[1]);
    if (s0 >= 0 && s1 >= 0) {
      dist[m] = fp_merge_bi_dist(bd, b, refs.pic[s0].c[0], c.mv[0][0], c.mv[0][1],
                                 refs.pic[s1].c[0], c.mv[1][0], c.mv[1][1], src, orig.stride,
                                 sh[wave].tmp, sh[wave].pred);
    } else {
      const int l = s0 >= 0 ? 0 : 1;
      dist[m] = fp_merge_uni_dist(bd, b, refs.pic[l ? s1 : s0].c[0], l ? c.mv[1][0] : c.mv[0][0],
                                  l ? c.mv[1][1] : c.mv[0][1], src, orig.stride, sh[wave].tmp,
                                  sh[wave].pred);
    }
  }
  if (lane != 0) return;
  fp_merge_write_ranking(dist, lambda_sqrt, &out[i]);
}

// Writes choice[i] (skip = 0) and chosen[i] for every CU, and the three prediction jobs
// inter[3 i + comp] of a CU where merge won.  plain: the plain run's records, not written;
// chosen is another array.
// grid: ceil(n / 256); block: 256
__global__ void __launch_bounds__(256)
fp_bi_merge_choice_kernel(FpBiRefsDev t, int n_refs, int n, const xvcgpu_fp_bi_refs_result *plain,
                          const xvcgpu_fp_merge_cand *cands, const int32_t *order, int n_listed,
                          const xvcgpu_fp_merge_ranking *rank, uint32_t merge_side_bits,
                          xvcgpu_fp_bi_merge_result *choice, xvcgpu_fp_bi_refs_result *chosen,
                          xvcgpu_inter_block *inter) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const xvcgpu_me_block b = t.me[0][0][i];
  // the plain record goes from array to array (the fields the stage never reads stay out of
  // private memory); a winner's fields follow
  chosen[i] = plain[i];
  const int search_list = plain[i].search_list;
  xvcgpu_fp_bi_merge_result c;
  if (search_list != 0 && search_list != 1) {   // all ones: no search result
    memset(&c, 0xff, sizeof(c));
    choice[i] = c;
    return;
  }
  memset(&c, 0, sizeof(c));
  c.merge_idx = -1;
  c.inter_dir = plain[i].inter_dir;
#pragma unroll
  for (int l = 0; l < 2; l++) {
    c.ref_idx[l] = plain[i].ref_idx[l];
    c.mv[l][0] = plain[i].mv[l][0];
    c.mv[l][1] = plain[i].mv[l][1];
  }
  c.cost_plain = plain[i].cost;
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
      const xvcgpu_fp_merge_cand cd = cands[(size_t)i * XVC_FP_MERGE_CANDS + m0];
      int slot[2];
      if (d0 != 0xffffffffu && fp_bi_merge_cand_slots(t, cd, n_refs, slot)) {
        c.cost_merge = fp_bi_cost(d0, merge_side_bits + fp_merge_idx_bits(m0), b.lambda16);
        if (c.cost_merge <= c.cost_plain) {   // (merge is evaluated first: it stays on a tie)
          c.use_merge = 1;
          c.merge_idx = m0;
          c.inter_dir = slot[0] >= 0 && slot[1] >= 0 ? 2 : (slot[0] >= 0 ? 0 : 1);
          xvcgpu_inter_block j;
          memset(&j, 0, sizeof(j));
          j.x = b.x;
          j.y = b.y;
          j.w = b.w;
          j.h = b.h;
#pragma unroll
          for (int l = 0; l < 2; l++) {
            const bool used = slot[l] >= 0;
            c.ref_idx[l] = used ? cd.ref_idx[l] : -1;
            c.mv[l][0] = used ? cd.mv[l][0] : 0;
            c.mv[l][1] = used ? cd.mv[l][1] : 0;
            j.ref[l] = (int8_t)slot[l];
            j.mv[l][0][0] = c.mv[l][0];
            j.mv[l][0][1] = c.mv[l][1];
          }
#pragma unroll
          for (int comp = 0; comp < 3; comp++) {
            j.comp = (uint8_t)comp;
            inter[3 * i + comp] = j;
          }
          chosen[i].inter_dir = c.inter_dir;
          chosen[i].cost = c.cost_merge;
#pragma unroll
          for (int l = 0; l < 2; l++) {
            chosen[i].ref_idx[l] = c.ref_idx[l];
            chosen[i].mv[l][0] = c.mv[l][0];
            chosen[i].mv[l][1] = c.mv[l][1];
          }
        }
      }
    }
  }
  c.cost = c.use_merge ? c.cost_merge : c.cost_plain;
  choice[i] = c;
}

// grid: ceil(n / 256); block: 256
__global__ void __launch_bounds__(256)
fp_bi_merge_skip_kernel(const int32_t *nnz, const int32_t *luma_tx_index, int n,
                        xvcgpu_fp_bi_merge_result *choice) {
  fp_merge_skip_body(nnz, luma_tx_index, n, choice);
}

#endif  // XVCGPU_K_FP_BI_MERGE_H_
