// k_fp_bi_back.h -- the decisions of InterSearch::SearchMotion for a B picture whose
// references all lie before it (PictureData::DetermineForceBipredL1MvdZero: every inter
// picture of a low-delay encode), between the launches of k_fp_bi_refs.h
// (xvcgpu_frame_pass_bi_back): one search per (list, picture) that is not a re-used one ->
// fp_bi_back_mvp_cost_kernel -> fp_bi_back_uni_fold_kernel -> the SearchBiIterative step of
// every picture of list 0 -> fp_bi_back_choice_kernel -> prediction, residual pipeline, CU
// records and tail as in the two-directional pass.
//
// What the flag changes (inter_search.cc):
//   - list 1, uni-directional (:470-471, :496-524): the candidate of picture r is the
//     predictor itself, vector difference zero, priced by EvalStartMvp (:967-997): SAD(orig,
//     luma prediction at ClipMv(mvp)) + ((GetMvpBits(0, 2) * lambda16) >> 16) = SAD +
//     (lambda16 >> 16).  The best on strict < in index order is cost_l1 and list 1's state.
//     A re-used picture is then done; a unique one is searched as before and its cost goes
//     into cost_l1_unique only (:564-571).
//   - SearchBiIterative (:410-413): one iteration, list 0 is refined whatever the costs say,
//     against the predictor vector of list 1's best picture.
//   - bits of a bi-directional state: list 1 adds RefIdxBits + GetMvpBits and no
//     vector-difference bits (GetForceMvdZero).
//   - a bi-directional CU carries list 1's predictor (unclipped: the prediction clips it as
//     MotionCompensationMv does) as its list-1 vector; a list-1 CU the unique picture's
//     searched vector.
// The job's single mvp stands for both AMVP entries, as in k_fp_bi_refs.h: index 0.
//
// fp_bi_back_mvp_cost_kernel: one wave per (CU, list-1 picture), two waves a workgroup, each
// with mc_metric_body's LDS (tmp 64 x 71, pred 64 x 64 16-bit entries: 34560 B a
// workgroup).  It reads the search job d_me[1][r][i] itself: no candidate array.  Shapes:
// bi_mc_luma (mc_filter_block) and wave_sad index a row by shift and mask, and the LDS holds
// 64 x 64, so every w, h in {4, 8, 16, 32, 64} is taken - the sides of 4 of a partition
// included (a 4 x 8 block is 32 lanes of one wave iteration).  Any other shape gets
// UINT32_MAX, and the fold marks the CU all ones as for an unsupported search.
//
// hipcc -Rpass-analysis=kernel-resource-usage, gfx950:
//   fp_bi_back_mvp_cost_kernel  152 VGPRs, 54 SGPRs, no scratch, LDS 34560 B, 2 waves / SIMD
//                               (the eight-tap sums unrolled; LDS allows four workgroups =
//                               eight waves a CU = two a SIMD, so the registers cost nothing)
//   fp_bi_back_uni_fold_kernel   62 VGPRs, 32 SGPRs, no scratch, no LDS, 8 waves / SIMD
//   fp_bi_back_choice_kernel     40 VGPRs, 26 SGPRs, no scratch, no LDS, 8 waves / SIMD (the
//                               searched list is known, so no table is indexed by it)
// The folds are kernels of their own: the instances of k_fp_bi_refs.h are not touched and
// their figures stay as its header has them.
#ifndef XVCGPU_K_FP_BI_BACK_H_
#define XVCGPU_K_FP_BI_BACK_H_

#include "k_fp_bi_refs.h"

// List 1's search jobs and picture slots as the predictor-cost kernel reads them
struct FpBiBackL1 {
  const xvcgpu_me_block *me[XVC_CS_MAX_REFS];
  int slot[XVC_CS_MAX_REFS];
  int num_ref;
};

// EvalStartMvp of every (CU, list-1 picture): out[i * XVC_CS_MAX_REFS + r] = SAD(orig, luma
// prediction of d_me[1][r][i] from refs[slot[1][r]] at its mvp) + (lambda16 >> 16); r >=
// num_ref: UINT32_MAX (written by the CU's first wave); a shape nobody takes: UINT32_MAX.
// grid: ceil(n * num_ref / 2); block: 128.
__global__ void __launch_bounds__(128)
fp_bi_back_mvp_cost_kernel(PlaneView orig, RefTable refs, FpBiBackL1 t, int bd, int n,
                           uint32_t *out) {
  __shared__ struct {
    int16_t tmp[64 * 71];
    uint16_t pred[64 * 64];
  } sh[2];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int g = __builtin_amdgcn_readfirstlane((int)blockIdx.x * 2 + wave);
  if (g >= n * t.num_ref) return;
  const int i = g / t.num_ref, r = g - i * t.num_ref;
  const xvcgpu_me_block *me = t.me[0];
  int slot = t.slot[0];
#pragma unroll
  for (int k = 1; k < XVC_CS_MAX_REFS; k++)
    if (k == r) {
      me = t.me[k];
      slot = t.slot[k];
    }
  uint32_t *o = out + (size_t)i * XVC_CS_MAX_REFS;
  if (r == 0 && lane == 0)
    for (int k = t.num_ref; k < XVC_CS_MAX_REFS; k++) o[k] = 0xffffffffu;
  const xvcgpu_me_block b = me[i];
  const bool pow2 = (b.w & (b.w - 1)) == 0 && (b.h & (b.h - 1)) == 0;
  if (!pow2 || b.w < 4 || b.h < 4 || b.w > 64 || b.h > 64 || slot >= refs.n) {
    if (lane == 0) o[r] = 0xffffffffu;
    return;
  }
  bi_mc_luma(bd, b, refs.pic[slot].c[0], b.mvp_x, b.mvp_y, sh[wave].tmp, sh[wave].pred);
  wave_sync();
  const uint16_t *src = orig.p + (ptrdiff_t)b.y * orig.stride + b.x;
  const uint64_t sad = wave_compare(XVC_METRIC_SAD, bd, 0, 0, b.w, b.h, src, orig.stride,
                                    sh[wave].pred, b.w);
  if (lane == 0) o[r] = (uint32_t)sad + (b.lambda16 >> 16);
}

// The mvp of list 1's job (r, i), r < num_ref[1], and the picture's slot
__device__ __forceinline__ void fp_bi_back_l1_mvp(const FpBiRefsDev &t, int r, int i, int *mx,
                                                  int *my, int *slot) {
#pragma unroll
  for (int rr = 0; rr < XVC_CS_MAX_REFS; rr++)
    if (rr == r) {
      const xvcgpu_me_block b = t.me[1][rr][i];
      *mx = b.mvp_x;
      *my = b.mvp_y;
      *slot = t.slot[1][rr];
    }
}

// fp_bi_refs_uni_fold_kernel under force_l1_mvd_zero.  List 0 as there.  List 1:
// cost_uni[1][r] = l1_mvp_cost[i * XVC_CS_MAX_REFS + r], cost_list[1] its minimum on strict <
// in index order, best_ref[1] its picture; a unique picture's search result is priced as
// there into cost_l1_unique / best_ref_l1_unique only.  search_list = 0: job [i * Rmax + k],
// k < num_ref[0]: blk = d_me[0][k][i], boot_mv = list 0's vector of k, other_mv = the mvp of
// d_me[1][best_ref[1]][i], slot bytes {slot[0][k], slot[1][best_ref[1]]}; k >= num_ref[0]: no
// job.  An unsupported search or predictor cost: the record all ones and no job.
// grid: ceil(n / 256); block: 256.
__global__ void __launch_bounds__(256)
fp_bi_back_uni_fold_kernel(FpBiRefsDev t, int n, const uint32_t *l1_mvp_cost,
                           xvcgpu_bi_block *jobs, uint8_t *slots,
                           xvcgpu_fp_bi_refs_result *choice) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  xvcgpu_fp_bi_refs_result c;
  memset(&c, 0, sizeof(c));
  int mvx[XVC_CS_MAX_REFS], mvy[XVC_CS_MAX_REFS];
  uint32_t best_cost[2] = {0xffffffffu, 0xffffffffu}, unique_cost = 0xffffffffu;
  int best[2] = {-1, -1}, best_unique = -1;
  bool bad = false;
#pragma unroll
  for (int r = 0; r < XVC_CS_MAX_REFS; r++) {
    c.cost_uni[0][r] = c.cost_uni[1][r] = 0xffffffffu;
    mvx[r] = mvy[r] = 0;
  }
#pragma unroll
  for (int r = 0; r < XVC_CS_MAX_REFS; r++) {
    if (r >= t.num_ref[0]) continue;
    const xvcgpu_me_result q = t.res[0][r][i];
    const xvcgpu_me_block b = t.me[0][r][i];
    bad = bad || q.subpel_dist == XVCGPU_ME_UNSUPPORTED;
    const uint32_t bits = t.side_uni[0] + fp_bi_ref_idx_bits(t.num_ref[0], r) + 1 +
                          fp_bi_mvd_bits(b, q.mv_x, q.mv_y);
    const uint32_t cost = fp_bi_cost(q.subpel_dist, bits, b.lambda16);
    c.cost_uni[0][r] = cost;
    mvx[r] = q.mv_x;
    mvy[r] = q.mv_y;
    if (cost < best_cost[0]) {
      best_cost[0] = cost;
      best[0] = r;
    }
  }
#pragma unroll
  for (int r = 0; r < XVC_CS_MAX_REFS; r++) {
    if (r >= t.num_ref[1]) continue;
    const uint32_t pc = l1_mvp_cost[(size_t)i * XVC_CS_MAX_REFS + r];
    bad = bad || pc == 0xffffffffu;
    c.cost_uni[1][r] = pc;
    if (pc < best_cost[1]) {
      best_cost[1] = pc;
      best[1] = r;
    }
    if (t.same[r] >= 0) continue;   // :521-523: a re-used picture is done
    const xvcgpu_me_result q = t.res[1][r][i];
    const xvcgpu_me_block b = t.me[1][r][i];
    bad = bad || q.subpel_dist == XVCGPU_ME_UNSUPPORTED;
    const uint32_t bits = t.side_uni[1] + fp_bi_ref_idx_bits(t.num_ref[1], r) + 1 +
                          fp_bi_mvd_bits(b, q.mv_x, q.mv_y);
    const uint32_t cost = fp_bi_cost(q.subpel_dist, bits, b.lambda16);
    if (cost < unique_cost) {
      unique_cost = cost;
      best_unique = r;
    }
  }
  const size_t at = (size_t)i * t.rmax;
  if (bad || best[0] < 0 || best[1] < 0) {
    memset(&c, 0xff, sizeof(c));
    choice[i] = c;
    for (int k = 0; k < t.rmax; k++) slots[2 * (at + k)] = slots[2 * (at + k) + 1] = XVC_FP_BI_NO_JOB;
    return;
  }
  int omx = 0, omy = 0, oslot = 0;
  fp_bi_back_l1_mvp(t, best[1], i, &omx, &omy, &oslot);
#pragma unroll
  for (int k = 0; k < XVC_CS_MAX_REFS; k++) {
    if (k >= t.rmax) continue;
    if (k >= t.num_ref[0]) {
      slots[2 * (at + k)] = slots[2 * (at + k) + 1] = XVC_FP_BI_NO_JOB;
      continue;
    }
    xvcgpu_bi_block j;
    j.blk = t.me[0][k][i];
    j.other_mv_x = omx;
    j.other_mv_y = omy;
    j.boot_mv_x = mvx[k];
    j.boot_mv_y = mvy[k];
    jobs[at + k] = j;
    slots[2 * (at + k)] = (uint8_t)t.slot[0][k];
    slots[2 * (at + k) + 1] = (uint8_t)oslot;
  }
  c.search_list = 0;
  c.cost_list[0] = best_cost[0];
  c.cost_list[1] = best_cost[1];
  c.cost_l1_unique = unique_cost;
  c.best_ref[0] = best[0];
  c.best_ref[1] = best[1];
  c.best_ref_l1_unique = best_unique;
  choice[i] = c;
}

// fp_bi_refs_choice_kernel under force_l1_mvd_zero: list 0's refined pairs in picture order
// from UINT32_MAX on strict <; bits = side_bits_bi + list 0's RefIdxBits + 1 + mvd bits +
// list 1's RefIdxBits(best_ref[1]) + 1 and no vector difference; ChooseUniOrBi(cost_l0,
// cost_l1_unique, cost_bi) unchanged.  A bi-directional CU's mv[1] is the mvp of
// d_me[1][best_ref[1]][i]; a list-1 CU carries the unique picture's searched vector.
// grid: ceil(n / 256); block: 256.
__global__ void __launch_bounds__(256)
fp_bi_back_choice_kernel(FpBiRefsDev t, int n, const xvcgpu_me_result *bi_res,
                         xvcgpu_fp_bi_refs_result *choice, xvcgpu_inter_block *inter) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const xvcgpu_me_block b00 = t.me[0][0][i];
  xvcgpu_fp_bi_refs_result c = choice[i];
  int dir = -1, slot_of[2] = {-1, -1};
  if (c.search_list == 0) {
    const int nr0 = t.num_ref[0];
    int pmx = 0, pmy = 0, slot_1 = 0;
    fp_bi_back_l1_mvp(t, c.best_ref[1], i, &pmx, &pmy, &slot_1);
    xvcgpu_me_block b0;
    xvcgpu_me_result q0;
    int slot_0 = 0;
    fp_bi_refs_entry(t, 0, c.best_ref[0], i, &b0, &q0, &slot_0);
    const uint32_t bits_1 = t.side_bi + fp_bi_ref_idx_bits(t.num_ref[1], c.best_ref[1]) + 1;
    uint32_t cost_bi = 0xffffffffu;
    int best_k = -1, bmx = 0, bmy = 0, bslot = 0;
#pragma unroll
    for (int k = 0; k < XVC_CS_MAX_REFS; k++) {
      c.bi_cost[k] = 0xffffffffu;
      c.bi_mv[k][0] = c.bi_mv[k][1] = 0;
      if (k >= nr0) continue;
      const xvcgpu_me_result r = bi_res[(size_t)i * t.rmax + k];
      const xvcgpu_me_block b = t.me[0][k][i];
      // (a refinement nobody ran - a class above the call's max_block_size - never wins)
      const uint32_t cost =
          r.subpel_dist == XVCGPU_ME_UNSUPPORTED
              ? 0xffffffffu
              : fp_bi_cost(r.subpel_dist,
                           bits_1 + fp_bi_ref_idx_bits(nr0, k) + 1 + fp_bi_mvd_bits(b, r.mv_x, r.mv_y),
                           b.lambda16);
      c.bi_cost[k] = cost;
      c.bi_mv[k][0] = r.mv_x;
      c.bi_mv[k][1] = r.mv_y;
      if (cost < cost_bi) {
        cost_bi = cost;
        best_k = k;
        bmx = r.mv_x;
        bmy = r.mv_y;
        bslot = t.slot[0][k];
      }
    }
    if (best_k < 0) {   // no step improved on nothing: the pair stays the uni-directional one
      best_k = c.best_ref[0];
      bmx = q0.mv_x;
      bmy = q0.mv_y;
      bslot = slot_0;
    }
    c.cost_bi = cost_bi;
    const uint32_t cost0 = c.cost_list[0], cost1u = c.cost_l1_unique;
    dir = (cost_bi <= cost0 && cost_bi <= cost1u) ? 2 : (cost0 <= cost1u ? 0 : 1);
    c.inter_dir = dir;
    c.ref_idx[0] = c.ref_idx[1] = -1;
    c.mv[0][0] = c.mv[0][1] = c.mv[1][0] = c.mv[1][1] = 0;
    if (dir == 2) {
      c.cost = cost_bi;
      c.ref_idx[0] = best_k;
      c.mv[0][0] = bmx;
      c.mv[0][1] = bmy;
      slot_of[0] = bslot;
      c.ref_idx[1] = c.best_ref[1];
      c.mv[1][0] = pmx;
      c.mv[1][1] = pmy;
      slot_of[1] = slot_1;
    } else if (dir == 0) {
      c.cost = cost0;
      c.ref_idx[0] = c.best_ref[0];
      c.mv[0][0] = q0.mv_x;
      c.mv[0][1] = q0.mv_y;
      slot_of[0] = slot_0;
    } else {
      xvcgpu_me_block bu;
      xvcgpu_me_result qu;
      int slot_u = 0;
      fp_bi_refs_entry(t, 1, c.best_ref_l1_unique, i, &bu, &qu, &slot_u);
      c.cost = cost1u;
      c.ref_idx[1] = c.best_ref_l1_unique;
      c.mv[1][0] = qu.mv_x;
      c.mv[1][1] = qu.mv_y;
      slot_of[1] = slot_u;
    }
    choice[i] = c;
  }
  xvcgpu_inter_block q;
  memset(&q, 0, sizeof(q));
  q.x = b00.x;
  q.y = b00.y;
  q.w = b00.w;
  q.h = b00.h;
  q.ref[0] = (int8_t)slot_of[0];
  q.ref[1] = (int8_t)slot_of[1];
  if (dir >= 0) {
    q.mv[0][0][0] = c.mv[0][0];
    q.mv[0][0][1] = c.mv[0][1];
    q.mv[1][0][0] = c.mv[1][0];
    q.mv[1][0][1] = c.mv[1][1];
  }
  for (int comp = 0; comp < 3; comp++) {
    q.comp = (uint8_t)comp;
    inter[3 * i + comp] = q;
  }
}

#endif  // XVCGPU_K_FP_BI_BACK_H_
