// k_fp_bi_refs.h -- the decisions of InterSearch::SearchMotion (inter_search.cc:198-259) for a
// whole B picture with up to XVC_CS_MAX_REFS reference pictures per list, between launches
// that exist (xvcgpu_frame_pass_bi_refs): one search per (list, picture) that is not a
// re-used one -> fp_bi_refs_uni_fold_kernel -> the SearchBiIterative step of every picture of
// the list that lost, by block class -> fp_bi_refs_choice_kernel -> the prediction
// (k_inter_pred.h) -> residual pipeline -> cu_info_from_choice_refs_kernel.
// Host twin: xvc_gpu::InterSearch::SearchMotionMultiBatch (host/xvc_gpu_ops.h), which reads
// every search result back to decide the next step.
//
// The folds: one thread per CU, 256-thread workgroups, plain loads and stores.  A job's
// single mvp stands for both AMVP entries of its (list, picture): the start index and
// EvalFinalMvpIdx's answer are both 0 and GetMvpBits(0, 2) = 1 is the constant in the prices.
// A list-1 picture that list 0 names too (same_poc_in_l0 >= 0) is not searched: SearchRefIdx
// takes list 0's distortion and vector (:536-542) and prices them with list 1's own predictor
// and index; the final choice compares against the best of the pictures only list 1 names
// (cost_l1_unique, :247-257).
//
// The refinement jobs lie by CU: job [i * Rmax + k] is CU i's step into picture k of its
// searched list, Rmax = max(num_ref); slot bytes {searched, other}, 255 = no job.  Launched
// through the CU list's search plan (bipred_search_refs_planned_kernel) a class instance
// runs over its own CUs only: workgroup g takes job order[g / Rmax] * Rmax + g % Rmax.  One
// launch per class over the class's adjacent bins (16: the three exact shapes and other16;
// 32: c32; 64: c64_team and c64_wave), which are one run of the plan's list; workgroups in
// list order, no XCD remap (a class's CUs are scattered over the picture anyway).
//
// The planned instance is bipred_search_body with the job index handed in; it adds one
// scalar load and a division by Rmax in front and leaves the body's budget as it is.
// hipcc -Rpass-analysis=kernel-resource-usage, gfx950, this instance and
// bipred_search_refs_kernel of the same class report the same figures:
//   <16>  78 VGPRs, 106 SGPRs, no scratch, LDS   5616 B, 6 waves / SIMD (4 waves a workgroup)
//   <32>  78 VGPRs, 106 SGPRs, no scratch, LDS  38544 B, 6 waves / SIMD (8 waves a workgroup)
//   <64>  82 VGPRs, 106 SGPRs, no scratch, LDS 146576 B, 2 waves / SIMD (8 waves a workgroup)
// What fits on a CU is decided by LDS for the two larger classes (160 KiB: four workgroups
// of the 32 class, one of the 64 class, = BI_WAVES's choice) and by registers for the 16
// class, as before.  The folds: uni fold 66 VGPRs, choice 48 VGPRs and 128 B / lane of
// scratch (its tables are indexed by the CU's own best pictures), CU records 18 VGPRs; one
// thread per CU, a few workgroups a picture.
#ifndef XVCGPU_K_FP_BI_REFS_H_
#define XVCGPU_K_FP_BI_REFS_H_

#include "dev_common.h"
#include "k_bipred.h"
#include "k_me_plan.h"
#include "xvcgpu_internal.h"

// dist + ((bits * lambda) >> 16) (SearchRefIdx :560-566, SearchBiIterative :418-424)
__device__ __forceinline__ uint32_t fp_bi_cost(uint32_t dist, uint32_t bits, uint32_t lambda16) {
  return dist + (uint32_t)(((uint64_t)bits * lambda16) >> 16);
}

// GetMvdBits of a list's vector against the job's predictor
__device__ __forceinline__ uint32_t fp_bi_mvd_bits(const xvcgpu_me_block &b, int mx, int my) {
  return d_mvd_bits(b.mvp_x, b.mvp_y, mx, my, (b.fullpel_mv & XVC_ME_FULLPEL_MV) ? 2 : 0);
}

// The pass's tables as the kernels read them.  res[1][r] of a re-used picture points at
// list 0's results of its twin (the host resolves it: the kernels read one array per entry).
struct FpBiRefsDev {
  const xvcgpu_me_block *me[2][XVC_CS_MAX_REFS];
  const xvcgpu_me_result *res[2][XVC_CS_MAX_REFS];
  int num_ref[2];
  int same[XVC_CS_MAX_REFS];   // list 1: the list-0 index of the same picture, or -1
  int slot[2][XVC_CS_MAX_REFS];
  int ref_poc[2][XVC_CS_MAX_REFS];
  uint32_t side_uni[2], side_bi;
  int rmax;
};

// The reference-index bits of GetInterPredBits (inter_search.cc:1091-1094, :1111-1113):
// truncated unary, the last index one bit less
__device__ __forceinline__ uint32_t fp_bi_ref_idx_bits(int num_ref, int r) {
  return num_ref <= 1 ? 0u : (uint32_t)(r + 1 - (r == num_ref - 1 ? 1 : 0));
}

// Prices every (list, picture) in index order, keeps the best per list on strict < and the
// best of list 1's unique pictures beside it, and writes the CU's Rmax refinement jobs of
// the list that lost (search_list = cost_0 <= cost_1 ? 1 : 0): blk = that (list, picture)'s
// search job, boot_mv = its uni-directional vector, other_mv = the other list's winner.
// choice: search_list, cost_list, cost_l1_unique, best_ref*, cost_uni; the rest zero until
// fp_bi_refs_choice_kernel.  A searched picture that answered XVCGPU_ME_UNSUPPORTED: the
// record all ones and no job.  grid: ceil(n / 256); block: 256.
__global__ void __launch_bounds__(256)
fp_bi_refs_uni_fold_kernel(FpBiRefsDev t, int n, xvcgpu_bi_block *jobs, uint8_t *slots,
                           xvcgpu_fp_bi_refs_result *choice) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  xvcgpu_fp_bi_refs_result c;
  memset(&c, 0, sizeof(c));
  int mvx[2][XVC_CS_MAX_REFS], mvy[2][XVC_CS_MAX_REFS];
  uint32_t best_cost[2] = {0xffffffffu, 0xffffffffu}, unique_cost = 0xffffffffu;
  int best[2] = {-1, -1}, best_unique = -1;
  bool bad = false;
#pragma unroll
  for (int l = 0; l < 2; l++)
#pragma unroll
    for (int r = 0; r < XVC_CS_MAX_REFS; r++) {
      c.cost_uni[l][r] = 0xffffffffu;
      mvx[l][r] = mvy[l][r] = 0;
      if (r >= t.num_ref[l]) continue;
      const xvcgpu_me_result q = t.res[l][r][i];
      const xvcgpu_me_block b = t.me[l][r][i];
      bad = bad || q.subpel_dist == XVCGPU_ME_UNSUPPORTED;
      const uint32_t bits = t.side_uni[l] + fp_bi_ref_idx_bits(t.num_ref[l], r) + 1 +
                            fp_bi_mvd_bits(b, q.mv_x, q.mv_y);
      const uint32_t cost = fp_bi_cost(q.subpel_dist, bits, b.lambda16);
      c.cost_uni[l][r] = cost;
      mvx[l][r] = q.mv_x;
      mvy[l][r] = q.mv_y;
      if (cost < best_cost[l]) {
        best_cost[l] = cost;
        best[l] = r;
      }
      if (l == 1 && t.same[r] < 0 && cost < unique_cost) {
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
  const int s = best_cost[0] <= best_cost[1] ? 1 : 0, o = 1 - s;
  int omx = 0, omy = 0, oslot = 0;
#pragma unroll
  for (int r = 0; r < XVC_CS_MAX_REFS; r++)
    if (r == best[o]) {
      omx = o ? mvx[1][r] : mvx[0][r];
      omy = o ? mvy[1][r] : mvy[0][r];
      oslot = o ? t.slot[1][r] : t.slot[0][r];
    }
#pragma unroll
  for (int k = 0; k < XVC_CS_MAX_REFS; k++) {
    if (k >= t.rmax) continue;
    if (k >= (s ? t.num_ref[1] : t.num_ref[0])) {
      slots[2 * (at + k)] = slots[2 * (at + k) + 1] = XVC_FP_BI_NO_JOB;
      continue;
    }
    xvcgpu_bi_block j;
    j.blk = (s ? t.me[1][k] : t.me[0][k])[i];
    j.other_mv_x = omx;
    j.other_mv_y = omy;
    j.boot_mv_x = s ? mvx[1][k] : mvx[0][k];
    j.boot_mv_y = s ? mvy[1][k] : mvy[0][k];
    jobs[at + k] = j;
    slots[2 * (at + k)] = (uint8_t)(s ? t.slot[1][k] : t.slot[0][k]);
    slots[2 * (at + k) + 1] = (uint8_t)oslot;
  }
  c.search_list = s;
  c.cost_list[0] = best_cost[0];
  c.cost_list[1] = best_cost[1];
  c.cost_l1_unique = unique_cost;
  c.best_ref[0] = best[0];
  c.best_ref[1] = best[1];
  c.best_ref_l1_unique = best_unique;
  choice[i] = c;
}

// One (list, picture)'s job and uni-directional result of CU i (r < num_ref[l])
__device__ __forceinline__ void fp_bi_refs_entry(const FpBiRefsDev &t, int l, int r, int i,
                                                 xvcgpu_me_block *b, xvcgpu_me_result *q,
                                                 int *slot) {
#pragma unroll
  for (int ll = 0; ll < 2; ll++)
#pragma unroll
    for (int rr = 0; rr < XVC_CS_MAX_REFS; rr++)
      if (ll == l && rr == r) {
        *b = t.me[ll][rr][i];
        *q = t.res[ll][rr][i];
        *slot = t.slot[ll][rr];
      }
}

// Prices the CU's refined pairs in picture order from UINT32_MAX on strict < (the searched
// list carries picture k's refined vector, the other list its uni-directional winner; each
// list's bits against its own (list, picture) predictor), ChooseUniOrBi(cost_l0,
// cost_l1_unique, cost_bi) (:247-257: bi where its cost is at most both, else list 0 on
// cost_l0 <= cost_l1_unique, else the best unique list-1 state), completes choice[i] and
// writes the CU's three prediction jobs inter[3 i + comp] with ref[l] = the table slot of
// the chosen picture, -1 for a list the CU does not use.  A CU marked all ones stays so and
// its jobs name no list.  grid: ceil(n / 256); block: 256.
__global__ void __launch_bounds__(256)
fp_bi_refs_choice_kernel(FpBiRefsDev t, int n, const xvcgpu_me_result *bi_res,
                         xvcgpu_fp_bi_refs_result *choice, xvcgpu_inter_block *inter) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const xvcgpu_me_block b00 = t.me[0][0][i];
  xvcgpu_fp_bi_refs_result c = choice[i];
  int dir = -1, slot_of[2] = {-1, -1};
  if (c.search_list == 0 || c.search_list == 1) {
    const int s = c.search_list, o = 1 - s;
    const int nr_s = s ? t.num_ref[1] : t.num_ref[0], nr_o = s ? t.num_ref[0] : t.num_ref[1];
    xvcgpu_me_block bo, bs;
    xvcgpu_me_result qo, qs;
    int slot_o = 0, slot_s = 0;
    fp_bi_refs_entry(t, o, c.best_ref[o], i, &bo, &qo, &slot_o);
    fp_bi_refs_entry(t, s, c.best_ref[s], i, &bs, &qs, &slot_s);
    const uint32_t bits_o = t.side_bi + fp_bi_ref_idx_bits(nr_o, c.best_ref[o]) + 1 +
                            fp_bi_mvd_bits(bo, qo.mv_x, qo.mv_y);
    uint32_t cost_bi = 0xffffffffu;
    int best_k = -1, bmx = 0, bmy = 0, bslot = 0;
#pragma unroll
    for (int k = 0; k < XVC_CS_MAX_REFS; k++) {
      c.bi_cost[k] = 0xffffffffu;
      c.bi_mv[k][0] = c.bi_mv[k][1] = 0;
      if (k >= nr_s) continue;
      const xvcgpu_me_result r = bi_res[(size_t)i * t.rmax + k];
      xvcgpu_me_block b;
      xvcgpu_me_result unused;
      int slot_k = 0;
      fp_bi_refs_entry(t, s, k, i, &b, &unused, &slot_k);
      // (a refinement nobody ran - a class above the call's max_block_size - never wins)
      const uint32_t cost =
          r.subpel_dist == XVCGPU_ME_UNSUPPORTED
              ? 0xffffffffu
              : fp_bi_cost(r.subpel_dist,
                           bits_o + fp_bi_ref_idx_bits(nr_s, k) + 1 + fp_bi_mvd_bits(b, r.mv_x, r.mv_y),
                           b.lambda16);
      c.bi_cost[k] = cost;
      c.bi_mv[k][0] = r.mv_x;
      c.bi_mv[k][1] = r.mv_y;
      if (cost < cost_bi) {
        cost_bi = cost;
        best_k = k;
        bmx = r.mv_x;
        bmy = r.mv_y;
        bslot = slot_k;
      }
    }
    if (best_k < 0) {   // no step improved on nothing: the pair stays the uni-directional one
      best_k = c.best_ref[s];
      bmx = qs.mv_x;
      bmy = qs.mv_y;
      bslot = slot_s;
    }
    c.cost_bi = cost_bi;
    const uint32_t cost0 = c.cost_list[0], cost1u = c.cost_l1_unique;
    dir = (cost_bi <= cost0 && cost_bi <= cost1u) ? 2 : (cost0 <= cost1u ? 0 : 1);
    c.inter_dir = dir;
    c.ref_idx[0] = c.ref_idx[1] = -1;
    c.mv[0][0] = c.mv[0][1] = c.mv[1][0] = c.mv[1][1] = 0;
    if (dir == 2) {
      c.cost = cost_bi;
      c.ref_idx[s] = best_k;
      c.mv[s][0] = bmx;
      c.mv[s][1] = bmy;
      slot_of[s] = bslot;
      c.ref_idx[o] = c.best_ref[o];
      c.mv[o][0] = qo.mv_x;
      c.mv[o][1] = qo.mv_y;
      slot_of[o] = slot_o;
    } else if (dir == 0) {
      const xvcgpu_me_result &q0 = s == 0 ? qs : qo;
      c.cost = cost0;
      c.ref_idx[0] = c.best_ref[0];
      c.mv[0][0] = q0.mv_x;
      c.mv[0][1] = q0.mv_y;
      slot_of[0] = s == 0 ? slot_s : slot_o;
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

struct FpBiRefsPocs {
  int poc[2][XVC_CS_MAX_REFS];
};

// cu_info_from_me_kernel (k_misc.h) for two lists: the deblocking records as the decoder
// fills them for a B picture (host/xvc_picture_decoder.cc:220-230) - ref_idx0 the chosen
// list-0 index, or -1 where list 0 is unused; ref_poc[l] the chosen picture's POC, or -1; all
// four corners the list's vector, an unused list zero.  grid: ceil(n / 256); block: 256.
__global__ void __launch_bounds__(256)
cu_info_from_choice_refs_kernel(const xvcgpu_me_block *blocks,
                                const xvcgpu_fp_bi_refs_result *choice, const int32_t *nnz,
                                const int32_t *luma_tx_index, int n, int qp_y, int qp_c,
                                FpBiRefsPocs pocs, xvcgpu_cu_info *cus) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const xvcgpu_me_block b = blocks[i];
  const xvcgpu_fp_bi_refs_result ch = choice[i];
  const bool used0 = ch.inter_dir == 0 || ch.inter_dir == 2;
  const bool used1 = ch.inter_dir == 1 || ch.inter_dir == 2;
  int poc0 = -1, poc1 = -1;
#pragma unroll
  for (int r = 0; r < XVC_CS_MAX_REFS; r++) {
    if (used0 && ch.ref_idx[0] == r) poc0 = pocs.poc[0][r];
    if (used1 && ch.ref_idx[1] == r) poc1 = pocs.poc[1][r];
  }
  xvcgpu_cu_info c;
  c.x = (uint16_t)b.x;
  c.y = (uint16_t)b.y;
  c.w = b.w;
  c.h = b.h;
  c.intra = 0;
  c.cbf_luma = nnz[luma_tx_index ? luma_tx_index[i] : i] != 0;
  c.qp_y = (int8_t)qp_y;
  c.qp_c = (int8_t)qp_c;
  c.ref_idx0 = used0 ? (int8_t)ch.ref_idx[0] : -1;
  c.reserved = 0;
  c.ref_poc[0] = poc0;
  c.ref_poc[1] = poc1;
  for (int k = 0; k < 4; k++) {
    c.mv[0][k][0] = used0 ? ch.mv[0][0] : 0;
    c.mv[0][k][1] = used0 ? ch.mv[0][1] : 0;
    c.mv[1][k][0] = used1 ? ch.mv[1][0] : 0;
    c.mv[1][k][1] = used1 ? ch.mv[1][1] : 0;
  }
  cus[i] = c;
}

// The refinement of one class's CUs (order[0 .. n_wg / jobs_per_cu): a run of the plan's
// list): workgroup g takes job order[g / jobs_per_cu] * jobs_per_cu + g % jobs_per_cu,
// wave-uniform.  grid: n_wg; block: 64 * BI_WAVES(MS).
template <int MS>
__global__ void __launch_bounds__(64 * BI_WAVES(MS))
bipred_search_refs_planned_kernel(PlaneView orig, RefTable refs, const uint8_t *slots, int bd,
                                  const xvcgpu_bi_block *jobs, const int *order, int n_wg,
                                  int jobs_per_cu, xvcgpu_me_result *out, int max_launched) {
  const int g = (int)blockIdx.x;
  if (g >= n_wg) return;
  const int cu = __builtin_amdgcn_readfirstlane(order[g / jobs_per_cu]);
  bipred_search_body<MS, false>(orig, orig, orig, bd, jobs, 0, out, max_launched, PlaneView(),
                                nullptr, &refs, slots, cu * jobs_per_cu + g % jobs_per_cu);
}

// The jobs of the CUs no instance takes: the XVCGPU_ME_UNSUPPORTED record where the slots
// name a job, as the 16 class's whole-list launch answers them.  One job per thread.
__global__ void __launch_bounds__(256)
bipred_refs_planned_unsupported_kernel(const int *order, int n_jobs, int jobs_per_cu,
                                       const uint8_t *slots, int n_refs,
                                       xvcgpu_me_result *out) {
  const int g = (int)(blockIdx.x * 256 + threadIdx.x);
  if (g >= n_jobs) return;
  const size_t ji = (size_t)order[g / jobs_per_cu] * jobs_per_cu + g % jobs_per_cu;
  if (slots[2 * ji] >= n_refs || slots[2 * ji + 1] >= n_refs) return;
  out[ji] = me2_unsupported_record();
}

#endif  // XVCGPU_K_FP_BI_REFS_H_
