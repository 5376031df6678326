// k_fp_bi.h -- the decisions of InterSearch::SearchMotion (inter_search.cc:198-259) for a
// whole B picture with one reference picture per list, between launches that exist
// (xvcgpu_frame_pass_bi): the two lists' searches -> fp_bi_uni_fold_kernel -> the
// SearchBiIterative step of either list (k_bipred.h) -> fp_bi_choice_kernel -> the
// prediction (k_inter_pred.h) -> residual pipeline -> cu_info_from_choice_kernel.
// Host twin: xvc_gpu::InterSearch::SearchMotionBatch (host/xvc_gpu_ops.h), which reads
// every search result back to decide the next step.
//
// One thread per CU, 256-thread workgroups, plain loads and stores.  A job's single mvp
// stands for both AMVP entries of its list: the start index and EvalFinalMvpIdx's answer
// are both 0 and GetMvpBits(0, 2) = 1 is the constant in the prices.
#ifndef XVCGPU_K_FP_BI_H_
#define XVCGPU_K_FP_BI_H_

#include "dev_common.h"
#include "xvcgpu_internal.h"

// dist + ((bits * lambda) >> 16) (SearchRefIdx :560-566, SearchBiIterative :418-424)
__device__ __forceinline__ uint32_t fp_bi_cost(uint32_t dist, uint32_t bits, uint32_t lambda16) {
  return dist + (uint32_t)(((uint64_t)bits * lambda16) >> 16);
}

// GetMvdBits of a list's vector against the job's predictor
__device__ __forceinline__ uint32_t fp_bi_mvd_bits(const xvcgpu_me_block &b, int mx, int my) {
  return d_mvd_bits(b.mvp_x, b.mvp_y, mx, my, (b.fullpel_mv & XVC_ME_FULLPEL_MV) ? 2 : 0);
}

// Prices both lists' uni-directional results and writes the refinement job of the list that
// lost (search_list = cost_0 <= cost_1 ? 1 : 0, :234) into that list's job array: blk = the
// list's search job, other_mv = the winner's vector, boot_mv = its own uni-directional
// vector.  The other list's slot gets a width-0 job, which the refinement kernel answers
// with the unsupported record and nobody reads.  choice: search_list and cost_uni, the rest
// zero until fp_bi_choice_kernel.  A list whose search answered XVCGPU_ME_UNSUPPORTED: the
// record all ones and a width-0 job in both slots.  grid: ceil(n / 256); block: 256.
__global__ void __launch_bounds__(256)
fp_bi_uni_fold_kernel(const xvcgpu_me_block *me0, const xvcgpu_me_block *me1,
                      const xvcgpu_me_result *res0, const xvcgpu_me_result *res1, int n,
                      uint32_t side_bits0, uint32_t side_bits1, xvcgpu_bi_block *jobs0,
                      xvcgpu_bi_block *jobs1, xvcgpu_fp_bi_result *choice) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const xvcgpu_me_result r0 = res0[i], r1 = res1[i];
  xvcgpu_bi_block none;
  memset(&none, 0, sizeof(none));
  xvcgpu_fp_bi_result c;
  if (r0.subpel_dist == XVCGPU_ME_UNSUPPORTED || r1.subpel_dist == XVCGPU_ME_UNSUPPORTED) {
    memset(&c, 0xff, sizeof(c));
    choice[i] = c;
    jobs0[i] = none;
    jobs1[i] = none;
    return;
  }
  const xvcgpu_me_block b0 = me0[i], b1 = me1[i];
  const uint32_t cost0 = fp_bi_cost(
      r0.subpel_dist, side_bits0 + 1 + fp_bi_mvd_bits(b0, r0.mv_x, r0.mv_y), b0.lambda16);
  const uint32_t cost1 = fp_bi_cost(
      r1.subpel_dist, side_bits1 + 1 + fp_bi_mvd_bits(b1, r1.mv_x, r1.mv_y), b1.lambda16);
  const int searched = cost0 <= cost1 ? 1 : 0;
  xvcgpu_bi_block j;
  j.blk = searched ? b1 : b0;
  j.other_mv_x = searched ? r0.mv_x : r1.mv_x;
  j.other_mv_y = searched ? r0.mv_y : r1.mv_y;
  j.boot_mv_x = searched ? r1.mv_x : r0.mv_x;
  j.boot_mv_y = searched ? r1.mv_y : r0.mv_y;
  jobs0[i] = searched ? none : j;
  jobs1[i] = searched ? j : none;
  memset(&c, 0, sizeof(c));
  c.search_list = searched;
  c.cost_uni[0] = cost0;
  c.cost_uni[1] = cost1;
  choice[i] = c;
}

// Prices the refined pair (the searched list carries the refined vector, the other list its
// uni-directional one; each difference against its own list's predictor), ChooseUniOrBi
// (:247-257: bi where its cost is at most both lists', else list 0 on cost_0 <= cost_1),
// completes choice[i] and writes the CU's three prediction jobs inter[3 i + comp]: slot l =
// list l, -1 for the list the CU does not use.  A CU marked all ones stays so and its jobs
// name no list (the prediction kernel then writes nothing).  grid: ceil(n / 256); block: 256.
__global__ void __launch_bounds__(256)
fp_bi_choice_kernel(const xvcgpu_me_block *me0, const xvcgpu_me_block *me1,
                    const xvcgpu_me_result *res0, const xvcgpu_me_result *res1,
                    const xvcgpu_me_result *bi_res0, const xvcgpu_me_result *bi_res1, int n,
                    uint32_t side_bits_bi, xvcgpu_fp_bi_result *choice,
                    xvcgpu_inter_block *inter) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const xvcgpu_me_block b0 = me0[i], b1 = me1[i];
  xvcgpu_fp_bi_result c = choice[i];
  int dir = -1;
  if (c.search_list == 0 || c.search_list == 1) {
    const int s = c.search_list;
    const xvcgpu_me_result bi = s ? bi_res1[i] : bi_res0[i];
    const xvcgpu_me_result r0 = res0[i], r1 = res1[i];
    const int mv0x = s ? r0.mv_x : bi.mv_x, mv0y = s ? r0.mv_y : bi.mv_y;
    const int mv1x = s ? bi.mv_x : r1.mv_x, mv1y = s ? bi.mv_y : r1.mv_y;
    const uint32_t bits = side_bits_bi + 2 + fp_bi_mvd_bits(b0, mv0x, mv0y) +
                          fp_bi_mvd_bits(b1, mv1x, mv1y);
    // (a refinement nobody ran - a class above the call's max_block_size - never wins)
    c.cost_bi = bi.subpel_dist == XVCGPU_ME_UNSUPPORTED
                    ? 0xffffffffu
                    : fp_bi_cost(bi.subpel_dist, bits, (s ? b1 : b0).lambda16);
    const uint32_t cost0 = c.cost_uni[0], cost1 = c.cost_uni[1];
    dir = (c.cost_bi <= cost0 && c.cost_bi <= cost1) ? 2 : (cost0 <= cost1 ? 0 : 1);
    c.inter_dir = dir;
    c.cost = dir == 2 ? c.cost_bi : (dir ? cost1 : cost0);
    c.mv[0][0] = dir == 2 ? mv0x : (dir == 0 ? r0.mv_x : 0);
    c.mv[0][1] = dir == 2 ? mv0y : (dir == 0 ? r0.mv_y : 0);
    c.mv[1][0] = dir == 2 ? mv1x : (dir == 1 ? r1.mv_x : 0);
    c.mv[1][1] = dir == 2 ? mv1y : (dir == 1 ? r1.mv_y : 0);
    c.bi_mv[0] = bi.mv_x;
    c.bi_mv[1] = bi.mv_y;
    choice[i] = c;
  }
  xvcgpu_inter_block q;
  memset(&q, 0, sizeof(q));
  q.x = b0.x;
  q.y = b0.y;
  q.w = b0.w;
  q.h = b0.h;
  q.ref[0] = (dir == 0 || dir == 2) ? 0 : -1;
  q.ref[1] = (dir == 1 || dir == 2) ? 1 : -1;
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

// cu_info_from_me_kernel (k_misc.h) for two lists: the deblocking records as the decoder
// fills them for a B picture (host/xvc_picture_decoder.cc:220-230) - ref_idx0 0, or -1
// where list 0 is unused; ref_poc[l] the list's POC, or -1; all four corners the list's
// vector, an unused list zero.  grid: ceil(n / 256); block: 256.
__global__ void __launch_bounds__(256)
cu_info_from_choice_kernel(const xvcgpu_me_block *blocks, const xvcgpu_fp_bi_result *choice,
                           const int32_t *nnz, const int32_t *luma_tx_index, int n, int qp_y,
                           int qp_c, int ref_poc0, int ref_poc1, xvcgpu_cu_info *cus) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const xvcgpu_me_block b = blocks[i];
  const xvcgpu_fp_bi_result ch = choice[i];
  const bool used0 = ch.inter_dir == 0 || ch.inter_dir == 2;
  const bool used1 = ch.inter_dir == 1 || ch.inter_dir == 2;
  xvcgpu_cu_info c;
  c.x = (uint16_t)b.x;
  c.y = (uint16_t)b.y;
  c.w = b.w;
  c.h = b.h;
  c.intra = 0;
  c.cbf_luma = nnz[luma_tx_index ? luma_tx_index[i] : i] != 0;
  c.qp_y = (int8_t)qp_y;
  c.qp_c = (int8_t)qp_c;
  c.ref_idx0 = used0 ? 0 : -1;
  c.reserved = 0;
  c.ref_poc[0] = used0 ? ref_poc0 : -1;
  c.ref_poc[1] = used1 ? ref_poc1 : -1;
  for (int k = 0; k < 4; k++) {
    c.mv[0][k][0] = used0 ? ch.mv[0][0] : 0;
    c.mv[0][k][1] = used0 ? ch.mv[0][1] : 0;
    c.mv[1][k][0] = used1 ? ch.mv[1][0] : 0;
    c.mv[1][k][1] = used1 ? ch.mv[1][1] : 0;
  }
  cus[i] = c;
}

#endif  // XVCGPU_K_FP_BI_H_
