// k_fp_affine.h -- the second SearchMotion run of InterSearch::CompressInter
// (inter_search.cc:74-99) for a whole P picture, between launches that exist
// (xvcgpu_frame_pass_affine): the plain search -> fp_affine_boot_kernel -> the affine search
// of the capable CUs only (affine_me_listed_kernel) -> fp_affine_choice_kernel -> the
// prediction (k_inter_pred.h: XVC_INTER_AFFINE jobs) -> residual pipeline ->
// cu_info_from_affine_choice_kernel -> the flat pass's tail.
// Host twin: the CU-state walk (k_cu_state.h and its host driver), which folds one CU at a
// time.
//
// The small kernels: one thread per CU (boot: per listed CU), 256-thread workgroups, plain
// loads and stores, no LDS, no atomics.  A job's mvp stands for both AMVP entries: start
// index and EvalFinalMvpIdx's answer are 0 and GetMvpBits(0, 2) = 1 is the constant in the
// prices.  Both prices keep the reference's 64-bit product (Bits * lambda >> 16, :563).
//
// The listed instance is affine_me_body with the job index handed in: one scalar load of
// the index and one of the job's flag byte in front, the body's budget as it is.
// hipcc -Rpass-analysis=kernel-resource-usage, gfx950: affine_me_kernel<NW> and the listed
// instance report the same figures,
//   <2>  132 VGPRs, 104 SGPRs, 32 B / lane scratch, LDS 11024 B, 3 waves / SIMD (2 waves a workgroup)
//   <4>  136 VGPRs, 104 SGPRs, 32 B / lane scratch, LDS 22048 B, 3 waves / SIMD (4 waves a workgroup)
//   <8>  144 VGPRs, 104 SGPRs, 32 B / lane scratch, LDS 44096 B, 3 waves / SIMD (8 waves a workgroup)
// (the scratch is affine_solve's, as before).  The folds: boot 9 VGPRs, choice 79 VGPRs (it
// holds two 68-byte prediction jobs' worth of registers; a few workgroups a picture), CU
// records 26 VGPRs; none with scratch or LDS.
#ifndef XVCGPU_K_FP_AFFINE_H_
#define XVCGPU_K_FP_AFFINE_H_

#include "dev_common.h"
#include "k_affine_me.h"
#include "k_fp_bi_refs.h"
#include "xvcgpu_internal.h"

// CodingUnit::CanUseAffine (coding_unit.h:251-257) on the sides the search has instances
// for, and a plain job the second run would repeat as it is (no fullpel vectors, no LIC)
__device__ __forceinline__ bool fp_affine_capable(const xvcgpu_me_block &b) {
  return (b.w == 16 || b.w == 32 || b.w == 64) && (b.h == 16 || b.h == 32 || b.h == 64) &&
         !(b.fullpel_mv & (XVC_ME_FULLPEL_MV | XVC_ME_USE_LIC));
}

// The exp-Golomb bits of corner 0's and corner 1's quarter-sample difference to the job's
// predictor (SetMvd<MotionVector3> :1034-1048, GetInterPredBits :1097-1101)
__device__ __forceinline__ uint32_t fp_affine_mvd_bits(const int32_t mvp[3][2],
                                                       const int32_t mv[3][2]) {
  return d_mvd_bits(mvp[0][0], mvp[0][1], mv[0][0], mv[0][1], 0) +
         d_mvd_bits(mvp[1][0], mvp[1][1], mv[1][0], mv[1][1], 0);
}

// The searched (translational) state's price: subpel_dist + (((side_bits + 1 + GetMvdBits(mvp,
// mv, fullpel ? 2 : 0)) * lambda16) >> 16).  Its callers: the choice below and the merge
// pass's (k_fp_merge.h).
__device__ __forceinline__ uint32_t fp_plain_cost(const xvcgpu_me_block &b,
                                                  const xvcgpu_me_result &q, uint32_t side_bits) {
  return fp_bi_cost(q.subpel_dist, side_bits + 1 + fp_bi_mvd_bits(b, q.mv_x, q.mv_y), b.lambda16);
}

// grid: ceil(n_listed / 256); block: 256.  n_cus bounds the indices of `order`.
__global__ void __launch_bounds__(256)
fp_affine_boot_kernel(const xvcgpu_me_result *res, const int32_t *order, int n_listed,
                      int n_cus, int pic_w, int pic_h, xvcgpu_affine_me_block *jobs) {
  const int g = blockIdx.x * 256 + threadIdx.x;
  if (g >= n_listed) return;
  const int i = order[g];
  if (i < 0 || i >= n_cus) return;
  const xvcgpu_me_result q = res[i];
  xvcgpu_affine_me_block *j = &jobs[i];
  int mx = 0, my = 0;
  uint8_t flags = XVC_AFFINE_ME_NO_JOB;
  if (q.subpel_dist != XVCGPU_ME_UNSUPPORTED) {
    mx = q.mv_x;
    my = q.mv_y;
    d_clip_mv(j->x, j->y, pic_w, pic_h, mx, my);
    flags = XVC_AFFINE_ME_HAS_BOOTSTRAP;
  }
#pragma unroll
  for (int k = 0; k < 3; k++) {
    j->bootstrap[k][0] = mx;
    j->bootstrap[k][1] = my;
  }
  j->flags = flags;
}

// grid: the class's listed jobs; block: 64 * NW.  order: the class's run of the list.
template <int NW>
__global__ void __launch_bounds__(64 * NW)
affine_me_listed_kernel(PlaneView orig, PlaneView ref, int bd,
                        const xvcgpu_affine_me_block *blocks, int n, const int32_t *order,
                        int n_listed, xvcgpu_affine_me_result *out) {
  const int g = (int)blockIdx.x;
  if (g >= n_listed) return;
  const int job = __builtin_amdgcn_readfirstlane(order[g]);
  if (job < 0 || job >= n) return;
  if (blocks[job].flags & XVC_AFFINE_ME_NO_JOB) return;
  affine_me_body<NW>(orig, ref, ref, bd, blocks, n, out, nullptr, nullptr, job);
}

// grid: ceil(n / 256); block: 256
__global__ void __launch_bounds__(256)
fp_affine_choice_kernel(const xvcgpu_me_block *me, const xvcgpu_me_result *res, int n,
                        const xvcgpu_affine_me_block *jobs,
                        const xvcgpu_affine_me_result *ares, uint32_t side_bits,
                        xvcgpu_fp_affine_result *choice, xvcgpu_inter_block *inter) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const xvcgpu_me_block b = me[i];
  const xvcgpu_me_result q = res[i];
  xvcgpu_inter_block p;
  memset(&p, 0, sizeof(p));
  p.x = b.x;
  p.y = b.y;
  p.w = b.w;
  p.h = b.h;
  p.ref[0] = p.ref[1] = -1;
  xvcgpu_fp_affine_result c;
  if (q.subpel_dist == XVCGPU_ME_UNSUPPORTED) {
    memset(&c, 0xff, sizeof(c));
  } else {
    memset(&c, 0, sizeof(c));
    c.cost_plain = fp_plain_cost(b, q, side_bits);
    c.cost_affine = 0xffffffffu;
    const xvcgpu_affine_me_block j = jobs[i];
    if (fp_affine_capable(b) && (j.flags & XVC_AFFINE_ME_HAS_BOOTSTRAP)) {
      const xvcgpu_affine_me_result r = ares[i];
      const uint32_t bits = side_bits + 1 + fp_affine_mvd_bits(j.mvp, r.mv);
      c.cost_affine = fp_bi_cost(r.dist, bits, j.lambda16);
      c.dist_affine = r.dist;
      c.iterations = r.iterations;
      if (c.cost_affine < c.cost_plain) {   // (:90: the first run's state on a tie)
        c.use_affine = 1;
#pragma unroll
        for (int k = 0; k < 3; k++) {
          c.mv[k][0] = r.mv[k][0];
          c.mv[k][1] = r.mv[k][1];
        }
      }
    }
    if (!c.use_affine) {
#pragma unroll
      for (int k = 0; k < 3; k++) {
        c.mv[k][0] = q.mv_x;
        c.mv[k][1] = q.mv_y;
      }
    }
    c.cost = c.use_affine ? c.cost_affine : c.cost_plain;
    p.ref[0] = 0;
    p.mv[0][0][0] = c.mv[0][0];
    p.mv[0][0][1] = c.mv[0][1];
    if (c.use_affine) {
      p.flags = XVC_INTER_AFFINE;
      p.mv[0][1][0] = c.mv[1][0];
      p.mv[0][1][1] = c.mv[1][1];
      p.mv[0][2][0] = c.mv[2][0];
      p.mv[0][2][1] = c.mv[2][1];
    }
  }
  choice[i] = c;
  for (int comp = 0; comp < 3; comp++) {
    p.comp = (uint8_t)comp;
    inter[3 * i + comp] = p;
  }
}

// cu_info_from_me_kernel (k_misc.h) with corners: the deblocking records as the decoder
// fills them for an affine CU (the fourth corner UR + DL - UL).  A CU whose record is all
// ones (no search result): the vectors as they stand there, as cu_info_from_me_kernel
// copies an unsupported result's.  grid: ceil(n / 256); block: 256.
__global__ void __launch_bounds__(256)
cu_info_from_affine_choice_kernel(const xvcgpu_me_block *blocks,
                                  const xvcgpu_fp_affine_result *choice, const int32_t *nnz,
                                  const int32_t *luma_tx_index, int n, int qp_y, int qp_c,
                                  int ref_poc, xvcgpu_cu_info *cus) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const xvcgpu_me_block b = blocks[i];
  const xvcgpu_fp_affine_result ch = choice[i];
  xvcgpu_cu_info c;
  c.x = (uint16_t)b.x;
  c.y = (uint16_t)b.y;
  c.w = b.w;
  c.h = b.h;
  c.intra = 0;
  c.cbf_luma = nnz[luma_tx_index ? luma_tx_index[i] : i] != 0;
  c.qp_y = (int8_t)qp_y;
  c.qp_c = (int8_t)qp_c;
  c.ref_idx0 = 0;
  c.reserved = 0;
  c.ref_poc[0] = ref_poc;
  c.ref_poc[1] = -1;
  const bool affine = ch.use_affine == 1;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const int s = affine ? (k < 3 ? k : 0) : 0;
    c.mv[0][k][0] = ch.mv[s][0];
    c.mv[0][k][1] = ch.mv[s][1];
    c.mv[1][k][0] = 0;
    c.mv[1][k][1] = 0;
  }
  if (affine) {
    c.mv[0][XVC_CORNER_DR][0] = ch.mv[1][0] + ch.mv[2][0] - ch.mv[0][0];
    c.mv[0][XVC_CORNER_DR][1] = ch.mv[1][1] + ch.mv[2][1] - ch.mv[0][1];
  }
  cus[i] = c;
}

#endif  // XVCGPU_K_FP_AFFINE_H_
