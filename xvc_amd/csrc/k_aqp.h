// k_aqp.h -- adaptive QP on the device: the QP CuEncoder::EncodeCtu (cu_encoder.cc:92-97)
// gives every CTU, pic_qp + CalcDeltaQpFromVariance (cu_encoder.cc:308-363), derived from
// the CTU statistic of ctu_variance_kernel (k_stats.h) and written into the job arrays of a
// frame pass (xvcgpu_frame_pass_aqp, xvcgpu_frame_pass_bi_refs_aqp), and the correction of
// the CU records the record kernels wrote with the picture's scalar QP.
// Host twin: xvc_gpu::AdaptiveQp::CalcDeltaQpFromVariance (host/xvc_gpu_ops.h), which reads
// the statistic back and calls std::log.
//
// The reference's int(kStrength * (1.5 * log(v) - 15 - 2 * (bd - 8))) clipped to -3 .. 7
// does not decrease in v; the host says it as ten thresholds (xvcgpu_aqp_table.var_min), the
// device counts the ones the statistic reaches.  No logarithm, no double on the device.
//
// Both kernels: one thread per CU, 256-thread workgroups, plain loads and stores, no LDS,
// no atomics.  The table is a kernel argument: every access to it has a compile-time index
// (the entry of the CU's delta is picked by compare-and-select steps over uniform scalar
// loads, component by component so that few of them are live at once), so nothing of it is
// copied to scratch.  Threads of one CTU store the same delta byte to d_ctu_dqp.
// hipcc -Rpass-analysis=kernel-resource-usage, gfx950:
//   aqp_apply_kernel       52 VGPRs, 86 SGPRs, no scratch, no LDS, 8 waves / SIMD
//   cu_info_set_qp_kernel   7 VGPRs, 10 SGPRs, no scratch, no LDS, 8 waves / SIMD
// (with the three components' constants selected in one loop the compiler reserved 196 B /
// lane of private segment it never used; selected per component it reserves none).
#ifndef XVCGPU_K_AQP_H_
#define XVCGPU_K_AQP_H_

#include "xvcgpu_internal.h"

// The job arrays of a pass: one per (list, picture), the same CUs in the same order
struct AqpMeArrays {
  xvcgpu_me_block *p[2 * XVC_CS_MAX_REFS];
};

// n_ctus: the CTUs of d_ctu_var (an index past them is clamped: a job outside the picture
// must not make the kernel read or write outside the arrays)
__global__ void __launch_bounds__(256)
aqp_apply_kernel(xvcgpu_aqp_table t, const unsigned long long *ctu_var, int n_ctus,
                 AqpMeArrays me, int n_me, xvcgpu_tx_block *tx, xvcgpu_rdoq_params *prm,
                 const int32_t *luma_tx_index, int n_cus, int8_t *cu_qp, int8_t *ctu_dqp) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n_cus) return;
  const xvcgpu_me_block *b = &me.p[0][i];
  const int x = b->x < 0 ? 0 : b->x, y = b->y < 0 ? 0 : b->y;
  int cx = x / t.ctu_size;
  if (cx > t.ctus_per_row - 1) cx = t.ctus_per_row - 1;
  int ctu = (y / t.ctu_size) * t.ctus_per_row + cx;
  if (ctu > n_ctus - 1) ctu = n_ctus - 1;
  const unsigned long long v = ctu_var[ctu];
  int d = 0;   // delta - XVC_AQP_DELTA_MIN
#pragma unroll
  for (int k = 0; k < XVC_AQP_DELTAS - 1; k++) d += v >= t.var_min[k] ? 1 : 0;
  int qp_y = t.qp_y[0], qp_c = t.qp_c[0];
  uint32_t lambda16 = t.lambda16[0];
#pragma unroll
  for (int k = 1; k < XVC_AQP_DELTAS; k++) {
    const bool hit = d == k;
    qp_y = hit ? t.qp_y[k] : qp_y;
    qp_c = hit ? t.qp_c[k] : qp_c;
    lambda16 = hit ? t.lambda16[k] : lambda16;
  }
#pragma unroll
  for (int k = 0; k < 2 * XVC_CS_MAX_REFS; k++)
    if (k < n_me) me.p[k][i].lambda16 = lambda16;
  const int t0 = luma_tx_index[i];
#pragma unroll
  for (int c = 0; c < 3; c++) {
    tx[t0 + c].qp = (int8_t)(c == 0 ? qp_y : qp_c);
    if (prm) {
      long long lam = t.rdoq_lambda[0][c], rdf = t.rdoq_rd_factor[0][c];
#pragma unroll
      for (int k = 1; k < XVC_AQP_DELTAS; k++) {
        lam = d == k ? t.rdoq_lambda[k][c] : lam;
        rdf = d == k ? t.rdoq_rd_factor[k][c] : rdf;
      }
      prm[t0 + c].lambda = lam;
      prm[t0 + c].rd_factor = rdf;
    }
  }
  cu_qp[2 * i] = (int8_t)qp_y;
  cu_qp[2 * i + 1] = (int8_t)qp_c;
  if (ctu_dqp) ctu_dqp[ctu] = (int8_t)(d + XVC_AQP_DELTA_MIN);
}

__global__ void __launch_bounds__(256)
cu_info_set_qp_kernel(xvcgpu_cu_info *cus, const int8_t *cu_qp, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  cus[i].qp_y = cu_qp[2 * i];
  cus[i].qp_c = cu_qp[2 * i + 1];
}

#endif  // XVCGPU_K_AQP_H_
