// xvc_frame_pass_aqp.cc -- C entry point (for ctypes / tests) of xvc_gpu::FramePass with
// SetAdaptiveQp (xvc_frame_pass.h): the P pass over the 16-sample CU grid with a QP per CTU,
// on borrowed handles.
#include <cstdint>
#include <cstring>
#include <vector>

#include "xvc_frame_pass.h"

extern "C" {

// n = the grid's CUs, n_ctus = the picture's 64x64 CTUs.  out_res[n], out_cus[n], out_ssd[2],
// out_ctu_dqp[n_ctus], out_cu_qp[2 n] after the pass has run (synchronises).
int xvc_host_frame_pass_aqp(xvcgpu_ctx *ctx, int width, int height, int bitdepth, int qp,
                            int aqp_strength, int search_range, xvcgpu_picture *orig,
                            xvcgpu_picture *ref, xvcgpu_picture *rec, int ref_poc, int n,
                            int n_ctus, xvcgpu_me_result *out_res, xvcgpu_cu_info *out_cus,
                            uint64_t *out_ssd, int8_t *out_ctu_dqp, int8_t *out_cu_qp) {
  if (!ctx || !orig || !ref || !rec || !out_res || !out_cus || !out_ssd || !out_ctu_dqp ||
      !out_cu_qp)
    return XVCGPU_INVALID_ARGUMENT;
  try {
    xvc_gpu::Context c(ctx);
    xvc_gpu::FramePass pass(c, width, height, bitdepth, qp, 16, search_range);
    pass.SetAdaptiveQp(aqp_strength);
    const std::vector<int8_t> none = pass.CtuDeltaQp();
    if (pass.num_cus() != n || none.size() != static_cast<size_t>(n_ctus))
      return XVCGPU_INVALID_ARGUMENT;
    xvc_gpu::Picture o(c, orig), f(c, ref), r(c, rec);
    pass.Run(o, f, &r, ref_poc);
    pass.Ssd(&out_ssd[0], &out_ssd[1]);
    const std::vector<xvcgpu_me_result> res = pass.MotionVectors();
    const std::vector<xvcgpu_cu_info> cus = pass.CuInfo();
    const std::vector<int8_t> dqp = pass.CtuDeltaQp(), cu_qp = pass.CuQp();
    std::memcpy(out_res, res.data(), res.size() * sizeof(res[0]));
    std::memcpy(out_cus, cus.data(), cus.size() * sizeof(cus[0]));
    std::memcpy(out_ctu_dqp, dqp.data(), dqp.size());
    std::memcpy(out_cu_qp, cu_qp.data(), cu_qp.size());
    return XVCGPU_OK;
  } catch (const xvc_gpu::Error &e) {
    return e.status;
  }
}

}  // extern "C"
