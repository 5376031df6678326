// xvc_frame_pass_merge.cc -- C entry point (for ctypes / tests) of xvc_gpu::FramePass with
// SetMerge (xvc_frame_pass.h): the P pass with merge mode over the cu x cu grid or a
// partition, on borrowed handles.
#include <cstdint>
#include <cstring>
#include <vector>

#include "xvc_frame_pass.h"

extern "C" {

// partition: n_parts rows (x, y, w, h), or NULL for the cu x cu grid.  n = the pass's CUs;
// merge_mv: n * 5 * 2 int32, list 0's candidate vectors.  out_res[n], out_rank[n],
// out_choice[n], out_chosen[n], out_cus[n], out_ssd[2] after the pass has run (synchronises).
int xvc_host_frame_pass_merge(xvcgpu_ctx *ctx, int width, int height, int bitdepth, int qp,
                              int cu, int search_range, const int32_t *partition, int n_parts,
                              xvcgpu_picture *orig, xvcgpu_picture *ref, xvcgpu_picture *rec,
                              int ref_poc, int n, const int32_t *merge_mv,
                              xvcgpu_me_result *out_res, xvcgpu_fp_merge_ranking *out_rank,
                              xvcgpu_fp_merge_result *out_choice, xvcgpu_me_result *out_chosen,
                              xvcgpu_cu_info *out_cus, uint64_t *out_ssd) {
  if (!ctx || !orig || !ref || !rec || !merge_mv || !out_res || !out_rank || !out_choice ||
      !out_chosen || !out_cus || !out_ssd)
    return XVCGPU_INVALID_ARGUMENT;
  try {
    xvc_gpu::Context c(ctx);
    std::unique_ptr<xvc_gpu::FramePass> pass;
    if (partition) {
      std::vector<xvc_gpu::CuRect> parts;
      for (int i = 0; i < n_parts; i++) {
        const xvc_gpu::CuRect p = {partition[4 * i], partition[4 * i + 1], partition[4 * i + 2],
                                   partition[4 * i + 3]};
        parts.push_back(p);
      }
      pass.reset(new xvc_gpu::FramePass(c, width, height, bitdepth, qp, parts, search_range));
    } else {
      pass.reset(new xvc_gpu::FramePass(c, width, height, bitdepth, qp, cu, search_range));
    }
    if (pass->num_cus() != n) return XVCGPU_INVALID_ARGUMENT;
    pass->SetMerge(merge_mv);
    xvc_gpu::Picture o(c, orig), f(c, ref), r(c, rec);
    pass->Run(o, f, &r, ref_poc);
    pass->Ssd(&out_ssd[0], &out_ssd[1]);
    const std::vector<xvcgpu_me_result> res = pass->MotionVectors();
    const std::vector<xvcgpu_fp_merge_ranking> rank = pass->MergeRank();
    const std::vector<xvcgpu_fp_merge_result> choice = pass->MergeChoice();
    const std::vector<xvcgpu_me_result> chosen = pass->ChosenResults();
    const std::vector<xvcgpu_cu_info> cus = pass->CuInfo();
    std::memcpy(out_res, res.data(), n * sizeof(res[0]));
    std::memcpy(out_rank, rank.data(), n * sizeof(rank[0]));
    std::memcpy(out_choice, choice.data(), n * sizeof(choice[0]));
    std::memcpy(out_chosen, chosen.data(), n * sizeof(chosen[0]));
    std::memcpy(out_cus, cus.data(), n * sizeof(cus[0]));
    return XVCGPU_OK;
  } catch (const xvc_gpu::Error &e) {
    return e.status;
  }
}

}  // extern "C"
