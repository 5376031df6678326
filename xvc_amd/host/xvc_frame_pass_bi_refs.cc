// xvc_frame_pass_bi_refs.cc -- C entry point (for ctypes / tests) of
// xvc_gpu::FramePassBiRefs (xvc_frame_pass.h): the B pass with several reference pictures
// per list over the 16-sample CU grid, on borrowed handles.
#include <cstdint>
#include <cstring>
#include <memory>
#include <vector>

#include "xvc_frame_pass.h"

namespace {

// SetMerge's inputs and where its records go
struct MergeIo {
  const int32_t *ref_idx, *mv;   // [n][5][2], [n][5][2][2]
  double lambda_sqrt;            // < 0: the QP's
  xvcgpu_fp_merge_ranking *out_rank;
  xvcgpu_fp_bi_merge_result *out_choice;
  xvcgpu_fp_bi_refs_result *out_chosen;
};

// low_delay: RefLists::low_delay; aqp_strength < 0: one QP; out_l1_mvp_cost[n * 3]: NULL or
// the predictor costs of a low_delay pass
int RunBiRefs(xvcgpu_ctx *ctx, int width, int height, int bitdepth, int qp, int cur_poc,
              bool low_delay, int aqp_strength, const int32_t *num_ref, const int32_t *pocs,
              xvcgpu_picture *orig, xvcgpu_picture *const *ref_pics, xvcgpu_picture *rec,
              const xvcgpu_me_block *blocks, int n, xvcgpu_fp_bi_refs_result *out_choice,
              xvcgpu_cu_info *out_cus, uint64_t *out_ssd, uint32_t *out_l1_mvp_cost,
              xvcgpu_fp_bi_affine_result *out_affine = nullptr, const MergeIo *merge = nullptr) {
  if (!ctx || !num_ref || !pocs || !orig || !ref_pics || !rec || !out_choice || !out_cus ||
      !out_ssd)
    return XVCGPU_INVALID_ARGUMENT;
  try {
    xvc_gpu::Context c(ctx);
    xvc_gpu::FramePassBiRefs::RefLists lists;
    lists.cur_poc = cur_poc;
    lists.low_delay = low_delay;
    for (int l = 0; l < 2; l++) {
      if (num_ref[l] < 1 || num_ref[l] > XVC_CS_MAX_REFS) return XVCGPU_INVALID_ARGUMENT;
      lists.poc[l].assign(pocs + XVC_CS_MAX_REFS * l, pocs + XVC_CS_MAX_REFS * l + num_ref[l]);
    }
    xvc_gpu::FramePassBiRefs pass(c, width, height, bitdepth, qp, lists);
    if (pass.num_cus() != n) return XVCGPU_INVALID_ARGUMENT;
    if (aqp_strength >= 0) pass.SetAdaptiveQp(aqp_strength);
    // (affine jobs carry the plain jobs' lambda)
    if (out_affine) pass.SetAffine(blocks && n ? blocks[0].lambda16 : 0);
    if (merge) pass.SetMerge(merge->ref_idx, merge->mv, 1, merge->lambda_sqrt);
    xvc_gpu::Picture o(c, orig), r(c, rec);
    // one view per handle: the lists name a re-used picture by the same object
    std::vector<std::unique_ptr<xvc_gpu::Picture>> views;
    std::vector<const xvc_gpu::Picture *> pics[2];
    for (int l = 0; l < 2; l++)
      for (int q = 0; q < num_ref[l]; q++) {
        xvcgpu_picture *h = ref_pics[XVC_CS_MAX_REFS * l + q];
        if (!h) return XVCGPU_INVALID_ARGUMENT;
        const xvc_gpu::Picture *view = nullptr;
        for (size_t k = 0; k < views.size(); k++)
          if (views[k]->get() == h) view = views[k].get();
        if (!view) {
          views.emplace_back(new xvc_gpu::Picture(c, h));
          view = views.back().get();
        }
        pics[l].push_back(view);
        if (blocks) {
          const xvcgpu_me_block *b = blocks + static_cast<size_t>(XVC_CS_MAX_REFS * l + q) * n;
          pass.SetJobs(l, q, std::vector<xvcgpu_me_block>(b, b + n));
        }
      }
    pass.Run(o, pics, &r);
    pass.Ssd(&out_ssd[0], &out_ssd[1]);
    const std::vector<xvcgpu_fp_bi_refs_result> choice = pass.Choices();
    const std::vector<xvcgpu_cu_info> cus = pass.CuInfo();
    std::memcpy(out_choice, choice.data(), choice.size() * sizeof(choice[0]));
    std::memcpy(out_cus, cus.data(), cus.size() * sizeof(cus[0]));
    if (out_affine) {
      const std::vector<xvcgpu_fp_bi_affine_result> both = pass.AffineChoices();
      std::memcpy(out_affine, both.data(), both.size() * sizeof(both[0]));
    }
    if (merge) {
      const std::vector<xvcgpu_fp_merge_ranking> rank = pass.MergeRank();
      const std::vector<xvcgpu_fp_bi_merge_result> won = pass.MergeChoice();
      const std::vector<xvcgpu_fp_bi_refs_result> chosen = pass.ChosenResults();
      std::memcpy(merge->out_rank, rank.data(), n * sizeof(rank[0]));
      std::memcpy(merge->out_choice, won.data(), n * sizeof(won[0]));
      std::memcpy(merge->out_chosen, chosen.data(), n * sizeof(chosen[0]));
    }
    if (out_l1_mvp_cost && low_delay) {
      const std::vector<uint32_t> cost = pass.L1MvpCost();
      std::memcpy(out_l1_mvp_cost, cost.data(), cost.size() * sizeof(cost[0]));
    }
    return XVCGPU_OK;
  } catch (const xvc_gpu::Error &e) {
    return e.status;
  }
}

}  // namespace

extern "C" {

// pocs[l * 3 + r], ref_pics[l * 3 + r] (NULL beyond num_ref[l]); blocks[(l * 3 + r) * n + i]:
// the search jobs per (list, picture), n = the grid's CUs (NULL: the class's own jobs).
// out_choice[n], out_cus[n], out_ssd[2] after the pass has run (synchronises).
int xvc_host_frame_pass_bi_refs(xvcgpu_ctx *ctx, int width, int height, int bitdepth, int qp,
                                int cur_poc, const int32_t *num_ref, const int32_t *pocs,
                                xvcgpu_picture *orig, xvcgpu_picture *const *ref_pics,
                                xvcgpu_picture *rec, const xvcgpu_me_block *blocks, int n,
                                xvcgpu_fp_bi_refs_result *out_choice, xvcgpu_cu_info *out_cus,
                                uint64_t *out_ssd) {
  return RunBiRefs(ctx, width, height, bitdepth, qp, cur_poc, false, -1, num_ref, pocs, orig,
                   ref_pics, rec, blocks, n, out_choice, out_cus, out_ssd, nullptr);
}

// The same with SetAffine (the jobs' lambda16 is blocks[0]'s); out_affine[n].
int xvc_host_frame_pass_bi_refs_affine(xvcgpu_ctx *ctx, int width, int height, int bitdepth,
                                       int qp, int cur_poc, const int32_t *num_ref,
                                       const int32_t *pocs, xvcgpu_picture *orig,
                                       xvcgpu_picture *const *ref_pics, xvcgpu_picture *rec,
                                       const xvcgpu_me_block *blocks, int n,
                                       xvcgpu_fp_bi_refs_result *out_choice,
                                       xvcgpu_cu_info *out_cus, uint64_t *out_ssd,
                                       xvcgpu_fp_bi_affine_result *out_affine) {
  if (!out_affine) return XVCGPU_INVALID_ARGUMENT;
  return RunBiRefs(ctx, width, height, bitdepth, qp, cur_poc, false, -1, num_ref, pocs, orig,
                   ref_pics, rec, blocks, n, out_choice, out_cus, out_ssd, nullptr, out_affine);
}

// The same with SetMerge: candidates ref_idx[n][5][2] and mv[n][5][2][2], merge_side_bits 1,
// lambda_sqrt (< 0: the QP's); out_rank[n], out_merge[n], out_chosen[n].
int xvc_host_frame_pass_bi_refs_merge(xvcgpu_ctx *ctx, int width, int height, int bitdepth,
                                      int qp, int cur_poc, const int32_t *num_ref,
                                      const int32_t *pocs, xvcgpu_picture *orig,
                                      xvcgpu_picture *const *ref_pics, xvcgpu_picture *rec,
                                      const xvcgpu_me_block *blocks, int n,
                                      const int32_t *ref_idx, const int32_t *mv,
                                      double lambda_sqrt, xvcgpu_fp_bi_refs_result *out_choice,
                                      xvcgpu_cu_info *out_cus, uint64_t *out_ssd,
                                      xvcgpu_fp_merge_ranking *out_rank,
                                      xvcgpu_fp_bi_merge_result *out_merge,
                                      xvcgpu_fp_bi_refs_result *out_chosen) {
  if (!ref_idx || !mv || !out_rank || !out_merge || !out_chosen) return XVCGPU_INVALID_ARGUMENT;
  const MergeIo io = {ref_idx, mv, lambda_sqrt, out_rank, out_merge, out_chosen};
  return RunBiRefs(ctx, width, height, bitdepth, qp, cur_poc, false, -1, num_ref, pocs, orig,
                   ref_pics, rec, blocks, n, out_choice, out_cus, out_ssd, nullptr, nullptr, &io);
}

// The same with RefLists::low_delay = true (lists that lie wholly before cur_poc), with
// adaptive QP where aqp_strength >= 0; out_l1_mvp_cost[n * XVC_CS_MAX_REFS] (may be NULL).
int xvc_host_frame_pass_bi_back(xvcgpu_ctx *ctx, int width, int height, int bitdepth, int qp,
                                int cur_poc, int aqp_strength, const int32_t *num_ref,
                                const int32_t *pocs, xvcgpu_picture *orig,
                                xvcgpu_picture *const *ref_pics, xvcgpu_picture *rec,
                                const xvcgpu_me_block *blocks, int n,
                                xvcgpu_fp_bi_refs_result *out_choice, xvcgpu_cu_info *out_cus,
                                uint64_t *out_ssd, uint32_t *out_l1_mvp_cost) {
  return RunBiRefs(ctx, width, height, bitdepth, qp, cur_poc, true, aqp_strength, num_ref, pocs,
                   orig, ref_pics, rec, blocks, n, out_choice, out_cus, out_ssd, out_l1_mvp_cost);
}

}  // extern "C"
