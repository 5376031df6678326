// xvc_frame_pass.h -- C++ host driver of the hot-path frame pass (the C++ twin
// of xvc_amd/pipeline.py::FramePass): what PictureEncoder::Encode
// (picture_encoder.cc:75-160) drives per picture once mode decision is taken
// out - for every CU the motion search (inter_search.cc:606-662) and
// CompressAndEvalCbf (:261-365), then DeblockPicture, PadBorder and the PSNR
// walk - all through the C-ABI, every picture and decision resident in HBM.
#ifndef XVC_AMD_HOST_XVC_FRAME_PASS_H_
#define XVC_AMD_HOST_XVC_FRAME_PASS_H_

#include <cmath>
#include <cstdint>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "xvc_gpu_ops.h"

namespace xvc_gpu {

// (ChromaQp and Lambda16: xvc_gpu_ops.h, beside the adaptive-QP table that needs them too)

// What a pass object holds for adaptive QP (FramePass::SetAdaptiveQp,
// FramePassBiRefs::SetAdaptiveQp): the table and the four arrays of xvcgpu_aqp_args, made
// once; every Run writes the arrays (xvcgpu_frame_pass_aqp, xvcgpu_frame_pass_bi_refs_aqp).
class AdaptiveQpArrays {
 public:
  AdaptiveQpArrays(const Context &ctx, int width, int height, int bitdepth, int pic_qp,
                   int aqp_strength, int n_cus, int ctu_size = 64)
      : var16_(ctx, static_cast<size_t>((width + 15) / 16) * ((height + 15) / 16)),
        ctu_var_(ctx, Ctus(width, height, ctu_size)),
        ctu_dqp_(ctx, Ctus(width, height, ctu_size)),
        cu_qp_(ctx, 2 * static_cast<size_t>(n_cus > 0 ? n_cus : 1)),
        n_cus_(n_cus) {
    args_ = xvcgpu_aqp_args();
    args_.table = AdaptiveQp::Table(pic_qp, bitdepth, aqp_strength, width, ctu_size);
    args_.d_var16 = var16_.data();
    args_.d_ctu_var = ctu_var_.data();
    args_.d_ctu_dqp = ctu_dqp_.data();
    args_.d_cu_qp = cu_qp_.data();
  }
  const xvcgpu_aqp_args *args() const { return &args_; }
  // the last Run's delta per CTU in raster order / {qp_y, qp_c} per CU (synchronise)
  std::vector<int8_t> CtuDeltaQp() const { return ctu_dqp_.ToHost(); }
  std::vector<int8_t> CuQp() const {
    std::vector<int8_t> v = cu_qp_.ToHost();
    v.resize(2 * static_cast<size_t>(n_cus_));
    return v;
  }

 private:
  static size_t Ctus(int width, int height, int ctu_size) {
    if (ctu_size != 16 && ctu_size != 32 && ctu_size != 64 && ctu_size != 128)
      throw Error(XVCGPU_INVALID_ARGUMENT, "AdaptiveQpArrays: ctu_size");
    return static_cast<size_t>((width + ctu_size - 1) / ctu_size) *
           ((height + ctu_size - 1) / ctu_size);
  }
  DeviceArray<uint64_t> var16_, ctu_var_;
  DeviceArray<int8_t> ctu_dqp_, cu_qp_;
  int n_cus_;
  xvcgpu_aqp_args args_;
};

// One CU of a partition: a luma rectangle.
struct CuRect {
  int x, y, w, h;
};

// pipeline.check_partition: origins on the 4-sample grid, sides of 4, 8, 16, 32 or 64 (or
// what the right / bottom picture edge leaves of such a side, a multiple of 4), every CU
// inside the picture, no two overlapping, the picture covered.  Throws Error
// (XVCGPU_INVALID_ARGUMENT) naming the first offending CU (for a hole: the first
// uncovered 4x4 cell).
inline void CheckPartition(int width, int height, const std::vector<CuRect> &parts) {
  const int cw = (width + 3) / 4, ch = (height + 3) / 4;
  std::vector<int32_t> seen(static_cast<size_t>(cw) * ch, -1);
  for (size_t i = 0; i < parts.size(); i++) {
    const CuRect &p = parts[i];
    std::ostringstream name;
    name << "partition: CU " << i << " (x=" << p.x << ", y=" << p.y << ", w=" << p.w
         << ", h=" << p.h << ")";
    if (p.w <= 0 || p.h <= 0 || p.x < 0 || p.y < 0 || p.x + p.w > width || p.y + p.h > height)
      throw Error(XVCGPU_INVALID_ARGUMENT, name.str() + " lies outside the picture");
    if (p.x % 4 || p.y % 4)
      throw Error(XVCGPU_INVALID_ARGUMENT, name.str() + ": origin not on the 4-sample grid");
    const int side[2] = {p.w, p.h}, at[2] = {p.x, p.y}, full[2] = {width, height};
    for (int k = 0; k < 2; k++) {
      const int s = side[k];
      const bool std_side = s == 4 || s == 8 || s == 16 || s == 32 || s == 64;
      const bool cut = at[k] + s == full[k] && s < 64 && s % 4 == 0;
      if (!std_side && !cut)
        throw Error(XVCGPU_INVALID_ARGUMENT,
                    name.str() + ": side is not 4, 8, 16, 32 or 64 (nor cut by the picture edge)");
    }
    for (int yy = p.y / 4; yy < (p.y + p.h + 3) / 4; yy++)
      for (int xx = p.x / 4; xx < (p.x + p.w + 3) / 4; xx++) {
        int32_t &c = seen[static_cast<size_t>(yy) * cw + xx];
        if (c >= 0) {
          name << " overlaps CU " << c;
          throw Error(XVCGPU_INVALID_ARGUMENT, name.str());
        }
        c = static_cast<int32_t>(i);
      }
  }
  for (size_t k = 0; k < seen.size(); k++)
    if (seen[k] < 0) {
      std::ostringstream m;
      m << "partition: no CU covers the samples at x=" << 4 * (k % cw) << ", y=" << 4 * (k / cw)
        << " (a gap)";
      throw Error(XVCGPU_INVALID_ARGUMENT, m.str());
    }
}

class FramePass {
 public:
  // The pass over a caller's CU partition (pipeline.FramePass(partition=...)): the luma
  // CU tree of a real picture in coding order, CUs of any mix of sizes.  QuantFast; the
  // search runs through a plan made here (xvcgpu_me_plan_create), the pass through
  // xvcgpu_frame_pass_planned.  A CU the search has no instance for (a side the picture
  // edge cut to 12, 24, ...) is refused.
  FramePass(const Context &ctx, int width, int height, int bitdepth, int qp,
            const std::vector<CuRect> &partition, int search_range = 96)
      : ctx_(ctx), w_(width), h_(height), bd_(bitdepth), qp_(qp), qp_c_(ChromaQp(qp)),
        plan_(nullptr) {
    CheckPartition(width, height, partition);
    map_stride_ = (width + 3) / 4;
    std::vector<int32_t> map(static_cast<size_t>(map_stride_) * ((height + 3) / 4), -1);
    std::vector<xvcgpu_me_block> me;
    std::vector<xvcgpu_tx_block> tx;
    std::vector<int32_t> luma;
    int side = 16, small = 16;
    for (size_t i = 0; i < partition.size(); i++) {
      const CuRect &p = partition[i];
      xvcgpu_me_block b = xvcgpu_me_block();
      b.x = static_cast<int16_t>(p.x);
      b.y = static_cast<int16_t>(p.y);
      b.w = static_cast<uint8_t>(p.w);
      b.h = static_cast<uint8_t>(p.h);
      b.depth_nonzero = 1;
      b.lambda16 = Lambda16(qp);
      b.search_range = search_range;
      for (int yy = p.y / 4; yy < (p.y + p.h) / 4; yy++)
        for (int xx = p.x / 4; xx < (p.x + p.w) / 4; xx++)
          map[static_cast<size_t>(yy) * map_stride_ + xx] = static_cast<int32_t>(i);
      me.push_back(b);
      luma.push_back(static_cast<int32_t>(3 * i));
      for (int c = 0; c < 3; c++) tx.push_back(TxBlockOf(p, c, c ? qp_c_ : qp));
      side = p.w > side ? p.w : side;
      side = p.h > side ? p.h : side;
      small = p.w < small ? p.w : small;
      small = p.h < small ? p.h : small;
    }
    // the kernels that take a CU whole hold CUs of 8 ... 16 samples a side: any other
    // partition takes the any-size middle
    form_ = side <= 16 && small >= 8 ? XVC_FP_FORM_RECON_FROM_ME : XVC_FP_FORM_RESIDUAL;
    me_shape_ = 0;
    max_cu_ = side <= 16 ? 16 : (side <= 32 ? 32 : 64);   // the search's block class
    Allocate(me, map);
    d_tx_.reset(new DeviceArray<xvcgpu_tx_block>(ctx, tx));
    d_luma_.reset(new DeviceArray<int32_t>(ctx, luma));
    pred_.reset(new Picture(ctx, width, height, bitdepth));
    ctx_.Check(xvcgpu_me_plan_create(ctx_.get(), d_me_->data(), n_cus_, max_cu_, &plan_));
    int32_t counts[XVCGPU_ME_PLAN_BINS] = {0};
    const xvcgpu_status st = xvcgpu_me_plan_counts(plan_, counts);
    if (st != XVCGPU_OK || counts[XVCGPU_ME_PLAN_UNSUPPORTED] > 0) {
      xvcgpu_me_plan_destroy(ctx_.get(), plan_);
      plan_ = nullptr;
      ctx_.Check(st);
      throw Error(XVCGPU_INVALID_ARGUMENT,
                  "partition: the motion search has no instance for some CUs (sides must be "
                  "4, 8, 16, 32 or 64)");
    }
  }

  FramePass(const Context &ctx, int width, int height, int bitdepth, int qp,
            int cu = 16, int search_range = 96)
      : ctx_(ctx), w_(width), h_(height), bd_(bitdepth), qp_(qp), qp_c_(ChromaQp(qp)),
        plan_(nullptr) {
    map_stride_ = (width + 3) / 4;
    std::vector<int32_t> map(static_cast<size_t>(map_stride_) * ((height + 3) / 4), -1);
    std::vector<xvcgpu_me_block> me;
    size_t sq16 = 0;   // jobs of the search's exact-shape kernel: 16x16 and 16x8
    for (int y = 0; y < height; y += cu)
      for (int x = 0; x < width; x += cu) {
        xvcgpu_me_block b = xvcgpu_me_block();
        b.x = static_cast<int16_t>(x);
        b.y = static_cast<int16_t>(y);
        b.w = static_cast<uint8_t>(width - x < cu ? width - x : cu);
        b.h = static_cast<uint8_t>(height - y < cu ? height - y : cu);
        b.depth_nonzero = 1;
        b.lambda16 = Lambda16(qp);
        b.search_range = search_range;
        for (int yy = y / 4; yy < (y + b.h) / 4; yy++)
          for (int xx = x / 4; xx < (x + b.w) / 4; xx++)
            map[static_cast<size_t>(yy) * map_stride_ + xx] = static_cast<int32_t>(me.size());
        sq16 += b.w == 16 && (b.h == 16 || b.h == 8);
        me.push_back(b);
      }
    // the search's shape word, as pipeline.FramePass sets it: the hint where at least 98 %
    // of the jobs have those shapes, and the word that no job has another where all do
    me_shape_ = me.empty() || 50 * sq16 < 49 * me.size() ? 0 : XVCGPU_ME_HINT_SQ16;
    if (!me.empty() && sq16 == me.size()) me_shape_ |= XVCGPU_ME_ONLY_SQ16;
    Allocate(me, map);
    max_cu_ = cu;
    form_ = XVC_FP_FORM_RECON_FROM_ME;
  }

  ~FramePass() {
    if (plan_) xvcgpu_me_plan_destroy(ctx_.get(), plan_);
  }
  FramePass(const FramePass &) = delete;
  FramePass &operator=(const FramePass &) = delete;

  // From now on every Run codes with adaptive QP (CuEncoder::EncodeCtu, cu_encoder.cc:92-97;
  // aqp_strength as encoder_settings.h:90, 13 by default there): qp is the picture's QP,
  // each 64x64 CTU gets qp + its delta, derived on the device from the original in front of
  // the search (xvcgpu_frame_pass_aqp).  The pass takes the form with a prediction picture
  // and transform blocks (RESIDUAL), which is the one that reads a QP per block; its
  // transform blocks are made here where the grid's fused form had none.
  void SetAdaptiveQp(int aqp_strength) {
    if (affine_) throw Error(XVCGPU_INVALID_ARGUMENT, "SetAdaptiveQp: not together with SetAffine");
    if (merge_) throw Error(XVCGPU_INVALID_ARGUMENT, "SetAdaptiveQp: not together with SetMerge");
    aqp_.reset(new AdaptiveQpArrays(ctx_, w_, h_, bd_, qp_, aqp_strength, n_cus_));
    if (!d_tx_) {
      std::vector<xvcgpu_tx_block> tx;
      std::vector<int32_t> luma;
      for (size_t i = 0; i < rects_.size(); i++) {
        luma.push_back(static_cast<int32_t>(3 * i));
        for (int c = 0; c < 3; c++) tx.push_back(TxBlockOf(rects_[i], c, c ? qp_c_ : qp_));
      }
      d_tx_.reset(new DeviceArray<xvcgpu_tx_block>(ctx_, tx));
      d_luma_.reset(new DeviceArray<int32_t>(ctx_, luma));
      pred_.reset(new Picture(ctx_, w_, h_, bd_));
    }
    form_ = XVC_FP_FORM_RESIDUAL;
  }
  // What a pass with affine motion takes beside the flat pass's jobs, on the host
  // (pipeline.FrameDescriptors.affine_jobs / affine_order: the same bytes): one job per CU
  // in CU order with the plain job's lambda16 and predictor (mvp_x, mvp_y at every corner),
  // the indices of the capable CUs - w and h each 16, 32 or 64 (CodingUnit::CanUseAffine,
  // coding_unit.h:251-257) - grouped by CU height 16, 32, 64 in CU order, and the args
  // block with the counts and side_bits (its pointers null).
  static xvcgpu_frame_pass_affine_args AffineJobs(const std::vector<CuRect> &rects,
                                                  uint32_t lambda16, int mvp_x, int mvp_y,
                                                  uint32_t side_bits,
                                                  std::vector<xvcgpu_affine_me_block> *jobs,
                                                  std::vector<int32_t> *order) {
    xvcgpu_frame_pass_affine_args f = xvcgpu_frame_pass_affine_args();
    f.side_bits = side_bits;
    jobs->clear();
    order->clear();
    for (size_t i = 0; i < rects.size(); i++) {
      xvcgpu_affine_me_block b = xvcgpu_affine_me_block();
      b.x = static_cast<int16_t>(rects[i].x);
      b.y = static_cast<int16_t>(rects[i].y);
      b.w = static_cast<uint8_t>(rects[i].w);
      b.h = static_cast<uint8_t>(rects[i].h);
      b.lambda16 = lambda16;
      for (int k = 0; k < 3; k++) {
        b.mvp[k][0] = mvp_x;
        b.mvp[k][1] = mvp_y;
      }
      jobs->push_back(b);
    }
    for (int cls = 0; cls < 3; cls++)
      for (size_t i = 0; i < rects.size(); i++) {
        const int w = rects[i].w, h = rects[i].h;
        if ((w == 16 || w == 32 || w == 64) && h == (16 << cls)) {
          order->push_back(static_cast<int32_t>(i));
          f.n_class[cls]++;
        }
      }
    return f;
  }

  // From now on every Run searches the CUs with both sides above 8 a second time with the
  // three-corner affine model, bootstrapped from the translational vector, and keeps the
  // cheaper state (InterSearch::CompressInter, inter_search.cc:74-99;
  // xvcgpu_frame_pass_affine).  The pass takes the form with a prediction picture and
  // transform blocks (RESIDUAL); they are made here where the grid's fused form had none.
  // Not together with SetAdaptiveQp.
  void SetAffine(uint32_t side_bits = 1) {
    if (aqp_) throw Error(XVCGPU_INVALID_ARGUMENT, "SetAffine: not together with SetAdaptiveQp");
    if (merge_) throw Error(XVCGPU_INVALID_ARGUMENT, "SetAffine: not together with SetMerge");
    std::vector<xvcgpu_affine_me_block> jobs;
    std::vector<int32_t> order;
    affine_args_ = AffineJobs(rects_, Lambda16(qp_), 0, 0, side_bits, &jobs, &order);
    if (order.empty()) order.push_back(0);   // (no empty device array; the counts say none)
    d_affine_.reset(new DeviceArray<xvcgpu_affine_me_block>(ctx_, jobs));
    d_order_.reset(new DeviceArray<int32_t>(ctx_, order));
    d_affine_res_.reset(new DeviceArray<xvcgpu_affine_me_result>(ctx_, jobs.size()));
    d_choice_.reset(new DeviceArray<xvcgpu_fp_affine_result>(ctx_, jobs.size()));
    d_inter_.reset(new DeviceArray<xvcgpu_inter_block>(ctx_, 3 * jobs.size()));
    affine_args_.d_affine = d_affine_->data();
    affine_args_.d_order = d_order_->data();
    affine_args_.d_affine_results = d_affine_res_->data();
    affine_args_.d_choice = d_choice_->data();
    affine_args_.d_inter = d_inter_->data();
    if (!d_tx_) {
      std::vector<xvcgpu_tx_block> tx;
      std::vector<int32_t> luma;
      for (size_t i = 0; i < rects_.size(); i++) {
        luma.push_back(static_cast<int32_t>(3 * i));
        for (int c = 0; c < 3; c++) tx.push_back(TxBlockOf(rects_[i], c, c ? qp_c_ : qp_));
      }
      d_tx_.reset(new DeviceArray<xvcgpu_tx_block>(ctx_, tx));
      d_luma_.reset(new DeviceArray<int32_t>(ctx_, luma));
      pred_.reset(new Picture(ctx_, w_, h_, bd_));
    }
    form_ = XVC_FP_FORM_RESIDUAL;
    affine_ = true;
  }
  // the last Run's record per CU (synchronises)
  std::vector<xvcgpu_fp_affine_result> AffineChoice() const { return d_choice_->ToHost(); }

  // What a pass with merge mode takes beside the flat pass's jobs, on the host
  // (pipeline.merge_cand_array / merge_args / lambda_sqrt_for_qp: the same bytes): the
  // candidates from list 0's vectors mv[n_cus][5][2] (1/16 pel, unclipped, merge-index
  // order; every candidate names picture 0 of list 0: ref_idx {0, -1}), the args block from
  // its numbers (pointers null), and sqrt(lambda) of a QP - the expression Lambda16 floors.
  static std::vector<xvcgpu_fp_merge_cand> MergeCands(const int32_t *mv, int n_cus) {
    std::vector<xvcgpu_fp_merge_cand> c(static_cast<size_t>(n_cus) * XVC_FP_MERGE_CANDS,
                                        xvcgpu_fp_merge_cand());
    for (size_t k = 0; k < c.size(); k++) {
      c[k].ref_idx[0] = 0;
      c[k].ref_idx[1] = -1;
      c[k].mv[0][0] = mv[2 * k];
      c[k].mv[0][1] = mv[2 * k + 1];
    }
    return c;
  }
  static xvcgpu_frame_pass_merge_args MergeArgs(int n_listed, uint32_t side_bits,
                                                uint32_t merge_side_bits, double lambda_sqrt) {
    xvcgpu_frame_pass_merge_args m = xvcgpu_frame_pass_merge_args();
    m.n_listed = n_listed;
    m.side_bits = side_bits;
    m.merge_side_bits = merge_side_bits;
    m.lambda_sqrt = lambda_sqrt;
    return m;
  }
  static double LambdaSqrtForQp(int qp) {
    return std::sqrt(0.57 * std::pow(2.0, (qp - 12) / 3.0));
  }

  // From now on every Run tries merge mode for every CU behind the search
  // (xvcgpu_frame_pass_merge): the five candidates mv[n_cus][5][2] are ranked as
  // InterSearch::SearchMergeCandidates ranks them and the best is taken where its
  // closed-form price is not above the searched state's; a merge CU without levels is a
  // skip CU.  Every form the pass has.  lambda_sqrt < 0: LambdaSqrtForQp(qp).  Not together
  // with SetAdaptiveQp or SetAffine.
  void SetMerge(const int32_t *mv, uint32_t side_bits = 1, uint32_t merge_side_bits = 1,
                double lambda_sqrt = -1.0) {
    if (aqp_ || affine_)
      throw Error(XVCGPU_INVALID_ARGUMENT, "SetMerge: not together with SetAdaptiveQp or SetAffine");
    const size_t n = static_cast<size_t>(n_cus_ > 0 ? n_cus_ : 1);
    std::vector<xvcgpu_fp_merge_cand> cands = MergeCands(mv, n_cus_);
    if (cands.empty()) cands.push_back(xvcgpu_fp_merge_cand());   // (no empty device array)
    merge_args_ = MergeArgs(n_cus_, side_bits, merge_side_bits,
                            lambda_sqrt < 0 ? LambdaSqrtForQp(qp_) : lambda_sqrt);
    d_cands_.reset(new DeviceArray<xvcgpu_fp_merge_cand>(ctx_, cands));
    d_rank_.reset(new DeviceArray<xvcgpu_fp_merge_ranking>(ctx_, n));
    d_merge_choice_.reset(new DeviceArray<xvcgpu_fp_merge_result>(ctx_, n));
    d_chosen_.reset(new DeviceArray<xvcgpu_me_result>(ctx_, n));
    merge_args_.d_cands = d_cands_->data();
    merge_args_.d_rank = d_rank_->data();
    merge_args_.d_choice = d_merge_choice_->data();
    merge_args_.d_chosen = d_chosen_->data();
    merge_ = true;
  }
  // the last Run's records per CU (synchronise)
  std::vector<xvcgpu_fp_merge_ranking> MergeRank() const { return d_rank_->ToHost(); }
  std::vector<xvcgpu_fp_merge_result> MergeChoice() const { return d_merge_choice_->ToHost(); }
  std::vector<xvcgpu_me_result> ChosenResults() const { return d_chosen_->ToHost(); }

  // the last Run's delta per CTU (raster order) and {qp_y, qp_c} per CU (synchronise)
  std::vector<int8_t> CtuDeltaQp() const { return aqp_->CtuDeltaQp(); }
  std::vector<int8_t> CuQp() const { return aqp_->CuQp(); }
  std::vector<xvcgpu_cu_info> CuInfo() const { return d_cus_->ToHost(); }

  // Enqueues one picture (asynchronous): rec becomes the padded reconstruction.
  // The whole sequence - search, CompressAndEvalCbf, deblocking, PadBorder,
  // PSNR parts - goes through one C call (xvcgpu_frame_pass).
  void Run(const Picture &orig, const Picture &ref, Picture *rec, int ref_poc = 0) {
    xvcgpu_frame_pass_args a = xvcgpu_frame_pass_args();
    a.orig = orig.get();
    a.ref = ref.get();
    a.rec = rec->get();
    a.d_me = d_me_->data();
    a.d_results = d_res_->data();
    a.n_cus = n_cus_;
    a.max_block_size = max_cu_;
    a.qp_y = qp_;
    a.qp_c = qp_c_;
    a.ref_poc = ref_poc;
    a.d_nnz = d_nnz_->data();
    a.d_cus_own = d_cus_->data();
    a.d_cus = d_cus_->data();
    a.n_cus_total = n_cus_;
    a.d_cu_map = d_map_->data();
    a.map_stride = map_stride_;
    a.db_y_begin = 0;
    a.db_y_end = a.dbh_y_end = h_;
    a.ssd_y_begin = 0;
    a.ssd_y_end = 1 << 30;
    a.shift_bitdepth = bd_;
    a.d_ssd = d_ssd_->data();
    a.me_shape = me_shape_;
    a.form = form_;
    const int phases = XVC_FP_ENCODE | XVC_FP_DEBLOCK_V | XVC_FP_DEBLOCK_H | XVC_FP_PAD |
                       XVC_FP_SSD;
    if (plan_ || aqp_ || affine_) {   // the residual form's arguments
      a.pred = pred_->get();
      a.d_tx = d_tx_->data();
      a.n_tx = 3 * n_cus_;
      a.d_luma_tx_index = d_luma_->data();
    }
    if (affine_) {
      ctx_.Check(xvcgpu_frame_pass_affine(ctx_.get(), &a, &affine_args_, plan_, phases));
      return;
    }
    if (merge_) {
      ctx_.Check(xvcgpu_frame_pass_merge(ctx_.get(), &a, &merge_args_, plan_, phases));
      return;
    }
    if (aqp_) {
      ctx_.Check(xvcgpu_frame_pass_aqp(ctx_.get(), &a, aqp_->args(), plan_, phases));
      return;
    }
    if (plan_) {   // a partition: the planned search
      ctx_.Check(xvcgpu_frame_pass_planned(ctx_.get(), &a, plan_, phases));
      return;
    }
    ctx_.Check(xvcgpu_frame_pass(ctx_.get(), &a, phases));
  }

  // SampleMetric::ComputePsnr parts of the last Run (synchronises).
  void Ssd(uint64_t *ssd, uint64_t *samples) const {
    std::vector<uint64_t> v = d_ssd_->ToHost();
    *ssd = v[0];
    *samples = v[1];
  }
  std::vector<xvcgpu_me_result> MotionVectors() const { return d_res_->ToHost(); }
  int num_cus() const { return n_cus_; }

 private:
  // Y, U or V block of a CU: block 3 * cu + comp
  static xvcgpu_tx_block TxBlockOf(const CuRect &p, int comp, int qp) {
    const int sh = comp ? 1 : 0;
    xvcgpu_tx_block t = xvcgpu_tx_block();
    t.x = static_cast<int16_t>(p.x >> sh);
    t.y = static_cast<int16_t>(p.y >> sh);
    t.w = static_cast<uint8_t>(p.w >> sh);
    t.h = static_cast<uint8_t>(p.h >> sh);
    t.comp = static_cast<uint8_t>(comp);
    t.qp = static_cast<int8_t>(qp);
    return t;
  }

  void Allocate(const std::vector<xvcgpu_me_block> &me, const std::vector<int32_t> &map) {
    n_cus_ = static_cast<int>(me.size());
    for (size_t i = 0; i < me.size(); i++) {
      const CuRect p = {me[i].x, me[i].y, me[i].w, me[i].h};
      rects_.push_back(p);
    }
    d_me_.reset(new DeviceArray<xvcgpu_me_block>(ctx_, me));
    d_map_.reset(new DeviceArray<int32_t>(ctx_, map));
    d_res_.reset(new DeviceArray<xvcgpu_me_result>(ctx_, me.size()));
    d_nnz_.reset(new DeviceArray<int32_t>(ctx_, 3 * me.size()));
    d_cus_.reset(new DeviceArray<xvcgpu_cu_info>(ctx_, me.size()));
    d_ssd_.reset(new DeviceArray<uint64_t>(ctx_, 2));
    ctx_.Check(xvcgpu_memset(ctx_.get(), d_cus_->data(), 0, me.size() * sizeof(xvcgpu_cu_info)));
  }

  const Context &ctx_;
  int w_, h_, bd_, qp_, qp_c_, n_cus_, map_stride_, max_cu_, me_shape_, form_;
  xvcgpu_me_plan *plan_;
  std::vector<CuRect> rects_;   // the CUs, in list order
  std::unique_ptr<AdaptiveQpArrays> aqp_;
  bool affine_ = false;
  xvcgpu_frame_pass_affine_args affine_args_;
  std::unique_ptr<DeviceArray<xvcgpu_affine_me_block>> d_affine_;
  std::unique_ptr<DeviceArray<int32_t>> d_order_;
  std::unique_ptr<DeviceArray<xvcgpu_affine_me_result>> d_affine_res_;
  std::unique_ptr<DeviceArray<xvcgpu_fp_affine_result>> d_choice_;
  std::unique_ptr<DeviceArray<xvcgpu_inter_block>> d_inter_;
  bool merge_ = false;
  xvcgpu_frame_pass_merge_args merge_args_;
  std::unique_ptr<DeviceArray<xvcgpu_fp_merge_cand>> d_cands_;
  std::unique_ptr<DeviceArray<xvcgpu_fp_merge_ranking>> d_rank_;
  std::unique_ptr<DeviceArray<xvcgpu_fp_merge_result>> d_merge_choice_;
  std::unique_ptr<DeviceArray<xvcgpu_me_result>> d_chosen_;
  std::unique_ptr<DeviceArray<xvcgpu_tx_block>> d_tx_;
  std::unique_ptr<DeviceArray<int32_t>> d_luma_;
  std::unique_ptr<Picture> pred_;
  std::unique_ptr<DeviceArray<xvcgpu_me_block>> d_me_;
  std::unique_ptr<DeviceArray<int32_t>> d_map_;
  std::unique_ptr<DeviceArray<xvcgpu_me_result>> d_res_;
  std::unique_ptr<DeviceArray<int32_t>> d_nnz_;
  std::unique_ptr<DeviceArray<xvcgpu_cu_info>> d_cus_;
  std::unique_ptr<DeviceArray<uint64_t>> d_ssd_;
};

// The frame pass of a B picture whose lists name 1 to XVC_CS_MAX_REFS reference pictures each
// (the C++ twin of pipeline.BiRefsFramePass): for every CU InterSearch::SearchMotion over two
// lists (inter_search.cc:198-259; the SearchBiIterative step :392-433) as the reference
// configures itself
// - one search per picture that list 0 has not searched already (inter_search.cc:536-542), the
// SearchBiIterative step into every picture of the list that lost, the choice against the
// best of the pictures only list 1 names (:247-257) - then CompressAndEvalCbf, the B picture's
// DeblockPicture, PadBorder and the PSNR walk: one C call (xvcgpu_frame_pass_bi_refs).
// Nothing is read back in between.  QuantFast (form RESIDUAL), closed-form side bits
// (fast_inter_pred_bits: 3 / 3 / 5).  The CUs are the cu x cu grid or, with a partition, a
// caller's CUs of any mix of sizes (searched through one plan per searched picture).  The work
// arrays between the launches are owned here.
class FramePassBiRefs {
 public:
  // The picture's POC and its lists' POCs; what the pass needs beyond them is derived:
  // same_poc_in_l0 (ReferencePictureLists::GetSamePocMappingFor), the table of distinct
  // pictures and force_l1_mvd_zero (PictureData::DetermineForceBipredL1MvdZero).
  // low_delay = false: lists that lie wholly before cur_poc are refused, as before.
  // low_delay = true: the pass of a picture with only back references
  // (xvcgpu_frame_pass_bi_back: list 1's candidate is the job's predictor, priced on the
  // device; list 0 is refined against it; no vector difference for list 1 of a
  // bi-directional CU); lists with a later picture are refused.
  struct RefLists {
    int cur_poc;
    std::vector<int> poc[2];
    bool low_delay;
    RefLists() : cur_poc(0), low_delay(false) {}
    RefLists(int cur, const std::vector<int> &l0, const std::vector<int> &l1, bool ld = false)
        : cur_poc(cur), low_delay(ld) {
      poc[0] = l0;
      poc[1] = l1;
    }
  };

  FramePassBiRefs(const Context &ctx, int width, int height, int bitdepth, int qp,
                  const RefLists &lists, int cu = 16, int search_range = 96)
      : ctx_(ctx), h_(height), bd_(bitdepth), qp_(qp), qp_c_(ChromaQp(qp)), plan_() {
    std::vector<CuRect> parts;
    for (int y = 0; y < height; y += cu)
      for (int x = 0; x < width; x += cu) {
        const CuRect p = {x, y, width - x < cu ? width - x : cu, height - y < cu ? height - y : cu};
        parts.push_back(p);
      }
    Build(width, height, lists, parts, search_range, cu, false);
  }
  FramePassBiRefs(const Context &ctx, int width, int height, int bitdepth, int qp,
                  const RefLists &lists, const std::vector<CuRect> &partition,
                  int search_range = 96)
      : ctx_(ctx), h_(height), bd_(bitdepth), qp_(qp), qp_c_(ChromaQp(qp)), plan_() {
    CheckPartition(width, height, partition);
    int side = 16;
    for (size_t i = 0; i < partition.size(); i++) {
      side = partition[i].w > side ? partition[i].w : side;
      side = partition[i].h > side ? partition[i].h : side;
    }
    Build(width, height, lists, partition, search_range, side <= 16 ? 16 : (side <= 32 ? 32 : 64),
          true);
  }
  ~FramePassBiRefs() { DestroyPlans(); }
  FramePassBiRefs(const FramePassBiRefs &) = delete;
  FramePassBiRefs &operator=(const FramePassBiRefs &) = delete;

  // New search jobs of (list, picture): predictors, flags, lambda, range; the CUs stay.
  void SetJobs(int list, int ref_idx, const std::vector<xvcgpu_me_block> &me) {
    if (list < 0 || list > 1 || ref_idx < 0 || ref_idx >= num_ref_[list] ||
        me.size() != static_cast<size_t>(n_cus_))
      throw Error(XVCGPU_INVALID_ARGUMENT, "FramePassBiRefs::SetJobs: no such (list, picture)");
    ctx_.Check(xvcgpu_memcpy_h2d(ctx_.get(), d_me_[list][ref_idx]->data(), me.data(),
                                 me.size() * sizeof(xvcgpu_me_block)));
  }

  // Enqueues one picture (asynchronous): rec becomes the padded reconstruction.  pics[l][r]:
  // the lists' pictures in the lists' order, the same object where they name the same POC.
  void Run(const Picture &orig, const std::vector<const Picture *> pics[2], Picture *rec) {
    xvcgpu_frame_pass_bi_refs_args b = xvcgpu_frame_pass_bi_refs_args();
    xvcgpu_frame_pass_args &a = b.p;
    a.orig = orig.get();
    a.rec = rec->get();
    a.n_cus = a.n_cus_total = n_cus_;
    a.max_block_size = max_cu_;
    a.qp_y = qp_;
    a.qp_c = qp_c_;
    a.d_nnz = d_nnz_->data();
    a.d_cus_own = d_cus_->data();
    a.d_cus = d_cus_->data();
    a.d_cu_map = d_map_->data();
    a.map_stride = map_stride_;
    a.db_y_begin = 0;
    a.db_y_end = a.dbh_y_end = h_;
    a.ssd_y_begin = 0;
    a.ssd_y_end = 1 << 30;
    a.shift_bitdepth = bd_;
    a.d_ssd = d_ssd_->data();
    a.pred = pred_->get();
    a.d_tx = d_tx_->data();
    a.n_tx = 3 * n_cus_;
    a.d_luma_tx_index = d_luma_->data();
    a.form = XVC_FP_FORM_RESIDUAL;
    b.n_refs = static_cast<int32_t>(distinct_.size());
    b.force_l1_mvd_zero = low_delay_ ? 1 : 0;
    const xvcgpu_me_plan *plans[2][XVC_CS_MAX_REFS] = {};
    for (int l = 0; l < 2; l++) {
      if (pics[l].size() != static_cast<size_t>(num_ref_[l]))
        throw Error(XVCGPU_INVALID_ARGUMENT, "FramePassBiRefs::Run: one picture per list entry");
      b.num_ref[l] = num_ref_[l];
      for (int r = 0; r < num_ref_[l]; r++) {
        const int k = slot_[l][r];
        if (b.refs[k] && b.refs[k] != pics[l][r]->get())
          throw Error(XVCGPU_INVALID_ARGUMENT,
                      "FramePassBiRefs::Run: the lists name one POC with two pictures");
        b.refs[k] = pics[l][r]->get();
        b.slot[l][r] = static_cast<uint8_t>(k);
        b.ref_poc[l][r] = poc_[l][r];
        b.d_me[l][r] = d_me_[l][r]->data();
        b.d_results[l][r] = d_res_[l][r] ? d_res_[l][r]->data() : nullptr;
        plans[l][r] = plan_[l][r];
      }
    }
    for (int r = 0; r < XVC_CS_MAX_REFS; r++)
      b.same_poc_in_l0[r] = static_cast<int8_t>(r < num_ref_[1] ? same_[r] : -1);
    b.side_bits_uni[0] = b.side_bits_uni[1] = 3;
    b.side_bits_bi = 5;
    b.d_bi_jobs = d_bi_jobs_->data();
    b.d_bi_results = d_bi_res_->data();
    b.d_bi_slots = d_bi_slots_->data();
    b.d_choice = d_choice_->data();
    b.d_inter = d_inter_->data();
    const int phases = XVC_FP_ENCODE | XVC_FP_DEBLOCK_V | XVC_FP_DEBLOCK_H | XVC_FP_PAD |
                       XVC_FP_SSD;
    if (low_delay_) {
      ctx_.Check(xvcgpu_frame_pass_bi_back(ctx_.get(), &b, d_l1_mvp_cost_->data(),
                                           aqp_ ? aqp_->args() : nullptr, plans, phases));
      return;
    }
    if (aqp_) {
      ctx_.Check(xvcgpu_frame_pass_bi_refs_aqp(ctx_.get(), &b, aqp_->args(), plans, phases));
      return;
    }
    if (affine_entry_) {   // (named by SetAffine alone: a program without it links without it)
      ctx_.Check(affine_entry_(ctx_.get(), &b, &affine_args_, plans, phases));
      return;
    }
    if (merge_entry_) {    // (named by SetMerge alone)
      ctx_.Check(merge_entry_(ctx_.get(), &b, &merge_args_, plans, phases));
      return;
    }
    ctx_.Check(xvcgpu_frame_pass_bi_refs(ctx_.get(), &b, plans, phases));
  }

  // What a B pass with merge mode takes beside the plain pass's jobs, on the host
  // (pipeline.bi_merge_cand_array / bi_merge_args: the same bytes): the candidates from
  // ref_idx[n_cus][5][2] (per list the picture's index in that list, -1: unused) and
  // mv[n_cus][5][2][2] (1/16 pel, unclipped; merge-index order), and the args block from its
  // numbers (pointers null).
  static std::vector<xvcgpu_fp_merge_cand> MergeCands(const int32_t *ref_idx, const int32_t *mv,
                                                      int n_cus) {
    std::vector<xvcgpu_fp_merge_cand> c(static_cast<size_t>(n_cus) * XVC_FP_MERGE_CANDS,
                                        xvcgpu_fp_merge_cand());
    for (size_t k = 0; k < c.size(); k++)
      for (int l = 0; l < 2; l++) {
        c[k].ref_idx[l] = static_cast<int8_t>(ref_idx[2 * k + l]);
        c[k].mv[l][0] = mv[4 * k + 2 * l];
        c[k].mv[l][1] = mv[4 * k + 2 * l + 1];
      }
    return c;
  }
  static xvcgpu_frame_pass_bi_merge_args MergeArgs(int n_listed, uint32_t merge_side_bits,
                                                   double lambda_sqrt) {
    xvcgpu_frame_pass_bi_merge_args m = xvcgpu_frame_pass_bi_merge_args();
    m.n_listed = n_listed;
    m.merge_side_bits = merge_side_bits;
    m.lambda_sqrt = lambda_sqrt;
    return m;
  }

  // From now on every Run tries merge mode for every CU behind the plain choice
  // (xvcgpu_frame_pass_bi_refs_merge): the five candidates per CU - of list 0, of list 1 or
  // bi-directional - are ranked as InterSearch::SearchMergeCandidates ranks them and the best
  // is taken where its closed-form price is not above the plain choice's; a merge CU without
  // levels is a skip CU.  lambda_sqrt < 0: FramePass::LambdaSqrtForQp(qp).  Not together
  // with low_delay, SetAffine or SetAdaptiveQp.
  void SetMerge(const int32_t *ref_idx, const int32_t *mv, uint32_t merge_side_bits = 1,
                double lambda_sqrt = -1.0) {
    if (low_delay_ || affine_entry_ || aqp_)
      throw Error(XVCGPU_INVALID_ARGUMENT,
                  "SetMerge: not together with low_delay, SetAffine or SetAdaptiveQp");
    const size_t n = static_cast<size_t>(n_cus_ > 0 ? n_cus_ : 1);
    std::vector<xvcgpu_fp_merge_cand> cands = MergeCands(ref_idx, mv, n_cus_);
    if (cands.empty()) cands.push_back(xvcgpu_fp_merge_cand());   // (no empty device array)
    merge_args_ = MergeArgs(n_cus_, merge_side_bits,
                            lambda_sqrt < 0 ? FramePass::LambdaSqrtForQp(qp_) : lambda_sqrt);
    d_cands_.reset(new DeviceArray<xvcgpu_fp_merge_cand>(ctx_, cands));
    d_rank_.reset(new DeviceArray<xvcgpu_fp_merge_ranking>(ctx_, n));
    d_merge_choice_.reset(new DeviceArray<xvcgpu_fp_bi_merge_result>(ctx_, n));
    d_chosen_.reset(new DeviceArray<xvcgpu_fp_bi_refs_result>(ctx_, n));
    merge_args_.d_cands = d_cands_->data();
    merge_args_.d_rank = d_rank_->data();
    merge_args_.d_choice = d_merge_choice_->data();
    merge_args_.d_chosen = d_chosen_->data();
    merge_entry_ = &xvcgpu_frame_pass_bi_refs_merge;
  }
  // the last Run's records per CU (synchronise)
  std::vector<xvcgpu_fp_merge_ranking> MergeRank() const { return d_rank_->ToHost(); }
  std::vector<xvcgpu_fp_bi_merge_result> MergeChoice() const { return d_merge_choice_->ToHost(); }
  std::vector<xvcgpu_fp_bi_refs_result> ChosenResults() const { return d_chosen_->ToHost(); }

  // What a B pass with affine motion takes beside the plain pass's jobs, on the host
  // (pipeline.bi_affine_jobs: the same bytes): E = 2 * Rmax jobs per CU, job [i * E + l * Rmax
  // + r] with the CU's rectangle, lambda16 and the predictor (mvp_x, mvp_y) at every corner for
  // r < num_ref[l], zero beyond; two slot bytes per job {slot[l][r], 255}, the first
  // XVC_FP_BI_NO_JOB beyond the list and for a re-used list-1 picture; the indices of the
  // capable CUs grouped by CU height 16, 32, 64 (FramePass::AffineJobs' list); the args block
  // with the counts (its pointers null).
  static xvcgpu_frame_pass_bi_affine_args AffineJobs(
      const std::vector<CuRect> &rects, uint32_t lambda16, int mvp_x, int mvp_y,
      const int num_ref[2], const int *same_poc_in_l0, const int slot[2][XVC_CS_MAX_REFS],
      std::vector<xvcgpu_affine_me_block> *jobs, std::vector<uint8_t> *slots,
      std::vector<int32_t> *order) {
    xvcgpu_frame_pass_bi_affine_args f = xvcgpu_frame_pass_bi_affine_args();
    const int rmax = num_ref[0] > num_ref[1] ? num_ref[0] : num_ref[1];
    jobs->assign(rects.size() * 2 * rmax, xvcgpu_affine_me_block());
    slots->assign(rects.size() * 4 * rmax, XVC_FP_BI_NO_JOB);
    std::vector<xvcgpu_affine_me_block> one;
    const xvcgpu_frame_pass_affine_args p =
        FramePass::AffineJobs(rects, lambda16, mvp_x, mvp_y, 0, &one, order);
    for (int k = 0; k < 3; k++) f.n_class[k] = p.n_class[k];
    for (size_t i = 0; i < rects.size(); i++)
      for (int l = 0; l < 2; l++)
        for (int r = 0; r < num_ref[l]; r++) {
          const size_t at = i * 2 * rmax + l * rmax + r;
          (*jobs)[at] = one[i];
          if (l == 0 || same_poc_in_l0[r] < 0) (*slots)[2 * at] = static_cast<uint8_t>(slot[l][r]);
        }
    return f;
  }

  // From now on every Run searches the CUs with both sides above 8 a second time with the
  // three-corner affine model into every picture of both lists, refines the list that lost as
  // SearchBiIterative does and keeps the cheaper state, the plain one on a tie
  // (InterSearch::CompressInter, inter_search.cc:74-99; xvcgpu_frame_pass_bi_refs_affine).
  // lambda16: the jobs' (0: the pass's QP's, as the plain jobs carry it until SetJobs); the
  // corner predictors are zero, as the plain jobs' are.  Not together with low_delay or
  // SetAdaptiveQp.
  void SetAffine(uint32_t lambda16 = 0) {
    if (low_delay_)
      throw Error(XVCGPU_INVALID_ARGUMENT,
                  "SetAffine: not together with low_delay (force_l1_mvd_zero)");
    if (aqp_) throw Error(XVCGPU_INVALID_ARGUMENT, "SetAffine: not together with SetAdaptiveQp");
    if (merge_entry_) throw Error(XVCGPU_INVALID_ARGUMENT, "SetAffine: not together with SetMerge");
    std::vector<xvcgpu_affine_me_block> jobs;
    std::vector<uint8_t> slots;
    std::vector<int32_t> order;
    affine_args_ = AffineJobs(rects_, lambda16 ? lambda16 : Lambda16(qp_), 0, 0, num_ref_, same_,
                              slot_, &jobs, &slots, &order);
    if (order.empty()) order.push_back(0);   // (no empty device array; the counts say none)
    const size_t n = rects_.size();
    d_affine_uni_.reset(new DeviceArray<xvcgpu_affine_me_block>(ctx_, jobs));
    d_affine_uni_slots_.reset(new DeviceArray<uint8_t>(ctx_, slots));
    d_affine_order_.reset(new DeviceArray<int32_t>(ctx_, order));
    d_affine_uni_res_.reset(new DeviceArray<xvcgpu_affine_me_result>(ctx_, jobs.size()));
    d_affine_bi_.reset(new DeviceArray<xvcgpu_affine_me_block>(ctx_, n * rmax_));
    d_affine_bi_res_.reset(new DeviceArray<xvcgpu_affine_me_result>(ctx_, n * rmax_));
    d_affine_bi_slots_.reset(new DeviceArray<uint8_t>(ctx_, 2 * n * rmax_));
    d_affine_choice_.reset(new DeviceArray<xvcgpu_fp_bi_affine_result>(ctx_, n));
    affine_args_.d_uni = d_affine_uni_->data();
    affine_args_.d_uni_results = d_affine_uni_res_->data();
    affine_args_.d_uni_slots = d_affine_uni_slots_->data();
    affine_args_.d_bi = d_affine_bi_->data();
    affine_args_.d_bi_results = d_affine_bi_res_->data();
    affine_args_.d_bi_slots = d_affine_bi_slots_->data();
    affine_args_.d_order = d_affine_order_->data();
    affine_args_.d_choice = d_affine_choice_->data();
    affine_entry_ = &xvcgpu_frame_pass_bi_refs_affine;
  }
  // with SetAffine: what both runs ended with per CU
  std::vector<xvcgpu_fp_bi_affine_result> AffineChoices() const {
    return d_affine_choice_->ToHost();
  }

  // From now on every Run codes with adaptive QP (FramePass::SetAdaptiveQp; the form is
  // RESIDUAL already): xvcgpu_frame_pass_bi_refs_aqp, or xvcgpu_frame_pass_bi_back with q.
  void SetAdaptiveQp(int aqp_strength) {
    if (affine_entry_)
      throw Error(XVCGPU_INVALID_ARGUMENT, "SetAdaptiveQp: not together with SetAffine");
    if (merge_entry_)
      throw Error(XVCGPU_INVALID_ARGUMENT, "SetAdaptiveQp: not together with SetMerge");
    aqp_.reset(new AdaptiveQpArrays(ctx_, w_, h_, bd_, qp_, aqp_strength, n_cus_));
  }
  std::vector<int8_t> CtuDeltaQp() const { return aqp_->CtuDeltaQp(); }
  std::vector<int8_t> CuQp() const { return aqp_->CuQp(); }

  // SampleMetric::ComputePsnr parts of the last Run (synchronises).
  void Ssd(uint64_t *ssd, uint64_t *samples) const {
    std::vector<uint64_t> v = d_ssd_->ToHost();
    *ssd = v[0];
    *samples = v[1];
  }
  // what SearchMotion ended with per CU, and the CU records the filter read
  std::vector<xvcgpu_fp_bi_refs_result> Choices() const { return d_choice_->ToHost(); }
  std::vector<xvcgpu_cu_info> CuInfo() const { return d_cus_->ToHost(); }
  // low_delay: the predictor cost per (CU, list-1 picture), [n_cus][XVC_CS_MAX_REFS]
  std::vector<uint32_t> L1MvpCost() const { return d_l1_mvp_cost_->ToHost(); }
  bool low_delay() const { return low_delay_; }
  // bytes of the work arrays between the launches, in the order of the args block and
  // d_l1_mvp_cost last (0 without low_delay)
  std::vector<size_t> WorkArrayBytes() const {
    const size_t n = static_cast<size_t>(n_cus_), jobs = n * rmax_;
    const size_t v[] = {jobs * sizeof(xvcgpu_bi_block), jobs * sizeof(xvcgpu_me_result), 2 * jobs,
                        n * sizeof(xvcgpu_fp_bi_refs_result), 3 * n * sizeof(xvcgpu_inter_block),
                        low_delay_ ? n * XVC_CS_MAX_REFS * sizeof(uint32_t) : 0};
    return std::vector<size_t>(v, v + 6);
  }
  int num_cus() const { return n_cus_; }
  int same_poc_in_l0(int ref_idx) const { return same_[ref_idx]; }

 private:
  void DestroyPlans() {
    for (int l = 0; l < 2; l++)
      for (int r = 0; r < XVC_CS_MAX_REFS; r++)
        if (plan_[l][r]) {
          xvcgpu_me_plan_destroy(ctx_.get(), plan_[l][r]);
          plan_[l][r] = nullptr;
        }
  }

  void Build(int width, int height, const RefLists &lists, const std::vector<CuRect> &parts,
             int search_range, int max_cu, bool planned) {
    bool only_back = true;
    for (int l = 0; l < 2; l++) {
      num_ref_[l] = static_cast<int>(lists.poc[l].size());
      if (num_ref_[l] < 1 || num_ref_[l] > XVC_CS_MAX_REFS)
        throw Error(XVCGPU_INVALID_ARGUMENT, "FramePassBiRefs: 1 .. XVC_CS_MAX_REFS pictures per list");
      for (int r = 0; r < num_ref_[l]; r++) {
        const int poc = lists.poc[l][r];
        poc_[l][r] = poc;
        only_back = only_back && poc < lists.cur_poc;
        size_t k = 0;
        while (k < distinct_.size() && distinct_[k] != poc) k++;
        if (k == distinct_.size()) distinct_.push_back(poc);
        slot_[l][r] = static_cast<int>(k);
      }
    }
    low_delay_ = lists.low_delay;
    if (low_delay_ && !only_back)
      throw Error(XVCGPU_INVALID_ARGUMENT,
                  "FramePassBiRefs: low_delay takes only lists that lie wholly before the "
                  "picture (force_l1_mvd_zero)");
    if (only_back && !low_delay_)
      throw Error(XVCGPU_INVALID_ARGUMENT,
                  "FramePassBiRefs: a picture with only back references (force_l1_mvd_zero) is "
                  "out of this pass's scope");
    for (int r = 0; r < XVC_CS_MAX_REFS; r++) {
      same_[r] = -1;
      for (int q = num_ref_[0] - 1; r < num_ref_[1] && q >= 0; q--)
        if (poc_[0][q] == poc_[1][r]) same_[r] = q;   // (the first list-0 index)
    }
    rmax_ = num_ref_[0] > num_ref_[1] ? num_ref_[0] : num_ref_[1];
    w_ = width;
    map_stride_ = (width + 3) / 4;
    max_cu_ = max_cu;
    n_cus_ = static_cast<int>(parts.size());
    rects_ = parts;
    std::vector<int32_t> map(static_cast<size_t>(map_stride_) * ((height + 3) / 4), -1);
    std::vector<xvcgpu_me_block> me;
    std::vector<xvcgpu_tx_block> tx;
    std::vector<int32_t> luma;
    for (size_t i = 0; i < parts.size(); i++) {
      const CuRect &p = parts[i];
      xvcgpu_me_block b = xvcgpu_me_block();
      b.x = static_cast<int16_t>(p.x);
      b.y = static_cast<int16_t>(p.y);
      b.w = static_cast<uint8_t>(p.w);
      b.h = static_cast<uint8_t>(p.h);
      b.depth_nonzero = 1;
      b.lambda16 = Lambda16(qp_);
      b.search_range = search_range;
      me.push_back(b);
      for (int yy = p.y / 4; yy < (p.y + p.h) / 4; yy++)
        for (int xx = p.x / 4; xx < (p.x + p.w) / 4; xx++)
          map[static_cast<size_t>(yy) * map_stride_ + xx] = static_cast<int32_t>(i);
      luma.push_back(static_cast<int32_t>(3 * i));
      for (int c = 0; c < 3; c++) {   // Y U V per CU: block 3 * cu + comp
        const int sh = c ? 1 : 0;
        xvcgpu_tx_block t = xvcgpu_tx_block();
        t.x = static_cast<int16_t>(p.x >> sh);
        t.y = static_cast<int16_t>(p.y >> sh);
        t.w = static_cast<uint8_t>(p.w >> sh);
        t.h = static_cast<uint8_t>(p.h >> sh);
        t.comp = static_cast<uint8_t>(c);
        t.qp = static_cast<int8_t>(c ? qp_c_ : qp_);
        tx.push_back(t);
      }
    }
    const size_t n = me.size();
    for (int l = 0; l < 2; l++)
      for (int r = 0; r < num_ref_[l]; r++) {
        d_me_[l][r].reset(new DeviceArray<xvcgpu_me_block>(ctx_, me));
        if (l == 0 || same_[r] < 0) d_res_[l][r].reset(new DeviceArray<xvcgpu_me_result>(ctx_, n));
      }
    d_bi_jobs_.reset(new DeviceArray<xvcgpu_bi_block>(ctx_, n * rmax_));
    d_bi_res_.reset(new DeviceArray<xvcgpu_me_result>(ctx_, n * rmax_));
    d_bi_slots_.reset(new DeviceArray<uint8_t>(ctx_, 2 * n * rmax_));
    d_choice_.reset(new DeviceArray<xvcgpu_fp_bi_refs_result>(ctx_, n));
    d_inter_.reset(new DeviceArray<xvcgpu_inter_block>(ctx_, 3 * n));
    if (low_delay_) d_l1_mvp_cost_.reset(new DeviceArray<uint32_t>(ctx_, n * XVC_CS_MAX_REFS));
    d_map_.reset(new DeviceArray<int32_t>(ctx_, map));
    d_tx_.reset(new DeviceArray<xvcgpu_tx_block>(ctx_, tx));
    d_luma_.reset(new DeviceArray<int32_t>(ctx_, luma));
    d_nnz_.reset(new DeviceArray<int32_t>(ctx_, 3 * n));
    d_cus_.reset(new DeviceArray<xvcgpu_cu_info>(ctx_, n));
    d_ssd_.reset(new DeviceArray<uint64_t>(ctx_, 2));
    ctx_.Check(xvcgpu_memset(ctx_.get(), d_cus_->data(), 0, n * sizeof(xvcgpu_cu_info)));
    pred_.reset(new Picture(ctx_, width, height, bd_));
    if (!planned) return;
    for (int l = 0; l < 2; l++)
      for (int r = 0; r < num_ref_[l]; r++) {
        if (!d_res_[l][r]) continue;   // a re-used picture is not searched
        int32_t counts[XVCGPU_ME_PLAN_BINS] = {0};
        xvcgpu_status st = xvcgpu_me_plan_create(ctx_.get(), d_me_[l][r]->data(), n_cus_, max_cu_,
                                                 &plan_[l][r]);
        if (st == XVCGPU_OK) st = xvcgpu_me_plan_counts(plan_[l][r], counts);
        if (st != XVCGPU_OK || counts[XVCGPU_ME_PLAN_UNSUPPORTED] > 0) {
          DestroyPlans();   // (no destructor behind a constructor that throws)
          ctx_.Check(st);
          throw Error(XVCGPU_INVALID_ARGUMENT,
                      "partition: the motion search has no instance for some CUs (sides must be "
                      "4, 8, 16, 32 or 64)");
        }
      }
  }

  const Context &ctx_;
  int h_, bd_, qp_, qp_c_, n_cus_, map_stride_, max_cu_, rmax_, w_;
  bool low_delay_;
  std::unique_ptr<AdaptiveQpArrays> aqp_;
  std::unique_ptr<DeviceArray<uint32_t>> d_l1_mvp_cost_;
  int num_ref_[2], poc_[2][XVC_CS_MAX_REFS], slot_[2][XVC_CS_MAX_REFS], same_[XVC_CS_MAX_REFS];
  std::vector<int> distinct_;
  xvcgpu_me_plan *plan_[2][XVC_CS_MAX_REFS];
  std::unique_ptr<DeviceArray<xvcgpu_me_block>> d_me_[2][XVC_CS_MAX_REFS];
  std::unique_ptr<DeviceArray<xvcgpu_me_result>> d_res_[2][XVC_CS_MAX_REFS], d_bi_res_;
  std::unique_ptr<DeviceArray<xvcgpu_bi_block>> d_bi_jobs_;
  std::unique_ptr<DeviceArray<uint8_t>> d_bi_slots_;
  std::unique_ptr<DeviceArray<xvcgpu_fp_bi_refs_result>> d_choice_;
  std::unique_ptr<DeviceArray<xvcgpu_inter_block>> d_inter_;
  std::unique_ptr<DeviceArray<int32_t>> d_map_, d_luma_, d_nnz_;
  std::unique_ptr<DeviceArray<xvcgpu_tx_block>> d_tx_;
  std::unique_ptr<DeviceArray<xvcgpu_cu_info>> d_cus_;
  std::unique_ptr<DeviceArray<uint64_t>> d_ssd_;
  std::unique_ptr<Picture> pred_;
  // SetAffine
  std::vector<CuRect> rects_;
  xvcgpu_frame_pass_bi_affine_args affine_args_;
  xvcgpu_status (*affine_entry_)(xvcgpu_ctx *, const xvcgpu_frame_pass_bi_refs_args *,
                                 const xvcgpu_frame_pass_bi_affine_args *,
                                 const xvcgpu_me_plan *const[2][XVC_CS_MAX_REFS], int) = nullptr;
  std::unique_ptr<DeviceArray<xvcgpu_affine_me_block>> d_affine_uni_, d_affine_bi_;
  std::unique_ptr<DeviceArray<xvcgpu_affine_me_result>> d_affine_uni_res_, d_affine_bi_res_;
  std::unique_ptr<DeviceArray<uint8_t>> d_affine_uni_slots_, d_affine_bi_slots_;
  std::unique_ptr<DeviceArray<int32_t>> d_affine_order_;
  std::unique_ptr<DeviceArray<xvcgpu_fp_bi_affine_result>> d_affine_choice_;
  // SetMerge
  xvcgpu_frame_pass_bi_merge_args merge_args_;
  xvcgpu_status (*merge_entry_)(xvcgpu_ctx *, const xvcgpu_frame_pass_bi_refs_args *,
                                const xvcgpu_frame_pass_bi_merge_args *,
                                const xvcgpu_me_plan *const[2][XVC_CS_MAX_REFS], int) = nullptr;
  std::unique_ptr<DeviceArray<xvcgpu_fp_merge_cand>> d_cands_;
  std::unique_ptr<DeviceArray<xvcgpu_fp_merge_ranking>> d_rank_;
  std::unique_ptr<DeviceArray<xvcgpu_fp_bi_merge_result>> d_merge_choice_;
  std::unique_ptr<DeviceArray<xvcgpu_fp_bi_refs_result>> d_chosen_;
};

}  // namespace xvc_gpu
#endif  // XVC_AMD_HOST_XVC_FRAME_PASS_H_
