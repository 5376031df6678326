// xvc_picture_decoder.h -- the reconstruction half of xvc::PictureDecoder
// (xvc_dec_lib/picture_decoder.cc:169-210) and xvc::CuDecoder::DecompressCu
// (xvc_dec_lib/cu_decoder.cc:84-138) on the device, behind the C-ABI
// (include/xvcgpu.h).  C++11 host code; the only thing it calls is xvcgpu_*.
//
// The reference decodes a picture CTU by CTU: parse a CTU (CABAC), then
// reconstruct its CUs one after the other.  Parsing is bit-serial and stays
// where it is; its result - the leaf CUs in coding order with their modes,
// final vectors, transform types and levels (include/xvc_syntax.h) - is the
// input here, and everything after it is decision-free:
//
//   reference (per CU, serial)                       here (per picture)
//   -----------------------------------------------  ------------------------------------
//   PictureData::MarkUsedInPic + neighbour lookups    one pass over the CU list builds the
//     (picture_data.cc:191-210, coding_unit.cc)       4x4 cell map and every CU's
//                                                     neighbour state at its coding time
//   InterPrediction::MotionCompensation               wave 0: one xvcgpu_inter_pred_batch
//     (inter_prediction.cc:710-738)                   over all inter CUs without LIC
//   IntraPrediction::FillReferenceState + Predict,    dependency waves over the real CU
//     LIC model (needs neighbouring reconstruction)   tree: wave(cu) = 1 + max(wave of the
//                                                     CUs whose samples it reads)
//   Quantize::Inverse, InverseTransform, AddClip      xvcgpu_inv_transform_batch per wave
//   DeblockingFilter::DeblockPicture (two CU trees    xvcgpu_deblock_tree (luma by the
//     in intra pictures, deblocking_filter.cc:56-77)  primary tree, chroma by the secondary)
//   YuvPicture::PadBorder                             xvcgpu_pad_border
//
// One host -> device copy per picture carries all job lists, the cell maps and
// the levels (a single packed staging buffer); the launches of a picture are
// 2 + 3 * waves, enqueued without any synchronisation.
#ifndef XVC_AMD_HOST_XVC_PICTURE_DECODER_H_
#define XVC_AMD_HOST_XVC_PICTURE_DECODER_H_

#include <cstdint>
#include <memory>
#include <vector>

#include "xvc_syntax.h"
#include "xvcgpu.h"

namespace xvc_gpu {

// What a CU reads from its neighbourhood, evaluated at its place in coding
// order (exposed for the host-side tests: compared with what the reference's
// IntraPrediction::DetermineNeighbors reported).
struct CuNeighbors {
  uint8_t flags[3];        // XVC_INTRA_HAS_* per component
  uint8_t above_right[3];  // CodingUnit::GetCuSizeAboveRight(comp)
  uint8_t below_left[3];   // CodingUnit::GetCuSizeBelowLeft(comp)
};

// The schedule of one picture (pure host data, no device work): exposed so the
// planning step can be tested without a GPU.
struct PicturePlan {
  int map_stride = 0, map_rows = 0;
  std::vector<int32_t> cell[2];       // per CU tree: coding index of the CU per 4x4 cell
  std::vector<int32_t> wave;          // per CU
  std::vector<CuNeighbors> neighbors; // per CU (intra CUs)
  int n_waves = 0;
  // jobs grouped by wave: wave w owns [first[w], first[w + 1]) of each list
  std::vector<xvcgpu_inter_block> inter;
  std::vector<int32_t> inter_first;
  std::vector<xvcgpu_intra_block> intra;
  std::vector<int32_t> intra_first;
  std::vector<xvcgpu_tx_block> tx;
  std::vector<uint32_t> tx_level_off;
  std::vector<int32_t> tx_nnz;
  std::vector<int32_t> tx_first;
  std::vector<xvcgpu_cu_info> cu_info;
  bool two_trees = false;
  int n_ref_slots = 0;
  int ref_slot[2][5];                 // [list][ref_idx] -> slot in the reference table
};

class PictureDecoder {
 public:
  PictureDecoder(xvcgpu_ctx *ctx, int width, int height, int bitdepth);
  ~PictureDecoder();
  PictureDecoder(const PictureDecoder &) = delete;
  PictureDecoder &operator=(const PictureDecoder &) = delete;

  // Host-only: does every field of the parsed syntax stay inside the picture,
  // the reference lists and the level array?  Decode refuses a picture that
  // does not (XVCGPU_INVALID_ARGUMENT); Plan may only be given one that does.
  static bool Validate(const xvc_picture_syntax &ps, const xvc_cu_syntax *cus,
                       const int16_t *levels);
  // Host-only: the schedule and job lists for a picture.
  static void Plan(const xvc_picture_syntax &ps, const xvc_cu_syntax *cus, const int16_t *levels,
                   PicturePlan *plan);

  // PictureDecoder::Decode after the parse (picture_decoder.cc:178-196): all CUs
  // of the picture into `rec`, in-loop filter, border extension.  ref_pics[l][i]
  // = the picture ReferencePictureLists::GetRefPic(l, i) names.  Asynchronous on
  // the context's stream; returns the status of the first failing call.
  xvcgpu_status Decode(const xvc_picture_syntax &ps, const xvc_cu_syntax *cus,
                       const int16_t *levels, const xvcgpu_picture *const ref_pics[2][5],
                       xvcgpu_picture *rec);

  // The same with the planning done: Decode = Validate + Plan + Issue.
  xvcgpu_status Issue(const PicturePlan &plan, const xvc_picture_syntax &ps, const int16_t *levels,
                      const xvcgpu_picture *const ref_pics[2][5], xvcgpu_picture *rec);
  // Issue in its parts: the layout of the picture's one upload, the copy of its parts
  // into page-locked memory (any thread), and the upload + launches.
  struct PackedPicture {
    size_t off[10], bytes[10], total;
    bool one_launch, tail_launch;
    int t0;
    std::vector<int32_t> tail_first;
  };
  void Layout(const PicturePlan &plan, const xvc_picture_syntax &ps, PackedPicture *L) const;
  static void PackInto(const PicturePlan &plan, const xvc_picture_syntax &ps,
                       const int16_t *levels, const PackedPicture &L, void *dst);
  xvcgpu_status IssuePacked(const PicturePlan &plan, const xvc_picture_syntax &ps,
                            const PackedPicture &L, const void *host_mem, xvcgpu_event *copied,
                            const xvcgpu_picture *const ref_pics[2][5], xvcgpu_picture *rec);
  // n pictures in decoding order; ref_index[(i * 2 + list) * 5 + k] = the position in
  // this sequence of picture i's reference (list, k), -1 = unused.  Planning of
  // picture i + 1 runs on a worker thread while picture i is uploaded and launched.
  xvcgpu_status DecodeSequence(int n, const xvc_picture_syntax *const *ps,
                               const xvc_cu_syntax *const *cus, const int16_t *const *levels,
                               const int32_t *ref_index, xvcgpu_picture *const *recs);
  // PictureDecoder::Postprocess: with d_out, picture i is also converted to the output
  // format of SetOutputFormat into d_out[i] (xvcgpu_output_bytes of it) on the lane
  // that decoded it, right after its in-loop filter and padding.
  xvcgpu_status DecodeSequence(int n, const xvc_picture_syntax *const *ps,
                               const xvc_cu_syntax *const *cus, const int16_t *const *levels,
                               const int32_t *ref_index, xvcgpu_picture *const *recs,
                               void *const *d_out);
  // The output fields of xvc_decoder_parameters (xvcgpu_output_format, unset fields
  // resolved per picture by xvcgpu_picture_convert_to) and the display size.
  void SetOutputFormat(const xvcgpu_output_format &fmt, int display_w, int display_h);

  // Picture-level parallelism (the reference decoder's picture threads,
  // xvc_dec_lib/thread_decoder.cc): a further lane = another context (its own stream)
  // with its own prediction scratch and staging buffers.  DecodeSequence deals the
  // pictures over the lanes in decoding order; a picture's kernels wait for the
  // pictures it references (events), so pictures that do not depend on each other -
  // the B pictures of one temporal layer - run side by side.  The context must be on
  // this decoder's device and stays the caller's.  With lanes the recs[] entries of a
  // DecodeSequence call must be distinct buffers (nothing orders a picture behind the
  // READERS of what its buffer held before): a repeated entry is XVCGPU_INVALID_ARGUMENT.
  xvcgpu_status AddLane(xvcgpu_ctx *ctx);
  int num_lanes() const { return 1 + static_cast<int>(lanes_.size()); }

  int last_num_waves() const { return last_waves_; }
  int last_num_launches() const { return last_launches_; }
  // Intra pictures: all dependency waves in one cooperative launch
  // (xvcgpu_intra_recon_waves; on by default) or a launch set per wave.
  void set_one_launch_intra(bool on) { use_waves_kernel_ = on; }

 private:
  xvcgpu_status EnsureStaging(int k, size_t bytes);
  // The picture's job lists, maps and levels go up in ONE queued copy from a
  // page-locked buffer; two buffers take turns so that Decode() of the next
  // picture can fill one while the copy of the previous is still in flight.
  struct HostSlot {
    void *mem;
    size_t cap;
    xvcgpu_event *copied;   // recorded behind the slot's upload
    bool in_flight;
  };
  xvcgpu_status AcquireHostSlot(size_t bytes, HostSlot **out);
  xvcgpu_ctx *ctx_;
  int width_, height_, bitdepth_;
  xvcgpu_picture *pred_;   // the prediction of the wave in flight (CuDecoder::temp_pred_)
  // device staging: two buffers take turns, the upload of picture i + 1 runs on the
  // context's copy stream while the kernels of picture i read the other one
  void *d_staging_[2];
  size_t staging_cap_[2];
  xvcgpu_event *kernels_done_[2];   // behind the last kernel that read d_staging_[k]
  bool staging_used_[2];
  int next_staging_;

  PicturePlan plan_;
  std::vector<PicturePlan> seq_plans_;   // DecodeSequence's ring (buffers kept between calls)
  // ... and the ring's page-locked memory: the planning threads pack the picture's
  // upload themselves (0.6 - 1.1 MB of maps and records per 1080p picture: 60 - 110 us
  // of copying that the issuing thread no longer does)
  struct SeqSlot {
    PackedPicture lay;
    void *mem;
    size_t cap;
    xvcgpu_event *copied;
    bool in_flight;
  };
  std::vector<SeqSlot> seq_slots_;
  int last_waves_, last_launches_;
  bool use_waves_kernel_;
  int tail_min_waves_;     // inter pictures: trailing all-intra waves in one launch from this many
  HostSlot host_[2];
  int next_host_;
  std::vector<std::unique_ptr<PictureDecoder>> lanes_;   // lanes 1 .. (this is lane 0)
  std::vector<xvcgpu_event *> pic_done_;                  // per position of a sequence
  bool has_output_ = false;                               // SetOutputFormat called
  xvcgpu_output_format output_ = {};
  int output_display_w_ = 0, output_display_h_ = 0;
};

}  // namespace xvc_gpu

// C entry points over the class (for bindings that cannot take C++ types, e.g.
// the ctypes tests): thin, no logic.
extern "C" {
typedef struct xvc_host_picture_decoder xvc_host_picture_decoder;
xvc_host_picture_decoder *xvc_host_picture_decoder_create(xvcgpu_ctx *ctx, int width, int height,
                                                          int bitdepth);
void xvc_host_picture_decoder_destroy(xvc_host_picture_decoder *d);
int xvc_host_picture_decoder_decode(xvc_host_picture_decoder *d, const xvc_picture_syntax *ps,
                                    const xvc_cu_syntax *cus, const int16_t *levels,
                                    const xvcgpu_picture *const *ref_pics /* [2][5] */,
                                    xvcgpu_picture *rec);
int xvc_host_picture_decoder_decode_sequence(xvc_host_picture_decoder *d, int n,
                                             const xvc_picture_syntax *const *ps,
                                             const xvc_cu_syntax *const *cus,
                                             const int16_t *const *levels,
                                             const int32_t *ref_index,
                                             xvcgpu_picture *const *recs);
// PictureDecoder::SetOutputFormat / DecodeSequence with d_out (one device buffer per
// picture, in decoding order)
int xvc_host_picture_decoder_set_output_format(xvc_host_picture_decoder *d,
                                               const xvcgpu_output_format *fmt,
                                               int display_w, int display_h);
int xvc_host_picture_decoder_decode_sequence_out(xvc_host_picture_decoder *d, int n,
                                                 const xvc_picture_syntax *const *ps,
                                                 const xvc_cu_syntax *const *cus,
                                                 const int16_t *const *levels,
                                                 const int32_t *ref_index,
                                                 xvcgpu_picture *const *recs,
                                                 void *const *d_out);
// a further picture lane on `ctx` (PictureDecoder::AddLane)
int xvc_host_picture_decoder_add_lane(xvc_host_picture_decoder *d, xvcgpu_ctx *ctx);
int xvc_host_picture_decoder_waves(const xvc_host_picture_decoder *d);
int xvc_host_picture_decoder_launches(const xvc_host_picture_decoder *d);
void xvc_host_picture_decoder_one_launch_intra(xvc_host_picture_decoder *d, int on);
// Host-only planning check: neighbour state per CU (9 bytes: flags[3],
// above_right[3], below_left[3]) and the wave of every CU.
int xvc_host_plan_picture(const xvc_picture_syntax *ps, const xvc_cu_syntax *cus,
                          const int16_t *levels, uint8_t *neighbors_out, int32_t *wave_out);
}

#endif  // XVC_AMD_HOST_XVC_PICTURE_DECODER_H_
