/*
 * xvcgpu.h -- C-ABI of libxvcgpu.so: the MI355X (gfx950) implementation of the
 * data-parallel part of xvc's per-CU encoder inner loop.
 *
 * This is the drop-in boundary.  The reference
 * has no device boundary: its "operator plug-in point" is three structs of
 * C function pointers called once per block (sample_metric.h:166-191,
 * inter_prediction.h:176-216) plus direct member calls for transforms,
 * dequant, deblocking and padding.  One block per call is tens of ns - far
 * below a kernel launch - so every entry point here is the BATCHED form of
 * one of those calls: same arithmetic, same argument meaning, N independent
 * blocks per launch.  The reference-side binding a maintainer would add is
 * shown in INTEGRATION.md.
 *
 * Conventions
 *  - plain C types only; no HIP/torch types.  Device memory is passed as
 *    `void *` device pointers obtained from xvcgpu_malloc() (or any HIP
 *    allocation of the same device, e.g. a torch tensor's data_ptr()).
 *  - every function returns an xvcgpu_status; xvcgpu_last_error() gives text.
 *    No exceptions cross the ABI (mirrors xvc_enc_return_code, xvcenc.h:34-45).
 *  - all launches go to the context's stream (xvcgpu_set_stream) and are
 *    asynchronous; xvcgpu_sync() waits.  Calls on one context must come from
 *    one thread at a time (the reference API is single-caller too,
 *    xvcenc.h:153-190); use one context per worker for concurrency, exactly
 *    as the reference uses one PictureEncoder per worker thread
 *    (thread_encoder.cc:99-159).
 *  - there is NO CPU fallback: without a gfx950 device xvcgpu_create() fails.
 */
#ifndef XVCGPU_H_
#define XVCGPU_H_

#include "xvcgpu_types.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef enum xvcgpu_status {
  XVCGPU_OK = 0,
  XVCGPU_INVALID_ARGUMENT = 10, /* cf. XVC_ENC_INVALID_ARGUMENT, xvcenc.h:37 */
  XVCGPU_NO_DEVICE = 20,
  XVCGPU_OUT_OF_MEMORY = 30,
  XVCGPU_DEVICE_ERROR = 40,
  XVCGPU_UNSUPPORTED = 50
} xvcgpu_status;

typedef struct xvcgpu_ctx xvcgpu_ctx;         /* one per device/worker      */
typedef struct xvcgpu_picture xvcgpu_picture; /* padded 4:2:0 planes in HBM */

/* ---- context ------------------------------------------------------------ */
xvcgpu_status xvcgpu_create(int device, xvcgpu_ctx **out);
void xvcgpu_destroy(xvcgpu_ctx *ctx);
const char *xvcgpu_last_error(const xvcgpu_ctx *ctx);
/* Version string "xvcgpu <major>.<minor> gfx950". Callable without a GPU. */
const char *xvcgpu_version(void);
/* The hipStream_t the context launches on (its own stream unless
 * xvcgpu_set_stream replaced it) - for callers that must order other work
 * after it, e.g. wrap it as torch.cuda.ExternalStream so that RCCL operations
 * are issued on the same stream as the kernels. */
void *xvcgpu_get_stream(const xvcgpu_ctx *ctx);
/* Launch on an external hipStream_t (e.g. torch's current stream, so kernels
 * order with torch copies and RCCL collectives); NULL = the device's default
 * stream.  xvcgpu_use_own_stream() returns to a private non-blocking stream
 * (the state after xvcgpu_create). */
xvcgpu_status xvcgpu_set_stream(xvcgpu_ctx *ctx, void *hip_stream);
xvcgpu_status xvcgpu_use_own_stream(xvcgpu_ctx *ctx);
/* Several contexts on one device = several queues the GPU drains concurrently
 * (the mirror of the reference's picture worker threads, thread_encoder.cc:
 * 99-159).  xvcgpu_use_priority_stream gives the context a private stream of
 * high (non-zero) or low priority: the low-priority queue fills the slots the
 * high-priority one leaves idle while its kernels ramp up and drain.
 * xvcgpu_wait_for(ctx, other): work queued on `ctx` after this call starts
 * only when everything queued on `other` before it has finished (an event). */
xvcgpu_status xvcgpu_use_priority_stream(xvcgpu_ctx *ctx, int high);
xvcgpu_status xvcgpu_wait_for(xvcgpu_ctx *ctx, xvcgpu_ctx *other);
xvcgpu_status xvcgpu_sync(xvcgpu_ctx *ctx);
/* on != 0: the short kernels that end a whole-picture xvcgpu_frame_pass (inverse
 * transform, the fused deblock / pad / PSNR tail) run on a second, high-priority
 * stream of the context, ordered with the rest of the pass by events - for several
 * picture chains in flight on one device, whose searches otherwise keep every CU
 * busy while another chain's 100-us tail waits.  Results do not depend on it. */
xvcgpu_status xvcgpu_set_short_kernel_priority(xvcgpu_ctx *ctx, int on);
/* HIP-event stopwatch on the context's stream (bench.py's timed region). */
xvcgpu_status xvcgpu_timer_begin(xvcgpu_ctx *ctx);
xvcgpu_status xvcgpu_timer_end(xvcgpu_ctx *ctx, float *elapsed_ms);
/* Several intervals in flight: record event `slot` (0..63) on the context's
 * stream now; later ask for the time between two recorded slots (waits for
 * slot_b only).  For timing one kernel while other streams keep the device
 * busy (bench.py's in-flight roofline figures). */
xvcgpu_status xvcgpu_timer_mark(xvcgpu_ctx *ctx, int slot);
xvcgpu_status xvcgpu_timer_between(xvcgpu_ctx *ctx, int slot_a, int slot_b,
                                   float *elapsed_ms);

/* ---- events and the RCCL exchange (xvc_amd/csrc/xvcgpu_comm.hip) ---------- *
 * Multi-GPU: one process and one communicator per GPU.  The ranks either code
 * independent pictures of a sub-GOP and ship each finished, padded reference
 * picture to the ranks that list it (the reference's only parallelism,
 * thread_encoder.cc:99-159; schedule: xvc_amd/host/xvc_picture_schedule.h), or
 * own CTU rows of one picture and trade the rows around a shard boundary for
 * the in-loop filter (deblocking_filter.cc:59-62).  Transfers are ncclSend /
 * ncclRecv on the communicator's own stream; events order them with the
 * kernels of the contexts:
 *   xvcgpu_event_record(ctx, ev)        ev = everything queued on ctx so far
 *   xvcgpu_comm_wait_event(comm, ev)    later transfers start after ev
 *   xvcgpu_comm_record_event(comm, ev)  ev = every transfer queued so far
 *   xvcgpu_event_wait(ctx, ev)          later kernels of ctx start after ev
 * Sends and receives that are enqueued in one agreed order on all ranks pair
 * up without deadlock; put transfers that may cross between
 * xvcgpu_comm_group_begin / _end (ncclGroupStart / ncclGroupEnd).
 * xvcgpu_comm_unique_id is called on one rank, its 128 bytes are handed to
 * the others by whatever started the processes (bench.py: torch.distributed's
 * store), then every rank calls xvcgpu_comm_create (collective). */
typedef struct xvcgpu_event xvcgpu_event;
typedef struct xvcgpu_comm xvcgpu_comm;
#define XVCGPU_COMM_ID_BYTES 128
xvcgpu_status xvcgpu_event_create(xvcgpu_ctx *ctx, xvcgpu_event **out);
void xvcgpu_event_destroy(xvcgpu_event *ev);
xvcgpu_status xvcgpu_event_record(xvcgpu_ctx *ctx, xvcgpu_event *ev);
xvcgpu_status xvcgpu_event_wait(xvcgpu_ctx *ctx, xvcgpu_event *ev);
xvcgpu_status xvcgpu_event_synchronize(xvcgpu_event *ev);
/* An upload that does not queue behind the context's kernels: on the context's COPY
 * stream (created on first use), after `after` (may be NULL: at once) - `done` is
 * recorded behind it; xvcgpu_event_wait(ctx, done) makes later kernels see the bytes.
 * The next picture's job lists go up while this picture's kernels run
 * (xvc_gpu::PictureDecoder, two device staging buffers taking turns). */
xvcgpu_status xvcgpu_upload_ahead(xvcgpu_ctx *ctx, void *d_dst, const void *h_src, size_t bytes,
                                  xvcgpu_event *after, xvcgpu_event *done);
xvcgpu_status xvcgpu_comm_unique_id(uint8_t id[XVCGPU_COMM_ID_BYTES]);
xvcgpu_status xvcgpu_comm_create(xvcgpu_ctx *ctx, const uint8_t id[XVCGPU_COMM_ID_BYTES],
                                 int world, int rank, xvcgpu_comm **out);
void xvcgpu_comm_destroy(xvcgpu_comm *comm);
int xvcgpu_comm_world(const xvcgpu_comm *comm);
int xvcgpu_comm_rank(const xvcgpu_comm *comm);
xvcgpu_status xvcgpu_comm_wait_event(xvcgpu_comm *comm, xvcgpu_event *ev);
xvcgpu_status xvcgpu_comm_record_event(xvcgpu_comm *comm, xvcgpu_event *ev);
xvcgpu_status xvcgpu_comm_sync(xvcgpu_comm *comm);
xvcgpu_status xvcgpu_comm_group_begin(xvcgpu_comm *comm);
xvcgpu_status xvcgpu_comm_group_end(xvcgpu_comm *comm);
/* The whole padded picture (all three planes with their borders: 7.8 MB at
 * 1080p, one message). */
xvcgpu_status xvcgpu_comm_send_picture(xvcgpu_comm *comm, const xvcgpu_picture *pic, int dst);
xvcgpu_status xvcgpu_comm_recv_picture(xvcgpu_comm *comm, xvcgpu_picture *pic, int src);
/* Rows [y0, y1) in luma rows (even; chroma planes move rows y0/2 .. y1/2) of
 * the components in comp_mask (bit c), with their horizontal borders: one
 * message per plane. */
xvcgpu_status xvcgpu_comm_send_rows(xvcgpu_comm *comm, const xvcgpu_picture *pic, int comp_mask,
                                    int y0, int y1, int dst);
xvcgpu_status xvcgpu_comm_recv_rows(xvcgpu_comm *comm, xvcgpu_picture *pic, int comp_mask, int y0,
                                    int y1, int src);
/* Any contiguous device range (CU metadata rows of a shard boundary). */
xvcgpu_status xvcgpu_comm_send_bytes(xvcgpu_comm *comm, const void *d_src, size_t bytes, int dst);
xvcgpu_status xvcgpu_comm_recv_bytes(xvcgpu_comm *comm, void *d_dst, size_t bytes, int src);
/* Sum over the ranks of n 64-bit counters in device memory (PSNR parts of row
 * shards), in place. */
xvcgpu_status xvcgpu_comm_all_reduce_sum_u64(xvcgpu_comm *comm, uint64_t *d_values, int n);

/* ---- recorded call sequences (HIP graphs) --------------------------------- *
 * The per-picture sequence of launches is short kernels (8-110 us each), so
 * the launch path matters.  xvcgpu_record_begin() puts the context's private
 * stream into capture: the xvcgpu_* calls that follow are recorded instead of
 * executed (no call that synchronises - sync, timer_end, free, upload,
 * download - may be made while recording); xvcgpu_record_end() returns the
 * recording as a replayable handle.  xvcgpu_replay() enqueues the whole
 * sequence with one submission; the recorded device pointers and pictures
 * must stay alive and are used as they were passed.  This has no counterpart
 * in the reference (it has no launch cost); it is the device-side analogue of
 * one PictureEncoder::Encode call (picture_encoder.cc:75-160). */
typedef struct xvcgpu_recording xvcgpu_recording;
xvcgpu_status xvcgpu_record_begin(xvcgpu_ctx *ctx);
xvcgpu_status xvcgpu_record_end(xvcgpu_ctx *ctx, xvcgpu_recording **out);
xvcgpu_status xvcgpu_replay(xvcgpu_ctx *ctx, xvcgpu_recording *rec);
void xvcgpu_recording_destroy(xvcgpu_recording *rec);

/* ---- raw device memory -------------------------------------------------- */
xvcgpu_status xvcgpu_malloc(xvcgpu_ctx *ctx, size_t bytes, void **dev_ptr);
xvcgpu_status xvcgpu_free(xvcgpu_ctx *ctx, void *dev_ptr);
xvcgpu_status xvcgpu_memcpy_h2d(xvcgpu_ctx *ctx, void *dst, const void *src,
                                size_t bytes);
xvcgpu_status xvcgpu_memcpy_d2h(xvcgpu_ctx *ctx, void *dst, const void *src,
                                size_t bytes);
xvcgpu_status xvcgpu_memset(xvcgpu_ctx *ctx, void *dst, int value, size_t bytes);
/* Page-locked host memory and the copy that does not wait: the upload is queued
 * on the context's stream (ordered with its kernels) and the call returns at
 * once - `src` must stay untouched until an event recorded after the call has
 * completed (xvcgpu_event_record / _synchronize).  With pageable `src` the
 * runtime stages the bytes itself and the call may block. */
/* (hipHostMalloc: the memory is also addressable by the device under the same pointer -
 * a kernel's small results can be written straight into it, visible to the host once
 * the stream has been synchronised: no copy kernel, no separate read-back.) */
xvcgpu_status xvcgpu_host_alloc(xvcgpu_ctx *ctx, size_t bytes, void **host_ptr);
xvcgpu_status xvcgpu_host_free(xvcgpu_ctx *ctx, void *host_ptr);
xvcgpu_status xvcgpu_memcpy_h2d_async(xvcgpu_ctx *ctx, void *dst, const void *src,
                                      size_t bytes);
/* The read-back that does not wait: queued on the context's stream behind the
 * kernels that produce `src`; `dst` (page-locked, or the call may block) holds the
 * bytes once xvcgpu_sync / an event recorded after the call has completed.  Several
 * result arrays of one step are fetched with one wait. */
xvcgpu_status xvcgpu_memcpy_d2h_async(xvcgpu_ctx *ctx, void *dst, const void *src,
                                      size_t bytes);

/* ---- pictures ----------------------------------------------------------- *
 * Device twin of YuvPicture (yuv_pic.cc:32-68): planar Y,U,V of 16-bit
 * samples, every plane surrounded by a replicated border.  The reference uses
 * 80 luma / 40 chroma samples; here the border is 128 / 64 and strides are
 * rounded to 64 samples so that every row starts 256-byte aligned in HBM.
 * All MV clipping rules (inter_prediction.cc:769-782) keep reads within 80.
 * bitdepth: the internal bit depth, 8 to 12, the odd depths 9 and 11 included
 * (anything else: XVCGPU_INVALID_ARGUMENT); every kernel family takes all five. */
#define XVCGPU_BORDER_LUMA 128
#define XVCGPU_BORDER_CHROMA 64

xvcgpu_status xvcgpu_picture_create(xvcgpu_ctx *ctx, int width, int height,
                                    int bitdepth, xvcgpu_picture **out);
/* Bytes needed by a picture of this size (for xvcgpu_picture_wrap). */
size_t xvcgpu_picture_bytes(int width, int height);
/* Build a picture over caller-owned device memory (e.g. a torch tensor) of at
 * least xvcgpu_picture_bytes() bytes, 256-byte aligned. */
xvcgpu_status xvcgpu_picture_wrap(xvcgpu_ctx *ctx, int width, int height,
                                  int bitdepth, void *dev_mem, size_t bytes,
                                  xvcgpu_picture **out);
void xvcgpu_picture_destroy(xvcgpu_picture *pic);
/* Host <-> device transfer of the visible area; planes are tightly described
 * by (pointer, stride in samples).  Cf. YuvPicture::CopyToSameBitdepth
 * (yuv_pic.cc:78-116) for the download direction. */
xvcgpu_status xvcgpu_picture_upload(xvcgpu_picture *pic,
                                    const uint16_t *const planes[3],
                                    const ptrdiff_t strides[3]);
xvcgpu_status xvcgpu_picture_download(const xvcgpu_picture *pic,
                                      uint16_t *const planes[3],
                                      const ptrdiff_t strides[3]);
/* Transfer including the border (tests of PadBorder). border_x/y <= 128/64
 * luma, halved for chroma. */
xvcgpu_status xvcgpu_picture_upload_padded(xvcgpu_picture *pic,
                                           const uint16_t *const planes[3],
                                           const ptrdiff_t strides[3],
                                           int border_luma);
xvcgpu_status xvcgpu_picture_download_padded(const xvcgpu_picture *pic,
                                             uint16_t *const planes[3],
                                             const ptrdiff_t strides[3],
                                             int border_luma);
/* Device pointer to sample (0,0) of a plane and its stride in samples. */
xvcgpu_status xvcgpu_picture_plane(const xvcgpu_picture *pic, int comp,
                                   void **dev_ptr, ptrdiff_t *stride);
xvcgpu_status xvcgpu_picture_copy(xvcgpu_ctx *ctx, xvcgpu_picture *dst,
                                  const xvcgpu_picture *src);

/* ---- P1: YuvPicture::PadBorder (yuv_pic.cc:118-150) --------------------- */
xvcgpu_status xvcgpu_pad_border(xvcgpu_ctx *ctx, xvcgpu_picture *pic);

/* ---- M1..M7: SampleMetric::Compare, Sample x Sample --------------------- *
 * (sample_metric.cc:171-223, fn table sample_metric.h:166-191).
 * One candidate = block (x,y,w,h) of component `comp` in pic `a` against the
 * block displaced by the full-pel vector (mv_x,mv_y) in pic `b`.
 * out[i] = static_cast<Distortion>(dist * weight), exactly as Compare(). */
typedef struct xvcgpu_metric_cand {
  int16_t x, y;       /* position in the component plane                    */
  uint8_t w, h;       /* size in the component plane                        */
  uint8_t metric;     /* xvcgpu_metric                                      */
  int8_t qp;          /* raw luma qp (structural SSD only)                  */
  int16_t mv_x, mv_y; /* full-pel displacement into `b`                     */
} xvcgpu_metric_cand;

xvcgpu_status xvcgpu_metric_batch(xvcgpu_ctx *ctx, const xvcgpu_picture *a,
                                  const xvcgpu_picture *b, int comp,
                                  double weight, int structural_strength,
                                  const xvcgpu_metric_cand *d_cands, int n,
                                  uint64_t *d_out);

/* ---- T4 building block: motion-compensate, then Compare ------------------- *
 * What InterSearch::GetSubpelDist (inter_search.cc:1022-1031), EvalStartMvp
 * (:966-997) and SearchMergeCandidates (:165-197) do per candidate MV:
 * MotionCompensationMv of the luma block (x,y,w,h) of `orig` from `ref` with
 * the 1/16-pel vector (mv_x,mv_y) (clipped inside, ClipMv), then
 * SampleMetric::CompareSample(orig, prediction) with `metric`.
 * out[i] = the Distortion (weight 1.0: luma). */
typedef struct xvcgpu_mc_metric_cand {
  int16_t x, y;         /* luma position                                     */
  uint8_t w, h;         /* luma size                                         */
  uint8_t metric;       /* xvcgpu_metric                                     */
  int8_t qp;            /* raw luma qp (structural SSD only)                 */
  int32_t mv_x, mv_y;   /* 1/16-pel vector into `ref`                        */
} xvcgpu_mc_metric_cand;

xvcgpu_status xvcgpu_mc_metric_batch(xvcgpu_ctx *ctx, const xvcgpu_picture *orig,
                                     const xvcgpu_picture *ref,
                                     int structural_strength,
                                     const xvcgpu_mc_metric_cand *d_cands, int n,
                                     uint64_t *d_out);

/* ---- T1 + T3 (+W1, I1, M1, M4): MotionEstNormal with TZ search ---------- *
 * (inter_search.cc:606-662, inter_tz_search.cc:84-171, inter_search.cc:
 * 893-964).  One result per xvcgpu_me_block, bit-identical to running the
 * reference search on that block with the same predictor inputs.
 * Blocks: w, h in {4, 8, 16, 32, 64} (4x4 included: the reference's RD search
 * tries it); x, y multiples of 4
 * inside the picture.  The descriptors live in device memory, so a job the
 * search cannot take (any other size, or larger than max_block_size of
 * xvcgpu_me_search_sized) is reported in its result slot instead of an error
 * code: the XVCGPU_ME_UNSUPPORTED record - fullpel_cost = subpel_dist =
 * 0xffffffff, vectors 0 (no real result has cost 0xffffffff).
 * flags: XVCGPU_ME_FULLPEL runs the TZ search; XVCGPU_ME_SUBPEL runs the
 * 9+8 point half/quarter-pel refinement starting from results[i].fullpel_*
 * (taken from the TZ search when both flags are set).  XVCGPU_ME_LIC_JOBS: the
 * batch holds jobs with XVC_ME_USE_LIC (xvcgpu_types.h: AC-only metrics,
 * GetFullpelMetric / GetSubpelMetric inter_search.cc:1059-1076); their kernel
 * instances are launched beside the plain ones.  Without the flag such a job
 * is reported unsupported.  XVCGPU_ME_HINT_SQ16: a performance hint, never a
 * change of results - the caller expects (almost) every job of the 16 class to
 * be a 16x16 (or 16x8) CU, as in a picture's frame pass on a 16-sample CU grid:
 * the both-phases search then runs a kernel that takes only those shapes (five
 * waves per SIMD) and a second, small one that answers the jobs of any other size
 * a few per wave, one after the other - more slowly, same results.
 * XVCGPU_ME_ONLY_SQ16 (with both phases, max_block_size 16): the caller's word that
 * every job IS a 16x16 or 16x8 block - the second kernel is not launched, and a job
 * of any other shape is answered with the XVCGPU_ME_UNSUPPORTED record. */
#define XVCGPU_ME_FULLPEL 1
#define XVCGPU_ME_SUBPEL 2
#define XVCGPU_ME_LIC_JOBS 4
#define XVCGPU_ME_HINT_SQ16 8
#define XVCGPU_ME_ONLY_SQ16 16
#define XVCGPU_ME_UNSUPPORTED 0xffffffffu /* fullpel_cost / subpel_dist of a job not taken */
xvcgpu_status xvcgpu_me_search(xvcgpu_ctx *ctx, const xvcgpu_picture *orig,
                               const xvcgpu_picture *ref, int flags,
                               const xvcgpu_me_block *d_blocks, int n,
                               xvcgpu_me_result *d_results);

/* Same, when the caller knows that no block of the batch exceeds
 * max_block_size (16, 32 or 64) in either dimension: only the kernel variants
 * whose LDS footprint is needed are launched. */
xvcgpu_status xvcgpu_me_search_sized(xvcgpu_ctx *ctx, const xvcgpu_picture *orig,
                                     const xvcgpu_picture *ref, int flags,
                                     const xvcgpu_me_block *d_blocks, int n,
                                     xvcgpu_me_result *d_results,
                                     int max_block_size);

/* ---- I1: MotionCompensationMv, uni-prediction --------------------------- *
 * (inter_prediction.cc:740-758 -> FilterLuma/FilterChroma :1387-1448).
 * Writes the predicted block of component blk.comp into `pred` at the CU's
 * position (pred plays the role of TransformEncoder's pred buffers,
 * transform_encoder.cc:45-47). */
xvcgpu_status xvcgpu_mc_batch(xvcgpu_ctx *ctx, const xvcgpu_picture *ref,
                              xvcgpu_picture *pred,
                              const xvcgpu_mc_block *d_blocks, int n);

/* I3 (LIC half): InterPrediction::MotionCompensationMv for uni-pred CUs that
 * use local illumination compensation (inter_prediction.cc:740-758,
 * LocalIlluminationComp :1555-1575, DeriveLicParams :1577-1663): the ordinary
 * prediction, then scale / offset from a linear model fitted to the block's
 * row above / column left: `rec` (the current picture's reconstruction, which
 * must hold the neighbouring CUs) against `ref` displaced by the rounded
 * full-pel vector.  Written into `pred` at the block's position.  The wave of
 * CUs of one call must not depend on each other's reconstruction. */
xvcgpu_status xvcgpu_mc_lic_batch(xvcgpu_ctx *ctx, const xvcgpu_picture *ref,
                                  const xvcgpu_picture *rec, xvcgpu_picture *pred,
                                  const xvcgpu_mc_lic_block *d_blocks, int n);

/* ---- N1: the decoder's inter prediction, any inter CU ---------------------- *
 * InterPrediction::MotionCompensation (inter_prediction.cc:710-738) for n
 * (CU, component) jobs: uni- or bi-prediction from any of the picture's
 * reference pictures (refs[0..n_refs): the job names a slot per list),
 * translational or affine (MotionCompAffine :1044-1136, for either output
 * precision), with or without local illumination compensation (:1555-1663; the
 * model reads the neighbouring reconstruction from `rec`, so the CUs of one
 * call must not depend on each other).  Written into `pred` at the CU's
 * position.  n_refs <= 10 (two lists of kMaxNumRefPics, common.h:144). */
xvcgpu_status xvcgpu_inter_pred_batch(xvcgpu_ctx *ctx, const xvcgpu_picture *const *refs,
                                      int n_refs, const xvcgpu_picture *rec,
                                      xvcgpu_picture *pred,
                                      const xvcgpu_inter_block *d_blocks, int n);

/* The same with the RD search's destination: InterPrediction::MotionCompensation
 * writes into whatever SampleBuffer the caller passes (the encoder's
 * temp_pred_ / bipred buffers, inter_search.cc:96-99, :417), not into the
 * picture - overlapping candidate CUs of one CTU are then independent jobs.
 * Block i goes to `scratch` at d_dst[i] (luma position; chroma at half of it);
 * `scratch` is any picture of the same bit depth and chroma format, its size
 * is unrelated to the references'.  `rec` is read at the CUs' own positions
 * (LIC jobs only) and has the references' size. */
xvcgpu_status xvcgpu_inter_pred_batch_to(xvcgpu_ctx *ctx, const xvcgpu_picture *const *refs,
                                         int n_refs, const xvcgpu_picture *rec,
                                         xvcgpu_picture *scratch,
                                         const xvcgpu_inter_block *d_blocks,
                                         const xvcgpu_block_pos *d_dst, int n);

/* n block copies src -> dst (pictures of any two sizes): how the originals of
 * candidate CUs are brought beside their scratch predictions, so that the
 * residual / metric batches address one geometry (the reference passes
 * orig_pic_ + the CU position and a temp buffer side by side,
 * transform_encoder.cc:203-215).  Blocks must lie inside both pictures; the
 * destination blocks of one call must not overlap. */
xvcgpu_status xvcgpu_copy_blocks(xvcgpu_ctx *ctx, const xvcgpu_picture *src,
                                 xvcgpu_picture *dst, const xvcgpu_copy_block *d_blocks,
                                 int n);

/* The same for the blocks of a picture's CU loop in CU order - block 3 * cu + comp,
 * Y U V each, CUs up to 16x16 (what xvcgpu_fwd_from_me_classify leaves behind) -,
 * in place on `rec`, which holds the prediction: the U and V blocks of a CU share
 * a wave, blocks without levels cost a look at their count.  Same results as
 * xvcgpu_inv_transform_batch(ctx, rec, rec, d_blocks, 3 * n_cus, ...). */
xvcgpu_status xvcgpu_inv_transform_cu_order(xvcgpu_ctx *ctx, xvcgpu_picture *rec,
                                            const xvcgpu_tx_block *d_blocks, int n_cus,
                                            const int16_t *d_levels,
                                            const uint32_t *d_level_offsets,
                                            const int32_t *d_nnz);

/* ---- I3 (affine half): MotionCompAffine -> Sample ------------------------- *
 * (inter_prediction.cc:1044-1136): the CU is cut into sub-blocks whose size
 * follows from the corner-MV differences, each sub-block gets its own MV
 * (8-bit-fraction interpolation of the corner MVs, clipped) and is
 * motion-compensated with the ordinary luma / chroma filters.  Chroma follows
 * the reference's C kernels (its SSE2 kernels differ on 2-wide blocks). */
xvcgpu_status xvcgpu_mc_affine_batch(xvcgpu_ctx *ctx, const xvcgpu_picture *ref,
                                     xvcgpu_picture *pred,
                                     const xvcgpu_mc_affine_block *d_blocks, int n);

/* ---- I2: MotionCompensation of bi-predicted CUs --------------------------- *
 * (inter_prediction.cc:710-738: MotionCompUniPred -> int16 for both lists,
 * :1156-1172, then AddAvgBi :1545-1547).  ref0 / ref1 are the list-0 / list-1
 * reference pictures; writes component blk.comp of the CU into `pred`. */
xvcgpu_status xvcgpu_mc_bipred_batch(xvcgpu_ctx *ctx, const xvcgpu_picture *ref0,
                                     const xvcgpu_picture *ref1,
                                     xvcgpu_picture *pred,
                                     const xvcgpu_mc_bi_block *d_blocks, int n);

/* ---- M2 + T2 + T7: bi-prediction refinement search ------------------------ *
 * One inner step of InterSearch::SearchBiIterative (inter_search.cc:392-433)
 * per job: predict from the OTHER list with job.other_mv (ref_other), form
 * the int16 target 2*orig - pred (SubtractWeighted, sample_buffer.h:147-161),
 * then MotionEstNormal(kFullSearch, bipred=true, mv_bootstrap) on ref_search
 * (:606-662): FullSearch over DetermineMinMaxMv(boot, 4) with kSad/kSadFast
 * on the target (:853-891) and SubpelSearch with SATD on the target
 * (:893-964).  d_results[i]: fullpel_x/y = FullSearch result, mv_x/y = final
 * MV, subpel_dist = the function's *out_dist (SATD >> 1, :660),
 * fullpel_cost = 0.  max_block_size as in xvcgpu_me_search_sized; jobs that
 * cannot be taken get the XVCGPU_ME_UNSUPPORTED record. */
xvcgpu_status xvcgpu_bipred_search(xvcgpu_ctx *ctx, const xvcgpu_picture *orig,
                                   const xvcgpu_picture *ref_other,
                                   const xvcgpu_picture *ref_search,
                                   const xvcgpu_bi_block *d_jobs, int n,
                                   xvcgpu_me_result *d_results,
                                   int max_block_size);
/* The same step for CUs that try local illumination compensation
 * (cu.GetUseLic()): the other list's prediction is the compensated one
 * (inter_prediction.cc:710-722 -> LocalIlluminationComp :1555-1575; the model
 * reads the current reconstruction `rec` around the CU, d_neighbours[i] names
 * the CUs above / left of job i - only x, y of the neighbours and the
 * XVC_LIC_HAS_* bits of xvcgpu_mc_lic_block are read), the full-pel stage
 * compares with kSadAcOnly[Fast] and the sub-pel stage with kSatdAcOnly
 * (inter_search.cc:1059-1076), both on the int16 target. */
xvcgpu_status xvcgpu_bipred_search_lic(xvcgpu_ctx *ctx, const xvcgpu_picture *orig,
                                       const xvcgpu_picture *ref_other,
                                       const xvcgpu_picture *ref_search,
                                       const xvcgpu_picture *rec,
                                       const xvcgpu_bi_block *d_jobs,
                                       const xvcgpu_mc_lic_block *d_neighbours, int n,
                                       xvcgpu_me_result *d_results, int max_block_size);


/* Same for all three components of every CU of a motion search batch, taking
 * the MV from d_results[i].mv_* (InterPrediction::MotionCompensation for a
 * uni-pred CU, inter_prediction.cc:710-722): decisions stay in HBM. */
xvcgpu_status xvcgpu_mc_from_me(xvcgpu_ctx *ctx, const xvcgpu_picture *ref,
                                xvcgpu_picture *pred,
                                const xvcgpu_me_block *d_blocks,
                                const xvcgpu_me_result *d_results, int n);
/* Device-side host-driver glue: fill the deblocking metadata of n uni-pred
 * inter CUs (what CuEncoder stores into CodingUnit, cu_encoder.cc:543-577)
 * from the search results and the luma non-zero counts of the residual batch.
 * d_luma_tx_index[i] = index of CU i's luma block in d_nnz (NULL: identity). */
xvcgpu_status xvcgpu_cu_info_from_me(xvcgpu_ctx *ctx,
                                     const xvcgpu_me_block *d_blocks,
                                     const xvcgpu_me_result *d_results,
                                     const int32_t *d_nnz,
                                     const int32_t *d_luma_tx_index, int n,
                                     int qp_y, int qp_c, int ref_poc,
                                     xvcgpu_cu_info *d_cus);

/* ---- X1 + Q + Q1 + X2 + R1: TransformAndReconstruct --------------------- *
 * (transform_encoder.cc:203-285) with the reference's non-RDO quantiser
 * RdoQuant::QuantFast as shipped (rdo_quant.cc:156-201: sign-data hiding
 * CoeffSignHideFast :448-573 included; XVC_TXF_* bits in
 * xvcgpu_tx_block.intra_pic select the restricted mode / the coefficient scan
 * of small intra CUs).  For block i:
 * resi = orig - pred; coeff = T(resi); level = Q(coeff) -> d_levels +
 * d_level_offsets[i] (w*h int16, row-major, stride w); d_nnz[i] = non-zero
 * count; rec = cbf ? clip(pred + T^-1(Q^-1(level))) : pred.
 * d_levels / d_level_offsets / d_nnz may be NULL when not wanted. */
xvcgpu_status xvcgpu_residual_batch(xvcgpu_ctx *ctx, const xvcgpu_picture *orig,
                                    const xvcgpu_picture *pred,
                                    xvcgpu_picture *rec,
                                    const xvcgpu_tx_block *d_blocks, int n,
                                    int16_t *d_levels,
                                    const uint32_t *d_level_offsets,
                                    int32_t *d_nnz);
/* The same with the quantiser the reference's encoder always runs (Q2:
 * RdoQuant::QuantRdo with CoeffSignHideRdo, rdo_quant.cc:203-446, :575-687;
 * selected by transform_encoder.cc:230 because encoder_settings.h:59 is
 * rdo_quant = true) for the blocks whose intra_pic field carries XVC_TXF_RDOQ;
 * the others take QuantFast as above.  d_params[i] belongs to d_blocks[i]
 * (lambda and rd_factor in fixed point, computed by the host from the
 * reference's doubles; which context snapshot; intra / inter CU);
 * d_contexts[d_params[i].ctx_index] = the CABAC context states of the syntax
 * writer the reference would pass (rdo_quant.cc:254), read through
 * ContextModel::GetEntropyBits only.  Levels, non-zero counts and the
 * reconstruction are bit-identical to the reference's for any block size
 * 2..64 x 2..64 and any transform type pair. */
xvcgpu_status xvcgpu_residual_rdoq_batch(xvcgpu_ctx *ctx, const xvcgpu_picture *orig,
                                         const xvcgpu_picture *pred, xvcgpu_picture *rec,
                                         const xvcgpu_tx_block *d_blocks, int n,
                                         int16_t *d_levels, const uint32_t *d_level_offsets,
                                         int32_t *d_nnz,
                                         const xvcgpu_rdoq_contexts *d_contexts,
                                         const xvcgpu_rdoq_params *d_params);
/* The same for the blocks of ONE CU state (n <= 64) whose original and prediction lie
 * elsewhere: block i reads its original at d_src_pos[2 i] of `orig` and its prediction
 * at d_src_pos[2 i + 1] of `pred` (positions in the plane of the block's component) and
 * writes its reconstruction at its own (x, y) of `rec` - the RD search's alternatives
 * of a CU (CompressAndEvalTransform's default / transform-select / skip candidates)
 * each reconstruct into their own slot of a scratch picture from the one prediction
 * and the original picture itself, without the two block copies that put them side by
 * side.  orig may have another size than pred / rec.
 * d_eval_cands != NULL: the evaluation's distortions in the same launch
 * (xvcgpu_eval_dist_batch's arithmetic, xvcgpu_eval_cand): candidates [0, n_eval_head)
 * - the prediction against the original, the cbf-zero distortions - and candidate
 * n_eval_head + i, priced by the workgroup that has just reconstructed block i;
 * d_eval_out[c] for every candidate.  With it a CompressAndEvalCbf is two launches:
 * the prediction, and this. */
xvcgpu_status xvcgpu_residual_rdoq_batch_at(xvcgpu_ctx *ctx, const xvcgpu_picture *orig,
                                            const xvcgpu_picture *pred, xvcgpu_picture *rec,
                                            const xvcgpu_tx_block *d_blocks, int n,
                                            int16_t *d_levels, const uint32_t *d_level_offsets,
                                            int32_t *d_nnz,
                                            const xvcgpu_rdoq_contexts *d_contexts,
                                            const xvcgpu_rdoq_params *d_params,
                                            const xvcgpu_block_pos *d_src_pos,
                                            int structural_strength,
                                            const xvcgpu_eval_cand *d_eval_cands, int n_eval_head,
                                            uint64_t *d_eval_out);


/* Q2 alone: RdoQuant::QuantRdo on coefficients the caller holds (the output
 * of xvcgpu_fwd_transform_batch; the levels go to xvcgpu_inv_transform_batch):
 * block i reads w*h int16 at d_coeffs + d_offsets[i] and writes its levels at
 * d_levels + d_offsets[i], d_nnz[i] = RdoQuant::QuantRdo's return value (all
 * levels zero when it is 0).  n_coeffs = the number of int16 in d_coeffs
 * (sizes the per-coefficient scratch).  Only w, h, comp, qp and the
 * XVC_TXF_NO_SIGN_HIDING / scan bits of a block are read.  This is the
 * throughput form: several blocks share a wave (16 blocks up to 8x8, 4 up to
 * 16x16).  Blocks whose XVC_RDOQ_NO_2X2 case applies (2-wide, rdo_quant_2x2
 * off) are NOT taken here: route them to xvcgpu_residual_batch. */
xvcgpu_status xvcgpu_quant_rdo_batch(xvcgpu_ctx *ctx, int bitdepth,
                                     const xvcgpu_tx_block *d_blocks, int n,
                                     const int16_t *d_coeffs, const uint32_t *d_offsets,
                                     size_t n_coeffs, int16_t *d_levels, int32_t *d_nnz,
                                     const xvcgpu_rdoq_contexts *d_contexts,
                                     const xvcgpu_rdoq_params *d_params);

/* The two calls above with the classification pass of the quantiser (which
 * blocks hold a coefficient that quantises to a level at all - at QP 32 one in
 * eight) done by the forward transform, on the coefficients it has at hand:
 * xvcgpu_fwd_from_me_classify = xvcgpu_fwd_from_me + the blocks' classes into
 * the context's scratch, zero levels and d_nnz = 0 for the blocks the quantiser
 * has nothing to do for (their coefficients are not stored);
 * xvcgpu_quant_rdo_classified_batch = xvcgpu_quant_rdo_batch over the SAME
 * blocks (3 per CU: Y, U, V, in CU order) without its own pass over all
 * coefficients.  Nothing else of the context's RDOQ entry points may run in
 * between.  Same results as the plain pair.  d_cus (optional, both calls): the
 * CUs' deblocking records (xvcgpu_cu_info_from_me) written on the way - the
 * forward call writes them with cbf_luma = 0, the quantiser sets the flag of
 * the CUs whose luma block keeps a level. */
xvcgpu_status xvcgpu_fwd_from_me_classify(xvcgpu_ctx *ctx, const xvcgpu_picture *orig,
                                          const xvcgpu_picture *ref, xvcgpu_picture *pred,
                                          const xvcgpu_me_block *d_blocks,
                                          const xvcgpu_me_result *d_results, int n, int qp_y,
                                          int qp_c, int ref_poc, int16_t *d_coeffs,
                                          const uint32_t *d_coeff_offsets, size_t n_coeffs,
                                          int16_t *d_levels, int32_t *d_nnz,
                                          xvcgpu_cu_info *d_cus);
/* ... and with the quantiser's context snapshots and per-block parameters (the
 * ones xvcgpu_quant_rdo_classified_batch will be given, blocks 3 * cu + comp):
 * the forward transform then also runs the all-zero proof
 * (xvcgpu_quant_rdo_set_prove_zero, below) on the coefficients it holds - no
 * launch of its own, no second read - unless the proof is switched off (mode 0).
 * Both null: xvcgpu_fwd_from_me_classify. */
xvcgpu_status xvcgpu_fwd_from_me_classify_prove(
    xvcgpu_ctx *ctx, const xvcgpu_picture *orig, const xvcgpu_picture *ref, xvcgpu_picture *pred,
    const xvcgpu_me_block *d_blocks, const xvcgpu_me_result *d_results, int n, int qp_y, int qp_c,
    int ref_poc, int16_t *d_coeffs, const uint32_t *d_coeff_offsets, size_t n_coeffs,
    int16_t *d_levels, int32_t *d_nnz, xvcgpu_cu_info *d_cus,
    const xvcgpu_rdoq_contexts *d_contexts, const xvcgpu_rdoq_params *d_params);
xvcgpu_status xvcgpu_quant_rdo_classified_batch(xvcgpu_ctx *ctx, int bitdepth,
                                                const xvcgpu_tx_block *d_blocks, int n,
                                                const int16_t *d_coeffs,
                                                const uint32_t *d_offsets, size_t n_coeffs,
                                                int16_t *d_levels, int32_t *d_nnz,
                                                const xvcgpu_rdoq_contexts *d_contexts,
                                                const xvcgpu_rdoq_params *d_params,
                                                xvcgpu_cu_info *d_cus);

/* Sizes the context's scratch for batches of up to n blocks / n_coeffs
 * coefficients now, so that later xvcgpu_quant_rdo_batch calls never allocate
 * (required before recording them, xvcgpu_record_begin). */
xvcgpu_status xvcgpu_quant_rdo_reserve(xvcgpu_ctx *ctx, int n, size_t n_coeffs);

/* The all-zero proof ahead of the quantiser's walk (k_rdoq.h, rdoq_prove_zero_kernel):
 * blocks for which RdoQuant::QuantRdo (rdo_quant.cc:223-446) is bound to return 0 -
 * provable from the plain quantised magnitudes and the context snapshot - get their
 * zero levels from one more launch and never reach the walk.  Results are the same
 * either way; the launch pays when the walk is throughput bound (large batches, few
 * surviving levels) and costs a few percent when it is latency bound.
 * mode: 0 never, 1 always, -1 (default) for batches of XVCGPU_PROVE_ZERO_AUTO_BLOCKS
 * blocks or more - and, where the batch follows xvcgpu_fwd_from_me_classify, which
 * knows the picture's QP, only from XVCGPU_PROVE_ZERO_AUTO_QP up (measured with the
 * proof as its own launch, frame passes/s without -> with: 3840x2160 QP 27 1475 ->
 * 1440, QP 32 1841 -> 2036; 7680x4320 QP 37 525 -> 551; 1920x1080 QP 32 6811 ->
 * 6696).  A batch that follows xvcgpu_fwd_from_me_classify_prove needs no launch:
 * that call has run the proof already, for any mode but 0.  The environment
 * variable XVCGPU_PROVE_ZERO (0 / 1), read by xvcgpu_create, sets the initial mode. */
#define XVCGPU_PROVE_ZERO_AUTO_BLOCKS 65536
#define XVCGPU_PROVE_ZERO_AUTO_QP 30
xvcgpu_status xvcgpu_quant_rdo_set_prove_zero(xvcgpu_ctx *ctx, int mode);

/* How the quantiser builds its class lists from the per-block classes (k_rdoq.h).
 * Two launches of 1024-thread workgroups: rdoq_count_kernel counts the classes of each
 * chunk of 4096 blocks, rdoq_scatter_kernel sums the chunks in front of its own and
 * writes the indices.  One launch of 128-thread workgroups: rdoq_lists_kernel, where
 * every workgroup of 512 blocks counts the classes in front of it itself - a read
 * that grows with the square of the batch.  The lists are the same either way.
 * mode: 0 two launches, 1 one launch, -1 (default) one launch for batches of up to
 * XVCGPU_RDOQ_ONE_LAUNCH_LISTS_MAX_BLOCKS blocks: twice a 1920x1080 picture's
 * 3 x 8160 = 24 480, half a 3840x2160 picture's 3 x 32 400 = 97 200. */
#define XVCGPU_RDOQ_ONE_LAUNCH_LISTS_MAX_BLOCKS (2 * 3 * 8160)
xvcgpu_status xvcgpu_quant_rdo_set_list_form(xvcgpu_ctx *ctx, int mode);

/* Diagnostics: the number of blocks of the last xvcgpu_quant_rdo_batch that
 * needed the walk, by class (out[0]: diagonal scan, up to four 4x4 sub-blocks;
 * out[1]: diagonal scan, up to sixteen, sides up to 32 - both walked with four
 * lanes per sub-block; out[2]: everything else - more sub-blocks, 64-point sides,
 * the horizontal / vertical scans, 2-wide blocks); blocks whose coefficients all
 * quantise to zero are settled by the classification pass and not counted.
 * Synchronises the stream. */
xvcgpu_status xvcgpu_quant_rdo_class_counts(xvcgpu_ctx *ctx, int32_t out[3]);
/* Tests: the class lists the context's last quantiser call built - counts[c] block
 * indices of class c, ascending, at lists + c * cap (lists: 3 * cap entries; a count
 * above cap is XVCGPU_INVALID_ARGUMENT).  Synchronises the stream. */
xvcgpu_status xvcgpu_debug_rdoq_lists(xvcgpu_ctx *ctx, int32_t counts[3], int32_t *lists,
                                      int cap);
/* The walk is two launches: the four-lane classes (out[0], out[1] above) and the
 * general class (out[2]), whose waves hold 255 vector registers - even with an empty
 * list that launch waits for room beside other streams' kernels (190 us in flight
 * per 2160p picture with three picture chains).  A caller whose batches only hold
 * diagonal-scan blocks with 4x4 sub-blocks, sides up to 32 and at most sixteen
 * sub-blocks (a frame pass of CUs up to 16x16, say) sets on = 1 and the general
 * launch is not made.  A block outside that promise is not quantised; the next
 * xvcgpu_sync reports it as XVCGPU_INVALID_ARGUMENT (xvcgpu_last_error says why). */
xvcgpu_status xvcgpu_quant_rdo_set_four_lane_only(xvcgpu_ctx *ctx, int on);

/* I1 + the above fused, for the uni-pred inter CUs of a motion search batch
 * (InterSearch::CompressAndEvalCbf without the RD bookkeeping,
 * inter_search.cc:261-365): for CU i and each component, motion-compensate
 * with d_results[i].mv_*, run TransformAndReconstruct (DCT-2, QuantFast) into
 * `rec`, store the non-zero count at d_nnz[3*i + comp] and - when d_cus is
 * given - CU i's deblocking metadata at d_cus[i].  The prediction stays in
 * LDS.  CUs up to 16x16 with both dimensions >= 8 (else use xvcgpu_mc_from_me
 * + xvcgpu_residual_batch + xvcgpu_cu_info_from_me, which compute the same). */
xvcgpu_status xvcgpu_recon_from_me(xvcgpu_ctx *ctx, const xvcgpu_picture *orig,
                                   const xvcgpu_picture *ref, xvcgpu_picture *rec,
                                   const xvcgpu_me_block *d_blocks,
                                   const xvcgpu_me_result *d_results, int n,
                                   int qp_y, int qp_c, int intra_pic, int ref_poc,
                                   int32_t *d_nnz, xvcgpu_cu_info *d_cus);

/* The front half of that pipeline alone, for a quantiser that runs as its own
 * kernel (xvcgpu_quant_rdo_batch): MotionCompensationMv of CU i into `pred`
 * (TransformEncoder's prediction buffer) and the forward transform of orig -
 * pred, coefficients of the CU's Y / U / V block at d_coeffs +
 * d_coeff_offsets[3 * i + comp] (as xvcgpu_fwd_transform_batch writes them).
 * CUs up to 16x16. */
xvcgpu_status xvcgpu_fwd_from_me(xvcgpu_ctx *ctx, const xvcgpu_picture *orig,
                                 const xvcgpu_picture *ref, xvcgpu_picture *pred,
                                 const xvcgpu_me_block *d_blocks,
                                 const xvcgpu_me_result *d_results, int n, int16_t *d_coeffs,
                                 const uint32_t *d_coeff_offsets);
/* The same with RdoQuant::QuantRdo (see xvcgpu_residual_rdoq_batch):
 * d_params[3 * i + comp] belongs to component comp of CU i; tx_flags = the
 * XVC_TXF_* bits common to all blocks (XVC_TXF_RDOQ is implied). */
xvcgpu_status xvcgpu_recon_from_me_rdoq(xvcgpu_ctx *ctx, const xvcgpu_picture *orig,
                                        const xvcgpu_picture *ref, xvcgpu_picture *rec,
                                        const xvcgpu_me_block *d_blocks,
                                        const xvcgpu_me_result *d_results, int n,
                                        int qp_y, int qp_c, int tx_flags, int ref_poc,
                                        int32_t *d_nnz, xvcgpu_cu_info *d_cus,
                                        const xvcgpu_rdoq_contexts *d_contexts,
                                        const xvcgpu_rdoq_params *d_params);

/* X1 only: coefficients of (orig - pred) for a host-side quantiser (RDOQ stays
 * on the host). Output layout as d_levels. */
xvcgpu_status xvcgpu_fwd_transform_batch(xvcgpu_ctx *ctx,
                                         const xvcgpu_picture *orig,
                                         const xvcgpu_picture *pred,
                                         const xvcgpu_tx_block *d_blocks, int n,
                                         int16_t *d_coeffs,
                                         const uint32_t *d_coeff_offsets);
/* Q1 + X2 + R1: Quantize::Inverse -> InverseTransform -> AddClip for levels
 * chosen by the host (decoder reconstruction shares this entry point,
 * cu_decoder.cc:102-138). d_nnz[i] == 0 copies pred; dc-only shortcut applied
 * when d_nnz[i] == 1 and level[0] != 0 (transform_encoder.cc:241). 
 * `pred` and `rec` may be the same picture (the prediction was written where
 * the reconstruction goes): the blocks without levels then cost nothing. */
xvcgpu_status xvcgpu_inv_transform_batch(xvcgpu_ctx *ctx,
                                         const xvcgpu_picture *pred,
                                         xvcgpu_picture *rec,
                                         const xvcgpu_tx_block *d_blocks, int n,
                                         const int16_t *d_levels,
                                         const uint32_t *d_level_offsets,
                                         const int32_t *d_nnz);
/* The same, and the RD loop's distortion of the coded block in the residual
 * domain (M6 short-short: SampleMetric::CompareShort on temp_resi_orig_ /
 * temp_resi_, transform_encoder.cc:69-77, sample_metric.cc:286-290):
 * d_dist[i] = sum((orig - pred - T^-1(Q^-1(level)))^2) >> 2 (bitdepth - 8) over
 * block i - what TransformAndReconstruct's caller prices an inter block with
 * (fast_inter_transform_dist); the chroma distortion weight (:275-276) is the
 * caller's.  For a block without levels the reconstructed residual is zero. */
xvcgpu_status xvcgpu_inv_transform_dist_batch(xvcgpu_ctx *ctx, const xvcgpu_picture *orig,
                                              const xvcgpu_picture *pred, xvcgpu_picture *rec,
                                              const xvcgpu_tx_block *d_blocks, int n,
                                              const int16_t *d_levels,
                                              const uint32_t *d_level_offsets,
                                              const int32_t *d_nnz, uint64_t *d_dist);

/* ---- C1, decision half ----------------------------------------------------- *
 * TransformEncoder::CompressAndEvalTransform's choice among a component's
 * alternatives (transform_encoder.cc:53-201: default transform, all-zero block,
 * transform skip, the transform-select indices) and the tail of
 * InterSearch::CompressAndEvalCbf (inter_search.cc:316-361: root-cbf-zero test,
 * gate of the transform-select second pass), batched.  The distortions are the
 * outputs of xvcgpu_residual_rdoq_batch + xvcgpu_metric_batch /
 * xvcgpu_inv_transform_dist_batch (device arrays the caller gathers into the
 * alternative records, or fills from the host); the bits are what the caller's
 * RdoSyntaxWriter prices each alternative with.  Costs are formed and compared
 * exactly as the reference does: dist + (Cost)(bits * lambda + 0.5), first
 * strictly cheaper alternative wins.  One thread per job. */
xvcgpu_status xvcgpu_tx_eval_batch(xvcgpu_ctx *ctx, const xvcgpu_tx_eval_job *d_jobs, int n,
                                   const xvcgpu_tx_eval_alt *d_alts,
                                   xvcgpu_tx_eval_result *d_out);
xvcgpu_status xvcgpu_root_cbf_batch(xvcgpu_ctx *ctx, const xvcgpu_root_cbf_job *d_jobs, int n,
                                    xvcgpu_root_cbf_result *d_out);

/* ---- D1..D4: DeblockingFilter::DeblockPicture --------------------------- *
 * (deblocking_filter.cc:56-77). d_cu_map: one int32 per 4x4 luma cell,
 * row-major, `map_stride` entries per row, ceil(height/4) rows, value = index
 * into d_cus or -1. subblock_size 4 (default) or 8 (restricted mode). */
xvcgpu_status xvcgpu_deblock(xvcgpu_ctx *ctx, xvcgpu_picture *rec,
                             const xvcgpu_cu_info *d_cus, int n_cus,
                             const int32_t *d_cu_map, int map_stride,
                             int pic_is_bipred, int beta_offset, int tc_offset,
                             int subblock_size);

/* One pass (0 = vertical edges, 1 = horizontal edges) restricted to the
 * subblock rows y in [y_begin, y_end): the unit of CTU-row sharding.  Pass 1
 * of a shard must include the first subblock row of the shard below
 * (y_end = shard_end + subblock_size) once that shard's pass-0 rows have been
 * received (scheme B).  xvcgpu_deblock() == pass 0 then
 * pass 1 over [0, height). */
xvcgpu_status xvcgpu_deblock_rows(xvcgpu_ctx *ctx, xvcgpu_picture *rec,
                                  const xvcgpu_cu_info *d_cus, int n_cus,
                                  const int32_t *d_cu_map, int map_stride,
                                  int pic_is_bipred, int beta_offset,
                                  int tc_offset, int subblock_size, int pass,
                                  int y_begin, int y_end);

/* One CU tree's share of DeblockPicture (deblocking_filter.cc:56-77): both
 * passes over the whole picture, filtering only the planes in comp_mask (1 =
 * luma, 2 = chroma, 3 = both).  An intra picture codes luma and chroma in two
 * CU trees (picture_data.cc:71-76): the primary tree filters luma on the
 * 4-sample grid, the secondary tree chroma on the 8-sample grid (:63-75).
 * xvcgpu_deblock() == comp_mask 3. */
xvcgpu_status xvcgpu_deblock_tree(xvcgpu_ctx *ctx, xvcgpu_picture *rec,
                                  const xvcgpu_cu_info *d_cus, int n_cus,
                                  const int32_t *d_cu_map, int map_stride,
                                  int pic_is_bipred, int beta_offset, int tc_offset,
                                  int subblock_size, int comp_mask);

/* The tail of PictureEncoder::Encode in one pass over the picture
 * (picture_encoder.cc:141-151; one launch + the fold of the SSD parts):
 * DeblockPicture (deblocking_filter.cc:56-77, both passes, luma and chroma, the
 * default 4-sample subblocks) of `src` -> `dst`, PadBorder of `dst`
 * (yuv_pic.cc:118-150) and, when `orig` is given, the luma ComparePicture parts
 * of xvcgpu_picture_ssd(orig, dst, 0, shift_bitdepth) in d_ssd[0..1].
 * `src` (the unfiltered reconstruction; its border is not read for the result)
 * and `dst` must be different pictures of the same size.  Only for pictures
 * whose CUs are all at least 8x8 (every coding edge on the 8-sample grid, so no
 * two edges interact): the caller knows its CU tree; other pictures take
 * xvcgpu_deblock + xvcgpu_pad_border + xvcgpu_picture_ssd.  Width and height
 * must be multiples of 8 (XVCGPU_INVALID_ARGUMENT otherwise). */
xvcgpu_status xvcgpu_deblock_pad_ssd(xvcgpu_ctx *ctx, const xvcgpu_picture *src,
                                     xvcgpu_picture *dst, const xvcgpu_picture *orig,
                                     const xvcgpu_cu_info *d_cus, int n_cus,
                                     const int32_t *d_cu_map, int map_stride,
                                     int pic_is_bipred, int beta_offset, int tc_offset,
                                     int shift_bitdepth, uint64_t *d_ssd);

/* ---- picture SSD / PSNR parts ------------------------------------------- *
 * SampleMetric::ComparePicture / ComputePsnr block walk (sample_metric.cc:
 * 37-155): per-64x64-block SSD, each >> 2*(shift_bitdepth-8), summed.
 * d_out[0] = distortion, d_out[1] = sample count. */
xvcgpu_status xvcgpu_picture_ssd(xvcgpu_ctx *ctx, const xvcgpu_picture *a,
                                 const xvcgpu_picture *b, int comp,
                                 int shift_bitdepth, uint64_t *d_out);
/* The share of the blocks whose first row (in the component plane) lies in
 * [y_begin, y_end): shares of disjoint row ranges covering the picture add up
 * to xvcgpu_picture_ssd - what one CU-row shard contributes. */
xvcgpu_status xvcgpu_picture_ssd_rows(xvcgpu_ctx *ctx, const xvcgpu_picture *a,
                                      const xvcgpu_picture *b, int comp,
                                      int shift_bitdepth, int y_begin, int y_end,
                                      uint64_t *d_out);

/* ---- whole-picture passes around the hot path -------------------------- *
 * Decision-free, HBM-bound passes the encoder / decoder run on whole pictures
 * before and after the per-CU work; on the device so that planes never have to
 * visit the host.  All on the context's stream.
 *
 * Resampler::ConvertFrom without resizing (resample.cc:32-63, :152-262): packed
 * planar 4:2:0 input in device memory (Y, U, V back to back, rows tightly
 * packed; 1 byte per sample when in_bitdepth == 8, else 2 little endian) ->
 * the picture at its internal bit depth (samples << (bd - in_bitdepth)); when
 * the picture is larger than the input (internal size rounded up to the
 * minimum CU size) the last column / row is repeated.  Visible area only: call
 * xvcgpu_pad_border afterwards if the picture is searched. */
xvcgpu_status xvcgpu_picture_import(xvcgpu_ctx *ctx, xvcgpu_picture *pic,
                                    const void *d_src, int in_width, int in_height,
                                    int in_bitdepth);
/* Resampler::ConvertTo without resizing (resample.cc:96-147,
 * CopyToBytesWithShift :304-338 with the sample functions :475-551): the
 * display_width x display_height top-left part of the picture -> packed planar
 * bytes at out_bitdepth (same layout as above): copy / left shift when
 * out_bitdepth >= bd, else the rounding down-shift or, with `dither`, the
 * reference's error-feedback down-shift whose remainder runs through all
 * samples of a plane in raster order (computed here as a parallel prefix
 * sum). */
xvcgpu_status xvcgpu_picture_export(xvcgpu_ctx *ctx, const xvcgpu_picture *pic,
                                    void *d_dst, int display_width, int display_height,
                                    int out_bitdepth, int dither);
/* PictureDecoder::Postprocess -> Resampler::ConvertTo (resample.cc:94-148) with
 * every output format of xvc_decoder_parameters: any size (the 8-tap up /
 * 12-tap down filters of resample::Resample), 4:0:0 / 4:2:0 / 4:2:2 / 4:4:4
 * (with the exact-2x bilinear chroma path), interleaved ARGB through the
 * BT.601 / 709 / 2020 matrices, 8-16 bit.  The display_width x display_height
 * top-left part of the picture -> d_dst, the reference's bytes: planar planes
 * back to back, rows tightly packed, 1 byte per sample at <= 8 bit, else 2
 * (little endian); ARGB is four values per pixel in the order
 * ConvertColorSpace writes them (R, G, B, alpha = max).  Unset fields of `fmt`
 * are resolved as Decoder resolves them; d_dst holds xvcgpu_output_bytes of the
 * resolved format (for ARGB, aligned to 4 bytes per value).
 *
 * Edge rule (the one deliberate deviation): positions outside the picture are
 * clamped to its internal size, i.e. the picture is read as if
 * YuvPicture::PadBorder had run.  The reference pads only pictures with
 * tid == 0 or below the highest layer (picture_decoder.cc:198-199); for those
 * the bytes are the reference's, for the others they are in the interior and
 * at the edge this is the defined value where the reference reads a stale
 * border.  The device border is never read and the picture never written.
 *
 * XVCGPU_INVALID_ARGUMENT, with nothing written: a display size below 2 or
 * beyond the picture, an output width or height of 1 or above 32768 (or more
 * than INT_MAX samples), an unknown chroma format or matrix, a bit depth
 * outside 8..16, and the bilinear chroma path at out = in depth + 1 (its shift
 * is undefined in the reference: 4:4:4 at bd + 1, ARGB from an 11-bit
 * picture).  One launch per picture; with dither on a shift plane, three. */
size_t xvcgpu_output_bytes(const xvcgpu_output_format *fmt);
xvcgpu_status xvcgpu_picture_convert_to(xvcgpu_ctx *ctx, const xvcgpu_picture *pic,
                                        int display_width, int display_height,
                                        const xvcgpu_output_format *fmt, void *d_dst);
/* Checksum::CalculateCrc (checksum.cc:46-92): CRC-16 (0x1021, preset 0xffff,
 * low byte of a sample first, 16 trailing zero bits).  mode 0 = kMinOverhead:
 * one value over Y,U,V, d_hash[0..1]; mode 1 = kMaxRobust: one per plane,
 * d_hash[0..5] (high byte first).  d_hash: 8 bytes of device memory.  (The
 * reference's default, MD5, is a serial chain and stays on the host.) */
xvcgpu_status xvcgpu_picture_crc(xvcgpu_ctx *ctx, const xvcgpu_picture *pic, int mode,
                                 uint8_t *d_hash);
/* CuEncoder::CalcDeltaQpFromVariance (cu_encoder.cc:308-357), the integer
 * part: d_var16[by * ceil(w/16) + bx] = calc_variance of the 16x16 luma block
 * (blocks that hang over the picture edge read the border); and, if d_ctu_var
 * is not NULL, per ctu_size x ctu_size CTU in raster order the statistic the
 * QP offset is computed from: 1 + sorted in-picture block variances[blocks/2].
 * The host applies strength * (1.5 * log(v) - 15 - 2 * (bd - 8)). */
xvcgpu_status xvcgpu_variance_map(xvcgpu_ctx *ctx, const xvcgpu_picture *pic,
                                  uint64_t *d_var16, int ctu_size, uint64_t *d_ctu_var);
/* PictureEncoder::DetermineAllowLic (picture_encoder.cc:230-281): *d_out = sum
 * over the sample values of |histogram(luma of a) - histogram(luma of b)|; the
 * caller compares with (int)(0.06 * w * h). */
xvcgpu_status xvcgpu_histogram_distance(xvcgpu_ctx *ctx, const xvcgpu_picture *a,
                                        const xvcgpu_picture *b, int64_t *d_out);

/* ---- intra prediction and SATD mode pre-selection ----------------------- *
 * IntraPrediction::FillReferenceState + Predict (intra_prediction.cc:81-147;
 * ComputeRefSamples :707-848, FilterRefSamples :850-871, planar / DC / angular
 * with the edge filters :365-558), 67-mode set with the default restriction
 * flags, for a batch of independent blocks: each job reads its reference
 * samples from `rec` (the neighbours it declares available must already be
 * reconstructed there) and writes the prediction of job.mode into `pred` at
 * the block's position.  Any component; comp 0 applies the luma rules
 * (filtered references, edge filters up to 16x16).  Chroma jobs may also ask for
 * mode XVC_INTRA_MODE_LM_CHROMA (PredLmChroma, :560-686, :873-906): the linear
 * model from the CU's own reconstructed luma, which must be in `rec` already
 * (availability = picture edges only, as in the reference). */
xvcgpu_status xvcgpu_intra_pred_batch(xvcgpu_ctx *ctx, const xvcgpu_picture *rec,
                                      xvcgpu_picture *pred,
                                      const xvcgpu_intra_block *d_jobs, int n);
/* The decoder's intra picture in ONE launch: all dependency waves of
 * CuDecoder::DecompressCu for intra CUs (cu_decoder.cc:100-166: Predict,
 * InverseTransform, AddClip).  Wave w = jobs d_wave_first[w] ..
 * d_wave_first[w + 1] of BOTH lists - d_jobs[k] (the prediction, any size / mode,
 * LM chroma included) and d_blocks[k] (the same block's transform job) - whose
 * reference samples come from waves < w; levels / offsets / nnz as for
 * xvcgpu_inv_transform_batch.  A cooperative launch (the workgroups meet at a
 * grid barrier between waves): XVCGPU_UNSUPPORTED when the device refuses it -
 * the caller then issues xvcgpu_intra_pred_batch + xvcgpu_inv_transform_batch
 * per wave, the same result. */
xvcgpu_status xvcgpu_intra_recon_waves(xvcgpu_ctx *ctx, xvcgpu_picture *rec,
                                       xvcgpu_picture *pred,
                                       const xvcgpu_intra_block *d_jobs,
                                       const xvcgpu_tx_block *d_blocks,
                                       const int32_t *d_wave_first, int n_waves,
                                       const int16_t *d_levels,
                                       const uint32_t *d_level_offsets,
                                       const int32_t *d_nnz);
/* The prediction + SATD loop of IntraSearch::DetermineSlowIntraModes
 * (intra_search.cc:189-305) for luma blocks, all 67 modes per job (the reference
 * evaluates the even modes, then the odd neighbours of the best ones: any
 * subset it asks for is in the table): d_dist[job * 67 + mode] =
 * SampleMetric(kSatd)::CompareSample(original block, prediction).  The host
 * adds bits * lambda_sqrt from its entropy coder state and sorts.
 * max_block_size: an upper bound (4..64) of the block sides in the batch; it
 * sizes the on-chip tiles (batches of small blocks run at higher occupancy).
 * A job with a larger side is answered with d_dist[job][mode] = 0xffffffff for
 * every mode (XVCGPU_INTRA_SATD_UNSUPPORTED). */
#define XVCGPU_INTRA_SATD_UNSUPPORTED 0xffffffffu
xvcgpu_status xvcgpu_intra_satd_batch(xvcgpu_ctx *ctx, const xvcgpu_picture *orig,
                                      const xvcgpu_picture *rec,
                                      const xvcgpu_intra_block *d_jobs, int n,
                                      uint32_t *d_dist, int max_block_size);

/* The fold of the fast pass kept on the device, for pipelines that do not want a
 * host round trip per batch: mode[cu] = first arg min over the 67 modes of
 * d_dist[cu][mode] (+ d_mode_cost[cu][mode] when not NULL: the caller's rate
 * term, e.g. bits * lambda_sqrt rounded).  Written to d_modes[cu] (may be NULL)
 * and, when given, into the `per_cu` (1..3) consecutive prediction jobs of the
 * CU (every component takes the luma mode, i.e. DM chroma) and into the scan
 * bits (XVC_TXF_SCAN_SHIFT) of its `per_cu` consecutive transform blocks, luma
 * block first, by TransformHelper::DetermineScanOrder (transform.cc:1614-1637).
 * The reference's own decision (stable sort by double cost, N best to the slow
 * RDO pass, intra_search.cc:236-303) remains host work on d_dist. */
xvcgpu_status xvcgpu_intra_select_modes(xvcgpu_ctx *ctx, const uint32_t *d_dist,
                                        const uint32_t *d_mode_cost, int n,
                                        int32_t *d_modes, xvcgpu_intra_block *d_jobs,
                                        xvcgpu_tx_block *d_blocks, int per_cu);

/* Predict + TransformAndReconstruct in one launch for intra blocks up to 16x16
 * (IntraSearch::PredictAndTransform, intra_search.cc:172-187, with QuantFast;
 * the decoder's CuDecoder::DecompressIntra when `orig` is NULL): job i =
 * d_jobs[i] (the prediction) + d_blocks[i] (its transform block: same
 * component, position and size).  The prediction never leaves the chip.
 * orig != NULL: levels / nnz are written as by xvcgpu_residual_batch (the three
 * arrays may be NULL); orig == NULL: they are read as by
 * xvcgpu_inv_transform_batch.  In place on `rec`; the jobs of one call must not
 * depend on each other.  Larger blocks, 2-wide blocks, the 4x4 DST and
 * transform skip are not taken (use xvcgpu_intra_pred_batch +
 * xvcgpu_residual_batch / xvcgpu_inv_transform_batch). */
xvcgpu_status xvcgpu_intra_recon_batch(xvcgpu_ctx *ctx, const xvcgpu_picture *orig,
                                       xvcgpu_picture *rec,
                                       const xvcgpu_intra_block *d_jobs,
                                       const xvcgpu_tx_block *d_blocks, int n,
                                       int16_t *d_levels, const uint32_t *d_level_offsets,
                                       int32_t *d_nnz);

/* ---- T5: affine motion estimation ------------------------------------------ *
 * InterSearch::MotionEstAffine (inter_search.cc:664-749) for n (CU, list,
 * ref_idx) jobs on one reference picture - uni-pred (orig is the original
 * picture, 7 iterations at most) or, XVC_AFFINE_ME_BIPRED, the refinement
 * search of SearchBiIterative (:394-435) against 2 * orig - the other list's
 * affine prediction from `ref_other` (may be NULL when no job has the flag):
 * prediction from the affine predictor (and the optional bootstrap vector),
 * then per iteration AffineGradientSearch (:751-851: Sobel gradients, the 4x5
 * normal equations, elimination with partial pivoting, lround), DeriveMvAffine
 * (inter_prediction.cc:615-630), MotionCompAffine and the SATD / mvd-bit cost.
 * The reference's float / double arithmetic is reproduced exactly (every sum of
 * the normal equations is an exact multiple of 1/64 below 2^53, so its order
 * does not matter; the elimination is the same IEEE double sequence).
 * w, h in {16, 32, 64} (CodingUnit::CanUseAffine); any other shape is answered
 * with dist = iterations = 0xffffffff (XVCGPU_AFFINE_ME_UNSUPPORTED). */
#define XVCGPU_AFFINE_ME_UNSUPPORTED 0xffffffffu
xvcgpu_status xvcgpu_affine_me_batch(xvcgpu_ctx *ctx, const xvcgpu_picture *orig,
                                     const xvcgpu_picture *ref,
                                     const xvcgpu_picture *ref_other,
                                     const xvcgpu_affine_me_block *d_blocks, int n,
                                     xvcgpu_affine_me_result *d_results);

/* ---- one step of a CU state's SearchMotion into all its reference pictures -------- *
 * InterSearch::SearchMotion (inter_search.cc:199-259) runs every step once per (list,
 * reference picture) of the CU: SearchRefIdx's EvalStartMvp and MotionEstNormal
 * (:536-578), SearchBiIterative's refinement per pair of pictures (:392-433), the affine
 * searches (:664-749).  With the single-picture entry points above that is one launch per
 * picture with one job each, one after the other.  The *_refs forms take the CU's
 * reference pictures as a table (refs[0 .. n_refs), n_refs <= 10 = 2 lists x
 * kMaxNumRefPics) and per job the slot(s) of the picture(s) it works on, so one step is
 * ONE launch whose jobs run side by side.  d_slots: one byte per job
 * (xvcgpu_me_search_refs, xvcgpu_mc_metric_batch_refs) or two (the searched picture, then
 * the other list's: xvcgpu_bipred_search_refs, xvcgpu_affine_me_batch_refs; a uni-pred
 * affine job may name 255 as its second); a first slot >= n_refs marks "no job": its
 * result is left as it was.
 * The jobs of a CU state all have the CU's size: block_class (16, 32 or 64 = the class of
 * max(w, h) as xvcgpu_me_search_sized forms it) / cu_height name the one set of kernel
 * instances that is launched; a job of another class is not searched (16: it is
 * answered XVCGPU_ME_UNSUPPORTED).  Results are those of the single-picture calls, job
 * for job.  No LIC jobs (XVCGPU_ME_LIC_JOBS is refused). */
xvcgpu_status xvcgpu_me_search_refs(xvcgpu_ctx *ctx, const xvcgpu_picture *orig,
                                    const xvcgpu_picture *const *refs, int n_refs, int flags,
                                    const xvcgpu_me_block *d_blocks, const uint8_t *d_slots,
                                    int n, xvcgpu_me_result *d_results, int block_class);
xvcgpu_status xvcgpu_bipred_search_refs(xvcgpu_ctx *ctx, const xvcgpu_picture *orig,
                                        const xvcgpu_picture *const *refs, int n_refs,
                                        const xvcgpu_bi_block *d_jobs, const uint8_t *d_slots,
                                        int n, xvcgpu_me_result *d_results, int block_class);
xvcgpu_status xvcgpu_mc_metric_batch_refs(xvcgpu_ctx *ctx, const xvcgpu_picture *orig,
                                          const xvcgpu_picture *const *refs, int n_refs,
                                          int structural_strength,
                                          const xvcgpu_mc_metric_cand *d_cands,
                                          const uint8_t *d_slots, int n, uint64_t *d_out);
xvcgpu_status xvcgpu_affine_me_batch_refs(xvcgpu_ctx *ctx, const xvcgpu_picture *orig,
                                          const xvcgpu_picture *const *refs, int n_refs,
                                          const xvcgpu_affine_me_block *d_blocks,
                                          const uint8_t *d_slots, int n,
                                          xvcgpu_affine_me_result *d_results, int cu_height);

/* ---- the folds of one SearchMotion chain --------------------------------------- *
 * A pass record - xvcgpu_cs_pass, include/xvcgpu_types.h - describes one SearchMotion of a CU; the three
 * calls below run the host logic of InterSearch::SearchRefIdx / SearchBiIterative /
 * SearchMotion (inter_search.cc:199-259, :392-578) between the batched searches, ON the
 * device, each reading the previous step's results and writing the next step's jobs -
 * a CU state is enqueued once and read back once (no host round trip inside):
 *
 *   xvcgpu_mc_metric_batch (SAD of both predictors)     -> d_start_dist
 *   xvcgpu_cs_start_fold   EvalStartMvp's choice        -> the search jobs' predictor
 *                          (+ previous_fullpel_, + the affine bootstrap vector)
 *   xvcgpu_me_search / xvcgpu_affine_me_batch           -> d_me_res / d_aff_res
 *   xvcgpu_cs_uni_fold     EvalFinalMvpIdx, SetMvd, GetInterPredBits (default bit
 *                          prices, include/xvc_inter_bits.h), the cost fold per list,
 *                          the list SearchBiIterative searches
 *                                                       -> the refinement job slots
 *   xvcgpu_bipred_search / xvcgpu_affine_me_batch       -> d_bi_res / d_aff_res
 *   xvcgpu_cs_bi_fold      the refinement's costs, the three-way choice (:247-257),
 *                          the affine pass against the plain one (:85-93),
 *                          HasZeroMvd                   -> d_results, the evaluation's
 *                                                          xvcgpu_inter_block jobs
 *
 * Refinement job slots of a pass: bi_job + (searched list * R + ref_idx) * R + other
 * ref_idx, R = XVC_CS_MAX_REFS; the fold fills the slots this state searches and empties
 * the others (block width 0: the search kernels return at once), so the host can issue
 * one launch per slot that exists without knowing which list won.  The affine pass's
 * slots and search jobs live in the xvcgpu_affine_me_block array.  A call folds the
 * passes [first, first + n) of d_passes / d_results (an affine pass names its plain
 * pass by absolute index; the plain pass must have been folded by an EARLIER launch of
 * the same fold - the affine pass reads and updates its result record -, i.e. a call
 * never holds a pass together with its plain pass).  A pass with
 * XVC_CS_FORCE_L1_MVD_ZERO or bi_iterations > 1 is answered XVC_CS_WHICH_UNSUPPORTED
 * (xvcgpu_types.h), not computed. */
xvcgpu_status xvcgpu_cs_start_fold(xvcgpu_ctx *ctx, const xvcgpu_cs_pass *d_passes, int first,
    int n,
                                   const uint64_t *d_start_dist, xvcgpu_me_block *d_me_jobs,
                                   const xvcgpu_me_result *d_me_res,
                                   xvcgpu_affine_me_block *d_aff_jobs,
                                   xvcgpu_cs_result *d_results, int pic_w, int pic_h);
xvcgpu_status xvcgpu_cs_uni_fold(xvcgpu_ctx *ctx, const xvcgpu_cs_pass *d_passes, int first,
    int n,
                                 const xvcgpu_me_result *d_me_res,
                                 const xvcgpu_affine_me_result *d_aff_res,
                                 xvcgpu_cs_result *d_results, xvcgpu_bi_block *d_bi_jobs,
                                 xvcgpu_affine_me_block *d_aff_jobs);
xvcgpu_status xvcgpu_cs_bi_fold(xvcgpu_ctx *ctx, const xvcgpu_cs_pass *d_passes, int first,
    int n,
                                const xvcgpu_me_result *d_bi_res,
                                const xvcgpu_affine_me_result *d_aff_res,
                                xvcgpu_cs_result *d_results, xvcgpu_inter_block *d_ev_inter);

/* The merge ranking's fold (xvcgpu_types.h: xvcgpu_cs_merge): rankings [first, first + n)
 * of d_merges / d_results; d_dist the SATDs, d_cands the ranking's prediction jobs,
 * d_ev_inter the evaluation slots.  One launch, no host decision. */
xvcgpu_status xvcgpu_cs_merge_fold(xvcgpu_ctx *ctx, const xvcgpu_cs_merge *d_merges, int first,
                                   int n, const uint64_t *d_dist,
                                   const xvcgpu_inter_block *d_cands,
                                   xvcgpu_cs_merge_result *d_results,
                                   xvcgpu_inter_block *d_ev_inter);

/* ---- many chains, one launch per step kind ---------------------------------------- *
 * The pictures of one chain (the picture being coded, its reference pictures, the three
 * scratch pictures of its evaluations, its level and result arrays) as a device-resident
 * record; xvcgpu_cs_segs_launch then runs n_segs segments of one kind - the same kernel
 * bodies as the single-chain entry points named in xvcgpu_types.h, grid y = segment - on
 * ctx's stream.  Segments of one call must not depend on each other (they are the
 * current steps of DIFFERENT chains); a chain's next step goes into a later call.
 * All segments of a call share i0 where it selects a kernel instance (ME / BI / AFFINE).
 * The kernels read the segment records from page-locked memory of the context (a ring of
 * two 4 MiB halves; a half is written again only after the launches that read it have
 * passed), so a call takes any number of segments. */
xvcgpu_status xvcgpu_cs_env_create(xvcgpu_ctx *ctx, const xvcgpu_picture *orig,
                                   const xvcgpu_picture *const *refs, int n_refs,
                                   xvcgpu_picture *s_orig, xvcgpu_picture *s_pred,
                                   xvcgpu_picture *s_rec, int16_t *d_levels,
                                   xvcgpu_cs_result *d_results, xvcgpu_cs_env **out);
void xvcgpu_cs_env_destroy(xvcgpu_cs_env *env);
xvcgpu_status xvcgpu_cs_segs_launch(xvcgpu_ctx *ctx, int kind, const xvcgpu_cs_seg *segs,
                                    int n_segs);
/* 1 in *done when everything recorded into ev has completed, without waiting */
xvcgpu_status xvcgpu_event_query(xvcgpu_event *ev, int *done);

/* All distortions of an evaluation (CompressAndEvalCbf, inter_search.cc:261-365) in one
 * launch: candidate i compares its block of `orig` with the same block of `pred`
 * (versus = 0: the cbf-zero distortion) or of `rec` (versus = 1: an alternative's
 * reconstruction) in component comp with `metric`, times its weight -
 * out[i] = (uint64)(dist * weight) as SampleMetric::CompareSample returns it
 * (sample_metric.cc:221-222).  xvcgpu_metric_batch is one component, one picture pair
 * and one weight per launch. */
xvcgpu_status xvcgpu_eval_dist_batch(xvcgpu_ctx *ctx, const xvcgpu_picture *orig,
                                     const xvcgpu_picture *pred, const xvcgpu_picture *rec,
                                     int structural_strength, const xvcgpu_eval_cand *d_cands,
                                     int n, uint64_t *d_out);

/* ---- multi-GPU staging --------------------------------------------------- *
 * n device-to-device copies (descriptors in device memory) in one launch: packs
 * the row slabs / CU metadata rows a rank exchanges with its neighbours into
 * one contiguous buffer per exchange and unpacks what arrived, so that an
 * exchange is a single collective instead of a dozen point-to-point
 * operations (each of which costs ~10 us of host time through
 * torch.distributed).  Segments must not overlap each other. */
xvcgpu_status xvcgpu_copy_segments(xvcgpu_ctx *ctx, const xvcgpu_copy_segment *d_segments,
                                   int n);

/* ---- a picture per call ------------------------------------------------- *
 * The per-picture sequence of the entry points above behind one call (host
 * cost of one call instead of six; nothing new is computed): the phases set in
 * a->phases run in the order ENCODE (InterSearch::SearchMotion +
 * CompressAndEvalCbf for the uni-pred CUs of a->d_me), DEBLOCK_V, DEBLOCK_H
 * (DeblockingFilter::DeblockPicture, by rows so that a row shard can exchange
 * its halo in between), PAD (YuvPicture::PadBorder), SSD (ComparePicture parts).
 * Asynchronous on the context's stream like its parts.
 *
 * ENCODE with n_cus > 0 runs the search (xvcgpu_me_search_sized with me_shape, or the
 * plan's) and then the launches of a->form, which the caller names:
 *
 *   form (XVC_FP_FORM_)  launches behind the search              fields read beside the common ones
 *   RECON_FROM_ME        xvcgpu_recon_from_me, or _rdoq where     d_nnz, d_cus_own (optional);
 *                        d_rdoq_params is set                    d_rdoq_params + d_rdoq_contexts
 *   FWD_FROM_ME          xvcgpu_fwd_from_me_classify_prove ->     d_rdoq_params, d_rdoq_contexts, d_tx,
 *                        xvcgpu_quant_rdo_classified_batch ->     n_tx == 3 * n_cus, d_coeffs, n_coeffs,
 *                        xvcgpu_inv_transform_cu_order           d_levels, d_level_off, d_nnz, d_cus_own,
 *                                                                tx_four_lane_only
 *   FWD_TRANSFORM        xvcgpu_mc_from_me ->                     pred, d_luma_tx_index and those of
 *                        xvcgpu_fwd_transform_batch ->            FWD_FROM_ME (any n_tx)
 *                        xvcgpu_quant_rdo_batch ->
 *                        xvcgpu_inv_transform_batch ->
 *                        xvcgpu_cu_info_from_me
 *   RESIDUAL             xvcgpu_mc_from_me ->                     pred, d_tx, n_tx, d_luma_tx_index,
 *                        xvcgpu_residual_batch ->                 d_nnz, d_cus_own; d_levels +
 *                        xvcgpu_cu_info_from_me                  d_level_off optional; no d_rdoq_params
 *   RESIDUAL_RDOQ        the same around                         those of RESIDUAL, d_rdoq_params,
 *                        xvcgpu_residual_rdoq_batch              d_rdoq_contexts
 *
 * Common: orig, ref, rec, d_me, d_results, n_cus, max_block_size, qp_y, qp_c, ref_poc.
 * RECON_FROM_ME and FWD_FROM_ME take a CU whole: max_block_size <= 16 and, with a plan, no
 * CU side below 8.  Form 0, a form the block cannot run or a missing field is
 * XVCGPU_INVALID_ARGUMENT with a message naming it (xvcgpu_last_error), decided before the
 * first launch: a refused call has enqueued nothing.  A set but unused field changes nothing.
 * With scratch_rec, all phases and all rows (and no CU side of 4 in the plan) the form
 * reconstructs into scratch_rec and the pass ends with xvcgpu_deblock_pad_ssd; FWD_FROM_ME
 * then runs its inverse transform and that tail on the context's high-priority stream where
 * it has one. */
xvcgpu_status xvcgpu_frame_pass(xvcgpu_ctx *ctx, const xvcgpu_frame_pass_args *a,
                                int phases);

/* The frame passes of n independent pictures (the pictures the reference's
 * picture-level worker threads code at the same time, thread_encoder.cc:99-159)
 * with every kernel launched ONCE for all of them: the n motion searches run
 * beside each other, then the n transforms, ... - kernels of one kind share the
 * chip far better than kernels of different pictures' different stages do.
 * Same results as n calls of xvcgpu_frame_pass(ctxs[i], args[i], phases).
 * Everything is enqueued on ctxs[0]'s stream; ctxs[i] lends picture i its
 * scratch (its own stream must be idle or the same stream).  Batched for
 * 2 <= n <= 4 whole pictures of one size and device that end with the fused tail
 * (scratch_rec given, all phases), all of form FWD_FROM_ME or all of form
 * RECON_FROM_ME with QuantFast; anything else falls back to the n single calls, each
 * on its own context. */
xvcgpu_status xvcgpu_frame_pass_multi(xvcgpu_ctx *const *ctxs,
                                      const xvcgpu_frame_pass_args *const *args, int n,
                                      int phases);

/* ---- the search of a fixed job list through a plan ----------------------- *
 * A caller that searches the same list again and again - the CUs of a picture's pass, a
 * real partition with 64x64 beside 8x4 beside 16x16 CUs - sorts it once:
 * xvcgpu_me_plan_create reads the n descriptors on the device (one launch) and writes,
 * per bin (XVCGPU_ME_PLAN_*, xvcgpu_types.h), the list of its job indices in list order;
 * it synchronises once to read the counts back (a set-up call, like
 * xvcgpu_quant_rdo_reserve) and owns device memory until xvcgpu_me_plan_destroy.
 * max_block_size as in xvcgpu_me_search_sized.  The plan looks at w, h and the
 * XVC_ME_USE_LIC bit of the descriptors only: positions, predictors, lambda may change
 * between searches, the shapes may not (d_blocks must stay alive and in place).
 * xvcgpu_me_search_planned: the results of xvcgpu_me_search_sized(flags, d_blocks, n,
 * max_block_size), record for record, with one launch per non-empty bin over that bin's
 * jobs only - the exact shapes 16x16, 16x8 and 8x8 through instances with the shape
 * compiled in (both phases).  flags: XVCGPU_ME_FULLPEL / _SUBPEL / _LIC_JOBS (without
 * the latter the LIC bins are answered unsupported, as there); the shape hints mean
 * nothing here.  The straggler-first record of the full-pel search is kept by one launch,
 * the one with the most jobs.  Never synchronises. */
typedef struct xvcgpu_me_plan xvcgpu_me_plan;
xvcgpu_status xvcgpu_me_plan_create(xvcgpu_ctx *ctx, const xvcgpu_me_block *d_blocks, int n,
                                    int max_block_size, xvcgpu_me_plan **out);
xvcgpu_status xvcgpu_me_plan_counts(const xvcgpu_me_plan *plan,
                                    int32_t counts[XVCGPU_ME_PLAN_BINS]);
void xvcgpu_me_plan_destroy(xvcgpu_ctx *ctx, xvcgpu_me_plan *plan);
xvcgpu_status xvcgpu_me_search_planned(xvcgpu_ctx *ctx, const xvcgpu_picture *orig,
                                       const xvcgpu_picture *ref, int flags,
                                       const xvcgpu_me_plan *plan,
                                       xvcgpu_me_result *d_results);

/* xvcgpu_frame_pass with the search of a->d_me run through `plan` (made from a->d_me,
 * a->n_cus and the class of a->max_block_size; anything else: XVCGPU_INVALID_ARGUMENT), for
 * a pass over CUs of any mix of sizes.  The forms are those of xvcgpu_frame_pass; the plan
 * knows the shapes, so RECON_FROM_ME or FWD_FROM_ME over a plan that holds a CU side of 4 is
 * refused (XVCGPU_INVALID_ARGUMENT, not a wrong picture): such a partition, or one with a CU
 * above 16x16, runs FWD_TRANSFORM, RESIDUAL or RESIDUAL_RDOQ.  Only those store QuantFast
 * levels (d_levels), whatever the shapes.  The fused tail (scratch_rec) covers CUs without a
 * side of 4: with one in the plan scratch_rec is ignored and the pass ends with the separate
 * deblocking, padding and SSD launches. */
xvcgpu_status xvcgpu_frame_pass_planned(xvcgpu_ctx *ctx, const xvcgpu_frame_pass_args *a,
                                        const xvcgpu_me_plan *plan, int phases);

/* ---- the frame pass of a B picture ---------------------------------------- *
 * InterSearch::SearchMotion for two lists (inter_search.cc:198-259) over a whole picture
 * without leaving the device, composed of launches that exist and three one-thread-per-CU
 * decision kernels between them (each with its own entry point below), with num_ref[l] = 1
 * .. XVC_CS_MAX_REFS pictures per list as the reference encoder codes a B picture: inside a
 * sub-GOP the lists name the same pictures in opposite order, SearchRefIdx then re-uses
 * list 0's result for list 1 (same_poc_in_l0[r] >= 0, :536-542) and the final choice is made
 * against the best of the pictures only list 1 names (cost_l1_unique, :247-257).  ENCODE
 * runs, on the context's stream, without synchronising or allocating:
 *
 *   1  one search per (l, r) that is not re-used (d_me[l][r] on refs[slot[l][r]] ->
 *      d_results[l][r]), sized or through plans[l][r]
 *   2  xvcgpu_fp_bi_refs_uni_fold
 *   3  the refinement by block class: without plans xvcgpu_bipred_search_refs once per class
 *      16, 32, 64 up to p.max_block_size over the whole job list (the 16 launch answers
 *      jobs of the other classes with the unsupported record, the later launches overwrite
 *      it); with plans xvcgpu_bipred_search_refs_planned
 *   4  xvcgpu_fp_bi_refs_choice
 *   5  xvcgpu_inter_pred_batch(refs, n_refs -> p.pred, d_inter)
 *   6  the residual pipeline of p.form
 *   7  xvcgpu_cu_info_from_choice_refs
 *
 * and the phases behind it are xvcgpu_frame_pass's with the deblocking filter's
 * pic_is_bipred = 1 (the fused tail under the same conditions).  One picture per list is
 * num_ref = {1, 1}, same_poc_in_l0[0] = -1, n_refs = 2, slot = {{0}, {1}}: Rmax = 1, one
 * refinement job per CU, every slot byte a job, RefIdxBits 0.  Scope: one
 * refinement iteration, translational motion (no LIC, no affine), a job's mvp standing for
 * both AMVP entries of its (list, picture), the caller's closed-form side bits (3 / 3 / 5)
 * to which the device adds RefIdxBits(num_ref, r) = num_ref <= 1 ? 0 : r + 1 - (r == num_ref
 * - 1), whole pictures, p.form FWD_TRANSFORM, RESIDUAL or RESIDUAL_RDOQ.  Not: pictures
 * with only back references (force_l1_mvd_zero, refused), more iterations, real AMVP
 * derivation, CABAC-priced bits, a multi-picture form, row shards.
 * plans[l][r]: one plan for every searched (l, r), made from d_me[l][r] / n_cus /
 * max_block_size, or all NULL (entries of re-used pictures are ignored).  Refused with
 * XVCGPU_INVALID_ARGUMENT and a message naming the field, before the first launch: num_ref
 * out of range, same_poc_in_l0[r] >= num_ref[0], a re-used entry whose slot or POC differs
 * from its twin's, a slot >= n_refs, force_l1_mvd_zero, a missing array, plans for some
 * searched entries only or not made from their jobs, the forms RECON_FROM_ME and
 * FWD_FROM_ME, part of a picture, a picture of another size or depth.
 *
 * The three decision kernels read the tables of the args block (num_ref, same_poc_in_l0,
 * slot, ref_poc, d_me, d_results, side bits, the work arrays; p.n_cus CUs; the cu_info form
 * also p.d_nnz, p.d_luma_tx_index, p.qp_y, p.qp_c, p.d_cus_own) and nothing else of it.
 * xvcgpu_fp_bi_refs_uni_fold: per (l, r) in index order dist and vector are the search's,
 * or list 0's of same_poc_in_l0[r] for a re-used picture; cost = dist + (((side_bits_uni[l]
 * + RefIdxBits + 1 + GetMvdBits against d_me[l][r]'s mvp) * lambda16) >> 16), a 64-bit
 * product; best per list on strict <; cost_l1_unique over the unique pictures only;
 * search_list = cost_0 <= cost_1 ? 1 : 0 =: s.  Job [i * Rmax + k], k < num_ref[s]: blk =
 * d_me[s][k][i], boot_mv = the uni-directional vector of (s, k), other_mv = the winner of
 * list 1 - s; slot bytes {slot[s][k], slot[1-s][best_ref[1-s]]}; k >= num_ref[s]: slot bytes
 * XVC_FP_BI_NO_JOB, the job untouched.  A CU with an XVCGPU_ME_UNSUPPORTED search result:
 * the record all ones, no job in any slot.
 * xvcgpu_fp_bi_refs_choice: walks k in picture order from UINT32_MAX on strict <; bits =
 * side_bits_bi + for both lists RefIdxBits + 1 + mvd bits of that list's (picture, vector)
 * against that (l, r) job's mvp; ChooseUniOrBi(cost_l0, cost_l1_unique, cost_bi): bi on <=
 * both, else list 0 on cost_l0 <= cost_l1_unique, else the best unique list-1 state; writes
 * the record and the CU's prediction jobs d_inter[3 i + comp] with ref[l] = the table slot of
 * the chosen picture, or -1.
 * xvcgpu_cu_info_from_choice_refs: xvcgpu_cu_info_from_me for two lists - ref_idx0 = the
 * chosen list-0 index or -1, ref_poc[l] = the chosen picture's POC or -1, the four corners
 * the list's vector (an unused list zero), cbf_luma from d_nnz[d_luma_tx_index[i]]. */
xvcgpu_status xvcgpu_fp_bi_refs_uni_fold(xvcgpu_ctx *ctx,
                                         const xvcgpu_frame_pass_bi_refs_args *a);
xvcgpu_status xvcgpu_fp_bi_refs_choice(xvcgpu_ctx *ctx, const xvcgpu_frame_pass_bi_refs_args *a);
xvcgpu_status xvcgpu_cu_info_from_choice_refs(xvcgpu_ctx *ctx,
                                              const xvcgpu_frame_pass_bi_refs_args *a);
/* The refinement jobs of a CU list laid out by CU (job [cu * jobs_per_cu + k], slot bytes as
 * xvcgpu_bipred_search_refs) through the CU list's search plan: one launch per non-empty
 * class of the plan (16: the exact-shape bins and other16; 32: c32; 64: both c64 bins) over
 * that class's CUs only, workgroup g taking job order[g / jobs_per_cu] * jobs_per_cu + g %
 * jobs_per_cu.  Results equal the per-class xvcgpu_bipred_search_refs launches record for
 * record (the CUs of the plan's unsupported bin get the unsupported record where their slots
 * name a job).  A plan with LIC jobs is refused.  jobs_per_cu: 1 .. XVC_CS_MAX_REFS. */
xvcgpu_status xvcgpu_bipred_search_refs_planned(xvcgpu_ctx *ctx, const xvcgpu_picture *orig,
                                                const xvcgpu_picture *const *refs, int n_refs,
                                                const xvcgpu_me_plan *plan, int jobs_per_cu,
                                                const xvcgpu_bi_block *d_jobs,
                                                const uint8_t *d_slots,
                                                xvcgpu_me_result *d_results);
xvcgpu_status xvcgpu_frame_pass_bi_refs(
    xvcgpu_ctx *ctx, const xvcgpu_frame_pass_bi_refs_args *a,
    const xvcgpu_me_plan *const plans[2][XVC_CS_MAX_REFS], int phases);

/* ---- the frame passes with adaptive QP ------------------------------------- *
 * CuEncoder::EncodeCtu (cu_encoder.cc:92-97) gives every CTU its own QP, pic_qp +
 * CalcDeltaQpFromVariance (cu_encoder.cc:308-363; on by default, encoder_settings.h:89-90),
 * and every CU below it runs with that Qp object: its lambda_sqrt in the search, its
 * quantiser step, its RDOQ constants, its QP in the deblocking filter.  Here the QP map is
 * derived on the device from xvcgpu_variance_map's CTU statistic through the thresholds of
 * the table (xvcgpu_types.h: xvcgpu_aqp_table) and written into the job arrays the passes
 * read anyway; nothing is read back.
 *
 * xvcgpu_aqp_apply: one thread per CU, 256-thread workgroups, plain loads and stores.  CU i
 * (origin d_me[0][i].x, .y; n_me = 1 .. 2 * XVC_CS_MAX_REFS job arrays of the same CUs)
 * lies in CTU (y / ctu_size) * ctus_per_row + x / ctu_size; delta = XVC_AQP_DELTA_MIN +
 * #{k : d_ctu_var[ctu] >= var_min[k]}.  With the table's entry of that delta it writes
 * lambda16 of job i in every d_me array, qp of the transform blocks d_luma_tx_index[i] + 0,
 * 1, 2 (qp_y, qp_c, qp_c), lambda and rd_factor of the same three records of d_rdoq_params
 * (NULL: QuantFast, nothing to write; ctx_index and flags stay), {qp_y, qp_c} into
 * d_cu_qp[2 i] and the delta into d_ctu_dqp[ctu] (NULL: not wanted; a CTU that holds no CU
 * origin is not written) - and no other byte of those records.  The jobs must lie inside
 * the picture d_ctu_var was computed for.
 * xvcgpu_cu_info_set_qp: qp_y / qp_c of d_cus_own[i] = d_cu_qp[2 i], [2 i + 1], i < n: the
 * correction behind xvcgpu_cu_info_from_me / xvcgpu_cu_info_from_choice_refs, which write the
 * picture's scalar QP.
 *
 * xvcgpu_frame_pass_aqp: xvcgpu_frame_pass (plan NULL) or xvcgpu_frame_pass_planned with, in
 * front of the search, xvcgpu_variance_map(a->orig -> q->d_var16, q->d_ctu_var) and
 * xvcgpu_aqp_apply (a->d_me, a->d_tx, a->d_rdoq_params, a->d_luma_tx_index), and between the
 * CU records and the tail xvcgpu_cu_info_set_qp(a->d_cus_own).  a->d_me, a->d_tx and
 * a->d_rdoq_params are written (device memory of the caller's, const in the block for the
 * flat pass's sake); a->qp_y and a->qp_c are not read for anything that stays.  The RDOQ
 * context snapshot stays the caller's (the picture-initial one of pic_qp).  A plan reads
 * lambda16 from a->d_me at search time (it keeps job indices, no copy of the jobs), so
 * the plan of the flat pass serves.
 * xvcgpu_frame_pass_bi_refs_aqp: the same around xvcgpu_frame_pass_bi_refs, over every
 * b->d_me[l][r] of the lists (re-used entries too: their lambda16 prices list 1's side; the
 * refinement jobs are copied from them behind the apply launch).
 * Forms: those with a prediction picture and d_tx - FWD_TRANSFORM, RESIDUAL, RESIDUAL_RDOQ.
 * RECON_FROM_ME and FWD_FROM_ME build their transform blocks from the scalar QP inside their
 * kernels (and FWD_FROM_ME's all-zero proof is keyed on one QP): refused, naming `form`.
 * Whole pictures with XVC_FP_ENCODE only; no multi-picture form.  Every check - those of the
 * flat pass included - happens before the first launch (XVCGPU_INVALID_ARGUMENT, the message
 * names the field: form, a missing array of q, the row ranges, ctu_size, ctus_per_row
 * against the width of orig); after them the call only enqueues: no synchronisation, no
 * allocation.  A table of strength 0 (every threshold above pic_qp's delta 0) gives the flat
 * pass's bytes. */
xvcgpu_status xvcgpu_aqp_apply(xvcgpu_ctx *ctx, const xvcgpu_aqp_table *table,
                               const uint64_t *d_ctu_var, xvcgpu_me_block *const *d_me,
                               int n_me, xvcgpu_tx_block *d_tx,
                               xvcgpu_rdoq_params *d_rdoq_params,
                               const int32_t *d_luma_tx_index, int n_cus, int8_t *d_cu_qp,
                               int8_t *d_ctu_dqp);
xvcgpu_status xvcgpu_cu_info_set_qp(xvcgpu_ctx *ctx, xvcgpu_cu_info *d_cus_own,
                                    const int8_t *d_cu_qp, int n);
xvcgpu_status xvcgpu_frame_pass_aqp(xvcgpu_ctx *ctx, const xvcgpu_frame_pass_args *a,
                                    const xvcgpu_aqp_args *q, const xvcgpu_me_plan *plan,
                                    int phases);
xvcgpu_status xvcgpu_frame_pass_bi_refs_aqp(
    xvcgpu_ctx *ctx, const xvcgpu_frame_pass_bi_refs_args *b, const xvcgpu_aqp_args *q,
    const xvcgpu_me_plan *const plans[2][XVC_CS_MAX_REFS], int phases);

/* ---- the frame pass of a B picture with only back references ---------------------- *
 * Every inter picture of a low-delay encode is a B picture whose two lists hold earlier
 * pictures only (PictureData::DetermineForceBipredL1MvdZero).  SearchMotion then codes list 1
 * of a bi-directional CU without a vector difference, and differs from the pass above so
 * (inter_search.cc):
 *   - list 1, uni-directional (:470-471, :496-524): the candidate of picture r is the job's
 *     mvp itself, kept unclipped, priced by EvalStartMvp (:967-997) = SAD(orig, luma
 *     prediction at ClipMv(mvp)) + ((GetMvpBits(0, 2) * lambda16) >> 16) = SAD + (lambda16 >>
 *     16); the best on strict < in index order is cost_list[1] / best_ref[1].  A re-used
 *     picture is then done (neither searched nor priced from list 0's result); a unique one
 *     is searched as above and priced into cost_l1_unique / best_ref_l1_unique only.
 *   - SearchBiIterative (:410-413): one iteration, search_list = 0 whatever the costs say:
 *     every picture k of list 0 is refined against the mvp of d_me[1][best_ref[1]],
 *     bootstrapped from list 0's own vector of k.
 *   - the bits of a bi-directional state: list 1 adds RefIdxBits + 1 and no vector-difference
 *     bits (GetForceMvdZero).
 *   - ChooseUniOrBi(cost_l0, cost_l1_unique, cost_bi) as above; a bi-directional CU's mv[1]
 *     is that mvp, a list-1 CU's the unique picture's searched vector.
 * xvcgpu_frame_pass_bi_back is xvcgpu_frame_pass_bi_refs (q NULL) or
 * xvcgpu_frame_pass_bi_refs_aqp (q given: the apply launch in front reaches lambda16 of every
 * d_me[l][r], which the predictor cost reads) with xvcgpu_fp_bi_back_mvp_cost in front of
 * the fold and the two folds below in place of steps 2 and 4; the searches, the refinement
 * launches, the prediction, the residual pipeline, xvcgpu_cu_info_from_choice_refs and the
 * tail are used as they are.  The args block is the same and must carry force_l1_mvd_zero =
 * 1: a block with 0 is refused naming the field (the block holds no current POC, so the flag
 * is the caller's word).  Every check of the pass above (the flag's aside) and a missing
 * d_l1_mvp_cost are refused before the first launch; after the checks the call only enqueues.
 * The record stays xvcgpu_fp_bi_refs_result with search_list = 0 and cost_uni[1][r] the
 * predictor's cost.
 *
 * xvcgpu_fp_bi_back_mvp_cost: one launch over all (CU, list-1 picture), one wave each:
 * d_l1_mvp_cost[i * XVC_CS_MAX_REFS + r] = the price above of d_me[1][r][i] on
 * refs[slot[1][r]] (reads p.orig, refs, n_refs, the tables); r >= num_ref[1]: UINT32_MAX.
 * Every CU shape with w, h in {4, 8, 16, 32, 64} is taken; any other gets UINT32_MAX.
 * xvcgpu_fp_bi_back_uni_fold: list 0 as xvcgpu_fp_bi_refs_uni_fold; list 1 from
 * d_l1_mvp_cost; job [i * Rmax + k], k < num_ref[0]: blk = d_me[0][k][i], boot_mv = list 0's
 * vector of k, other_mv = the mvp of d_me[1][best_ref[1]][i], slot bytes {slot[0][k],
 * slot[1][best_ref[1]]}; k >= num_ref[0]: XVC_FP_BI_NO_JOB.  A CU with an unsupported search
 * result or predictor cost: the record all ones, no job.
 * xvcgpu_fp_bi_back_choice: xvcgpu_fp_bi_refs_choice with the bits and vectors above. */
xvcgpu_status xvcgpu_fp_bi_back_mvp_cost(xvcgpu_ctx *ctx,
                                         const xvcgpu_frame_pass_bi_refs_args *a,
                                         uint32_t *d_l1_mvp_cost);
xvcgpu_status xvcgpu_fp_bi_back_uni_fold(xvcgpu_ctx *ctx,
                                         const xvcgpu_frame_pass_bi_refs_args *a,
                                         const uint32_t *d_l1_mvp_cost);
xvcgpu_status xvcgpu_fp_bi_back_choice(xvcgpu_ctx *ctx, const xvcgpu_frame_pass_bi_refs_args *a);
xvcgpu_status xvcgpu_frame_pass_bi_back(
    xvcgpu_ctx *ctx, const xvcgpu_frame_pass_bi_refs_args *a, uint32_t *d_l1_mvp_cost,
    const xvcgpu_aqp_args *q /* NULL: one QP */,
    const xvcgpu_me_plan *const plans[2][XVC_CS_MAX_REFS], int phases);

/* ---- the P frame pass with affine motion ---------------------------------------- *
 * InterSearch::CompressInter (inter_search.cc:74-99): every CU that CanUseAffine is searched
 * twice, translational and with the three-corner model, and keeps the cheaper state.  The
 * pass composes launches that exist with four small ones (k_fp_affine.h); nothing is read
 * back.  xvcgpu_types.h: xvcgpu_fp_affine_result, xvcgpu_frame_pass_affine_args.
 *
 * xvcgpu_fp_affine_boot: one thread per listed CU (d_order[0 .. n_listed)), 256-thread
 * workgroups.  d_affine[i].bootstrap = the plain result's vector through ClipMv (the CU's
 * position in a pic_w x pic_h picture) at all three corners - DeriveMvAffine(mv, mv),
 * inter_prediction.cc:615-630: the third corner equals the first - and flags =
 * XVC_AFFINE_ME_HAS_BOOTSTRAP.  A plain result of XVCGPU_ME_UNSUPPORTED gives no job:
 * flags = XVC_AFFINE_ME_NO_JOB, bootstrap zero.  No other byte of the job is written, no
 * job outside the list is touched.
 * xvcgpu_affine_me_listed: xvcgpu_affine_me_batch over the jobs d_order names - workgroup
 * g of the instance of class c (NW = 2, 4, 8 waves for CU heights 16, 32, 64) takes job
 * d_order[first_c + g]; one launch per non-empty class.  d_order must be grouped as
 * n_class says (a job of another height than its class's is left alone).  Results equal
 * xvcgpu_affine_me_batch's record for record; records outside the list, and those of
 * XVC_AFFINE_ME_NO_JOB jobs, are not touched.
 * xvcgpu_fp_affine_choice: one thread per CU.  cost_plain = subpel_dist + (((side_bits + 1 +
 * GetMvdBits(mvp, mv, fullpel ? 2 : 0)) * lambda16) >> 16), cost_affine = dist +
 * (((side_bits + 1 + the exp-Golomb bits of corner 0's and corner 1's quarter-sample
 * difference to d_affine[i].mvp) * d_affine[i].lambda16) >> 16), both with 64-bit products
 * and kept in 32 bits; affine only where cost_affine < cost_plain.  A CU counts as searched
 * where it is capable (xvcgpu_types.h) and its job carries XVC_AFFINE_ME_HAS_BOOTSTRAP.
 * Writes d_choice[i] and d_inter[3 i + comp]: ref = {0, -1}, and XVC_INTER_AFFINE with the
 * three corners or the plain vector at corner 0; an unsupported plain search: the record
 * all ones, jobs with ref = {-1, -1}.
 * xvcgpu_cu_info_from_affine_choice: xvcgpu_cu_info_from_me with corners - an affine CU's
 * mv[0][UL, UR, DL] the result and DR = UR + DL - UL, else all four the vector; list 1
 * unused (ref_poc -1, vectors zero); cbf_luma from d_nnz[d_luma_tx_index[i]] (NULL: d_nnz[i]).
 *
 * xvcgpu_frame_pass_affine: the search (plan NULL: sized; else planned) -> boot -> the listed
 * search -> choice -> xvcgpu_inter_pred_batch({a->ref} -> a->pred, f->d_inter) -> the
 * residual pipeline of a->form -> the record kernel -> the tail exactly as xvcgpu_frame_pass
 * runs it, fused or separate.  Forms: FWD_TRANSFORM, RESIDUAL, RESIDUAL_RDOQ; the _from_me
 * forms predict inside their kernels and are refused, naming `form`.  Every check - the flat
 * pass's included - happens before the first launch (XVCGPU_INVALID_ARGUMENT, the message
 * names the field): a missing array, n_class counts below 0 or above n_cus in sum, part of
 * a picture, phases without XVC_FP_ENCODE, a plan with LIC jobs.  After them the call only
 * enqueues: no synchronisation, no allocation.  With no capable CU the pass gives
 * xvcgpu_frame_pass's bytes. */
xvcgpu_status xvcgpu_fp_affine_boot(xvcgpu_ctx *ctx, const xvcgpu_me_result *d_results,
                                    const int32_t *d_order, int n_listed, int pic_w,
                                    int pic_h, xvcgpu_affine_me_block *d_affine);
xvcgpu_status xvcgpu_affine_me_listed(xvcgpu_ctx *ctx, const xvcgpu_picture *orig,
                                      const xvcgpu_picture *ref,
                                      const xvcgpu_affine_me_block *d_blocks, int n,
                                      const int32_t *d_order, const int32_t n_class[3],
                                      xvcgpu_affine_me_result *d_results);
xvcgpu_status xvcgpu_fp_affine_choice(xvcgpu_ctx *ctx, const xvcgpu_me_block *d_me,
                                      const xvcgpu_me_result *d_results, int n_cus,
                                      const xvcgpu_frame_pass_affine_args *f);
xvcgpu_status xvcgpu_cu_info_from_affine_choice(
    xvcgpu_ctx *ctx, const xvcgpu_me_block *d_me, const xvcgpu_fp_affine_result *d_choice,
    const int32_t *d_nnz, const int32_t *d_luma_tx_index, int n, int qp_y, int qp_c,
    int ref_poc, xvcgpu_cu_info *d_cus_own);
xvcgpu_status xvcgpu_frame_pass_affine(xvcgpu_ctx *ctx, const xvcgpu_frame_pass_args *a,
                                       const xvcgpu_frame_pass_affine_args *f,
                                       const xvcgpu_me_plan *plan, int phases);

/* ---- the P frame pass with merge mode --------------------------------------------- *
 * CuEncoder::CompressInterPic runs CompressMerge before CompressInter (cu_encoder.cc:
 * 469-481): the CU takes one of five candidate motions and codes no vector difference; a
 * merge CU that keeps no level is a skip CU.  The pass puts a merge stage between the search
 * and the rest of the flat pass: launches that exist and three small ones (k_fp_merge.h);
 * nothing is read back.  xvcgpu_types.h: xvcgpu_fp_merge_cand, xvcgpu_fp_merge_ranking,
 * xvcgpu_fp_merge_result, xvcgpu_frame_pass_merge_args.  One list, one reference picture;
 * a B picture's lists: xvcgpu_frame_pass_bi_refs_merge, further down.
 *
 * Inputs per CU: XVC_FP_MERGE_CANDS = 5 candidates (constants::kNumInterMergeCandidates) in
 * merge-index order, m->d_cands[5 i + m]; vectors in 1/16 pel, unclipped; an input, as a
 * job's mvp is (no GetMergeCandidates derivation).  A candidate is valid only with ref_idx =
 * {0, -1}.
 *
 * xvcgpu_fp_merge_rank: InterSearch::SearchMergeCandidates (inter_search.cc:165-197).  One
 * wave per listed CU (m->d_order[0 .. n_listed), strictly ascending; NULL: the CUs 0 ..
 * n_listed - 1), two waves a workgroup; the CU's geometry is its plain job's.  dist[m] is the
 * SATD (XVC_METRIC_SATD) of the original luma block against the luma prediction at
 * ClipMv(mv[m]).  cost[m] = (double)dist[m] + (double)bits(m) * lambda_sqrt, bits(m) = m + 1 -
 * (m == 4), without contraction (-ffp-contract=off).  std::stable_sort is an insertion sort
 * that moves only on strictly smaller.  num = 4, lowered to k for every k = 4 .. 0 with
 * cost[k] > cost[0] * 1.25.  An invalid candidate, or a CU shape outside w, h in {4, 8, 16,
 * 32, 64}, gets dist = UINT32_MAX and ranks behind every real one.  Writes m->d_rank[i] of
 * the listed CUs: dist[5] by merge index, cost[5] sorted, order[5], num; records outside the
 * list are not touched.
 * xvcgpu_fp_merge_choice: one thread per CU.  The pass's own rule in the closed-form bits
 * every frame pass here uses - NOT the reference's RD comparison, which needs the entropy
 * coder.  m0 = order[0]; cost_merge = dist[m0] + (((merge_side_bits + bits(m0)) * lambda16)
 * >> 16); cost_plain = subpel_dist + (((side_bits + 1 + GetMvdBits(mvp, mv, fullpel ? 2 : 0))
 * * lambda16) >> 16) as xvcgpu_fp_affine_choice forms it; both with the plain job's lambda16,
 * a 64-bit product, kept in 32 bits.  Merge where cost_merge <= cost_plain: the reference
 * evaluates merge first and a later mode replaces it only on strict < (save_if_best_cost,
 * cu_encoder.cc:449-481).  use_merge = 0, cost_merge = UINT32_MAX, merge_idx = -1 where
 * dist[m0] == UINT32_MAX, where the plain job carries XVC_ME_USE_LIC and where the list does
 * not name the CU.  Writes m->d_choice[i] (skip = 0) and m->d_chosen[i]: a copy of
 * d_results[i], and where merge won mv_x, mv_y the candidate's unclipped vector and
 * subpel_dist = dist[m0].  A plain search answered with XVCGPU_ME_UNSUPPORTED: the record all
 * ones, the chosen result the unsupported record unchanged.
 * xvcgpu_fp_merge_skip: one thread per CU.  d_choice[i].skip = use_merge && no transform block
 * of the CU has a level (SetSkipFlag(!GetHasAnyCbf()), cu_encoder.cc:639): d_nnz[t], [t + 1],
 * [t + 2] (Y, U, V) with t = d_luma_tx_index[i], NULL: t = 3 i.  The layouts: the forms with a
 * prediction picture (FWD_TRANSFORM, RESIDUAL, RESIDUAL_RDOQ) keep a CU's counts at
 * d_luma_tx_index[i] + 0, 1, 2 (FrameDescriptors); RECON_FROM_ME and FWD_FROM_ME at 3 i + comp
 * (their kernels index the blocks 3 * cu + comp).  An all-ones record is left alone; nothing
 * but `skip` is written.  The forced-skip evaluation (CompressSkipOnly as an RD alternative)
 * is not part of the pass.
 *
 * xvcgpu_frame_pass_merge: the search (plan NULL: sized; else planned) -> rank -> choice ->
 * the launches of a->form behind the search exactly as xvcgpu_frame_pass runs them, on a copy
 * of the block whose d_results is m->d_chosen (everything behind the search reads d_me and
 * the results' mv_x / mv_y only; the prediction clips the vector, the CU records keep it
 * unclipped) -> skip -> the tail exactly as xvcgpu_frame_pass runs it, fused or separate.
 * All five forms.  a->d_results keeps the search's answer.  Every check - the flat pass's
 * included - happens before the first launch (XVCGPU_INVALID_ARGUMENT, the message names the
 * field): a missing array, n_listed outside [0, n_cus], part of a picture, phases without
 * XVC_FP_ENCODE, lambda_sqrt not finite or below 0.  After them the call only enqueues: no
 * synchronisation, no allocation.  With n_listed = 0 the pass gives xvcgpu_frame_pass's
 * bytes. */
xvcgpu_status xvcgpu_fp_merge_rank(xvcgpu_ctx *ctx, const xvcgpu_picture *orig,
                                   const xvcgpu_picture *ref, const xvcgpu_me_block *d_me,
                                   int n_cus, const xvcgpu_frame_pass_merge_args *m);
xvcgpu_status xvcgpu_fp_merge_choice(xvcgpu_ctx *ctx, const xvcgpu_me_block *d_me,
                                     const xvcgpu_me_result *d_results, int n_cus,
                                     const xvcgpu_frame_pass_merge_args *m);
xvcgpu_status xvcgpu_fp_merge_skip(xvcgpu_ctx *ctx, const int32_t *d_nnz,
                                   const int32_t *d_luma_tx_index, int n_cus,
                                   xvcgpu_fp_merge_result *d_choice);
xvcgpu_status xvcgpu_frame_pass_merge(xvcgpu_ctx *ctx, const xvcgpu_frame_pass_args *a,
                                      const xvcgpu_frame_pass_merge_args *m,
                                      const xvcgpu_me_plan *plan, int phases);

/* ---- the B frame pass with affine motion ---------------------------------------- *
 * CompressInter's second SearchMotion run (three-corner model, both lists, the
 * SearchBiIterative step on affine vectors) behind the plain run of
 * xvcgpu_frame_pass_bi_refs; k_fp_bi_affine.h; nothing is read back.  xvcgpu_types.h:
 * xvcgpu_fp_bi_affine_result, xvcgpu_frame_pass_bi_affine_args.  E = 2 * Rmax, Rmax =
 * max(num_ref); uni-directional job [i * E + l * Rmax + r], refinement job [i * Rmax + k].
 * The four small entries take the pass's two blocks and read the tables of `a`
 * (num_ref, same_poc_in_l0, slot, ref_poc, d_me, d_results, side bits, d_choice, d_inter).
 *
 * xvcgpu_fp_bi_affine_boot: one thread per (listed CU, e < E).  A job whose first slot byte
 * is XVC_FP_BI_NO_JOB is not touched; else bootstrap = the plain result's vector of (l, r)
 * through ClipMv at all three corners and flags = XVC_AFFINE_ME_HAS_BOOTSTRAP, or, for a
 * plain result of XVCGPU_ME_UNSUPPORTED, flags = XVC_AFFINE_ME_NO_JOB and bootstrap zero.
 * xvcgpu_affine_me_listed_refs: affine_me over the jobs of the listed CUs, per_cu jobs per
 * CU, every picture in one launch per non-empty height class (NW = 2, 4, 8 for heights 16,
 * 32, 64): workgroup g of class c takes job d_order[first_c + g / per_cu] * per_cu + g %
 * per_cu; the searched plane is refs[d_slots[2 job]], with XVC_AFFINE_ME_BIPRED the other
 * list's refs[d_slots[2 job + 1]].  A first slot byte >= n_refs, or XVC_AFFINE_ME_NO_JOB:
 * the result is not touched.  Results equal xvcgpu_affine_me_batch_refs' record for record.
 * xvcgpu_fp_bi_affine_uni_fold: one thread per CU.  A CU counts as searched where d_me[0][0]
 * says it is capable and every job of its E that names a picture carries
 * XVC_AFFINE_ME_HAS_BOOTSTRAP.  Per (l, r) in index order: dist and vectors are the search's,
 * for a re-used list-1 entry list 0's of same_poc_in_l0[r]; cost = dist + (((side_bits_uni[l]
 * + RefIdxBits(num_ref[l], r) + 1 + the exp-Golomb bits of corner 0's and corner 1's
 * quarter-sample difference to that job's mvp) * lambda16) >> 16), 64-bit product kept in 32
 * bits; best per list on strict <, cost_l1_unique over the unique pictures; search_list =
 * cost_0 <= cost_1 ? 1 : 0.  Writes the fold's fields of d_choice[i] and the CU's Rmax
 * refinement jobs: the (s, k) job's x, y, w, h, lambda16, mvp; bootstrap = the affine vectors
 * of (s, k); other_mv = the winner of list 1 - s; flags HAS_BOOTSTRAP | BIPRED; slot bytes
 * {slot[s][k], slot[1-s][best_ref[1-s]]}, XVC_FP_BI_NO_JOB first for k >= num_ref[s].  A CU
 * that was not searched: no-job slots only.
 * xvcgpu_fp_bi_affine_choice: one thread per CU.  k in picture order from UINT32_MAX on
 * strict <; bits = side_bits_bi + for both lists RefIdxBits + 1 + the corner bits against
 * that (l, r) job's mvp; ChooseUniOrBi(cost_l0, cost_l1_unique, cost_bi) as
 * xvcgpu_fp_bi_refs_choice; affine only where cost_affine < a->d_choice[i].cost.  Writes
 * f->d_choice[i]; where affine wins rewrites a->d_inter[3 i + comp] (XVC_INTER_AFFINE, ref[l]
 * = the slot or -1, three corners per used list), else leaves them.
 * xvcgpu_cu_info_from_bi_affine_choice: xvcgpu_cu_info_from_choice_refs with corners (an
 * affine CU's used list: UL, UR, DL and DR = UR + DL - UL).
 *
 * xvcgpu_frame_pass_bi_refs_affine: launches 1-4 of xvcgpu_frame_pass_bi_refs unchanged ->
 * boot -> the listed search over the E jobs -> uni fold -> the listed search over the
 * refinement jobs -> choice -> xvcgpu_inter_pred_batch -> the residual pipeline of the form
 * -> the record kernel -> the B tail.  Every check of xvcgpu_frame_pass_bi_refs (a set
 * force_l1_mvd_zero, the _from_me forms, part of a picture, plans with LIC jobs) and of `f`
 * (a missing array, n_class) happens before the first launch; then the call only enqueues. */
xvcgpu_status xvcgpu_fp_bi_affine_boot(xvcgpu_ctx *ctx, const xvcgpu_frame_pass_bi_refs_args *a,
                                       const xvcgpu_frame_pass_bi_affine_args *f);
xvcgpu_status xvcgpu_affine_me_listed_refs(xvcgpu_ctx *ctx, const xvcgpu_picture *orig,
                                           const xvcgpu_picture *const *refs, int n_refs,
                                           const xvcgpu_affine_me_block *d_blocks,
                                           const uint8_t *d_slots, int n_cus, int per_cu,
                                           const int32_t *d_order, const int32_t n_class[3],
                                           xvcgpu_affine_me_result *d_results);
xvcgpu_status xvcgpu_fp_bi_affine_uni_fold(xvcgpu_ctx *ctx,
                                           const xvcgpu_frame_pass_bi_refs_args *a,
                                           const xvcgpu_frame_pass_bi_affine_args *f);
xvcgpu_status xvcgpu_fp_bi_affine_choice(xvcgpu_ctx *ctx,
                                         const xvcgpu_frame_pass_bi_refs_args *a,
                                         const xvcgpu_frame_pass_bi_affine_args *f);
xvcgpu_status xvcgpu_cu_info_from_bi_affine_choice(xvcgpu_ctx *ctx,
                                                   const xvcgpu_frame_pass_bi_refs_args *a,
                                                   const xvcgpu_frame_pass_bi_affine_args *f);
xvcgpu_status xvcgpu_frame_pass_bi_refs_affine(
    xvcgpu_ctx *ctx, const xvcgpu_frame_pass_bi_refs_args *a,
    const xvcgpu_frame_pass_bi_affine_args *f,
    const xvcgpu_me_plan *const plans[2][XVC_CS_MAX_REFS], int phases);

/* ---- the B frame pass with merge mode --------------------------------------------- *
 * CompressMerge before CompressInter (cu_encoder.cc:469-481) for a B picture: a merge stage
 * between xvcgpu_fp_bi_refs_choice and the prediction of xvcgpu_frame_pass_bi_refs; launches
 * that exist and three new ones (k_fp_bi_merge.h); nothing is read back.  xvcgpu_types.h:
 * xvcgpu_fp_merge_cand, xvcgpu_fp_merge_ranking, xvcgpu_fp_bi_merge_result,
 * xvcgpu_frame_pass_bi_merge_args.  The small entries take the pass's two blocks and read
 * the tables of `a` (num_ref, slot, refs, d_me[0][0], d_choice, d_inter).
 *
 * Inputs per CU: XVC_FP_MERGE_CANDS = 5 candidates in merge-index order, m->d_cands[5 i + m];
 * vectors in 1/16 pel, unclipped; an input, as a job's mvp is (no GetMergeCandidates
 * derivation).  A candidate is valid when each ref_idx[l] is -1 or in 0 .. num_ref[l] - 1 and
 * at least one list is used.  The picture for list l is refs[slot[l][ref_idx[l]]].
 *
 * xvcgpu_fp_bi_merge_rank: InterSearch::SearchMergeCandidates (inter_search.cc:165-197) with
 * MotionCompensation's two branches (inter_prediction.cc:710-738).  One wave per listed CU
 * (m->d_order[0 .. n_listed), strictly ascending; NULL: the CUs 0 .. n_listed - 1), two waves a
 * workgroup; the CU's geometry is that of d_me[0][0][i].  One list used: dist[m] is the SATD
 * (XVC_METRIC_SATD) of the original luma block against the luma prediction at ClipMv(mv[l])
 * from that list's picture.  Both lists used: each list's luma prediction is taken at ClipMv
 * of its own vector in the 14-bit intermediate form (MotionCompRefList with post_filter =
 * false), AddAvgBi follows (:1545-1547: (p0 + p1 + (1 << (s - 1)) + 2 * 8192) >> s clipped to
 * the depth, s = max(2, 14 - depth) + 1), and dist[m] is the SATD against that.  No prediction
 * goes to memory.  cost, the stable sort and num: as xvcgpu_fp_merge_rank.  A candidate that
 * is invalid, or whose CU shape is outside w, h in {4, 8, 16, 32, 64}, gets dist = UINT32_MAX.
 * Writes m->d_rank[i] of the listed CUs; records outside the list are not touched.
 * xvcgpu_fp_bi_merge_choice: one thread per CU.  m0 = order[0]; cost_merge = dist[m0] +
 * (((merge_side_bits + bits(m0)) * lambda16) >> 16) with the lambda16 of d_me[0][0][i], a
 * 64-bit product, kept in 32 bits; compared with the plain run's a->d_choice[i].cost.  Merge
 * where cost_merge <= cost: the reference evaluates merge first and a later mode replaces it
 * only on strict <.  No merge - use_merge = 0, cost_merge = UINT32_MAX, merge_idx = -1 - where
 * dist[m0] == UINT32_MAX, where the list does not name the CU and where the plain job
 * d_me[0][0][i] carries XVC_ME_USE_LIC (and for a candidate m0 that is not valid, whatever
 * the ranking record says).  Writes m->d_choice[i] (skip = 0) and m->d_chosen[i]: a copy of
 * a->d_choice[i], and where merge won inter_dir, ref_idx, mv (an unused list gets -1 and zero)
 * and cost are the candidate's.  For a merge winner the CU's three jobs a->d_inter[3 i + comp]
 * are rewritten: ref[l] the table slot or -1, the vectors unclipped; other jobs are left
 * alone.  a->d_choice is not written.  A plain record of all ones stays all ones in both
 * outputs.
 * xvcgpu_fp_bi_merge_skip: xvcgpu_fp_merge_skip on xvcgpu_fp_bi_merge_result records:
 * d_choice[i].skip = use_merge && d_nnz[t], [t + 1], [t + 2] are all zero, t =
 * d_luma_tx_index[i], NULL: t = 3 i.  An all-ones record is left alone.
 *
 * xvcgpu_frame_pass_bi_refs_merge: the launches of xvcgpu_frame_pass_bi_refs up to its choice
 * unchanged -> rank -> choice -> xvcgpu_inter_pred_batch over a->d_inter -> the residual
 * pipeline of the form -> xvcgpu_cu_info_from_choice_refs on a copy of the block whose
 * d_choice is m->d_chosen (ref_poc, ref_idx0 and the vectors are the chosen state's) -> skip
 * -> the B tail.  Every check of xvcgpu_frame_pass_bi_refs (a set force_l1_mvd_zero, the
 * _from_me forms, part of a picture, plans with LIC jobs) and of `m` happens before the first
 * launch (XVCGPU_INVALID_ARGUMENT, the message names the field): a missing array (d_cands,
 * d_rank, d_choice, d_chosen, p.d_nnz), m->d_chosen or m->d_choice that is a->d_choice or
 * each other, n_listed outside [0, n_cus], phases without
 * XVC_FP_ENCODE, lambda_sqrt not finite or below 0.  After them the call only enqueues: no
 * synchronisation, no allocation.  With n_listed = 0 the pass gives
 * xvcgpu_frame_pass_bi_refs' bytes.  Not together with affine motion, adaptive QP or
 * force_l1_mvd_zero. */
xvcgpu_status xvcgpu_fp_bi_merge_rank(xvcgpu_ctx *ctx, const xvcgpu_frame_pass_bi_refs_args *a,
                                      const xvcgpu_frame_pass_bi_merge_args *m);
xvcgpu_status xvcgpu_fp_bi_merge_choice(xvcgpu_ctx *ctx, const xvcgpu_frame_pass_bi_refs_args *a,
                                        const xvcgpu_frame_pass_bi_merge_args *m);
xvcgpu_status xvcgpu_fp_bi_merge_skip(xvcgpu_ctx *ctx, const int32_t *d_nnz,
                                      const int32_t *d_luma_tx_index, int n_cus,
                                      xvcgpu_fp_bi_merge_result *d_choice);
xvcgpu_status xvcgpu_frame_pass_bi_refs_merge(
    xvcgpu_ctx *ctx, const xvcgpu_frame_pass_bi_refs_args *a,
    const xvcgpu_frame_pass_bi_merge_args *m,
    const xvcgpu_me_plan *const plans[2][XVC_CS_MAX_REFS], int phases);

/* ---- tables (host side, no GPU needed) ---------------------------------- *
 * The 8-bit-fraction transform matrices the kernels use (transform_data.cc:
 * 109-796), for table-equality tests. out: size*size int16 row-major. */
xvcgpu_status xvcgpu_get_transform_matrix(int tx_type, int size, int16_t *out);

#ifdef __cplusplus
}
#endif
#endif /* XVCGPU_H_ */
