// xvcgpu.hip -- C-ABI implementation of libxvcgpu.so (see include/xvcgpu.h).
// gfx950 only; no CPU fallback anywhere in this file.
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <new>
#include <vector>

#include "k_deblock.h"
#include "k_tail.h"
#include "k_me.h"
#include "k_me2.h"
#include "k_me_plan.h"
#include "k_metric.h"
#include "k_misc.h"
#include "k_pad.h"
#include "k_tx.h"
#include "k_tx2.h"
#include "k_recon.h"
#include "k_bipred.h"
#include "k_stats.h"
#include "k_output.h"
#include "k_intra.h"
#include "k_affine_me.h"
#include "k_inter_pred.h"
#include "k_multi.h"
#include "k_rd.h"
#include "k_intra_waves.h"
#include "k_cu_state.h"
#include "k_cs_engine.h"
#include "k_fp_bi_refs.h"
#include "k_fp_bi_back.h"
#include "k_aqp.h"
#include "k_fp_affine.h"
#include "k_fp_merge.h"
#include "k_fp_bi_affine.h"
#include "k_fp_bi_merge.h"
#include "xvcgpu_internal.h"

namespace {

xvcgpu_status fail(xvcgpu_ctx *ctx, xvcgpu_status st, const char *what,
                   hipError_t e = hipSuccess) {
  if (ctx) {
    ctx->err = what;
    if (e != hipSuccess) {
      ctx->err += ": ";
      ctx->err += hipGetErrorString(e);
    }
  }
  return st;
}

#define HIP_TRY(ctx, call)                                              \
  do {                                                                  \
    hipError_t e_ = (call);                                             \
    if (e_ != hipSuccess) return fail(ctx, XVCGPU_DEVICE_ERROR, #call, e_); \
  } while (0)

#define CHECK_LAUNCH(ctx, name)                                          \
  do {                                                                   \
    hipError_t e_ = hipGetLastError();                                   \
    if (e_ != hipSuccess) return fail(ctx, XVCGPU_DEVICE_ERROR, name, e_); \
  } while (0)

inline int round_up(int v, int m) { return (v + m - 1) / m * m; }

// Grow-only scratch of a context: *slot holds room for *cap units (items, tiles, rows,
// blocks - the caller's measure).  Where `want` is more, the old buffer is freed once the
// context's stream - whose work may still use it - has drained, and `bytes` are
// allocated, zeroed on the context's stream where the scratch's readers rely on that.
template <typename T>
xvcgpu_status grow_scratch(xvcgpu_ctx *ctx, T **slot, int *cap, int want, size_t bytes,
                           bool zero, const char *what) {
  if (want <= *cap) return XVCGPU_OK;
  if (*slot) {
    hipStreamSynchronize(ctx->stream);
    hipFree(*slot);
    *slot = nullptr;
    *cap = 0;
  }
  const hipError_t e = hipMalloc(slot, bytes);
  if (e != hipSuccess) return fail(ctx, XVCGPU_OUT_OF_MEMORY, what, e);
  if (zero) hipMemsetAsync(*slot, 0, bytes, ctx->stream);
  *cap = want;
  return XVCGPU_OK;
}

// the context's RDOQ scratch as the kernels see it (the layout: k_rdoq.h)
RdoqLists rdoq_lists_of(const xvcgpu_ctx *ctx) {
  return rdoq_scratch_lists(ctx->d_rdoq_lists, ctx->rdoq_lists_cap);
}

// Blocks visited by ComparePicture on a w x h plane (sample_metric.cc:64-88).
inline int ssd_items(int w, int h) {
  const int mbx = w & ~(w - 1), mby = h & ~(h - 1);
  const int ncx = (w > 64 ? (w - 64 + 63) / 64 : 0) + (w - (w & ~63)) / mbx;
  const int ncy = (h > 64 ? (h - 64 + 63) / 64 : 0) + (h - (h & ~63)) / mby;
  return ncx * ncy;
}

// 64x64 tiles of xvcgpu_deblock_pad_ssd (k_tail.h).
inline int tail_tiles(int w, int h) { return ((w + 63) / 64) * ((h + 63) / 64); }

// Plane geometry shared by create / wrap / bytes.
struct Geometry {
  int w[3], h[3], border[3], stride[3], rows[3];
  size_t offset[3];  // byte offset of the plane's first padded row
  size_t bytes;
};

Geometry geometry(int width, int height) {
  Geometry g;
  size_t off = 0;
  for (int c = 0; c < 3; c++) {
    g.w[c] = c ? width / 2 : width;
    g.h[c] = c ? height / 2 : height;
    g.border[c] = c ? XVCGPU_BORDER_CHROMA : XVCGPU_BORDER_LUMA;
    g.stride[c] = round_up(g.w[c] + 2 * g.border[c], 64);
    g.rows[c] = g.h[c] + 2 * g.border[c];
    g.offset[c] = off;
    off += (size_t)g.stride[c] * g.rows[c] * sizeof(uint16_t);
    off = (off + 255) & ~(size_t)255;
  }
  g.bytes = off;
  return g;
}

bool valid_size(int width, int height, int bitdepth) {
  return width >= 8 && height >= 8 && (width % 8) == 0 && (height % 8) == 0 &&
         width <= 16384 && height <= 16384 && bitdepth >= 8 && bitdepth <= 12;
}

void init_views(xvcgpu_picture *p) {
  const Geometry g = geometry(p->w, p->h);
  for (int c = 0; c < 3; c++) {
    PlaneView &v = p->v.c[c];
    v.w = g.w[c];
    v.h = g.h[c];
    v.border = g.border[c];
    v.stride = g.stride[c];
    v.p = reinterpret_cast<uint16_t *>(static_cast<char *>(p->base) + g.offset[c]) +
          (size_t)g.border[c] * g.stride[c] + g.border[c];
  }
  p->v.bd = p->bd;
}

// Both residual kernels over one batch: the one-wave-per-job kernel takes the
// blocks up to 16x16, the scanning general-path kernel the rest.
#ifndef XVCGPU_INV_ONE_LAUNCH_MAX
#define XVCGPU_INV_ONE_LAUNCH_MAX 16384
#endif
template <int MODE>
void launch_residual(xvcgpu_ctx *ctx, const PicView &o, const PicView &p,
                            const PicView &r, const xvcgpu_tx_block *d_blocks, int n,
                            int16_t *d_levels, const uint32_t *d_off, int32_t *d_nnz,
                            unsigned long long *d_dist = nullptr, bool small_only = false) {
  // a decoded picture's dependency wave (a few thousand blocks, small and large mixed):
  // one launch, a workgroup per block - the two kernels below one behind the other are
  // two launches on the picture's critical path (5 + 12 us and the gap between them)
  if (MODE == TX_MODE_INV && !d_dist && !small_only && n <= XVCGPU_INV_ONE_LAUNCH_MAX &&
      ctx->inv_one_launch) {
    hipLaunchKernelGGL((residual_cu_kernel<MODE, false>), dim3(n), dim3(TX_THREADS), 0,
                       ctx->stream, o, p, r, d_blocks, n, d_levels, d_off, d_nnz,
                       ctx->d_tx_tables, ctx->d_tx_tables_t, xvcgpu_tx_layout(), nullptr, nullptr);
    return;
  }
  const int n_wg = (n + TX2_WAVES - 1) / TX2_WAVES;
  hipLaunchKernelGGL(residual_wave_kernel<MODE>, dim3((n_wg + 7) / 8 * 8),
                     dim3(64 * TX2_WAVES), 0, ctx->stream, o, p, r, d_blocks, n,
                     d_levels, d_off, d_nnz, ctx->d_tx_tables, ctx->d_tx_tables_t,
                     xvcgpu_tx_layout(), nullptr, nullptr, d_dist);
  // (the caller knows that every block is at most 16x16: the general-path kernel
  // would find nothing to do - and still be a launch on the picture's critical path)
  if (small_only) return;
  // general path: one workgroup per block (a workgroup whose block the wave
  // kernel took retires at once); only batches far beyond a picture's worth of a
  // decoder's dependency wave take the scanning form, whose few workgroups each
  // walk their share of the large blocks one after the other (it took 0.98 ms for
  // the ~2800 blocks - 500 of them 32x32 / 64x64 - of a 1080p B picture's first
  // wave: nearly all of that picture's 1.3 ms)
  if (n <= 65536)
    hipLaunchKernelGGL(residual_per_job_kernel<MODE>, dim3(n), dim3(TX_THREADS), 0, ctx->stream,
                       o, p, r, d_blocks, n, d_levels, d_off, d_nnz, ctx->d_tx_tables,
                       xvcgpu_tx_layout(), d_dist);
  else
    hipLaunchKernelGGL(residual_kernel<MODE>, dim3((n + TX_THREADS - 1) / TX_THREADS),
                       dim3(TX_THREADS), 0, ctx->stream, o, p, r, d_blocks, n, d_levels,
                       d_off, d_nnz, ctx->d_tx_tables, xvcgpu_tx_layout(), nullptr, nullptr,
                       d_dist);
}

// TransformAndReconstruct with the RDO quantiser for the blocks that ask for it
void launch_residual_rdoq(xvcgpu_ctx *ctx, const PicView &o, const PicView &p,
                          const PicView &r, const xvcgpu_tx_block *d_blocks, int n,
                          int16_t *d_levels, const uint32_t *d_off, int32_t *d_nnz,
                          const xvcgpu_rdoq_contexts *d_ctx, const xvcgpu_rdoq_params *d_prm,
                          const xvcgpu_block_pos *d_src_pos = nullptr,
                          const xvcgpu_eval_cand *d_ecands = nullptr, int n_head = 0,
                          uint64_t *d_eout = nullptr, int strength = 0) {
  // a CU state's evaluation: its few blocks as one launch, a workgroup each
  if (n <= 64) {
    hipLaunchKernelGGL((residual_cu_kernel<TX_MODE_FULL, true>), dim3(n + (d_ecands ? n_head : 0)),
                       dim3(TX_THREADS), 0,
                       ctx->stream, o, p, r, d_blocks, n, d_levels, d_off, d_nnz,
                       ctx->d_tx_tables, ctx->d_tx_tables_t, xvcgpu_tx_layout(), d_ctx, d_prm,
                       d_src_pos, d_ecands, n_head, d_eout, strength);
    return;
  }
  const int n_wg = (n + TX2_WAVES - 1) / TX2_WAVES;
  hipLaunchKernelGGL((residual_wave_kernel<TX_MODE_FULL, true>), dim3((n_wg + 7) / 8 * 8),
                     dim3(64 * TX2_WAVES), 0, ctx->stream, o, p, r, d_blocks, n,
                     d_levels, d_off, d_nnz, ctx->d_tx_tables, ctx->d_tx_tables_t,
                     xvcgpu_tx_layout(), d_ctx, d_prm);
  // the blocks beyond 16x16 (and the 2-wide ones): a workgroup each - the scanning
  // form runs the large blocks of its 256 descriptors one after the other, which a
  // batch of RD-search candidates (a third of them 32x32 / 64x64) turns into the
  // whole launch's duration
  if (n <= 262144)
    hipLaunchKernelGGL((residual_per_job_kernel<TX_MODE_FULL, true>), dim3(n), dim3(TX_THREADS),
                       0, ctx->stream, o, p, r, d_blocks, n, d_levels, d_off, d_nnz,
                       ctx->d_tx_tables, xvcgpu_tx_layout(), nullptr, d_ctx, d_prm);
  else
    hipLaunchKernelGGL((residual_kernel<TX_MODE_FULL, true>),
                       dim3((n + TX_THREADS - 1) / TX_THREADS), dim3(TX_THREADS), 0, ctx->stream,
                       o, p, r, d_blocks, n, d_levels, d_off, d_nnz, ctx->d_tx_tables,
                       xvcgpu_tx_layout(), d_ctx, d_prm);
}

// xvcgpu_frame_pass_multi: one kernel's argument block for n pictures,
// fill(picture, its context, its slot)
template <typename T, typename F>
MultiArgs<T> multi_args(xvcgpu_ctx *const *ctxs, const xvcgpu_frame_pass_args *const *args, int n,
                        F fill) {
  MultiArgs<T> m;
  for (int i = 0; i < n; i++) fill(args[i], ctxs[i], m.a[i]);
  return m;
}

// one wave per job, ME2_WAVES(MS) of them a workgroup: the workgroups padded to 8 (the XCDs)
dim3 me2_grid(int n, int waves, unsigned y = 1) {
  const int n_wg = (n + waves - 1) / waves;
  return dim3((n_wg + 7) / 8 * 8, y);
}
// the sub-pel team: one workgroup per job, padded likewise
dim3 me_team_grid(int n, unsigned y = 1) { return dim3((n + 7) / 8 * 8, y); }

// An instance of the search kernels: the class, the phases compiled in, LIC or not.
template <int MS_, int PH_, bool LIC_>
struct MeInst { static constexpr int MS = MS_, PH = PH_; static constexpr bool LIC = LIC_; };
// The launches of class MS for the phases PHASES, LIC or not, in order (the table of
// DESIGN.md section 8): wave(MeInst) per wave instance, team() for the four-wave team.
// - The 16 class runs both phases fused (measured faster than two launches: waves in the
//   latency-bound full-pel search overlap waves in the VALU-bound sub-pel search on the same
//   SIMD); a single-phase call gets an instance with only that phase's registers and LDS.
// - Every other class, and every LIC job, gets one launch per phase: the larger classes'
//   sub-pel instance holds 23 / 76 KB of LDS per wave (one workgroup per CU), and fused with
//   it the full-pel search runs at that occupancy too (32x32: 36 + 64 us apart, 120 us fused;
//   32x16: 38 + 112 vs 198; tools/time_me_classes.py).
// - The 64 class's jobs on the packed sub-pel path go to the team; its <64, SUBPEL> wave
//   instance leaves those alone.
template <int MS, int PHASES, bool LIC, class Wave, class Team>
void me_class_launches(Wave &&wave, Team &&team) {
  if constexpr (MS == 16 && !LIC && PHASES == 3) {
    wave(MeInst<16, 3, false>());
  } else {
    if constexpr ((PHASES & XVCGPU_ME_FULLPEL) != 0) wave(MeInst<MS, XVCGPU_ME_FULLPEL, LIC>());
    if constexpr ((PHASES & XVCGPU_ME_SUBPEL) != 0) {
      wave(MeInst<MS, XVCGPU_ME_SUBPEL, LIC>());
      if constexpr (MS == 64 && !LIC) team();
    }
  }
}
// (the class, then the phases too, as run-time values; another class: nothing)
template <int PHASES, bool LIC, class Wave, class Team>
void me_launches_of(int cls, Wave &&wave, Team &&team) {
  if (cls == 16) me_class_launches<16, PHASES, LIC>(wave, team);
  else if (cls == 32) me_class_launches<32, PHASES, LIC>(wave, team);
  else if (cls == 64) me_class_launches<64, PHASES, LIC>(wave, team);
}
template <bool LIC, class Wave, class Team>
void me_launches(int cls, int ph, Wave &&wave, Team &&team) {
  if (ph == 3) me_launches_of<3, LIC>(cls, wave, team);
  else if (ph == XVCGPU_ME_FULLPEL) me_launches_of<XVCGPU_ME_FULLPEL, LIC>(cls, wave, team);
  else if (ph == XVCGPU_ME_SUBPEL) me_launches_of<XVCGPU_ME_SUBPEL, LIC>(cls, wave, team);
}

// Is instance <ms, inst_ph, lic> (inst_ph 0: the team) among its class's launches for ph?
bool me_class_has(int ms, bool lic, int ph, int inst_ph) {
  bool has = false;
  auto wave = [&](auto inst) { has |= decltype(inst)::PH == inst_ph; };
  auto team = [&] { has |= inst_ph == 0; };
  if (lic) me_launches<true>(ms, ph, wave, team);
  else me_launches<false>(ms, ph, wave, team);
  return has;
}

// What one planned search hands to its launches, and a launch over slots [at, at + cnt)
struct MePlanCall {
  hipStream_t stream;
  PicView orig, ref;
  const xvcgpu_me_block *blocks;
  const int *order;
  xvcgpu_me_result *results;
  const TzCand *tz_pattern;
};
template <int MS, int PH, bool LIC, int FW = 0, int FH = 0>
void me_plan_launch(const MePlanCall &c, int at, int cnt, const Me2Sched &sched) {
  hipLaunchKernelGGL((me_plan_kernel<MS, PH, LIC, FW, FH>), me2_grid(cnt, ME2_WAVES(MS)),
                     dim3(64 * ME2_WAVES(MS)), 0, c.stream, c.orig, c.ref, c.blocks, c.order + at,
                     cnt, c.results, c.tz_pattern, sched);
}
void me_plan_launch_team(const MePlanCall &c, int at, int cnt, const Me2Sched &) {
  hipLaunchKernelGGL((me_plan_team_kernel<64, 4>), me_team_grid(cnt), dim3(256), 0, c.stream,
                     c.orig, c.ref, c.blocks, c.order + at, cnt, c.results);
}

}  // namespace

extern "C" {

const char *xvcgpu_version(void) { return "xvcgpu 0.1 gfx950"; }

xvcgpu_status xvcgpu_create(int device, xvcgpu_ctx **out) {
  if (!out) return XVCGPU_INVALID_ARGUMENT;
  *out = nullptr;
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0 || device < 0 ||
      device >= count)
    return XVCGPU_NO_DEVICE;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) != hipSuccess) return XVCGPU_NO_DEVICE;
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) return XVCGPU_NO_DEVICE;
  xvcgpu_ctx *ctx = new (std::nothrow) xvcgpu_ctx();
  if (!ctx) return XVCGPU_OUT_OF_MEMORY;
  ctx->device = device;
  ctx->stream = nullptr;
  ctx->hi_stream = nullptr;
  ctx->copy_stream = nullptr;
  ctx->own_stream = false;
  ctx->d_tx_tables = nullptr;
  ctx->d_tx_tables_t = nullptr;
  ctx->d_tz_pattern = nullptr;
  ctx->d_ssd_part = nullptr;
  ctx->d_tail_part = nullptr;
  ctx->tail_cap = 0;
  ctx->ssd_part_cap = 0;
  ctx->d_stats = nullptr;
  ctx->stats_rows_cap = 0;
  ctx->d_rdoq_lists = nullptr;
  ctx->rdoq_lists_cap = 0;
  ctx->d_crc_tables = nullptr;
  ctx->d_intra_done = nullptr;
  ctx->intra_done_cap = 0;
  ctx->intra_waves_grid = 0;
  ctx->rdoq_four_lane_only = 0;
  ctx->h_rdoq_misuse = nullptr;
  ctx->h_seg_ring = nullptr;
  ctx->seg_ring_pos = 0;
  ctx->seg_ring_half = 0;
  ctx->seg_ring_ev[0] = ctx->seg_ring_ev[1] = nullptr;
  ctx->seg_ring_used[0] = ctx->seg_ring_used[1] = false;
  {
    ctx->rdoq_qp_hint = -1;
    ctx->rdoq_classified_proved = false;
    const char *e = getenv("XVCGPU_PROVE_ZERO");   // 0 / 1; default: by batch size
    ctx->rdoq_prove_zero = (e && (e[0] == '0' || e[0] == '1') && !e[1]) ? e[0] - '0' : -1;
    ctx->rdoq_list_form = -1;
    ctx->rdoq_last_n = 0;
  }
  for (int i = 0; i < 64; i++) ctx->ev_pool[i] = nullptr;
  ctx->d_me_rot = nullptr;
  ctx->me_epoch = 0;
  {
    const char *e = getenv("XVCGPU_INV_ONE_LAUNCH");   // 0: the two-kernel form (comparisons)
    ctx->inv_one_launch = !(e && e[0] == '0' && !e[1]);
  }
  if (hipSetDevice(device) != hipSuccess ||
      hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) {
    delete ctx;
    return XVCGPU_DEVICE_ERROR;
  }
  ctx->own_stream = true;
  hipEventCreate(&ctx->ev0);
  hipEventCreate(&ctx->ev1);
  hipEventCreateWithFlags(&ctx->ev_sync, hipEventDisableTiming);
  const TxTableLayout &lay = xvcgpu_tx_layout();
  if (hipMalloc(&ctx->d_tx_tables, lay.total * sizeof(int16_t)) != hipSuccess ||
      hipMemcpy(ctx->d_tx_tables, xvcgpu_tx_host_tables(),
                lay.total * sizeof(int16_t), hipMemcpyHostToDevice) != hipSuccess ||
      hipMalloc(&ctx->d_tx_tables_t, lay.total * sizeof(int16_t)) != hipSuccess ||
      hipMemcpy(ctx->d_tx_tables_t, xvcgpu_tx_host_tables_t(),
                lay.total * sizeof(int16_t), hipMemcpyHostToDevice) != hipSuccess) {
    xvcgpu_destroy(ctx);
    return XVCGPU_OUT_OF_MEMORY;
  }
  if (hipMalloc(&ctx->d_me_rot, 3 * sizeof(Me2Rot)) != hipSuccess ||
      hipMemset(ctx->d_me_rot, 0x7f, 3 * sizeof(Me2Rot)) != hipSuccess) {
    xvcgpu_destroy(ctx);
    return XVCGPU_OUT_OF_MEMORY;
  }
  {
    uint32_t bits[128];
    if (hipMemcpyFromSymbol(bits, HIP_SYMBOL(kEntropyBits), sizeof(bits)) != hipSuccess ||
        hipMemcpyToSymbol(HIP_SYMBOL(gEntropyBits), bits, sizeof(bits)) != hipSuccess) {
      xvcgpu_destroy(ctx);
      return XVCGPU_DEVICE_ERROR;
    }
  }
  {
    TzCand pattern[TZ_MAX_CANDS];
    const int np = tz_pattern_build(pattern);
    if (np != TZ_MAX_CANDS ||
        hipMalloc(&ctx->d_tz_pattern, sizeof(pattern)) != hipSuccess ||
        hipMemcpy(ctx->d_tz_pattern, pattern, sizeof(pattern),
                  hipMemcpyHostToDevice) != hipSuccess) {
      xvcgpu_destroy(ctx);
      return XVCGPU_OUT_OF_MEMORY;
    }
  }
  // the flag the four-lane-only promise is checked with (xvcgpu_quant_rdo_set_four_lane_only):
  // allocated here, not on first use - that first use may sit inside a stream capture
  if (hipHostMalloc(reinterpret_cast<void **>(&ctx->h_rdoq_misuse), sizeof(int),
                    hipHostMallocMapped) != hipSuccess) {
    xvcgpu_destroy(ctx);
    return XVCGPU_OUT_OF_MEMORY;
  }
  *ctx->h_rdoq_misuse = 0;
  *out = ctx;
  return XVCGPU_OK;
}

void xvcgpu_destroy(xvcgpu_ctx *ctx) {
  if (!ctx) return;
  hipSetDevice(ctx->device);
  hipStreamSynchronize(ctx->stream);
  if (ctx->d_tx_tables) hipFree(ctx->d_tx_tables);
  if (ctx->d_tx_tables_t) hipFree(ctx->d_tx_tables_t);
  if (ctx->d_tz_pattern) hipFree(ctx->d_tz_pattern);
  if (ctx->d_ssd_part) hipFree(ctx->d_ssd_part);
  if (ctx->d_tail_part) hipFree(ctx->d_tail_part);
  if (ctx->d_stats) hipFree(ctx->d_stats);
  if (ctx->d_rdoq_lists) hipFree(ctx->d_rdoq_lists);
  if (ctx->h_rdoq_misuse) hipHostFree(ctx->h_rdoq_misuse);
  if (ctx->h_seg_ring) {
    hipHostFree(ctx->h_seg_ring);
    hipEventDestroy(ctx->seg_ring_ev[0]);
    hipEventDestroy(ctx->seg_ring_ev[1]);
  }
  if (ctx->d_crc_tables) hipFree(ctx->d_crc_tables);
  if (ctx->d_intra_done) hipFree(ctx->d_intra_done);
  if (ctx->d_me_rot) hipFree(ctx->d_me_rot);
  hipEventDestroy(ctx->ev0);
  hipEventDestroy(ctx->ev1);
  hipEventDestroy(ctx->ev_sync);
  if (ctx->copy_stream) hipStreamDestroy(ctx->copy_stream);
  if (ctx->hi_stream) {
    hipStreamDestroy(ctx->hi_stream);
    hipEventDestroy(ctx->ev_hi_in);
    hipEventDestroy(ctx->ev_hi_out);
  }
  for (int i = 0; i < 64; i++)
    if (ctx->ev_pool[i]) hipEventDestroy(ctx->ev_pool[i]);
  if (ctx->own_stream && ctx->stream) hipStreamDestroy(ctx->stream);
  delete ctx;
}

const char *xvcgpu_last_error(const xvcgpu_ctx *ctx) {
  return ctx ? ctx->err.c_str() : "null context";
}

xvcgpu_status xvcgpu_set_stream(xvcgpu_ctx *ctx, void *hip_stream) {
  if (!ctx) return XVCGPU_INVALID_ARGUMENT;
  if (ctx->own_stream && ctx->stream) {
    hipStreamSynchronize(ctx->stream);
    hipStreamDestroy(ctx->stream);
  }
  // NULL is a valid hipStream_t: the device's default stream
  ctx->stream = static_cast<hipStream_t>(hip_stream);
  ctx->own_stream = false;
  return XVCGPU_OK;
}

void *xvcgpu_get_stream(const xvcgpu_ctx *ctx) {
  return ctx ? static_cast<void *>(ctx->stream) : nullptr;
}

xvcgpu_status xvcgpu_use_own_stream(xvcgpu_ctx *ctx) {
  if (!ctx) return XVCGPU_INVALID_ARGUMENT;
  if (ctx->own_stream) return XVCGPU_OK;
  hipStreamSynchronize(ctx->stream);
  HIP_TRY(ctx, hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking));
  ctx->own_stream = true;
  return XVCGPU_OK;
}

xvcgpu_status xvcgpu_use_priority_stream(xvcgpu_ctx *ctx, int high) {
  if (!ctx) return XVCGPU_INVALID_ARGUMENT;
  int lo = 0, hi = 0;  // numerically lower = higher priority
  HIP_TRY(ctx, hipDeviceGetStreamPriorityRange(&lo, &hi));
  hipStreamSynchronize(ctx->stream);
  hipStream_t st = nullptr;
  HIP_TRY(ctx, hipStreamCreateWithPriority(&st, hipStreamNonBlocking, high ? hi : lo));
  if (ctx->own_stream && ctx->stream) hipStreamDestroy(ctx->stream);
  ctx->stream = st;
  ctx->own_stream = true;
  return XVCGPU_OK;
}

xvcgpu_status xvcgpu_set_short_kernel_priority(xvcgpu_ctx *ctx, int on) {
  if (!ctx) return XVCGPU_INVALID_ARGUMENT;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (!on) {
    if (ctx->hi_stream) {
      hipStreamSynchronize(ctx->hi_stream);
      hipStreamDestroy(ctx->hi_stream);
      hipEventDestroy(ctx->ev_hi_in);
      hipEventDestroy(ctx->ev_hi_out);
      ctx->hi_stream = nullptr;
    }
    return XVCGPU_OK;
  }
  if (ctx->hi_stream) return XVCGPU_OK;
  int lo = 0, hi = 0;  // numerically lower = higher priority
  HIP_TRY(ctx, hipDeviceGetStreamPriorityRange(&lo, &hi));
  HIP_TRY(ctx, hipStreamCreateWithPriority(&ctx->hi_stream, hipStreamNonBlocking, hi));
  HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->ev_hi_in, hipEventDisableTiming));
  HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->ev_hi_out, hipEventDisableTiming));
  return XVCGPU_OK;
}

xvcgpu_status xvcgpu_wait_for(xvcgpu_ctx *ctx, xvcgpu_ctx *other) {
  if (!ctx || !other) return XVCGPU_INVALID_ARGUMENT;
  if (ctx == other || ctx->stream == other->stream) return XVCGPU_OK;
  HIP_TRY(ctx, hipEventRecord(other->ev_sync, other->stream));
  HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, other->ev_sync, 0));
  return XVCGPU_OK;
}

// Every host-side wait ends here: a broken four-lane-only promise
// (xvcgpu_quant_rdo_set_four_lane_only) is reported by the first wait that follows the walk,
// whichever entry point it is.
xvcgpu_status xvcgpu_internal_after_wait(xvcgpu_ctx *ctx) {
  if (ctx && ctx->h_rdoq_misuse && *ctx->h_rdoq_misuse) {
    *ctx->h_rdoq_misuse = 0;
    return fail(ctx, XVCGPU_INVALID_ARGUMENT,
                "quant_rdo: a block outside the four-lane classes in a batch declared "
                "xvcgpu_quant_rdo_set_four_lane_only (its levels were not computed)");
  }
  return XVCGPU_OK;
}

xvcgpu_status xvcgpu_sync(xvcgpu_ctx *ctx) {
  if (!ctx) return XVCGPU_INVALID_ARGUMENT;
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return xvcgpu_internal_after_wait(ctx);
}

xvcgpu_status xvcgpu_timer_begin(xvcgpu_ctx *ctx) {
  if (!ctx) return XVCGPU_INVALID_ARGUMENT;
  HIP_TRY(ctx, hipEventRecord(ctx->ev0, ctx->stream));
  return XVCGPU_OK;
}

xvcgpu_status xvcgpu_timer_end(xvcgpu_ctx *ctx, float *elapsed_ms) {
  if (!ctx || !elapsed_ms) return XVCGPU_INVALID_ARGUMENT;
  HIP_TRY(ctx, hipEventRecord(ctx->ev1, ctx->stream));
  HIP_TRY(ctx, hipEventSynchronize(ctx->ev1));
  HIP_TRY(ctx, hipEventElapsedTime(elapsed_ms, ctx->ev0, ctx->ev1));
  return XVCGPU_OK;
}

xvcgpu_status xvcgpu_timer_mark(xvcgpu_ctx *ctx, int slot) {
  if (!ctx || slot < 0 || slot >= 64) return XVCGPU_INVALID_ARGUMENT;
  if (!ctx->ev_pool[slot]) HIP_TRY(ctx, hipEventCreate(&ctx->ev_pool[slot]));
  HIP_TRY(ctx, hipEventRecord(ctx->ev_pool[slot], ctx->stream));
  return XVCGPU_OK;
}

xvcgpu_status xvcgpu_timer_between(xvcgpu_ctx *ctx, int slot_a, int slot_b,
                                   float *elapsed_ms) {
  if (!ctx || !elapsed_ms || slot_a < 0 || slot_a >= 64 || slot_b < 0 || slot_b >= 64 ||
      !ctx->ev_pool[slot_a] || !ctx->ev_pool[slot_b])
    return XVCGPU_INVALID_ARGUMENT;
  HIP_TRY(ctx, hipEventSynchronize(ctx->ev_pool[slot_b]));
  HIP_TRY(ctx, hipEventElapsedTime(elapsed_ms, ctx->ev_pool[slot_a], ctx->ev_pool[slot_b]));
  return XVCGPU_OK;
}

struct xvcgpu_recording {
  hipGraph_t graph;
  hipGraphExec_t exec;
};

xvcgpu_status xvcgpu_record_begin(xvcgpu_ctx *ctx) {
  if (!ctx) return XVCGPU_INVALID_ARGUMENT;
  if (!ctx->own_stream)
    return fail(ctx, XVCGPU_UNSUPPORTED, "recording needs the private stream");
  HIP_TRY(ctx, hipStreamBeginCapture(ctx->stream, hipStreamCaptureModeThreadLocal));
  return XVCGPU_OK;
}

xvcgpu_status xvcgpu_record_end(xvcgpu_ctx *ctx, xvcgpu_recording **out) {
  if (!ctx || !out) return XVCGPU_INVALID_ARGUMENT;
  *out = nullptr;
  hipGraph_t graph = nullptr;
  HIP_TRY(ctx, hipStreamEndCapture(ctx->stream, &graph));
  hipGraphExec_t exec = nullptr;
  hipError_t e = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
  if (e != hipSuccess) {
    hipGraphDestroy(graph);
    return fail(ctx, XVCGPU_DEVICE_ERROR, "hipGraphInstantiate", e);
  }
  xvcgpu_recording *r = new (std::nothrow) xvcgpu_recording();
  if (!r) {
    hipGraphExecDestroy(exec);
    hipGraphDestroy(graph);
    return XVCGPU_OUT_OF_MEMORY;
  }
  r->graph = graph;
  r->exec = exec;
  *out = r;
  return XVCGPU_OK;
}

xvcgpu_status xvcgpu_replay(xvcgpu_ctx *ctx, xvcgpu_recording *rec) {
  if (!ctx || !rec) return XVCGPU_INVALID_ARGUMENT;
  HIP_TRY(ctx, hipGraphLaunch(rec->exec, ctx->stream));
  return XVCGPU_OK;
}

void xvcgpu_recording_destroy(xvcgpu_recording *rec) {
  if (!rec) return;
  hipGraphExecDestroy(rec->exec);
  hipGraphDestroy(rec->graph);
  delete rec;
}

xvcgpu_status xvcgpu_malloc(xvcgpu_ctx *ctx, size_t bytes, void **dev_ptr) {
  if (!ctx || !dev_ptr) return XVCGPU_INVALID_ARGUMENT;
  hipSetDevice(ctx->device);
  hipError_t e = hipMalloc(dev_ptr, bytes ? bytes : 1);
  if (e != hipSuccess) return fail(ctx, XVCGPU_OUT_OF_MEMORY, "hipMalloc", e);
  return XVCGPU_OK;
}

xvcgpu_status xvcgpu_free(xvcgpu_ctx *ctx, void *dev_ptr) {
  if (!ctx) return XVCGPU_INVALID_ARGUMENT;
  if (dev_ptr) {
    hipStreamSynchronize(ctx->stream);
    HIP_TRY(ctx, hipFree(dev_ptr));
  }
  return XVCGPU_OK;
}

xvcgpu_status xvcgpu_memcpy_h2d(xvcgpu_ctx *ctx, void *dst, const void *src,
                                size_t bytes) {
  if (!ctx || (!dst && bytes) || (!src && bytes)) return XVCGPU_INVALID_ARGUMENT;
  if (!bytes) return XVCGPU_OK;
  HIP_TRY(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return XVCGPU_OK;
}

xvcgpu_status xvcgpu_host_alloc(xvcgpu_ctx *ctx, size_t bytes, void **host_ptr) {
  if (!ctx || !host_ptr || !bytes) return XVCGPU_INVALID_ARGUMENT;
  *host_ptr = nullptr;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (hipHostMalloc(host_ptr, bytes, hipHostMallocDefault) != hipSuccess) {
    (void)hipGetLastError();
    *host_ptr = nullptr;
    return XVCGPU_OUT_OF_MEMORY;
  }
  return XVCGPU_OK;
}

xvcgpu_status xvcgpu_host_free(xvcgpu_ctx *ctx, void *host_ptr) {
  if (!ctx) return XVCGPU_INVALID_ARGUMENT;
  if (host_ptr) HIP_TRY(ctx, hipHostFree(host_ptr));
  return XVCGPU_OK;
}

xvcgpu_status xvcgpu_memcpy_h2d_async(xvcgpu_ctx *ctx, void *dst, const void *src,
                                      size_t bytes) {
  if (!ctx || (!dst && bytes) || (!src && bytes)) return XVCGPU_INVALID_ARGUMENT;
  if (!bytes) return XVCGPU_OK;
  HIP_TRY(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, ctx->stream));
  return XVCGPU_OK;
}

xvcgpu_status xvcgpu_memcpy_d2h_async(xvcgpu_ctx *ctx, void *dst, const void *src,
                                      size_t bytes) {
  if (!ctx || (!dst && bytes) || (!src && bytes)) return XVCGPU_INVALID_ARGUMENT;
  if (!bytes) return XVCGPU_OK;
  HIP_TRY(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream));
  return XVCGPU_OK;
}

xvcgpu_status xvcgpu_memcpy_d2h(xvcgpu_ctx *ctx, void *dst, const void *src,
                                size_t bytes) {
  if (!ctx || (!dst && bytes) || (!src && bytes)) return XVCGPU_INVALID_ARGUMENT;
  if (!bytes) return XVCGPU_OK;
  HIP_TRY(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return xvcgpu_internal_after_wait(ctx);
}

xvcgpu_status xvcgpu_memset(xvcgpu_ctx *ctx, void *dst, int value, size_t bytes) {
  if (!ctx || (!dst && bytes)) return XVCGPU_INVALID_ARGUMENT;
  if (!bytes) return XVCGPU_OK;
  HIP_TRY(ctx, hipMemsetAsync(dst, value, bytes, ctx->stream));
  return XVCGPU_OK;
}

static xvcgpu_status ensure_ssd_part(xvcgpu_ctx *ctx, int items);
static xvcgpu_status ensure_stats(xvcgpu_ctx *ctx, int rows);
static xvcgpu_status ensure_tail(xvcgpu_ctx *ctx, int tiles);

/* ---- pictures ---- */
size_t xvcgpu_picture_bytes(int width, int height) {
  if (!valid_size(width, height, 8)) return 0;
  return geometry(width, height).bytes;
}

xvcgpu_status xvcgpu_picture_wrap(xvcgpu_ctx *ctx, int width, int height,
                                  int bitdepth, void *dev_mem, size_t bytes,
                                  xvcgpu_picture **out) {
  if (!ctx || !out) return XVCGPU_INVALID_ARGUMENT;
  *out = nullptr;
  if (!valid_size(width, height, bitdepth))
    return fail(ctx, XVCGPU_INVALID_ARGUMENT, "picture size/bitdepth");
  if (!dev_mem || bytes < geometry(width, height).bytes ||
      (reinterpret_cast<uintptr_t>(dev_mem) & 255))
    return fail(ctx, XVCGPU_INVALID_ARGUMENT, "picture memory");
  xvcgpu_picture *p = new (std::nothrow) xvcgpu_picture();
  if (!p) return XVCGPU_OUT_OF_MEMORY;
  p->ctx = ctx;
  p->w = width;
  p->h = height;
  p->bd = bitdepth;
  p->base = dev_mem;
  p->bytes = bytes;
  p->own = false;
  init_views(p);
  xvcgpu_status st = ensure_ssd_part(ctx, ssd_items(width, height));
  if (st == XVCGPU_OK) st = ensure_stats(ctx, 2 * height);
  if (st == XVCGPU_OK) st = ensure_tail(ctx, tail_tiles(width, height));
  if (st != XVCGPU_OK) {
    delete p;
    return st;
  }
  *out = p;
  return XVCGPU_OK;
}

xvcgpu_status xvcgpu_picture_create(xvcgpu_ctx *ctx, int width, int height,
                                    int bitdepth, xvcgpu_picture **out) {
  if (!ctx || !out) return XVCGPU_INVALID_ARGUMENT;
  *out = nullptr;
  if (!valid_size(width, height, bitdepth))
    return fail(ctx, XVCGPU_INVALID_ARGUMENT, "picture size/bitdepth");
  const size_t bytes = geometry(width, height).bytes;
  void *mem = nullptr;
  xvcgpu_status st = xvcgpu_malloc(ctx, bytes, &mem);
  if (st != XVCGPU_OK) return st;
  hipMemsetAsync(mem, 0, bytes, ctx->stream);
  st = xvcgpu_picture_wrap(ctx, width, height, bitdepth, mem, bytes, out);
  if (st != XVCGPU_OK) {
    hipFree(mem);
    return st;
  }
  (*out)->own = true;
  return XVCGPU_OK;
}

void xvcgpu_picture_destroy(xvcgpu_picture *pic) {
  if (!pic) return;
  if (pic->own && pic->base) {
    hipStreamSynchronize(pic->ctx->stream);
    hipFree(pic->base);
  }
  delete pic;
}

static xvcgpu_status transfer(const xvcgpu_picture *pic,
                              const uint16_t *const planes[3],
                              const ptrdiff_t strides[3], int border_luma,
                              bool upload) {
  if (!pic || !planes || !strides) return XVCGPU_INVALID_ARGUMENT;
  xvcgpu_ctx *ctx = pic->ctx;
  if (border_luma < 0 || border_luma > XVCGPU_BORDER_LUMA || (border_luma & 1))
    return fail(ctx, XVCGPU_INVALID_ARGUMENT, "border");
  for (int c = 0; c < 3; c++) {
    if (!planes[c]) continue;
    const PlaneView &v = pic->v.c[c];
    const int b = c ? border_luma / 2 : border_luma;
    uint16_t *dev = v.p - (ptrdiff_t)b * v.stride - b;
    // host pointer addresses sample (0,0); step back to the border start
    uint16_t *host = const_cast<uint16_t *>(planes[c]) - (ptrdiff_t)b * strides[c] - b;
    const size_t wbytes = (size_t)(v.w + 2 * b) * sizeof(uint16_t);
    const size_t rows = v.h + 2 * b;
    hipError_t e;
    if (upload)
      e = hipMemcpy2DAsync(dev, (size_t)v.stride * 2, host, (size_t)strides[c] * 2,
                           wbytes, rows, hipMemcpyHostToDevice, ctx->stream);
    else
      e = hipMemcpy2DAsync(host, (size_t)strides[c] * 2, dev, (size_t)v.stride * 2,
                           wbytes, rows, hipMemcpyDeviceToHost, ctx->stream);
    if (e != hipSuccess) return fail(ctx, XVCGPU_DEVICE_ERROR, "hipMemcpy2DAsync", e);
  }
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  return XVCGPU_OK;
}

xvcgpu_status xvcgpu_picture_upload(xvcgpu_picture *pic,
                                    const uint16_t *const planes[3],
                                    const ptrdiff_t strides[3]) {
  return transfer(pic, planes, strides, 0, true);
}
xvcgpu_status xvcgpu_picture_download(const xvcgpu_picture *pic,
                                      uint16_t *const planes[3],
                                      const ptrdiff_t strides[3]) {
  return transfer(pic, const_cast<const uint16_t *const *>(planes), strides, 0, false);
}
xvcgpu_status xvcgpu_picture_upload_padded(xvcgpu_picture *pic,
                                           const uint16_t *const planes[3],
                                           const ptrdiff_t strides[3],
                                           int border_luma) {
  return transfer(pic, planes, strides, border_luma, true);
}
xvcgpu_status xvcgpu_picture_download_padded(const xvcgpu_picture *pic,
                                             uint16_t *const planes[3],
                                             const ptrdiff_t strides[3],
                                             int border_luma) {
  return transfer(pic, const_cast<const uint16_t *const *>(planes), strides,
                  border_luma, false);
}

xvcgpu_status xvcgpu_picture_plane(const xvcgpu_picture *pic, int comp,
                                   void **dev_ptr, ptrdiff_t *stride) {
  if (!pic || comp < 0 || comp > 2 || !dev_ptr || !stride)
    return XVCGPU_INVALID_ARGUMENT;
  *dev_ptr = pic->v.c[comp].p;
  *stride = pic->v.c[comp].stride;
  return XVCGPU_OK;
}

xvcgpu_status xvcgpu_picture_copy(xvcgpu_ctx *ctx, xvcgpu_picture *dst,
                                  const xvcgpu_picture *src) {
  if (!ctx || !dst || !src) return XVCGPU_INVALID_ARGUMENT;
  if (dst->w != src->w || dst->h != src->h)
    return fail(ctx, XVCGPU_INVALID_ARGUMENT, "picture size mismatch");
  HIP_TRY(ctx, hipMemcpyAsync(dst->base, src->base, geometry(src->w, src->h).bytes,
                              hipMemcpyDeviceToDevice, ctx->stream));
  return XVCGPU_OK;
}

/* ---- kernels ---- */
xvcgpu_status xvcgpu_pad_border(xvcgpu_ctx *ctx, xvcgpu_picture *pic) {
  if (!ctx || !pic) return XVCGPU_INVALID_ARGUMENT;
  hipLaunchKernelGGL(pad_border_kernel, dim3(pic->h + 2 * XVCGPU_BORDER_LUMA, 3),
                     dim3(128), 0, ctx->stream, pic->v);
  CHECK_LAUNCH(ctx, "pad_border");
  return XVCGPU_OK;
}

xvcgpu_status xvcgpu_metric_batch(xvcgpu_ctx *ctx, const xvcgpu_picture *a,
                                  const xvcgpu_picture *b, int comp,
                                  double weight, int structural_strength,
                                  const xvcgpu_metric_cand *d_cands, int n,
                                  uint64_t *d_out) {
  if (!ctx || !a || !b || comp < 0 || comp > 2 || n < 0 || (n && (!d_cands || !d_out)))
    return XVCGPU_INVALID_ARGUMENT;
  if (n == 0) return XVCGPU_OK;
  hipLaunchKernelGGL(metric_batch_kernel, dim3((n + 3) / 4), dim3(256), 0,
                     ctx->stream, a->v.c[comp], b->v.c[comp], a->bd, weight,
                     structural_strength, d_cands, n, d_out);
  CHECK_LAUNCH(ctx, "metric_batch");
  return XVCGPU_OK;
}

xvcgpu_status xvcgpu_mc_metric_batch(xvcgpu_ctx *ctx, const xvcgpu_picture *orig,
                                     const xvcgpu_picture *ref,
                                     int structural_strength,
                                     const xvcgpu_mc_metric_cand *d_cands, int n,
                                     uint64_t *d_out) {
  if (!ctx || !orig || !ref || n < 0 || (n && (!d_cands || !d_out)))
    return XVCGPU_INVALID_ARGUMENT;
  if (orig->w != ref->w || orig->h != ref->h || orig->bd != ref->bd)
    return fail(ctx, XVCGPU_INVALID_ARGUMENT, "picture mismatch");
  if (n == 0) return XVCGPU_OK;
  hipLaunchKernelGGL(mc_metric_kernel, dim3((n + 1) / 2), dim3(128), 0, ctx->stream,
                     orig->v.c[0], ref->v.c[0], orig->bd, structural_strength, d_cands,
                     n, d_out);
  CHECK_LAUNCH(ctx, "mc_metric_batch");
  return XVCGPU_OK;
}

// the search's block class: the smallest of 16 / 32 / 64 that holds max_block_size
static int me_class_of(int max_block_size) {
  return max_block_size > 32 ? 64 : (max_block_size > 16 ? 32 : 16);
}

// A context's next full-pel search rotates its three straggler-first records (k_me2.h).
// The epoch only matters modulo 3 and is kept there: no overflow, slot indices always 0..2
static Me2Sched me_sched_next(xvcgpu_ctx *ctx) {
  const int e = ctx->me_epoch = (ctx->me_epoch + 1) % 3;
  return Me2Sched{ctx->d_me_rot + e, ctx->d_me_rot + (e + 1) % 3, ctx->d_me_rot + (e + 2) % 3};
}

xvcgpu_status xvcgpu_me_search_sized(xvcgpu_ctx *ctx, const xvcgpu_picture *orig,
                                     const xvcgpu_picture *ref, int flags,
                                     const xvcgpu_me_block *d_blocks, int n,
                                     xvcgpu_me_result *d_results,
                                     int max_block_size) {
  if (!ctx || !orig || !ref || n < 0 || (n && (!d_blocks || !d_results)) ||
      !(flags & (XVCGPU_ME_FULLPEL | XVCGPU_ME_SUBPEL)) || max_block_size < 4 ||
      max_block_size > 64)
    return XVCGPU_INVALID_ARGUMENT;
  if (orig->w != ref->w || orig->h != ref->h || orig->bd != ref->bd)
    return fail(ctx, XVCGPU_INVALID_ARGUMENT, "picture mismatch");
  if (n == 0) return XVCGPU_OK;
  // every class kernel runs over the whole list and skips the jobs of the other classes
  Me2Sched sched = {nullptr, nullptr, nullptr};
  if (flags & XVCGPU_ME_FULLPEL) sched = me_sched_next(ctx);
  const int ml = me_class_of(max_block_size), ph = flags & 3;
  const bool lic_jobs = (flags & XVCGPU_ME_LIC_JOBS) != 0;
  // The sized form's own: the fused 16-class launch as the exact-shape kernel plus the
  // leftover kernel (XVCGPU_ME_HINT_SQ16), or the exact-shape kernel alone
  // (XVCGPU_ME_ONLY_SQ16 - the caller's word only counts where it can be kept: both
  // phases, the 16 class alone).
  const bool sq16 = (flags & (XVCGPU_ME_HINT_SQ16 | XVCGPU_ME_ONLY_SQ16)) != 0;
  const bool only_sq16 = (flags & XVCGPU_ME_ONLY_SQ16) && ph == 3 && max_block_size <= 16;
  auto wave = [&](auto inst) {
    typedef decltype(inst) I;
    const dim3 grid = me2_grid(n, ME2_WAVES(I::MS)), block(64 * ME2_WAVES(I::MS));
    if constexpr (I::MS == 16 && I::PH == 3 && !I::LIC) {
      if (sq16) {
        hipLaunchKernelGGL(me_search_sq16_kernel, grid, block, 0, ctx->stream, orig->v, ref->v,
                           d_blocks, n, d_results, ctx->d_tz_pattern, sched, ml, lic_jobs,
                           only_sq16);
        if (!only_sq16)
          hipLaunchKernelGGL(me_search_leftover_kernel, dim3((n + 63) / 64), dim3(64), 0,
                             ctx->stream, orig->v, ref->v, d_blocks, n, d_results,
                             ctx->d_tz_pattern, ml, lic_jobs);
        return;
      }
    }
    hipLaunchKernelGGL((me_search_wave_kernel<I::MS, I::PH, I::LIC>), grid, block, 0,
                       ctx->stream, orig->v, ref->v, d_blocks, n, d_results, ctx->d_tz_pattern,
                       sched, ml, lic_jobs);
  };
  auto team = [&] {
    hipLaunchKernelGGL((me_subpel_team_kernel<64, 4>), me_team_grid(n), dim3(256), 0,
                       ctx->stream, orig->v, ref->v, d_blocks, n, d_results);
  };
  for (int cls = 16; cls <= ml; cls *= 2) me_launches<false>(cls, ph, wave, team);
  // jobs of CUs that try local illumination compensation (XVC_ME_USE_LIC): their own instances
  for (int cls = 16; lic_jobs && cls <= ml; cls *= 2) me_launches<true>(cls, ph, wave, team);
  CHECK_LAUNCH(ctx, "me_search");
  return XVCGPU_OK;
}

#ifdef XVCGPU_TRACE
// developer build only (tools/trace_me.py): copy out the ME phase timestamps
xvcgpu_status xvcgpu_debug_me_trace(unsigned long long *out, int n_jobs) {
  hipDeviceSynchronize();
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_me2_trace),
                             sizeof(unsigned long long) * 24 * (size_t)n_jobs) == hipSuccess
             ? XVCGPU_OK
             : XVCGPU_DEVICE_ERROR;
}
#endif

#ifdef XVCGPU_TRACE
// developer build only (tools/trace_rdoq.py): the walk's section clock readings
xvcgpu_status xvcgpu_debug_rdoq_trace(unsigned long long *out, int n_rows) {
  hipDeviceSynchronize();
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_rq_trace),
                             sizeof(unsigned long long) * 16 * (size_t)n_rows) == hipSuccess
             ? XVCGPU_OK
             : XVCGPU_DEVICE_ERROR;
}
#endif

// tests: the class lists the context's last quantiser call built (list c at lists + c * cap)
xvcgpu_status xvcgpu_debug_rdoq_lists(xvcgpu_ctx *ctx, int32_t counts[3], int32_t *lists,
                                      int cap) {
  if (!ctx || !counts || !lists || cap < 0) return XVCGPU_INVALID_ARGUMENT;
  counts[0] = counts[1] = counts[2] = 0;
  if (!ctx->d_rdoq_lists || !ctx->rdoq_last_n) return XVCGPU_OK;
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  const RdoqLists l = rdoq_lists_of(ctx);
  HIP_TRY(ctx, hipMemcpy(counts, l.count, 3 * sizeof(int32_t), hipMemcpyDeviceToHost));
  for (int c = 0; c < 3; c++) {
    if (counts[c] < 0 || counts[c] > ctx->rdoq_last_n)
      return fail(ctx, XVCGPU_DEVICE_ERROR, "rdoq list count out of range");
    if (counts[c] > cap) return fail(ctx, XVCGPU_INVALID_ARGUMENT, "rdoq lists: cap too small");
    if (counts[c])
      HIP_TRY(ctx, hipMemcpy(lists + (size_t)c * cap, l.list[c], counts[c] * sizeof(int32_t),
                             hipMemcpyDeviceToHost));
  }
  return XVCGPU_OK;
}

xvcgpu_status xvcgpu_me_search(xvcgpu_ctx *ctx, const xvcgpu_picture *orig,
                               const xvcgpu_picture *ref, int flags,
                               const xvcgpu_me_block *d_blocks, int n,
                               xvcgpu_me_result *d_results) {
  return xvcgpu_me_search_sized(ctx, orig, ref, flags, d_blocks, n, d_results, 64);
}

/* ---- the search through a plan (k_me_plan.h) ---- */
struct xvcgpu_me_plan {
  const xvcgpu_me_block *d_blocks;
  int n, max_launched;
  int *d_order;    // n job indices, bin after bin, list order inside a bin
  int *d_offsets;  // XVCGPU_ME_PLAN_BINS + 2 (device copy of `first`)
  // first slot of every bin, n, and the number of jobs with a side below 8
  int first[XVCGPU_ME_PLAN_BINS + 2];
  int n_small() const { return first[XVCGPU_ME_PLAN_BINS + 1]; }
};

xvcgpu_status xvcgpu_me_plan_create(xvcgpu_ctx *ctx, const xvcgpu_me_block *d_blocks, int n,
                                    int max_block_size, xvcgpu_me_plan **out) {
  if (!ctx || !out || n < 0 || (n && !d_blocks) || max_block_size < 4 || max_block_size > 64)
    return XVCGPU_INVALID_ARGUMENT;
  xvcgpu_me_plan *p = new (std::nothrow) xvcgpu_me_plan();
  if (!p) return fail(ctx, XVCGPU_OUT_OF_MEMORY, "me_plan");
  p->d_blocks = d_blocks;
  p->n = n;
  p->max_launched = me_class_of(max_block_size);
  if (n > 0) {
    hipError_t e = hipMalloc(&p->d_order, sizeof(int) * (size_t)n);
    if (e == hipSuccess) e = hipMalloc(&p->d_offsets, sizeof(int) * (XVCGPU_ME_PLAN_BINS + 2));
    if (e == hipSuccess) {
      hipLaunchKernelGGL(me_plan_kernel_build, dim3(1), dim3(ME_PLAN_THREADS), 0, ctx->stream,
                         d_blocks, n, p->max_launched, p->d_order, p->d_offsets);
      e = hipGetLastError();
    }
    if (e == hipSuccess)
      e = hipMemcpyAsync(p->first, p->d_offsets, sizeof(p->first), hipMemcpyDeviceToHost,
                         ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess || p->first[XVCGPU_ME_PLAN_BINS] != n) {
      hipFree(p->d_order);
      hipFree(p->d_offsets);
      delete p;
      return fail(ctx, e == hipErrorOutOfMemory ? XVCGPU_OUT_OF_MEMORY : XVCGPU_DEVICE_ERROR,
                  "me_plan_create", e);
    }
  }
  *out = p;
  return XVCGPU_OK;
}

xvcgpu_status xvcgpu_me_plan_counts(const xvcgpu_me_plan *plan,
                                    int32_t counts[XVCGPU_ME_PLAN_BINS]) {
  if (!plan || !counts) return XVCGPU_INVALID_ARGUMENT;
  for (int k = 0; k < XVCGPU_ME_PLAN_BINS; k++) counts[k] = plan->first[k + 1] - plan->first[k];
  return XVCGPU_OK;
}

void xvcgpu_me_plan_destroy(xvcgpu_ctx *ctx, xvcgpu_me_plan *plan) {
  (void)ctx;
  if (!plan) return;
  if (plan->d_order) hipFree(plan->d_order);
  if (plan->d_offsets) hipFree(plan->d_offsets);
  delete plan;
}

// The planned search's launches, in launch order: one row per (bins, instance).  A row runs
// where me_class_launches has its instance among the class's launches for the asked
// phases - the exact-shape rows with the fused call only, the whole 16 class through the
// any-size instance with a single phase -, its depth condition holds and its bins have jobs.
struct MePlanRow {
  int first, end;   // the bins [first, end)
  int ms, ph;       // the instance: class, phases (3 fused, 1 full-pel, 2 sub-pel; 0: the team)
  bool lic;
  int depth;        // 0: any bit depth; 1: up to 10 bit (me2_subpel_fast); -1: above
  void (*launch)(const MePlanCall &c, int at, int cnt, const Me2Sched &sched);
};
static const MePlanRow kMePlanRows[] = {
    {XVCGPU_ME_PLAN_16X16, XVCGPU_ME_PLAN_16X8, 16, 3, false, 0, me_plan_launch<16, 3, false, 16, 16>},
    {XVCGPU_ME_PLAN_16X8, XVCGPU_ME_PLAN_8X8, 16, 3, false, 0, me_plan_launch<16, 3, false, 16, 8>},
    {XVCGPU_ME_PLAN_8X8, XVCGPU_ME_PLAN_OTHER16, 16, 3, false, 0, me_plan_launch<16, 3, false, 8, 8>},
    {XVCGPU_ME_PLAN_OTHER16, XVCGPU_ME_PLAN_C32, 16, 3, false, 0, me_plan_launch<16, 3, false>},
    {XVCGPU_ME_PLAN_16X16, XVCGPU_ME_PLAN_C32, 16, 1, false, 0, me_plan_launch<16, 1, false>},
    {XVCGPU_ME_PLAN_16X16, XVCGPU_ME_PLAN_C32, 16, 2, false, 0, me_plan_launch<16, 2, false>},
    {XVCGPU_ME_PLAN_C32, XVCGPU_ME_PLAN_C64_TEAM, 32, 1, false, 0, me_plan_launch<32, 1, false>},
    {XVCGPU_ME_PLAN_C32, XVCGPU_ME_PLAN_C64_TEAM, 32, 2, false, 0, me_plan_launch<32, 2, false>},
    {XVCGPU_ME_PLAN_C64_TEAM, XVCGPU_ME_PLAN_LIC16, 64, 1, false, 0, me_plan_launch<64, 1, false>},
    {XVCGPU_ME_PLAN_C64_TEAM, XVCGPU_ME_PLAN_LIC16, 64, 2, false, -1, me_plan_launch<64, 2, false>},
    {XVCGPU_ME_PLAN_C64_WAVE, XVCGPU_ME_PLAN_LIC16, 64, 2, false, 1, me_plan_launch<64, 2, false>},
    {XVCGPU_ME_PLAN_C64_TEAM, XVCGPU_ME_PLAN_C64_WAVE, 64, 0, false, 1, me_plan_launch_team},
    {XVCGPU_ME_PLAN_LIC16, XVCGPU_ME_PLAN_LIC32, 16, 1, true, 0, me_plan_launch<16, 1, true>},
    {XVCGPU_ME_PLAN_LIC16, XVCGPU_ME_PLAN_LIC32, 16, 2, true, 0, me_plan_launch<16, 2, true>},
    {XVCGPU_ME_PLAN_LIC32, XVCGPU_ME_PLAN_LIC64, 32, 1, true, 0, me_plan_launch<32, 1, true>},
    {XVCGPU_ME_PLAN_LIC32, XVCGPU_ME_PLAN_LIC64, 32, 2, true, 0, me_plan_launch<32, 2, true>},
    {XVCGPU_ME_PLAN_LIC64, XVCGPU_ME_PLAN_UNSUPPORTED, 64, 1, true, 0, me_plan_launch<64, 1, true>},
    {XVCGPU_ME_PLAN_LIC64, XVCGPU_ME_PLAN_UNSUPPORTED, 64, 2, true, 0, me_plan_launch<64, 2, true>},
};

xvcgpu_status xvcgpu_me_search_planned(xvcgpu_ctx *ctx, const xvcgpu_picture *orig,
                                       const xvcgpu_picture *ref, int flags,
                                       const xvcgpu_me_plan *plan,
                                       xvcgpu_me_result *d_results) {
  if (!ctx || !orig || !ref || !plan || (plan->n && !d_results) ||
      !(flags & (XVCGPU_ME_FULLPEL | XVCGPU_ME_SUBPEL)))
    return XVCGPU_INVALID_ARGUMENT;
  if (orig->w != ref->w || orig->h != ref->h || orig->bd != ref->bd)
    return fail(ctx, XVCGPU_INVALID_ARGUMENT, "picture mismatch");
  if (plan->n == 0) return XVCGPU_OK;
  Me2Sched sched = {nullptr, nullptr, nullptr};
  if (flags & XVCGPU_ME_FULLPEL) sched = me_sched_next(ctx);
  const int *first = plan->first;
  const int ph = flags & 3;
  const bool lic_jobs = (flags & XVCGPU_ME_LIC_JOBS) != 0;
  const MePlanCall call = {ctx->stream, orig->v, ref->v, plan->d_blocks, plan->d_order, d_results,
                           ctx->d_tz_pattern};
  // the jobs of every row in this search: 0 where it does not run or its bins are empty
  constexpr int kRows = sizeof(kMePlanRows) / sizeof(kMePlanRows[0]);
  int jobs[kRows];
  // The straggler-first record (k_me2.h) counts positions inside one launch's job list: it
  // is kept by ONE launch, the non-LIC full-pel row with the most jobs, from search to search
  // of the same plan; the other launches run in list order.  (No such row: nobody rotates
  // and nobody resets the third record - stale values are clamped by me2_rotated_wg.)
  int keeper = -1;
  for (int k = 0; k < kRows; k++) {
    const MePlanRow &r = kMePlanRows[k];
    const bool depth_ok = r.depth == 0 || (r.depth > 0) == (orig->bd <= 10);
    const bool runs = me_class_has(r.ms, r.lic, ph, r.ph) && depth_ok && (!r.lic || lic_jobs);
    jobs[k] = runs ? first[r.end] - first[r.first] : 0;
    if (!r.lic && (r.ph & XVCGPU_ME_FULLPEL) && jobs[k] > (keeper < 0 ? 0 : jobs[keeper]))
      keeper = k;
  }
  const Me2Sched none = {nullptr, nullptr, nullptr};
  for (int k = 0; k < kRows; k++)
    if (jobs[k] > 0)
      kMePlanRows[k].launch(call, first[kMePlanRows[k].first], jobs[k], k == keeper ? sched : none);
  // LIC jobs not announced: nobody takes them
  const int bad_from = lic_jobs ? XVCGPU_ME_PLAN_UNSUPPORTED : XVCGPU_ME_PLAN_LIC16;
  const int bad = first[XVCGPU_ME_PLAN_BINS] - first[bad_from];
  if (bad > 0)
    hipLaunchKernelGGL(me_plan_unsupported_kernel, dim3((bad + 255) / 256), dim3(256), 0,
                       ctx->stream, plan->d_order + first[bad_from], bad, d_results);
  CHECK_LAUNCH(ctx, "me_search_planned");
  return XVCGPU_OK;
}

xvcgpu_status xvcgpu_mc_batch(xvcgpu_ctx *ctx, const xvcgpu_picture *ref,
                              xvcgpu_picture *pred,
                              const xvcgpu_mc_block *d_blocks, int n) {
  if (!ctx || !ref || !pred || n < 0 || (n && !d_blocks))
    return XVCGPU_INVALID_ARGUMENT;
  if (pred->w != ref->w || pred->h != ref->h)
    return fail(ctx, XVCGPU_INVALID_ARGUMENT, "picture mismatch");
  if (n == 0) return XVCGPU_OK;
  hipLaunchKernelGGL(mc_batch_kernel, dim3(n), dim3(256), 0, ctx->stream, ref->v,
                     pred->v, d_blocks, n);
  CHECK_LAUNCH(ctx, "mc_batch");
  return XVCGPU_OK;
}

xvcgpu_status xvcgpu_mc_lic_batch(xvcgpu_ctx *ctx, const xvcgpu_picture *ref,
                                  const xvcgpu_picture *rec, xvcgpu_picture *pred,
                                  const xvcgpu_mc_lic_block *d_blocks, int n) {
  if (!ctx || !ref || !rec || !pred || n < 0 || (n && !d_blocks))
    return XVCGPU_INVALID_ARGUMENT;
  if (pred->w != ref->w || pred->h != ref->h || rec->w != ref->w || rec->h != ref->h ||
      rec->bd != ref->bd || pred->bd != ref->bd)
    return fail(ctx, XVCGPU_INVALID_ARGUMENT, "picture mismatch");
  if (n == 0) return XVCGPU_OK;
  hipLaunchKernelGGL(mc_lic_kernel, dim3(n), dim3(256), 0, ctx->stream, ref->v, rec->v,
                     pred->v, d_blocks, n);
  CHECK_LAUNCH(ctx, "mc_lic_batch");
  return XVCGPU_OK;
}

static xvcgpu_status inter_pred_launch(xvcgpu_ctx *ctx, const xvcgpu_picture *const *refs,
                                       int n_refs, const xvcgpu_picture *rec,
                                       xvcgpu_picture *pred, const xvcgpu_inter_block *d_blocks,
                                       const xvcgpu_block_pos *d_dst, int n) {
  if (!ctx || !refs || n_refs < 1 || n_refs > XVC_MAX_REF_SLOTS || !rec || !pred || n < 0 ||
      (n && !d_blocks))
    return XVCGPU_INVALID_ARGUMENT;
  // a scratch destination has its own size; the pictures of the sequence agree
  if (rec->bd != pred->bd || (!d_dst && (rec->w != pred->w || rec->h != pred->h)))
    return fail(ctx, XVCGPU_INVALID_ARGUMENT, "picture mismatch");
  RefTable t;
  memset(&t, 0, sizeof(t));
  for (int i = 0; i < n_refs; i++) {
    if (!refs[i]) return XVCGPU_INVALID_ARGUMENT;
    if (refs[i]->w != rec->w || refs[i]->h != rec->h || refs[i]->bd != rec->bd)
      return fail(ctx, XVCGPU_INVALID_ARGUMENT, "reference picture mismatch");
    t.pic[i] = refs[i]->v;
  }
  t.n = n_refs;
  if (n == 0) return XVCGPU_OK;
  hipLaunchKernelGGL(inter_pred_kernel, dim3(n), dim3(256), 0, ctx->stream, t, rec->v,
                     pred->v, d_blocks, n, d_dst, rec->w, rec->h);
  CHECK_LAUNCH(ctx, "inter_pred_batch");
  return XVCGPU_OK;
}

xvcgpu_status xvcgpu_inter_pred_batch(xvcgpu_ctx *ctx, const xvcgpu_picture *const *refs,
                                      int n_refs, const xvcgpu_picture *rec,
                                      xvcgpu_picture *pred,
                                      const xvcgpu_inter_block *d_blocks, int n) {
  return inter_pred_launch(ctx, refs, n_refs, rec, pred, d_blocks, nullptr, n);
}

xvcgpu_status xvcgpu_inter_pred_batch_to(xvcgpu_ctx *ctx, const xvcgpu_picture *const *refs,
                                         int n_refs, const xvcgpu_picture *rec,
                                         xvcgpu_picture *scratch,
                                         const xvcgpu_inter_block *d_blocks,
                                         const xvcgpu_block_pos *d_dst, int n) {
  if (n && !d_dst) return XVCGPU_INVALID_ARGUMENT;
  return inter_pred_launch(ctx, refs, n_refs, rec, scratch, d_blocks, d_dst, n);
}

xvcgpu_status xvcgpu_copy_blocks(xvcgpu_ctx *ctx, const xvcgpu_picture *src,
                                 xvcgpu_picture *dst, const xvcgpu_copy_block *d_blocks,
                                 int n) {
  if (!ctx || !src || !dst || n < 0 || (n && !d_blocks)) return XVCGPU_INVALID_ARGUMENT;
  if (src->bd != dst->bd) return fail(ctx, XVCGPU_INVALID_ARGUMENT, "picture mismatch");
  if (n == 0) return XVCGPU_OK;
  hipLaunchKernelGGL(copy_blocks_kernel, dim3((n + 3) / 4), dim3(256), 0, ctx->stream, src->v,
                     dst->v, d_blocks, n);
  CHECK_LAUNCH(ctx, "copy_blocks");
  return XVCGPU_OK;
}

xvcgpu_status xvcgpu_mc_affine_batch(xvcgpu_ctx *ctx, const xvcgpu_picture *ref,
                                     xvcgpu_picture *pred,
                                     const xvcgpu_mc_affine_block *d_blocks, int n) {
  if (!ctx || !ref || !pred || n < 0 || (n && !d_blocks)) return XVCGPU_INVALID_ARGUMENT;
  if (pred->w != ref->w || pred->h != ref->h)
    return fail(ctx, XVCGPU_INVALID_ARGUMENT, "picture mismatch");
  if (n == 0) return XVCGPU_OK;
  hipLaunchKernelGGL(mc_affine_kernel, dim3(n), dim3(256), 0, ctx->stream, ref->v,
                     pred->v, d_blocks, n);
  CHECK_LAUNCH(ctx, "mc_affine_batch");
  return XVCGPU_OK;
}

xvcgpu_status xvcgpu_mc_bipred_batch(xvcgpu_ctx *ctx, const xvcgpu_picture *ref0,
                                     const xvcgpu_picture *ref1, xvcgpu_picture *pred,
                                     const xvcgpu_mc_bi_block *d_blocks, int n) {
  if (!ctx || !ref0 || !ref1 || !pred || n < 0 || (n && !d_blocks))
    return XVCGPU_INVALID_ARGUMENT;
  if (pred->w != ref0->w || pred->h != ref0->h || ref1->w != ref0->w ||
      ref1->h != ref0->h || ref1->bd != ref0->bd)
    return fail(ctx, XVCGPU_INVALID_ARGUMENT, "picture mismatch");
  if (n == 0) return XVCGPU_OK;
  hipLaunchKernelGGL(mc_bipred_kernel, dim3(n), dim3(256), 0, ctx->stream, ref0->v,
                     ref1->v, pred->v, d_blocks, n);
  CHECK_LAUNCH(ctx, "mc_bipred_batch");
  return XVCGPU_OK;
}

static xvcgpu_status bipred_search_launch(xvcgpu_ctx *ctx, const xvcgpu_picture *orig,
                                          const xvcgpu_picture *ref_other,
                                          const xvcgpu_picture *ref_search,
                                          const xvcgpu_picture *rec,
                                          const xvcgpu_bi_block *d_jobs,
                                          const xvcgpu_mc_lic_block *d_nb, int n,
                                          xvcgpu_me_result *d_results, int max_block_size) {
  if (!ctx || !orig || !ref_other || !ref_search || n < 0 ||
      (n && (!d_jobs || !d_results)) || max_block_size < 4 || max_block_size > 64 ||
      ((rec != nullptr) != (d_nb != nullptr)))
    return XVCGPU_INVALID_ARGUMENT;
  if (orig->w != ref_other->w || orig->h != ref_other->h ||
      orig->bd != ref_other->bd || orig->w != ref_search->w ||
      orig->h != ref_search->h || orig->bd != ref_search->bd ||
      (rec && (rec->w != orig->w || rec->h != orig->h || rec->bd != orig->bd)))
    return fail(ctx, XVCGPU_INVALID_ARGUMENT, "picture mismatch");
  if (n == 0) return XVCGPU_OK;
  const dim3 grid((n + 7) / 8 * 8);
  const int bi_max = me_class_of(max_block_size);
#define BI_LAUNCH(MS)                                                                        \
  do {                                                                                       \
    if (rec)                                                                                 \
      hipLaunchKernelGGL((bipred_search_kernel<MS, true>), grid, dim3(64 * BI_WAVES(MS)), 0, \
                         ctx->stream, orig->v.c[0], ref_other->v.c[0], ref_search->v.c[0],   \
                         orig->bd, d_jobs, n, d_results, bi_max, rec->v.c[0], d_nb);         \
    else                                                                                     \
      hipLaunchKernelGGL((bipred_search_kernel<MS, false>), grid, dim3(64 * BI_WAVES(MS)), 0,\
                         ctx->stream, orig->v.c[0], ref_other->v.c[0], ref_search->v.c[0],   \
                         orig->bd, d_jobs, n, d_results, bi_max, PlaneView(), nullptr);      \
  } while (0)
  BI_LAUNCH(16);
  if (max_block_size > 16) BI_LAUNCH(32);
  if (max_block_size > 32) BI_LAUNCH(64);
#undef BI_LAUNCH
  CHECK_LAUNCH(ctx, "bipred_search");
  return XVCGPU_OK;
}

xvcgpu_status xvcgpu_bipred_search(xvcgpu_ctx *ctx, const xvcgpu_picture *orig,
                                   const xvcgpu_picture *ref_other,
                                   const xvcgpu_picture *ref_search,
                                   const xvcgpu_bi_block *d_jobs, int n,
                                   xvcgpu_me_result *d_results, int max_block_size) {
  return bipred_search_launch(ctx, orig, ref_other, ref_search, nullptr, d_jobs, nullptr, n,
                              d_results, max_block_size);
}

xvcgpu_status xvcgpu_bipred_search_lic(xvcgpu_ctx *ctx, const xvcgpu_picture *orig,
                                       const xvcgpu_picture *ref_other,
                                       const xvcgpu_picture *ref_search,
                                       const xvcgpu_picture *rec,
                                       const xvcgpu_bi_block *d_jobs,
                                       const xvcgpu_mc_lic_block *d_neighbours, int n,
                                       xvcgpu_me_result *d_results, int max_block_size) {
  if (!rec || !d_neighbours) return XVCGPU_INVALID_ARGUMENT;
  return bipred_search_launch(ctx, orig, ref_other, ref_search, rec, d_jobs, d_neighbours, n,
                              d_results, max_block_size);
}

xvcgpu_status xvcgpu_mc_from_me(xvcgpu_ctx *ctx, const xvcgpu_picture *ref,
                                xvcgpu_picture *pred,
                                const xvcgpu_me_block *d_blocks,
                                const xvcgpu_me_result *d_results, int n) {
  if (!ctx || !ref || !pred || n < 0 || (n && (!d_blocks || !d_results)))
    return XVCGPU_INVALID_ARGUMENT;
  if (pred->w != ref->w || pred->h != ref->h)
    return fail(ctx, XVCGPU_INVALID_ARGUMENT, "picture mismatch");
  if (n == 0) return XVCGPU_OK;
  hipLaunchKernelGGL(mc_from_me_kernel, dim3(n, 3), dim3(256), 0, ctx->stream,
                     ref->v, pred->v, d_blocks, d_results, n);
  CHECK_LAUNCH(ctx, "mc_from_me");
  return XVCGPU_OK;
}

xvcgpu_status xvcgpu_cu_info_from_me(xvcgpu_ctx *ctx,
                                     const xvcgpu_me_block *d_blocks,
                                     const xvcgpu_me_result *d_results,
                                     const int32_t *d_nnz,
                                     const int32_t *d_luma_tx_index, int n,
                                     int qp_y, int qp_c, int ref_poc,
                                     xvcgpu_cu_info *d_cus) {
  if (!ctx || n < 0 || (n && (!d_blocks || !d_results || !d_nnz || !d_cus)))
    return XVCGPU_INVALID_ARGUMENT;
  if (n == 0) return XVCGPU_OK;
  hipLaunchKernelGGL(cu_info_from_me_kernel, dim3((n + 255) / 256), dim3(256), 0,
                     ctx->stream, d_blocks, d_results, d_nnz, d_luma_tx_index, n,
                     qp_y, qp_c, ref_poc, d_cus);
  CHECK_LAUNCH(ctx, "cu_info_from_me");
  return XVCGPU_OK;
}

xvcgpu_status xvcgpu_recon_from_me(xvcgpu_ctx *ctx, const xvcgpu_picture *orig,
                                   const xvcgpu_picture *ref, xvcgpu_picture *rec,
                                   const xvcgpu_me_block *d_blocks,
                                   const xvcgpu_me_result *d_results, int n,
                                   int qp_y, int qp_c, int intra_pic, int ref_poc,
                                   int32_t *d_nnz, xvcgpu_cu_info *d_cus) {
  if (!ctx || !orig || !ref || !rec || n < 0 || (n && (!d_blocks || !d_results)))
    return XVCGPU_INVALID_ARGUMENT;
  if (orig->w != ref->w || orig->h != ref->h || rec->w != ref->w || rec->h != ref->h)
    return fail(ctx, XVCGPU_INVALID_ARGUMENT, "picture mismatch");
  if (n == 0) return XVCGPU_OK;
  hipLaunchKernelGGL(recon_from_me_kernel<false>, dim3(XcdPairJobs<RECON_WAVES>::grid(2 * n)),
                     dim3(64 * RECON_WAVES), 0,
                     ctx->stream, orig->v, ref->v, rec->v, d_blocks, d_results, n, qp_y,
                     qp_c, intra_pic, ref_poc, d_nnz, d_cus, ctx->d_tx_tables,
                     ctx->d_tx_tables_t, xvcgpu_tx_layout(), nullptr, nullptr);
  CHECK_LAUNCH(ctx, "recon_from_me");
  return XVCGPU_OK;
}

xvcgpu_status xvcgpu_fwd_from_me(xvcgpu_ctx *ctx, const xvcgpu_picture *orig,
                                 const xvcgpu_picture *ref, xvcgpu_picture *pred,
                                 const xvcgpu_me_block *d_blocks,
                                 const xvcgpu_me_result *d_results, int n, int16_t *d_coeffs,
                                 const uint32_t *d_coeff_offsets) {
  if (!ctx || !orig || !ref || !pred || n < 0 ||
      (n && (!d_blocks || !d_results || !d_coeffs || !d_coeff_offsets)))
    return XVCGPU_INVALID_ARGUMENT;
  if (orig->w != ref->w || orig->h != ref->h || pred->w != ref->w || pred->h != ref->h)
    return fail(ctx, XVCGPU_INVALID_ARGUMENT, "picture mismatch");
  if (n == 0) return XVCGPU_OK;
  hipLaunchKernelGGL((recon_from_me_kernel<false, true>), dim3(XcdPairJobs<RECON_WAVES>::grid(2 * n)),
                     dim3(64 * RECON_WAVES), 0,
                     ctx->stream, orig->v, ref->v, pred->v, d_blocks, d_results, n, 0, 0, 0, 0,
                     nullptr, nullptr, ctx->d_tx_tables, ctx->d_tx_tables_t, xvcgpu_tx_layout(),
                     nullptr, nullptr, d_coeffs, d_coeff_offsets);
  CHECK_LAUNCH(ctx, "fwd_from_me");
  return XVCGPU_OK;
}

xvcgpu_status xvcgpu_recon_from_me_rdoq(xvcgpu_ctx *ctx, const xvcgpu_picture *orig,
                                        const xvcgpu_picture *ref, xvcgpu_picture *rec,
                                        const xvcgpu_me_block *d_blocks,
                                        const xvcgpu_me_result *d_results, int n,
                                        int qp_y, int qp_c, int tx_flags, int ref_poc,
                                        int32_t *d_nnz, xvcgpu_cu_info *d_cus,
                                        const xvcgpu_rdoq_contexts *d_contexts,
                                        const xvcgpu_rdoq_params *d_params) {
  if (!ctx || !orig || !ref || !rec || n < 0 ||
      (n && (!d_blocks || !d_results || !d_contexts || !d_params)))
    return XVCGPU_INVALID_ARGUMENT;
  if (orig->w != ref->w || orig->h != ref->h || rec->w != ref->w || rec->h != ref->h)
    return fail(ctx, XVCGPU_INVALID_ARGUMENT, "picture mismatch");
  if (n == 0) return XVCGPU_OK;
  hipLaunchKernelGGL(recon_from_me_kernel<true>, dim3(XcdPairJobs<RECON_WAVES>::grid(2 * n)),
                     dim3(64 * RECON_WAVES), 0,
                     ctx->stream, orig->v, ref->v, rec->v, d_blocks, d_results, n, qp_y,
                     qp_c, tx_flags | XVC_TXF_RDOQ, ref_poc, d_nnz, d_cus, ctx->d_tx_tables,
                     ctx->d_tx_tables_t, xvcgpu_tx_layout(), d_contexts, d_params);
  CHECK_LAUNCH(ctx, "recon_from_me_rdoq");
  return XVCGPU_OK;
}

xvcgpu_status xvcgpu_residual_batch(xvcgpu_ctx *ctx, const xvcgpu_picture *orig,
                                    const xvcgpu_picture *pred,
                                    xvcgpu_picture *rec,
                                    const xvcgpu_tx_block *d_blocks, int n,
                                    int16_t *d_levels,
                                    const uint32_t *d_level_offsets,
                                    int32_t *d_nnz) {
  if (!ctx || !orig || !pred || !rec || n < 0 || (n && !d_blocks))
    return XVCGPU_INVALID_ARGUMENT;
  if (n == 0) return XVCGPU_OK;
  launch_residual<TX_MODE_FULL>(ctx, orig->v, pred->v, rec->v, d_blocks, n, d_levels,
                                d_level_offsets, d_nnz);
  CHECK_LAUNCH(ctx, "residual_batch");
  return XVCGPU_OK;
}

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
                                            uint64_t *d_eval_out) {
  if (!ctx || !orig || !pred || !rec || n < 0 || n_eval_head < 0 || n_eval_head > 64 ||
      (n && (!d_blocks || !d_contexts || !d_params || !d_src_pos)) ||
      ((d_eval_cands != nullptr) != (d_eval_out != nullptr)))
    return XVCGPU_INVALID_ARGUMENT;
  if (orig->bd != pred->bd || rec->bd != pred->bd || rec->w != pred->w || rec->h != pred->h)
    return fail(ctx, XVCGPU_INVALID_ARGUMENT, "picture mismatch");
  if (n > 64) return fail(ctx, XVCGPU_UNSUPPORTED, "residual_rdoq_batch_at: a CU state's blocks (<= 64)");
  if (n == 0) return XVCGPU_OK;
  launch_residual_rdoq(ctx, orig->v, pred->v, rec->v, d_blocks, n, d_levels, d_level_offsets,
                       d_nnz, d_contexts, d_params, d_src_pos, d_eval_cands, n_eval_head,
                       d_eval_out, structural_strength);
  CHECK_LAUNCH(ctx, "residual_rdoq_batch_at");
  return XVCGPU_OK;
}

xvcgpu_status xvcgpu_residual_rdoq_batch(xvcgpu_ctx *ctx, const xvcgpu_picture *orig,
                                         const xvcgpu_picture *pred, xvcgpu_picture *rec,
                                         const xvcgpu_tx_block *d_blocks, int n,
                                         int16_t *d_levels, const uint32_t *d_level_offsets,
                                         int32_t *d_nnz,
                                         const xvcgpu_rdoq_contexts *d_contexts,
                                         const xvcgpu_rdoq_params *d_params) {
  if (!ctx || !orig || !pred || !rec || n < 0 || (n && (!d_blocks || !d_contexts || !d_params)))
    return XVCGPU_INVALID_ARGUMENT;
  if (orig->w != pred->w || orig->h != pred->h || rec->w != pred->w || rec->h != pred->h ||
      orig->bd != pred->bd || rec->bd != pred->bd)
    return fail(ctx, XVCGPU_INVALID_ARGUMENT, "picture mismatch");
  if (n == 0) return XVCGPU_OK;
  launch_residual_rdoq(ctx, orig->v, pred->v, rec->v, d_blocks, n, d_levels, d_level_offsets,
                       d_nnz, d_contexts, d_params);
  CHECK_LAUNCH(ctx, "residual_rdoq_batch");
  return XVCGPU_OK;
}

// workgroups per class of quant_rdo_packed_kernel (k_rdoq.h); -DRDOQ_GRID16= ... at build
// time is the knob for experiments, nothing reads the environment
#ifndef RDOQ_GRID16
#define RDOQ_GRID16 8192   // blocks of up to sixteen sub-blocks: one per wave
#endif
#ifndef RDOQ_GRID4
#define RDOQ_GRID4 2048    // blocks of up to four sub-blocks: four per wave
#endif
#ifndef RDOQ_GRID64
#define RDOQ_GRID64 512
#endif

// Scratch of the packed quantiser: the class lists, their counters and the per-block
// classes (k_rdoq.h: rdoq_scratch_lists), with a quarter of headroom; grown by the
// first batch of a size, or ahead of it by xvcgpu_quant_rdo_reserve.
static xvcgpu_status ensure_rdoq_scratch(xvcgpu_ctx *ctx, int n) {
  if (n <= ctx->rdoq_lists_cap) return XVCGPU_OK;   // (the headroom is for the next batch)
  const int cap = rdoq_scratch_cap(n);
  return grow_scratch(ctx, &ctx->d_rdoq_lists, &ctx->rdoq_lists_cap, cap, rdoq_scratch_bytes(cap),
                      false, "rdoq lists");
}

xvcgpu_status xvcgpu_quant_rdo_class_counts(xvcgpu_ctx *ctx, int32_t out[3]) {
  if (!ctx || !out) return XVCGPU_INVALID_ARGUMENT;
  out[0] = out[1] = out[2] = 0;
  if (!ctx->d_rdoq_lists) return XVCGPU_OK;
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  HIP_TRY(ctx, hipMemcpy(out, rdoq_lists_of(ctx).count, 3 * sizeof(int32_t),
                         hipMemcpyDeviceToHost));
  return XVCGPU_OK;
}

xvcgpu_status xvcgpu_quant_rdo_set_prove_zero(xvcgpu_ctx *ctx, int mode) {
  if (!ctx || mode < -1 || mode > 1) return XVCGPU_INVALID_ARGUMENT;
  ctx->rdoq_prove_zero = mode;
  return XVCGPU_OK;
}

xvcgpu_status xvcgpu_quant_rdo_set_list_form(xvcgpu_ctx *ctx, int mode) {
  if (!ctx || mode < -1 || mode > 1) return XVCGPU_INVALID_ARGUMENT;
  ctx->rdoq_list_form = mode;
  return XVCGPU_OK;
}

xvcgpu_status xvcgpu_quant_rdo_set_four_lane_only(xvcgpu_ctx *ctx, int on) {
  if (!ctx) return XVCGPU_INVALID_ARGUMENT;
  ctx->rdoq_four_lane_only = on ? 1 : 0;
  return XVCGPU_OK;
}

xvcgpu_status xvcgpu_quant_rdo_reserve(xvcgpu_ctx *ctx, int n, size_t n_coeffs) {
  if (!ctx || n < 0) return XVCGPU_INVALID_ARGUMENT;
  (void)n_coeffs;   // the per-coefficient records live in LDS
  return ensure_rdoq_scratch(ctx, n);
}

// The class sizes are only known on the device: a bounded number of workgroups per
// class that walk their list (k_rdoq.h), for a batch of n blocks
struct RdoqGrids {
  int g16, g4, g64;
};
static RdoqGrids rdoq_walk_grids(int n) {
  return {std::min(n, RDOQ_GRID16), std::min((n + 3) / 4, RDOQ_GRID4), std::min(n, RDOQ_GRID64)};
}

// classified: the blocks' classes are already in the context's RdoqLists::cls
// (written by the forward transform of xvcgpu_frame_pass, FwdClassify); four_only: the
// general class's launch is skipped (xvcgpu_quant_rdo_set_four_lane_only, or the frame
// pass's tx_four_lane_only)
static xvcgpu_status quant_rdo_launch(xvcgpu_ctx *ctx, int bitdepth,
                                      const xvcgpu_tx_block *d_blocks, int n,
                                      const int16_t *d_coeffs, const uint32_t *d_offsets,
                                      size_t n_coeffs, int16_t *d_levels, int32_t *d_nnz,
                                      const xvcgpu_rdoq_contexts *d_contexts,
                                      const xvcgpu_rdoq_params *d_params, bool classified,
                                      bool four_only, xvcgpu_cu_info *d_cu_patch = nullptr) {
  if (!ctx || n < 0 || bitdepth < 8 || bitdepth > 12 ||
      (n && (!d_blocks || !d_coeffs || !d_offsets || !d_levels || !d_contexts || !d_params ||
             !n_coeffs)))
    return XVCGPU_INVALID_ARGUMENT;
  if (n == 0) return XVCGPU_OK;
  {
    const xvcgpu_status st_ = ensure_rdoq_scratch(ctx, n);
    if (st_ != XVCGPU_OK) return st_;
  }
  const RdoqLists l = rdoq_lists_of(ctx);
  if (!classified)
    hipLaunchKernelGGL(rdoq_classify_kernel, dim3((n + 3) / 4), dim3(256), 0, ctx->stream,
                       bitdepth, d_blocks, n, d_coeffs, d_offsets, d_levels, d_nnz, l);
  // the blocks the walk is bound to return 0 for leave the lists here (k_rdoq.h)
  const int qp_hint = classified ? ctx->rdoq_qp_hint : -1;
  // (the classes a proving forward call left behind stay proved until the next one)
  const bool proved_already = classified && ctx->rdoq_classified_proved;
  if (!proved_already &&
      (ctx->rdoq_prove_zero > 0 ||
       (ctx->rdoq_prove_zero < 0 && n >= XVCGPU_PROVE_ZERO_AUTO_BLOCKS &&
        (qp_hint < 0 || qp_hint >= XVCGPU_PROVE_ZERO_AUTO_QP))))
    hipLaunchKernelGGL(rdoq_prove_zero_kernel, dim3((n + RQ_PROVE_BLOCKS - 1) / RQ_PROVE_BLOCKS),
                       dim3(256), 0, ctx->stream,
                       bitdepth, d_blocks, n, d_coeffs, d_offsets, d_levels, d_nnz, d_contexts,
                       d_params, l);
  // the class lists: one launch of small workgroups for small batches, count + scatter
  // above the threshold (k_rdoq.h, xvcgpu_quant_rdo_set_list_form)
  if (ctx->rdoq_list_form > 0 ||
      (ctx->rdoq_list_form < 0 && n <= XVCGPU_RDOQ_ONE_LAUNCH_LISTS_MAX_BLOCKS)) {
    hipLaunchKernelGGL(rdoq_lists_kernel, dim3((n + RDOQ_LISTS_CHUNK - 1) / RDOQ_LISTS_CHUNK),
                       dim3(RDOQ_LISTS_THREADS), 0, ctx->stream, n, l);
  } else {
    const int chunks = (n + RDOQ_CHUNK - 1) / RDOQ_CHUNK;
    hipLaunchKernelGGL(rdoq_count_kernel, dim3(chunks), dim3(1024), 0, ctx->stream, n, l);
    hipLaunchKernelGGL(rdoq_scatter_kernel, dim3(chunks), dim3(1024), 0, ctx->stream, n, l);
  }
  ctx->rdoq_last_n = n;
  const RdoqGrids g = rdoq_walk_grids(n);
  // (the general class's launch holds 255 vector registers a wave: even with an empty list
  // it waits for room beside other streams' kernels - 190 us in flight at 2160p; a caller
  // that knows its blocks says so and the launch is not made)
  hipLaunchKernelGGL(quant_rdo_packed4_kernel, dim3(g.g16 + g.g4), dim3(64), 0, ctx->stream,
                     bitdepth, d_blocks, l, g.g16, d_coeffs, d_offsets, d_levels, d_nnz,
                     d_contexts, d_params, d_cu_patch, four_only ? ctx->h_rdoq_misuse : nullptr);
  if (!four_only)
    hipLaunchKernelGGL(quant_rdo_packed_kernel, dim3(g.g64), dim3(64), 0, ctx->stream,
                       bitdepth, d_blocks, l, d_coeffs, d_offsets, d_levels, d_nnz,
                       d_contexts, d_params, d_cu_patch);
  CHECK_LAUNCH(ctx, "quant_rdo_batch");
  return XVCGPU_OK;
}

xvcgpu_status xvcgpu_quant_rdo_batch(xvcgpu_ctx *ctx, int bitdepth,
                                     const xvcgpu_tx_block *d_blocks, int n,
                                     const int16_t *d_coeffs, const uint32_t *d_offsets,
                                     size_t n_coeffs, int16_t *d_levels, int32_t *d_nnz,
                                     const xvcgpu_rdoq_contexts *d_contexts,
                                     const xvcgpu_rdoq_params *d_params) {
  return quant_rdo_launch(ctx, bitdepth, d_blocks, n, d_coeffs, d_offsets, n_coeffs, d_levels,
                          d_nnz, d_contexts, d_params, false, ctx && ctx->rdoq_four_lane_only);
}

xvcgpu_status xvcgpu_quant_rdo_classified_batch(xvcgpu_ctx *ctx, int bitdepth,
                                                const xvcgpu_tx_block *d_blocks, int n,
                                                const int16_t *d_coeffs,
                                                const uint32_t *d_offsets, size_t n_coeffs,
                                                int16_t *d_levels, int32_t *d_nnz,
                                                const xvcgpu_rdoq_contexts *d_contexts,
                                                const xvcgpu_rdoq_params *d_params,
                                                xvcgpu_cu_info *d_cus) {
  return quant_rdo_launch(ctx, bitdepth, d_blocks, n, d_coeffs, d_offsets, n_coeffs, d_levels,
                          d_nnz, d_contexts, d_params, true, ctx && ctx->rdoq_four_lane_only,
                          d_cus);
}

xvcgpu_status xvcgpu_fwd_from_me_classify(xvcgpu_ctx *ctx, const xvcgpu_picture *orig,
                                          const xvcgpu_picture *ref, xvcgpu_picture *pred,
                                          const xvcgpu_me_block *d_blocks,
                                          const xvcgpu_me_result *d_results, int n, int qp_y,
                                          int qp_c, int ref_poc, int16_t *d_coeffs,
                                          const uint32_t *d_coeff_offsets, size_t n_coeffs,
                                          int16_t *d_levels, int32_t *d_nnz,
                                          xvcgpu_cu_info *d_cus) {
  return xvcgpu_fwd_from_me_classify_prove(ctx, orig, ref, pred, d_blocks, d_results, n, qp_y, qp_c,
                                           ref_poc, d_coeffs, d_coeff_offsets, n_coeffs, d_levels,
                                           d_nnz, d_cus, nullptr, nullptr);
}

xvcgpu_status xvcgpu_fwd_from_me_classify_prove(
    xvcgpu_ctx *ctx, const xvcgpu_picture *orig, const xvcgpu_picture *ref, xvcgpu_picture *pred,
    const xvcgpu_me_block *d_blocks, const xvcgpu_me_result *d_results, int n, int qp_y, int qp_c,
    int ref_poc, int16_t *d_coeffs, const uint32_t *d_coeff_offsets, size_t n_coeffs,
    int16_t *d_levels, int32_t *d_nnz, xvcgpu_cu_info *d_cus,
    const xvcgpu_rdoq_contexts *d_contexts, const xvcgpu_rdoq_params *d_params) {
  if ((d_contexts == nullptr) != (d_params == nullptr)) return XVCGPU_INVALID_ARGUMENT;
  if (!ctx || !orig || !ref || !pred || n < 0 ||
      (n && (!d_blocks || !d_results || !d_coeffs || !d_coeff_offsets || !d_levels || !d_nnz)))
    return XVCGPU_INVALID_ARGUMENT;
  if (orig->w != ref->w || orig->h != ref->h || pred->w != ref->w || pred->h != ref->h)
    return fail(ctx, XVCGPU_INVALID_ARGUMENT, "picture mismatch");
  if (n == 0) return XVCGPU_OK;
  {
    const xvcgpu_status st = ensure_rdoq_scratch(ctx, 3 * n);
    if (st != XVCGPU_OK) return st;
  }
  ctx->rdoq_qp_hint = qp_y;
  FwdClassify fc;
  fc.cls = rdoq_lists_of(ctx).cls;
  fc.levels = d_levels;
  fc.nnz = d_nnz;
  // the all-zero proof where the coefficients are at hand, unless it is switched off;
  // the quantiser's own launch of it is then not needed
  const bool prove = d_contexts && ctx->rdoq_prove_zero != 0;
  fc.rq_ctx = prove ? d_contexts : nullptr;
  fc.rq_prm = prove ? d_params : nullptr;
  fc.pv = nullptr;
  ctx->rdoq_classified_proved = prove;
  hipLaunchKernelGGL((recon_from_me_kernel<false, true>), dim3(XcdPairJobs<RECON_WAVES>::grid(2 * n)),
                     dim3(64 * RECON_WAVES), 0,
                     ctx->stream, orig->v, ref->v, pred->v, d_blocks, d_results, n, qp_y, qp_c, 0,
                     ref_poc, nullptr, d_cus, ctx->d_tx_tables, ctx->d_tx_tables_t,
                     xvcgpu_tx_layout(), nullptr, nullptr, d_coeffs, d_coeff_offsets, fc);
  CHECK_LAUNCH(ctx, "fwd_from_me_classify");
  return XVCGPU_OK;
}

xvcgpu_status xvcgpu_fwd_transform_batch(xvcgpu_ctx *ctx,
                                         const xvcgpu_picture *orig,
                                         const xvcgpu_picture *pred,
                                         const xvcgpu_tx_block *d_blocks, int n,
                                         int16_t *d_coeffs,
                                         const uint32_t *d_coeff_offsets) {
  if (!ctx || !orig || !pred || n < 0 ||
      (n && (!d_blocks || !d_coeffs || !d_coeff_offsets)))
    return XVCGPU_INVALID_ARGUMENT;
  if (n == 0) return XVCGPU_OK;
  launch_residual<TX_MODE_FWD>(ctx, orig->v, pred->v, pred->v, d_blocks, n, d_coeffs,
                               d_coeff_offsets, (int32_t *)nullptr);
  CHECK_LAUNCH(ctx, "fwd_transform_batch");
  return XVCGPU_OK;
}

xvcgpu_status xvcgpu_inv_transform_batch(xvcgpu_ctx *ctx,
                                         const xvcgpu_picture *pred,
                                         xvcgpu_picture *rec,
                                         const xvcgpu_tx_block *d_blocks, int n,
                                         const int16_t *d_levels,
                                         const uint32_t *d_level_offsets,
                                         const int32_t *d_nnz) {
  if (!ctx || !pred || !rec || n < 0 ||
      (n && (!d_blocks || !d_levels || !d_level_offsets || !d_nnz)))
    return XVCGPU_INVALID_ARGUMENT;
  if (n == 0) return XVCGPU_OK;
  launch_residual<TX_MODE_INV>(ctx, pred->v, pred->v, rec->v, d_blocks, n,
                               const_cast<int16_t *>(d_levels), d_level_offsets,
                               const_cast<int32_t *>(d_nnz));
  CHECK_LAUNCH(ctx, "inv_transform_batch");
  return XVCGPU_OK;
}

xvcgpu_status xvcgpu_inv_transform_cu_order(xvcgpu_ctx *ctx, xvcgpu_picture *rec,
                                            const xvcgpu_tx_block *d_blocks, int n_cus,
                                            const int16_t *d_levels,
                                            const uint32_t *d_level_offsets,
                                            const int32_t *d_nnz) {
  if (!ctx || !rec || n_cus < 0 ||
      (n_cus && (!d_blocks || !d_levels || !d_level_offsets || !d_nnz)))
    return XVCGPU_INVALID_ARGUMENT;
  if (n_cus == 0) return XVCGPU_OK;
  hipLaunchKernelGGL(inv_cu_pairs_kernel, dim3(XcdPairJobs<INV_PAIRS_WAVES>::grid(2 * n_cus)),
                     dim3(64 * INV_PAIRS_WAVES), 0, ctx->stream, rec->v, d_blocks, n_cus,
                     const_cast<int16_t *>(d_levels), d_level_offsets,
                     const_cast<int32_t *>(d_nnz), ctx->d_tx_tables, ctx->d_tx_tables_t,
                     xvcgpu_tx_layout());
  CHECK_LAUNCH(ctx, "inv_transform_cu_order");
  return XVCGPU_OK;
}

xvcgpu_status xvcgpu_inv_transform_dist_batch(xvcgpu_ctx *ctx, const xvcgpu_picture *orig,
                                              const xvcgpu_picture *pred, xvcgpu_picture *rec,
                                              const xvcgpu_tx_block *d_blocks, int n,
                                              const int16_t *d_levels,
                                              const uint32_t *d_level_offsets,
                                              const int32_t *d_nnz, uint64_t *d_dist) {
  if (!ctx || !orig || !pred || !rec || n < 0 ||
      (n && (!d_blocks || !d_levels || !d_level_offsets || !d_nnz || !d_dist)))
    return XVCGPU_INVALID_ARGUMENT;
  if (orig->w != pred->w || orig->h != pred->h || orig->bd != pred->bd)
    return fail(ctx, XVCGPU_INVALID_ARGUMENT, "picture mismatch");
  if (n == 0) return XVCGPU_OK;
  launch_residual<TX_MODE_INV>(ctx, orig->v, pred->v, rec->v, d_blocks, n,
                               const_cast<int16_t *>(d_levels), d_level_offsets,
                               const_cast<int32_t *>(d_nnz),
                               reinterpret_cast<unsigned long long *>(d_dist));
  CHECK_LAUNCH(ctx, "inv_transform_dist_batch");
  return XVCGPU_OK;
}

xvcgpu_status xvcgpu_tx_eval_batch(xvcgpu_ctx *ctx, const xvcgpu_tx_eval_job *d_jobs, int n,
                                   const xvcgpu_tx_eval_alt *d_alts,
                                   xvcgpu_tx_eval_result *d_out) {
  if (!ctx || n < 0 || (n && (!d_jobs || !d_alts || !d_out))) return XVCGPU_INVALID_ARGUMENT;
  if (n == 0) return XVCGPU_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipLaunchKernelGGL(tx_eval_kernel, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, d_jobs, n,
                     d_alts, d_out);
  CHECK_LAUNCH(ctx, "tx_eval_batch");
  return XVCGPU_OK;
}

xvcgpu_status xvcgpu_root_cbf_batch(xvcgpu_ctx *ctx, const xvcgpu_root_cbf_job *d_jobs, int n,
                                    xvcgpu_root_cbf_result *d_out) {
  if (!ctx || n < 0 || (n && (!d_jobs || !d_out))) return XVCGPU_INVALID_ARGUMENT;
  if (n == 0) return XVCGPU_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipLaunchKernelGGL(root_cbf_kernel, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, d_jobs, n,
                     d_out);
  CHECK_LAUNCH(ctx, "root_cbf_batch");
  return XVCGPU_OK;
}

static xvcgpu_status deblock_rows_masked(xvcgpu_ctx *ctx, xvcgpu_picture *rec,
                                         const xvcgpu_cu_info *d_cus, int n_cus,
                                         const int32_t *d_cu_map, int map_stride,
                                         int pic_is_bipred, int beta_offset,
                                         int tc_offset, int subblock_size, int pass,
                                         int y_begin, int y_end, int comp_mask) {
  if (!ctx || !rec || !d_cus || n_cus <= 0 || !d_cu_map ||
      map_stride < (rec->w + 3) / 4 || (subblock_size != 4 && subblock_size != 8) ||
      (pass != 0 && pass != 1) || y_begin < 0 || (y_begin % subblock_size) != 0)
    return XVCGPU_INVALID_ARGUMENT;
  if (y_end > rec->h) y_end = rec->h;
  if (y_end <= y_begin) return XVCGPU_OK;
  DbParams d;
  d.bd = rec->bd;
  d.pic_w = rec->w;
  d.pic_h = rec->h;
  d.bipred = pic_is_bipred;
  d.beta_off = beta_offset;
  d.tc_off = tc_offset;
  d.sub = subblock_size;
  d.y_begin = y_begin;
  d.y_end = y_end;
  d.cus = d_cus;
  d.map = d_cu_map;
  d.map_stride = map_stride;
  d.map_rows = (rec->h + 3) / 4;
  d.comp_mask = comp_mask;
  const int nx = (rec->w + subblock_size - 1) / subblock_size;
  const int ny = (y_end - y_begin + subblock_size - 1) / subblock_size;
  const dim3 grid((nx + 63) / 64, ny);
  if (pass == 0)
    hipLaunchKernelGGL(deblock_pass_kernel<true>, grid, dim3(64), 0, ctx->stream, d,
                       rec->v);
  else
    hipLaunchKernelGGL(deblock_pass_kernel<false>, grid, dim3(64), 0, ctx->stream, d,
                       rec->v);
  CHECK_LAUNCH(ctx, "deblock_rows");
  return XVCGPU_OK;
}

xvcgpu_status xvcgpu_deblock_rows(xvcgpu_ctx *ctx, xvcgpu_picture *rec,
                                  const xvcgpu_cu_info *d_cus, int n_cus,
                                  const int32_t *d_cu_map, int map_stride,
                                  int pic_is_bipred, int beta_offset,
                                  int tc_offset, int subblock_size, int pass,
                                  int y_begin, int y_end) {
  return deblock_rows_masked(ctx, rec, d_cus, n_cus, d_cu_map, map_stride, pic_is_bipred,
                             beta_offset, tc_offset, subblock_size, pass, y_begin, y_end, 3);
}

xvcgpu_status xvcgpu_deblock_tree(xvcgpu_ctx *ctx, xvcgpu_picture *rec,
                                  const xvcgpu_cu_info *d_cus, int n_cus,
                                  const int32_t *d_cu_map, int map_stride,
                                  int pic_is_bipred, int beta_offset, int tc_offset,
                                  int subblock_size, int comp_mask) {
  if (!rec || comp_mask < 1 || comp_mask > 3) return XVCGPU_INVALID_ARGUMENT;
  xvcgpu_status st = deblock_rows_masked(ctx, rec, d_cus, n_cus, d_cu_map, map_stride,
                                         pic_is_bipred, beta_offset, tc_offset,
                                         subblock_size, 0, 0, rec->h, comp_mask);
  if (st != XVCGPU_OK) return st;
  return deblock_rows_masked(ctx, rec, d_cus, n_cus, d_cu_map, map_stride, pic_is_bipred,
                             beta_offset, tc_offset, subblock_size, 1, 0, rec->h, comp_mask);
}

xvcgpu_status xvcgpu_deblock(xvcgpu_ctx *ctx, xvcgpu_picture *rec,
                             const xvcgpu_cu_info *d_cus, int n_cus,
                             const int32_t *d_cu_map, int map_stride,
                             int pic_is_bipred, int beta_offset, int tc_offset,
                             int subblock_size) {
  if (!rec) return XVCGPU_INVALID_ARGUMENT;
  xvcgpu_status st = xvcgpu_deblock_rows(ctx, rec, d_cus, n_cus, d_cu_map, map_stride,
                                         pic_is_bipred, beta_offset, tc_offset,
                                         subblock_size, 0, 0, rec->h);
  if (st != XVCGPU_OK) return st;
  return xvcgpu_deblock_rows(ctx, rec, d_cus, n_cus, d_cu_map, map_stride,
                             pic_is_bipred, beta_offset, tc_offset, subblock_size, 1,
                             0, rec->h);
}

// Scratch for the per-block results of xvcgpu_picture_ssd; grown when a larger
// picture is created, so no allocation happens on the measurement path.
static xvcgpu_status ensure_ssd_part(xvcgpu_ctx *ctx, int items) {
  return grow_scratch(ctx, &ctx->d_ssd_part, &ctx->ssd_part_cap, items,
                      sizeof(unsigned long long) * 2 * items, false, "ssd scratch");
}

xvcgpu_status xvcgpu_picture_ssd(xvcgpu_ctx *ctx, const xvcgpu_picture *a,
                                 const xvcgpu_picture *b, int comp,
                                 int shift_bitdepth, uint64_t *d_out) {
  return xvcgpu_picture_ssd_rows(ctx, a, b, comp, shift_bitdepth, 0, 1 << 30, d_out);
}

xvcgpu_status xvcgpu_picture_ssd_rows(xvcgpu_ctx *ctx, const xvcgpu_picture *a,
                                      const xvcgpu_picture *b, int comp,
                                      int shift_bitdepth, int y_begin, int y_end,
                                      uint64_t *d_out) {
  if (!ctx || !a || !b || comp < 0 || comp > 2 || !d_out || shift_bitdepth < 8)
    return XVCGPU_INVALID_ARGUMENT;
  if (a->w != b->w || a->h != b->h)
    return fail(ctx, XVCGPU_INVALID_ARGUMENT, "picture mismatch");
  const PlaneView pa = a->v.c[comp], pb = b->v.c[comp];
  const int items = ssd_items(pa.w, pa.h);
  {
    const xvcgpu_status st = ensure_ssd_part(ctx, items);
    if (st != XVCGPU_OK) return st;
  }
  if (items > 0)
    hipLaunchKernelGGL(picture_ssd_kernel, dim3(items), dim3(256), 0, ctx->stream, pa,
                       pb, 2 * (shift_bitdepth - 8), y_begin, y_end, ctx->d_ssd_part);
  hipLaunchKernelGGL(picture_ssd_sum_kernel, dim3(1), dim3(64 * SSD_SUM_WAVES), 0, ctx->stream,
                     ctx->d_ssd_part, items,
                     reinterpret_cast<unsigned long long *>(d_out));
  CHECK_LAUNCH(ctx, "picture_ssd");
  return XVCGPU_OK;
}

// Scratch of xvcgpu_deblock_pad_ssd: per-tile results; sized when a picture is
// created.
static xvcgpu_status ensure_tail(xvcgpu_ctx *ctx, int tiles) {
  return grow_scratch(ctx, &ctx->d_tail_part, &ctx->tail_cap, tiles,
                      sizeof(unsigned long long) * (2 * (size_t)tiles + 2), true, "tail scratch");
}

xvcgpu_status xvcgpu_deblock_pad_ssd(xvcgpu_ctx *ctx, const xvcgpu_picture *src,
                                     xvcgpu_picture *dst, const xvcgpu_picture *orig,
                                     const xvcgpu_cu_info *d_cus, int n_cus,
                                     const int32_t *d_cu_map, int map_stride,
                                     int pic_is_bipred, int beta_offset, int tc_offset,
                                     int shift_bitdepth, uint64_t *d_ssd) {
  if (!ctx || !src || !dst || src == dst || src->base == dst->base || !d_cus || n_cus <= 0 ||
      !d_cu_map || map_stride < (dst->w + 3) / 4 || (orig && (!d_ssd || shift_bitdepth < 8)))
    return XVCGPU_INVALID_ARGUMENT;
  if (src->w != dst->w || src->h != dst->h || src->bd != dst->bd ||
      (orig && (orig->w != dst->w || orig->h != dst->h)))
    return fail(ctx, XVCGPU_INVALID_ARGUMENT, "picture mismatch");
  if ((dst->w & 7) || (dst->h & 7))
    return fail(ctx, XVCGPU_INVALID_ARGUMENT, "deblock_pad_ssd: picture size not a multiple of 8");
  const int tiles = tail_tiles(dst->w, dst->h);
  {
    const xvcgpu_status st = ensure_tail(ctx, tiles);
    if (st != XVCGPU_OK) return st;
  }
  DbParams d;
  d.bd = dst->bd;
  d.pic_w = dst->w;
  d.pic_h = dst->h;
  d.bipred = pic_is_bipred;
  d.beta_off = beta_offset;
  d.tc_off = tc_offset;
  d.sub = 4;
  d.y_begin = 0;
  d.y_end = dst->h;
  d.cus = d_cus;
  d.map = d_cu_map;
  d.map_stride = map_stride;
  d.map_rows = (dst->h + 3) / 4;
  d.comp_mask = 3;
  unsigned long long *part = ctx->d_tail_part;
  if (orig) {
    hipLaunchKernelGGL(deblock_tail_kernel<true>, dim3((tiles + 7) / 8 * 8), dim3(256), 0, ctx->stream, d,
                       src->v, dst->v, orig->v.c[0], 2 * (shift_bitdepth - 8), part);
    hipLaunchKernelGGL(picture_ssd_sum_kernel, dim3(1), dim3(64 * SSD_SUM_WAVES), 0, ctx->stream,
                       part, tiles, reinterpret_cast<unsigned long long *>(d_ssd));
  } else {
    hipLaunchKernelGGL(deblock_tail_kernel<false>, dim3((tiles + 7) / 8 * 8), dim3(256), 0, ctx->stream, d,
                       src->v, dst->v, dst->v.c[0], 0, part);
  }
  CHECK_LAUNCH(ctx, "deblock_pad_ssd");
  return XVCGPU_OK;
}

/* ---- whole-picture passes around the hot path (k_stats.h) ---- */
static const int kStatsHistWords = 4096;

// Scratch of the statistics passes; like the SSD scratch it is sized when a
// picture is created, never on a measurement path.
static xvcgpu_status ensure_stats(xvcgpu_ctx *ctx, int rows) {
  return grow_scratch(ctx, &ctx->d_stats, &ctx->stats_rows_cap, rows,
                      sizeof(uint32_t) * ((size_t)kStatsHistWords + rows), true, "stats scratch");
}

xvcgpu_status xvcgpu_picture_import(xvcgpu_ctx *ctx, xvcgpu_picture *pic,
                                    const void *d_src, int in_width, int in_height,
                                    int in_bitdepth) {
  if (!ctx || !pic || !d_src) return XVCGPU_INVALID_ARGUMENT;
  if (in_width < 2 || in_height < 2 || (in_width & 1) || (in_height & 1) ||
      in_width > pic->w || in_height > pic->h || in_bitdepth < 8 ||
      in_bitdepth > pic->bd || in_bitdepth > 16)
    return fail(ctx, XVCGPU_INVALID_ARGUMENT, "import: input size/bitdepth");
  ImportArgs a;
  const size_t bps = in_bitdepth > 8 ? 2 : 1;
  const uint8_t *src = static_cast<const uint8_t *>(d_src);
  for (int c = 0; c < 3; c++) {
    a.src[c] = src;
    a.in_w[c] = c ? in_width >> 1 : in_width;
    a.in_h[c] = c ? in_height >> 1 : in_height;
    src += (size_t)a.in_w[c] * a.in_h[c] * bps;
  }
  a.wide = in_bitdepth > 8;
  a.upshift = pic->bd - in_bitdepth;
  hipLaunchKernelGGL(picture_import_kernel, dim3(pic->h, 3), dim3(256), 0, ctx->stream,
                     pic->v, a);
  CHECK_LAUNCH(ctx, "picture_import");
  return XVCGPU_OK;
}

xvcgpu_status xvcgpu_picture_export(xvcgpu_ctx *ctx, const xvcgpu_picture *pic,
                                    void *d_dst, int display_width, int display_height,
                                    int out_bitdepth, int dither) {
  if (!ctx || !pic || !d_dst) return XVCGPU_INVALID_ARGUMENT;
  {  // the scratch is sized by the pictures created on THIS context; a picture of
     // another context (or a larger one) must not run into it
    const xvcgpu_status st_ = ensure_stats(ctx, 2 * pic->h);
    if (st_ != XVCGPU_OK) return st_;
  }
  if (display_width < 2 || display_height < 2 || (display_width & 1) ||
      (display_height & 1) || display_width > pic->w || display_height > pic->h ||
      out_bitdepth < 1 || out_bitdepth > 16)
    return fail(ctx, XVCGPU_INVALID_ARGUMENT, "export: output size/bitdepth");
  ExportArgs a;
  a.wide = out_bitdepth > 8;
  const size_t bps = a.wide ? 2 : 1;
  uint8_t *dst = static_cast<uint8_t *>(d_dst);
  int rows = 0;
  for (int c = 0; c < 3; c++) {
    a.dst[c] = dst;
    a.w[c] = c ? display_width >> 1 : display_width;
    a.h[c] = c ? display_height >> 1 : display_height;
    a.row_base[c] = rows;
    rows += a.h[c];
    dst += (size_t)a.w[c] * a.h[c] * bps;
  }
  // CopyToBytesWithShift's dispatch (resample.cc:304-338)
  a.smax = (1 << out_bitdepth) - 1;
  if (out_bitdepth >= pic->bd || (!a.wide && pic->bd <= 8)) {
    a.mode = 0;
    a.shift = a.wide ? out_bitdepth - pic->bd : 0;
  } else {
    a.mode = dither ? 2 : 1;
    a.shift = pic->bd - out_bitdepth;
  }
  uint32_t *row_words = ctx->d_stats + kStatsHistWords;
  a.row_carry = row_words;
  if (a.mode == 2) {
    hipLaunchKernelGGL(export_row_sums_kernel, dim3(a.h[0], 3), dim3(256), 0, ctx->stream,
                       pic->v, a, row_words);
    hipLaunchKernelGGL(export_row_scan_kernel, dim3(3), dim3(256), 0, ctx->stream, a,
                       row_words);
  }
  hipLaunchKernelGGL(picture_export_kernel, dim3(a.h[0], 3), dim3(256), 0, ctx->stream,
                     pic->v, a);
  CHECK_LAUNCH(ctx, "picture_export");
  return XVCGPU_OK;
}

/* ---- output formats (Resampler::ConvertTo) ---- */
static const int kOutMaxDim = 32768;

// util::ScaleSizeX / ScaleSizeY of an output format, plane c
static int out_plane_w(int w, int cf, int c) { return c == 0 || cf >= 3 ? w : w >> 1; }
static int out_plane_h(int h, int cf, int c) { return c == 0 || cf >= 2 ? h : h >> 1; }

static bool out_format_valid(const xvcgpu_output_format &f) {
  if (f.width < 2 || f.height < 2 || f.width > kOutMaxDim || f.height > kOutMaxDim) return false;
  if (f.chroma_format < 0 || f.chroma_format > 4) return false;
  if (f.color_matrix < 0 || f.color_matrix > 3) return false;
  if (f.bitdepth < 8 || f.bitdepth > 16) return false;
  return true;
}

// util::GetTotalNumSamples; the reference holds it in an int
static int64_t out_total_samples(const xvcgpu_output_format &f) {
  const int64_t luma = (int64_t)f.width * f.height;
  if (f.chroma_format == 4) return 4 * luma;
  if (f.chroma_format == 0) return luma;
  return luma + 2 * (int64_t)out_plane_w(f.width, f.chroma_format, 1) *
                    out_plane_h(f.height, f.chroma_format, 1);
}

size_t xvcgpu_output_bytes(const xvcgpu_output_format *fmt) {
  if (!fmt || !out_format_valid(*fmt)) return 0;
  const int64_t n = out_total_samples(*fmt);
  if (n > INT32_MAX) return 0;
  return (size_t)n * (fmt->bitdepth > 8 ? 2 : 1);
}

// resample.cc GetFilterFromScale
static int out_filter_from_scale(int scale) {
  const int k = XVC_OUT_SCALE_ONE;
  if (scale > 15 * k / 4) return 7;
  if (scale > 20 * k / 7) return 6;
  if (scale > 5 * k / 2) return 5;
  if (scale > 2 * k) return 4;
  if (scale > 5 * k / 3) return 3;
  if (scale > 5 * k / 4) return 2;
  if (scale > 20 * k / 19) return 1;
  return 0;
}

// Output rows per tile of a resampled plane: the most (<= XVC_OUT_MAX_TR) whose
// every tile needs at most XVC_OUT_TMP_ROWS filtered source rows.
static int out_resample_tile_rows(int dh, int scale_y) {
  for (int tr = XVC_OUT_MAX_TR; tr > 1; tr >>= 1) {
    int64_t worst = 0;
    for (int y0 = 0; y0 < dh; y0 += tr) {
      const int64_t y1 = std::min(y0 + tr, dh) - 1;
      worst = std::max(worst, ((y1 * scale_y) >> 15) - (((int64_t)y0 * scale_y) >> 15));
    }
    if (worst + 12 <= XVC_OUT_TMP_ROWS) return tr;
  }
  return 1;
}

xvcgpu_status xvcgpu_picture_convert_to(xvcgpu_ctx *ctx, const xvcgpu_picture *pic,
                                        int display_width, int display_height,
                                        const xvcgpu_output_format *fmt, void *d_dst) {
  if (!ctx || !pic || !fmt || !d_dst) return XVCGPU_INVALID_ARGUMENT;
  if (display_width < 2 || display_height < 2 || display_width > pic->w ||
      display_height > pic->h)
    return fail(ctx, XVCGPU_INVALID_ARGUMENT, "convert_to: display size");
  // Decoder's defaults (decoder.cc:162-176); the source is 4:2:0
  xvcgpu_output_format f = *fmt;
  if (f.width == 0) f.width = display_width;
  if (f.height == 0) f.height = display_height;
  if (f.chroma_format == 255) f.chroma_format = 1;
  if (f.bitdepth == 0) f.bitdepth = pic->bd;
  if (!out_format_valid(f) || out_total_samples(f) > INT32_MAX)
    return fail(ctx, XVCGPU_INVALID_ARGUMENT, "convert_to: output format");
  const int cf = f.chroma_format, bd = pic->bd;
  const bool argb = cf == 4;
  // CopyToWithResize produces ARGB's components at kColorConversionBitdepth
  const int dst_bd = argb ? 12 : f.bitdepth;
  if (argb && ((uintptr_t)d_dst & (f.bitdepth > 8 ? 7 : 3)))
    return fail(ctx, XVCGPU_INVALID_ARGUMENT, "convert_to: ARGB destination alignment");
  {
    const xvcgpu_status st_ = ensure_stats(ctx, 2 * pic->h);
    if (st_ != XVCGPU_OK) return st_;
  }
  OutArgs a;
  memset(&a, 0, sizeof(a));
  a.np = cf == 0 ? 1 : 3;
  a.wide = dst_bd > 8;
  a.smax = (1 << dst_bd) - 1;
  a.dst = static_cast<uint8_t *>(d_dst);
  ExportArgs ex;  // the dithered shift planes, for the export carry kernels
  memset(&ex, 0, sizeof(ex));
  bool dither_rows = false;
  int carry_rows = 0, total_blocks = 0, max_rows = 0;
  size_t off = 0;
  for (int c = 0; c < a.np; c++) {
    OutPlane &q = a.p[c];
    const int sw = c ? display_width >> 1 : display_width;
    const int sh = c ? display_height >> 1 : display_height;
    q.src_c = c;
    q.dw = out_plane_w(f.width, cf, c);
    q.dh = out_plane_h(f.height, cf, c);
    q.iw = pic->v.c[c].w;
    q.ih = pic->v.c[c].h;
    q.dst_off = off;
    off += (size_t)q.dw * q.dh * (a.wide ? 2 : 1);
    // ConvertTo's plain path (same size, 4:2:0 or 4:0:0) is this branch for every plane
    if (q.dw == sw && q.dh == sh) {
      q.kind = kOutShift;
      if (dst_bd >= bd || (!a.wide && bd <= 8)) {
        q.mode = 0;
        q.shift = a.wide ? dst_bd - bd : 0;
      } else {
        q.mode = f.dither ? 2 : 1;
        q.shift = bd - dst_bd;
      }
      if (q.mode == 2) {
        dither_rows = true;
        q.row_base = carry_rows;
        ex.w[c] = q.dw;
        ex.h[c] = q.dh;
        ex.row_base[c] = carry_rows;
        ex.shift = q.shift;
        carry_rows += q.dh;
        max_rows = std::max(max_rows, q.dh);
      }
    } else if (c && q.dw == 2 * sw && q.dh == 2 * sh) {
      q.kind = kOutBilinear;
      q.shift = dst_bd - bd;
      if (q.shift == 1)
        return fail(ctx, XVCGPU_INVALID_ARGUMENT,
                    "convert_to: bilinear chroma at out = in bitdepth + 1 (undefined)");
      q.tile_rows = XVC_OUT_POINT_TR;
    } else {
      q.kind = kOutResample;
      q.scale_x = ((sw << 15) + (q.dw >> 1)) / q.dw;
      q.scale_y = ((sh << 15) + (q.dh >> 1)) / q.dh;
      q.filt_x = out_filter_from_scale(q.scale_x);
      q.filt_y = out_filter_from_scale(q.scale_y);
      q.shift_hor = std::max(bd - 10, 0);
      q.shift_ver = 12 - q.shift_hor + bd - dst_bd;
      q.tile_rows = out_resample_tile_rows(q.dh, q.scale_y);
    }
  }
  if (argb) {
    // one tile grid for the three components: the smallest tile height
    int tr = XVC_OUT_MAX_TR;
    bool filter = false;
    for (int c = 0; c < 3; c++) {
      if (a.p[c].kind == kOutShift) a.p[c].tile_rows = XVC_OUT_POINT_TR;
      filter |= a.p[c].kind == kOutResample;
      tr = std::min(tr, a.p[c].tile_rows);
    }
    for (int c = 0; c < 3; c++) {
      a.p[c].tile_rows = tr;
      a.p[c].tiles_x = (a.p[c].dw + XVC_OUT_TW - 1) / XVC_OUT_TW;
    }
    a.argb_wide = f.bitdepth > 8;
    a.argb_max = (1 << f.bitdepth) - 1;
    a.argb_shift = 10 + 12 - f.bitdepth;
    static const int kM[4][3][3] = {  // ConvertColorSpace kM: default (= 709), 601, 709, 2020
        {{1192, 0, 1877}, {1192, -223, -558}, {1192, 2212, 0}},
        {{1192, 0, 1671}, {1192, -410, -851}, {1192, 2112, 0}},
        {{1192, 0, 1877}, {1192, -223, -558}, {1192, 2212, 0}},
        {{1192, 0, 1758}, {1192, -196, -681}, {1192, 2243, 0}}};
    memcpy(a.m, kM[f.color_matrix], sizeof(a.m));
    const int blocks = a.p[0].tiles_x * ((a.p[0].dh + tr - 1) / tr);
    if (filter)
      hipLaunchKernelGGL(output_argb_kernel<true>, dim3(blocks), dim3(256), 0, ctx->stream,
                         pic->v, a);
    else
      hipLaunchKernelGGL(output_argb_kernel<false>, dim3(blocks), dim3(256), 0, ctx->stream,
                         pic->v, a);
    CHECK_LAUNCH(ctx, "output_argb");
    return XVCGPU_OK;
  }
  for (int c = 0; c < a.np; c++) {
    OutPlane &q = a.p[c];
    if (q.kind == kOutShift) {
      q.blocks = q.dh;
    } else {
      q.tiles_x = (q.dw + XVC_OUT_TW - 1) / XVC_OUT_TW;
      q.blocks = q.tiles_x * ((q.dh + q.tile_rows - 1) / q.tile_rows);
    }
    total_blocks += q.blocks;
  }
  uint32_t *row_words = ctx->d_stats + kStatsHistWords;  // 2 * pic->h rows >= carry_rows
  a.row_carry = row_words;
  if (dither_rows) {
    hipLaunchKernelGGL(export_row_sums_kernel, dim3(max_rows, 3), dim3(256), 0, ctx->stream,
                       pic->v, ex, row_words);
    hipLaunchKernelGGL(export_row_scan_kernel, dim3(3), dim3(256), 0, ctx->stream, ex,
                       row_words);
  }
  bool filter = false;
  for (int c = 0; c < a.np; c++) filter |= a.p[c].kind == kOutResample;
  if (filter)
    hipLaunchKernelGGL(output_planar_kernel<true>, dim3(total_blocks), dim3(256), 0,
                       ctx->stream, pic->v, a);
  else
    hipLaunchKernelGGL(output_planar_kernel<false>, dim3(total_blocks), dim3(256), 0,
                       ctx->stream, pic->v, a);
  CHECK_LAUNCH(ctx, "output_planar");
  return XVCGPU_OK;
}

xvcgpu_status xvcgpu_picture_crc(xvcgpu_ctx *ctx, const xvcgpu_picture *pic, int mode,
                                 uint8_t *d_hash) {
  if (!ctx || !pic || !d_hash || mode < 0 || mode > 1) return XVCGPU_INVALID_ARGUMENT;
  {  // the scratch is sized by the pictures created on THIS context; a picture of
     // another context (or a larger one) must not run into it
    const xvcgpu_status st_ = ensure_stats(ctx, 2 * pic->h);
    if (st_ != XVCGPU_OK) return st_;
  }
  static const CrcPow2 pow2 = [] {
    CrcPow2 t;
    uint32_t v = 2;  // x
    for (int i = 0; i < 48; i++) {
      t.v[i] = (uint16_t)v;
      v = crc_mulmod(v, v);
    }
    return t;
  }();
  CrcArgs a;
  a.pow2 = pow2;
  a.wide = pic->bd > 8;
  a.mode = mode;
  if (!ctx->d_crc_tables) {
    static CrcTables host[2];
    crc_build_tables(host[0], pow2, 0);
    crc_build_tables(host[1], pow2, 1);
    hipError_t e = hipMalloc(&ctx->d_crc_tables, sizeof(host));
    if (e != hipSuccess) return fail(ctx, XVCGPU_OUT_OF_MEMORY, "hipMalloc", e);
    HIP_TRY(ctx, hipMemcpy(ctx->d_crc_tables, host, sizeof(host), hipMemcpyHostToDevice));
  }
  // one word per workgroup and plane in the row scratch (3 * ceil(h / 4) <= 2 * h)
  uint32_t *words = ctx->d_stats + kStatsHistWords;
  const int n_wg = (pic->h + 3) / 4;
  hipLaunchKernelGGL(crc_rows_kernel, dim3(n_wg, 3), dim3(256), 0, ctx->stream, pic->v, a,
                     ctx->d_crc_tables + a.wide, words);
  hipLaunchKernelGGL(crc_finish_kernel, dim3(1), dim3(256), 0, ctx->stream, pic->v, mode,
                     n_wg, words, d_hash);
  CHECK_LAUNCH(ctx, "picture_crc");
  return XVCGPU_OK;
}

xvcgpu_status xvcgpu_variance_map(xvcgpu_ctx *ctx, const xvcgpu_picture *pic,
                                  uint64_t *d_var16, int ctu_size, uint64_t *d_ctu_var) {
  if (!ctx || !pic || !d_var16) return XVCGPU_INVALID_ARGUMENT;
  if (d_ctu_var && ctu_size != 16 && ctu_size != 32 && ctu_size != 64 && ctu_size != 128)
    return fail(ctx, XVCGPU_INVALID_ARGUMENT, "variance_map: ctu size");
  const int bw = (pic->w + 15) / 16, bh = (pic->h + 15) / 16;
  hipLaunchKernelGGL(variance_map_kernel, dim3((bw * bh + 3) / 4), dim3(256), 0,
                     ctx->stream, pic->v.c[0], bw, bw * bh,
                     reinterpret_cast<unsigned long long *>(d_var16));
  if (d_ctu_var) {
    const int n = ((pic->w + ctu_size - 1) / ctu_size) * ((pic->h + ctu_size - 1) / ctu_size);
    hipLaunchKernelGGL(ctu_variance_kernel, dim3((n + 255) / 256), dim3(256), 0, ctx->stream,
                       reinterpret_cast<const unsigned long long *>(d_var16), pic->w, pic->h,
                       ctu_size, reinterpret_cast<unsigned long long *>(d_ctu_var));
  }
  CHECK_LAUNCH(ctx, "variance_map");
  return XVCGPU_OK;
}

xvcgpu_status xvcgpu_histogram_distance(xvcgpu_ctx *ctx, const xvcgpu_picture *a,
                                        const xvcgpu_picture *b, int64_t *d_out) {
  if (!ctx || !a || !b || !d_out) return XVCGPU_INVALID_ARGUMENT;
  {  // the scratch is sized by the pictures created on THIS context; a picture of
     // another context (or a larger one) must not run into it
    const xvcgpu_status st_ = ensure_stats(ctx, 2 * a->h);
    if (st_ != XVCGPU_OK) return st_;
  }
  if (a->w != b->w || a->h != b->h || a->bd != b->bd || a->bd > 12)
    return fail(ctx, XVCGPU_INVALID_ARGUMENT, "picture mismatch");
  const int buckets = 1 << a->bd;
  const int rows_per_wg = (a->h + 511) / 512;
  const int n_wg = (a->h + rows_per_wg - 1) / rows_per_wg;
  int *hist = reinterpret_cast<int *>(ctx->d_stats);
  hipLaunchKernelGGL(histogram_diff_kernel, dim3(n_wg), dim3(256), sizeof(int) * buckets,
                     ctx->stream, a->v.c[0], b->v.c[0], buckets, rows_per_wg, hist);
  hipLaunchKernelGGL(histogram_abs_sum_kernel, dim3(1), dim3(256), 0, ctx->stream, hist,
                     buckets, reinterpret_cast<long long *>(d_out));
  CHECK_LAUNCH(ctx, "histogram_distance");
  return XVCGPU_OK;
}


/* ---- intra prediction / SATD mode pre-selection (k_intra.h) ---- */
xvcgpu_status xvcgpu_intra_pred_batch(xvcgpu_ctx *ctx, const xvcgpu_picture *rec,
                                      xvcgpu_picture *pred,
                                      const xvcgpu_intra_block *d_jobs, int n) {
  if (!ctx || !rec || !pred || (!d_jobs && n > 0) || n < 0) return XVCGPU_INVALID_ARGUMENT;
  if (rec->w != pred->w || rec->h != pred->h || rec->bd != pred->bd)
    return fail(ctx, XVCGPU_INVALID_ARGUMENT, "picture mismatch");
  if (n == 0) return XVCGPU_OK;
  hipLaunchKernelGGL(intra_pred_kernel, dim3(n), dim3(256), 0, ctx->stream, rec->v, pred->v,
                     d_jobs, n);
  CHECK_LAUNCH(ctx, "intra_pred_batch");
  return XVCGPU_OK;
}

#ifndef XVCGPU_INTRA_WAVES_GRID
#define XVCGPU_INTRA_WAVES_GRID 128
#endif
xvcgpu_status xvcgpu_intra_recon_waves(xvcgpu_ctx *ctx, xvcgpu_picture *rec,
                                       xvcgpu_picture *pred,
                                       const xvcgpu_intra_block *d_jobs,
                                       const xvcgpu_tx_block *d_blocks,
                                       const int32_t *d_wave_first, int n_waves,
                                       const int16_t *d_levels,
                                       const uint32_t *d_level_offsets,
                                       const int32_t *d_nnz) {
  if (!ctx || !rec || !pred || n_waves < 0 ||
      (n_waves && (!d_jobs || !d_blocks || !d_wave_first || !d_levels || !d_level_offsets ||
                   !d_nnz)))
    return XVCGPU_INVALID_ARGUMENT;
  if (rec->w != pred->w || rec->h != pred->h || rec->bd != pred->bd)
    return fail(ctx, XVCGPU_INVALID_ARGUMENT, "picture mismatch");
  if (n_waves == 0) return XVCGPU_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  // a wave of a 1080p picture holds a few dozen jobs: a fraction of the chip's
  // workgroup slots is enough (all of them must be resident together)
  int &grid = ctx->intra_waves_grid;   // 0: not asked yet, < 0: refused
  if (grid == 0) {
    int per_cu = 0, cus = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, intra_waves_kernel, 256, 0) !=
            hipSuccess ||
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device) !=
            hipSuccess ||
        per_cu < 1 || cus < 1)
      grid = -1;
    else
      grid = cus * per_cu < XVCGPU_INTRA_WAVES_GRID ? cus * per_cu : XVCGPU_INTRA_WAVES_GRID;
  }
  if (grid < 0) return XVCGPU_UNSUPPORTED;
  // the waves' counters
  if (ctx->intra_done_cap < n_waves) {   // (grown with headroom for the next picture)
    const xvcgpu_status st =
        grow_scratch(ctx, &ctx->d_intra_done, &ctx->intra_done_cap, n_waves + 256,
                     sizeof(int) * (size_t)(n_waves + 256), false, "intra wave counters");
    if (st != XVCGPU_OK) return st;
  }
  HIP_TRY(ctx, hipMemsetAsync(ctx->d_intra_done, 0, sizeof(int) * (size_t)n_waves, ctx->stream));
  int *done = ctx->d_intra_done;
  PicView rv = rec->v, pv = pred->v;
  int16_t *lv = const_cast<int16_t *>(d_levels);
  int32_t *nz = const_cast<int32_t *>(d_nnz);
  const int16_t *tables = ctx->d_tx_tables;
  TxTableLayout lay = xvcgpu_tx_layout();
  void *args[] = {&rv, &pv, &d_jobs, &d_blocks, &d_wave_first, &n_waves, &lv, &d_level_offsets,
                  &nz, &tables, &lay, &done};
  if (hipLaunchCooperativeKernel(reinterpret_cast<const void *>(intra_waves_kernel), dim3(grid),
                                 dim3(256), args, 0, ctx->stream) != hipSuccess) {
    (void)hipGetLastError();
    return XVCGPU_UNSUPPORTED;
  }
  CHECK_LAUNCH(ctx, "intra_recon_waves");
  return XVCGPU_OK;
}

xvcgpu_status xvcgpu_intra_satd_batch(xvcgpu_ctx *ctx, const xvcgpu_picture *orig,
                                      const xvcgpu_picture *rec,
                                      const xvcgpu_intra_block *d_jobs, int n,
                                      uint32_t *d_dist, int max_block_size) {
  if (!ctx || !orig || !rec || (!d_jobs && n > 0) || n < 0 || (!d_dist && n > 0) ||
      max_block_size < 4 || max_block_size > 64)
    return XVCGPU_INVALID_ARGUMENT;
  if (rec->w != orig->w || rec->h != orig->h || rec->bd != orig->bd)
    return fail(ctx, XVCGPU_INVALID_ARGUMENT, "picture mismatch");
  if (n == 0) return XVCGPU_OK;
  // workgroups per job: enough to put ~2 workgroups on every CU, at most one
  // mode per wave (67 modes / 4 waves -> 17)
  int split = (2 * 256 + n - 1) / n;
  split = split < 1 ? 1 : (split > 17 ? 17 : split);
  const dim3 grid(n, split);
  if (max_block_size <= 16)
    hipLaunchKernelGGL(intra_satd_kernel<16>, grid, dim3(256), 0, ctx->stream, orig->v,
                       rec->v, d_jobs, n, d_dist);
  else if (max_block_size <= 32)
    hipLaunchKernelGGL(intra_satd_kernel<32>, grid, dim3(256), 0, ctx->stream, orig->v,
                       rec->v, d_jobs, n, d_dist);
  else
    hipLaunchKernelGGL(intra_satd_kernel<64>, grid, dim3(256), 0, ctx->stream, orig->v,
                       rec->v, d_jobs, n, d_dist);
  CHECK_LAUNCH(ctx, "intra_satd_batch");
  return XVCGPU_OK;
}

xvcgpu_status xvcgpu_intra_recon_batch(xvcgpu_ctx *ctx, const xvcgpu_picture *orig,
                                       xvcgpu_picture *rec,
                                       const xvcgpu_intra_block *d_jobs,
                                       const xvcgpu_tx_block *d_blocks, int n,
                                       int16_t *d_levels, const uint32_t *d_level_offsets,
                                       int32_t *d_nnz) {
  if (!ctx || !rec || n < 0 || (n && (!d_jobs || !d_blocks))) return XVCGPU_INVALID_ARGUMENT;
  // decoder form (no original): the levels are an input and must be there
  if (!orig && n && (!d_levels || !d_level_offsets || !d_nnz)) return XVCGPU_INVALID_ARGUMENT;
  if (orig && (orig->w != rec->w || orig->h != rec->h || orig->bd != rec->bd))
    return fail(ctx, XVCGPU_INVALID_ARGUMENT, "picture mismatch");
  if (n == 0) return XVCGPU_OK;
  const dim3 grid((n + TX2_WAVES - 1) / TX2_WAVES), block(64 * TX2_WAVES);
  if (orig)
    hipLaunchKernelGGL(intra_recon_wave_kernel<TX_MODE_FULL>, grid, block, 0, ctx->stream,
                       orig->v, rec->v, d_jobs, d_blocks, n, d_levels, d_level_offsets, d_nnz,
                       ctx->d_tx_tables, ctx->d_tx_tables_t, xvcgpu_tx_layout());
  else
    hipLaunchKernelGGL(intra_recon_wave_kernel<TX_MODE_INV>, grid, block, 0, ctx->stream,
                       rec->v, rec->v, d_jobs, d_blocks, n, d_levels, d_level_offsets, d_nnz,
                       ctx->d_tx_tables, ctx->d_tx_tables_t, xvcgpu_tx_layout());
  CHECK_LAUNCH(ctx, "intra_recon_batch");
  return XVCGPU_OK;
}

xvcgpu_status xvcgpu_intra_select_modes(xvcgpu_ctx *ctx, const uint32_t *d_dist,
                                        const uint32_t *d_mode_cost, int n,
                                        int32_t *d_modes, xvcgpu_intra_block *d_jobs,
                                        xvcgpu_tx_block *d_blocks, int per_cu) {
  if (!ctx || n < 0 || (n && !d_dist) || per_cu < 0 || per_cu > 3 ||
      ((d_jobs || d_blocks) && per_cu == 0))
    return XVCGPU_INVALID_ARGUMENT;
  if (n == 0) return XVCGPU_OK;
  hipLaunchKernelGGL(intra_select_kernel, dim3((n + 3) / 4), dim3(256), 0, ctx->stream,
                     d_dist, d_mode_cost, n, d_modes, d_jobs, d_blocks, per_cu);
  CHECK_LAUNCH(ctx, "intra_select_modes");
  return XVCGPU_OK;
}

/* ---- a picture per call ---- */
static const int kFramePassAll =
    XVC_FP_ENCODE | XVC_FP_DEBLOCK_V | XVC_FP_DEBLOCK_H | XVC_FP_PAD | XVC_FP_SSD;

// What a call runs (frame_pass_resolve): form 0 = no search, nothing behind it; fused_tail:
// the form reconstructs into scratch_rec and one launch ends the pass; tail_on_hi: inverse
// transform and that launch on ctx->hi_stream
struct FramePassForm {
  int form;
  bool fused_tail, tail_on_hi;
};

// The form the caller names checked against what it can run (the table in xvcgpu.h): every
// refusal names the field and happens here, before anything is enqueued.  plan: null = none
static xvcgpu_status frame_pass_resolve(xvcgpu_ctx *ctx, const xvcgpu_frame_pass_args *a,
                                        int phases, const xvcgpu_me_plan *plan,
                                        FramePassForm *r) {
  if (!ctx || !a || !a->rec) return XVCGPU_INVALID_ARGUMENT;
  // All phases over a whole picture of a size the fused tail (k_tail.h) covers, with its
  // scratch picture: the pass can end with that one launch instead of five.  (It covers CUs
  // without a side of 4: a plan that holds one makes the pass end with the separate launches)
  const bool whole = a->scratch_rec && (phases & kFramePassAll) == kFramePassAll &&
                     a->n_cus > 0 && a->n_cus == a->n_cus_total && a->db_y_begin == 0 &&
                     a->db_y_end >= a->rec->h && a->dbh_y_end >= a->rec->h &&
                     a->ssd_y_begin == 0 && a->ssd_y_end >= a->rec->h &&
                     !(a->rec->w & 7) && !(a->rec->h & 7);
  *r = {0, whole && !(plan && plan->n_small() > 0), false};
  if (!(phases & XVC_FP_ENCODE) || a->n_cus <= 0) return XVCGPU_OK;
  const int form = a->form;
#define FP_NEED(cond, what) \
  if (!(cond)) return fail(ctx, XVCGPU_INVALID_ARGUMENT, "frame_pass: " what)
  FP_NEED(form >= XVC_FP_FORM_RECON_FROM_ME && form <= XVC_FP_FORM_RESIDUAL_RDOQ,
          "form is not one of XVC_FP_FORM_*");
  FP_NEED(a->orig && a->ref && a->d_me && a->d_results, "orig, ref, d_me and d_results");
  const bool rdoq = a->d_rdoq_params != nullptr;
  FP_NEED(!rdoq || a->d_rdoq_contexts, "d_rdoq_params without d_rdoq_contexts");
  if (form == XVC_FP_FORM_RECON_FROM_ME || form == XVC_FP_FORM_FWD_FROM_ME) {
    // the kernels that take a CU whole hold CUs of 8 ... 16 samples a side; the plan
    // knows whether every job is one
    FP_NEED(a->max_block_size <= 16, "this form needs max_block_size <= 16");
    FP_NEED(!(plan && plan->n_small() > 0), "this form needs a plan without a CU side below 8");
  } else {   // the prediction picture and the residual pipeline behind it
    FP_NEED(a->pred && a->d_luma_tx_index, "this form needs pred and d_luma_tx_index");
  }
  if (form != XVC_FP_FORM_RECON_FROM_ME)
    FP_NEED(a->d_tx && a->d_nnz && a->d_cus_own, "this form needs d_tx, d_nnz and d_cus_own");
  if (form == XVC_FP_FORM_FWD_FROM_ME || form == XVC_FP_FORM_FWD_TRANSFORM) {
    FP_NEED(rdoq, "this form needs d_rdoq_params and d_rdoq_contexts");
    FP_NEED(a->d_coeffs && a->d_levels && a->d_level_off,
            "this form needs d_coeffs, d_levels and d_level_off");
  }
  if (form == XVC_FP_FORM_FWD_FROM_ME)   // transform blocks in CU order: 3 * cu + comp
    FP_NEED(a->n_tx == 3 * a->n_cus, "fwd_from_me needs n_tx == 3 * n_cus");
  if (form == XVC_FP_FORM_RESIDUAL) FP_NEED(!rdoq, "residual is QuantFast: no d_rdoq_params");
  if (form == XVC_FP_FORM_RESIDUAL_RDOQ) FP_NEED(rdoq, "residual_rdoq needs d_rdoq_params");
#undef FP_NEED
  r->form = form;
  // the rest of the pass - inverse transform and the fused tail, two short kernels - on the
  // high-priority stream: beside other pictures' searches (long-lived waves on every CU)
  // their workgroups otherwise wait for slots many times their own duration
  // (profiles/r03_bench_4320p_kernel_stats.csv: the tail 2152 us in flight against 118 alone)
  r->tail_on_hi = ctx->hi_stream && r->fused_tail && form == XVC_FP_FORM_FWD_FROM_ME;
  return XVCGPU_OK;
}

// The forms; rec: where the unfiltered reconstruction goes
static xvcgpu_status fp_recon_from_me(xvcgpu_ctx *ctx, const xvcgpu_frame_pass_args *a,
                                      xvcgpu_picture *rec) {
  if (a->d_rdoq_params)
    return xvcgpu_recon_from_me_rdoq(ctx, a->orig, a->ref, rec, a->d_me, a->d_results, a->n_cus,
                                     a->qp_y, a->qp_c, 0, a->ref_poc, a->d_nnz, a->d_cus_own,
                                     a->d_rdoq_contexts, a->d_rdoq_params);
  return xvcgpu_recon_from_me(ctx, a->orig, a->ref, rec, a->d_me, a->d_results, a->n_cus,
                              a->qp_y, a->qp_c, 0, a->ref_poc, a->d_nnz, a->d_cus_own);
}

// the packed quantiser; the caller's word about its blocks holds for this call's batch
static xvcgpu_status fp_quant_rdo(xvcgpu_ctx *ctx, const xvcgpu_frame_pass_args *a,
                                  bool classified) {
  return quant_rdo_launch(ctx, a->rec->bd, a->d_tx, a->n_tx, a->d_coeffs, a->d_level_off,
                          a->n_coeffs, a->d_levels, a->d_nnz, a->d_rdoq_contexts,
                          a->d_rdoq_params, classified,
                          ctx->rdoq_four_lane_only || a->tx_four_lane_only,
                          classified ? a->d_cus_own : nullptr);
}

// Prediction + forward transform in one kernel: the prediction goes straight into the
// reconstruction's picture (the inverse half then works in place and skips the blocks
// without levels), the kernel classifies the blocks for the quantiser on the way, proves
// the blocks it can all zero (k_rdoq.h) and writes the CU records.  *main_stream: set
// where the pass goes on on ctx->hi_stream
static xvcgpu_status fp_fwd_from_me(xvcgpu_ctx *ctx, const xvcgpu_frame_pass_args *a,
                                    xvcgpu_picture *rec, bool tail_on_hi,
                                    hipStream_t *main_stream) {
  xvcgpu_status st = xvcgpu_fwd_from_me_classify_prove(
      ctx, a->orig, a->ref, rec, a->d_me, a->d_results, a->n_cus, a->qp_y, a->qp_c, a->ref_poc,
      a->d_coeffs, a->d_level_off, a->n_coeffs, a->d_levels, a->d_nnz, a->d_cus_own,
      a->d_rdoq_contexts, a->d_rdoq_params);
  if (st == XVCGPU_OK) st = fp_quant_rdo(ctx, a, true);
  if (st != XVCGPU_OK) return st;
  if (tail_on_hi) {
    HIP_TRY(ctx, hipEventRecord(ctx->ev_hi_in, ctx->stream));
    HIP_TRY(ctx, hipStreamWaitEvent(ctx->hi_stream, ctx->ev_hi_in, 0));
    *main_stream = ctx->stream;
    ctx->stream = ctx->hi_stream;
  }
  // blocks 3 * cu + comp, CUs up to 16x16: the U and V blocks of a CU share a wave
  return xvcgpu_inv_transform_cu_order(ctx, rec, a->d_tx, a->n_cus, a->d_levels,
                                       a->d_level_off, a->d_nnz);
}

// The form's residual pipeline behind a prediction picture, over the transform blocks: whole
// with QuantFast or RDOQ, or split around the packed quantiser
static xvcgpu_status fp_residual(xvcgpu_ctx *ctx, const xvcgpu_frame_pass_args *a,
                                 xvcgpu_picture *rec, int form) {
  if (form == XVC_FP_FORM_RESIDUAL)
    return xvcgpu_residual_batch(ctx, a->orig, a->pred, rec, a->d_tx, a->n_tx, a->d_levels,
                                 a->d_level_off, a->d_nnz);
  if (form == XVC_FP_FORM_RESIDUAL_RDOQ)
    return xvcgpu_residual_rdoq_batch(ctx, a->orig, a->pred, rec, a->d_tx, a->n_tx, a->d_levels,
                                      a->d_level_off, a->d_nnz, a->d_rdoq_contexts,
                                      a->d_rdoq_params);
  xvcgpu_status st = xvcgpu_fwd_transform_batch(ctx, a->orig, a->pred, a->d_tx, a->n_tx,
                                                a->d_coeffs, a->d_level_off);
  if (st == XVCGPU_OK) st = fp_quant_rdo(ctx, a, false);
  if (st == XVCGPU_OK)
    st = xvcgpu_inv_transform_batch(ctx, a->pred, rec, a->d_tx, a->n_tx, a->d_levels,
                                    a->d_level_off, a->d_nnz);
  return st;
}

// CUs of any size: the prediction picture, the form's residual pipeline, the CU records
static xvcgpu_status fp_from_pred(xvcgpu_ctx *ctx, const xvcgpu_frame_pass_args *a,
                                  xvcgpu_picture *rec, int form) {
  xvcgpu_status st = xvcgpu_mc_from_me(ctx, a->ref, a->pred, a->d_me, a->d_results, a->n_cus);
  if (st == XVCGPU_OK) st = fp_residual(ctx, a, rec, form);
  if (st != XVCGPU_OK) return st;
  return xvcgpu_cu_info_from_me(ctx, a->d_me, a->d_results, a->d_nnz, a->d_luma_tx_index,
                                a->n_cus, a->qp_y, a->qp_c, a->ref_poc, a->d_cus_own);
}

// How a pass ends: the fused tail's one launch from scratch_rec, or the phases' separate
// launches.  pic_is_bipred: the deblocking filter's word for a B picture
static xvcgpu_status fp_tail(xvcgpu_ctx *ctx, const xvcgpu_frame_pass_args *a, int phases,
                             bool fused_tail, int pic_is_bipred) {
  if (fused_tail)
    return xvcgpu_deblock_pad_ssd(ctx, a->scratch_rec, a->rec, a->orig, a->d_cus, a->n_cus_total,
                                  a->d_cu_map, a->map_stride, pic_is_bipred, 0, 0,
                                  a->shift_bitdepth, a->d_ssd);
  xvcgpu_status st = XVCGPU_OK;
  if (phases & XVC_FP_DEBLOCK_V)
    st = xvcgpu_deblock_rows(ctx, a->rec, a->d_cus, a->n_cus_total, a->d_cu_map, a->map_stride,
                             pic_is_bipred, 0, 0, 4, 0, a->db_y_begin, a->db_y_end);
  if (st == XVCGPU_OK && (phases & XVC_FP_DEBLOCK_H))
    st = xvcgpu_deblock_rows(ctx, a->rec, a->d_cus, a->n_cus_total, a->d_cu_map, a->map_stride,
                             pic_is_bipred, 0, 0, 4, 1, a->db_y_begin, a->dbh_y_end);
  if (st == XVCGPU_OK && (phases & XVC_FP_PAD)) st = xvcgpu_pad_border(ctx, a->rec);
  if (st == XVCGPU_OK && (phases & XVC_FP_SSD))
    st = xvcgpu_picture_ssd_rows(ctx, a->orig, a->rec, 0, a->shift_bitdepth, a->ssd_y_begin,
                                 a->ssd_y_end, a->d_ssd);
  return st;
}

// One list's search of the pass, through its plan or sized.  The pass's jobs are the CUs of
// its grid: where the caller's shape word says that they are (almost) all 16x16 (16x8 in the
// bottom row of a 1080-line picture) the search's exact-shape kernel (a pass of smaller CUs
// must not take it: its jobs would all be left to the few waves of the leftover kernel)
static xvcgpu_status fp_search(xvcgpu_ctx *ctx, const xvcgpu_frame_pass_args *a,
                               const xvcgpu_picture *ref, const xvcgpu_me_block *d_me,
                               xvcgpu_me_result *d_results, const xvcgpu_me_plan *plan) {
  const int flags = XVCGPU_ME_FULLPEL | XVCGPU_ME_SUBPEL;
  if (plan) return xvcgpu_me_search_planned(ctx, a->orig, ref, flags, plan, d_results);
  return xvcgpu_me_search_sized(
      ctx, a->orig, ref, flags | (a->me_shape & (XVCGPU_ME_HINT_SQ16 | XVCGPU_ME_ONLY_SQ16)),
      d_me, a->n_cus, d_results, a->max_block_size);
}

/* ---- adaptive QP (k_aqp.h) ---- */
static xvcgpu_status aqp_apply_launch(xvcgpu_ctx *ctx, const xvcgpu_aqp_table *t,
                                      const uint64_t *d_ctu_var, int n_ctus,
                                      xvcgpu_me_block *const *d_me, int n_me,
                                      xvcgpu_tx_block *d_tx, xvcgpu_rdoq_params *d_rdoq_params,
                                      const int32_t *d_luma_tx_index, int n_cus, int8_t *d_cu_qp,
                                      int8_t *d_ctu_dqp) {
  if (!ctx || !t || n_cus < 0 || n_me < 1 || n_me > 2 * XVC_CS_MAX_REFS || !d_me)
    return XVCGPU_INVALID_ARGUMENT;
  if (t->ctu_size != 16 && t->ctu_size != 32 && t->ctu_size != 64 && t->ctu_size != 128)
    return fail(ctx, XVCGPU_INVALID_ARGUMENT, "aqp_apply: ctu_size");
  if (t->ctus_per_row < 1) return fail(ctx, XVCGPU_INVALID_ARGUMENT, "aqp_apply: ctus_per_row");
  AqpMeArrays me = {};
  for (int k = 0; k < n_me; k++) {
    if (!d_me[k]) return fail(ctx, XVCGPU_INVALID_ARGUMENT, "aqp_apply: d_me");
    me.p[k] = d_me[k];
  }
  if (n_cus && (!d_ctu_var || !d_tx || !d_luma_tx_index || !d_cu_qp))
    return fail(ctx, XVCGPU_INVALID_ARGUMENT,
                "aqp_apply: d_ctu_var, d_tx, d_luma_tx_index and d_cu_qp");
  if (n_cus == 0) return XVCGPU_OK;
  hipLaunchKernelGGL(aqp_apply_kernel, dim3((n_cus + 255) / 256), dim3(256), 0, ctx->stream, *t,
                     reinterpret_cast<const unsigned long long *>(d_ctu_var), n_ctus, me, n_me,
                     d_tx, d_rdoq_params, d_luma_tx_index, n_cus, d_cu_qp, d_ctu_dqp);
  CHECK_LAUNCH(ctx, "aqp_apply");
  return XVCGPU_OK;
}

xvcgpu_status xvcgpu_aqp_apply(xvcgpu_ctx *ctx, const xvcgpu_aqp_table *table,
                               const uint64_t *d_ctu_var, xvcgpu_me_block *const *d_me,
                               int n_me, xvcgpu_tx_block *d_tx,
                               xvcgpu_rdoq_params *d_rdoq_params,
                               const int32_t *d_luma_tx_index, int n_cus, int8_t *d_cu_qp,
                               int8_t *d_ctu_dqp) {
  // (the caller's word that the jobs lie inside the picture of d_ctu_var: no clamp)
  return aqp_apply_launch(ctx, table, d_ctu_var, 0x7fffffff, d_me, n_me, d_tx, d_rdoq_params,
                          d_luma_tx_index, n_cus, d_cu_qp, d_ctu_dqp);
}

xvcgpu_status xvcgpu_cu_info_set_qp(xvcgpu_ctx *ctx, xvcgpu_cu_info *d_cus_own,
                                    const int8_t *d_cu_qp, int n) {
  if (!ctx || n < 0 || (n && (!d_cus_own || !d_cu_qp))) return XVCGPU_INVALID_ARGUMENT;
  if (n == 0) return XVCGPU_OK;
  hipLaunchKernelGGL(cu_info_set_qp_kernel, dim3((n + 255) / 256), dim3(256), 0, ctx->stream,
                     d_cus_own, d_cu_qp, n);
  CHECK_LAUNCH(ctx, "cu_info_set_qp");
  return XVCGPU_OK;
}

// What an adaptive-QP pass asks beyond the flat pass's checks (frame_pass_resolve ran:
// a, a->rec are there and, with a form, a->orig): every refusal names its field, nothing
// is enqueued
static xvcgpu_status fp_aqp_check(xvcgpu_ctx *ctx, const xvcgpu_frame_pass_args *a,
                                  const xvcgpu_aqp_args *q, int phases) {
#define FPQ_NEED(cond, what) \
  if (!(cond)) return fail(ctx, XVCGPU_INVALID_ARGUMENT, "frame_pass_aqp: " what)
  FPQ_NEED(phases & XVC_FP_ENCODE, "phases: the QP map is applied in front of XVC_FP_ENCODE");
  FPQ_NEED(a->n_cus == a->n_cus_total && a->db_y_begin == 0 && a->db_y_end >= a->rec->h &&
               a->dbh_y_end >= a->rec->h && a->ssd_y_begin == 0 && a->ssd_y_end >= a->rec->h,
           "whole pictures only (no row shard)");
  if (a->n_cus <= 0) return XVCGPU_OK;
  FPQ_NEED(a->form == XVC_FP_FORM_FWD_TRANSFORM || a->form == XVC_FP_FORM_RESIDUAL ||
               a->form == XVC_FP_FORM_RESIDUAL_RDOQ,
           "the form must be one with a prediction picture and d_tx: FWD_TRANSFORM, RESIDUAL "
           "or RESIDUAL_RDOQ");
  FPQ_NEED(q->d_var16 && q->d_ctu_var && q->d_cu_qp, "d_var16, d_ctu_var and d_cu_qp");
  const int cs = q->table.ctu_size;
  FPQ_NEED(cs == 16 || cs == 32 || cs == 64 || cs == 128, "table.ctu_size");
  FPQ_NEED(q->table.ctus_per_row == (a->orig->w + cs - 1) / cs,
           "table.ctus_per_row does not fit the width of orig");
#undef FPQ_NEED
  return XVCGPU_OK;
}

// In front of the search: the CTU statistic of orig, then the QP map into the job arrays
static xvcgpu_status fp_aqp_front(xvcgpu_ctx *ctx, const xvcgpu_frame_pass_args *a,
                                  const xvcgpu_aqp_args *q, xvcgpu_me_block *const *d_me,
                                  int n_me) {
  const int cs = q->table.ctu_size;
  xvcgpu_status st = xvcgpu_variance_map(ctx, a->orig, q->d_var16, cs, q->d_ctu_var);
  if (st != XVCGPU_OK) return st;
  // (the job arrays are device memory of the caller's; the block says const for the flat pass)
  return aqp_apply_launch(ctx, &q->table, q->d_ctu_var,
                          q->table.ctus_per_row * ((a->orig->h + cs - 1) / cs), d_me, n_me,
                          const_cast<xvcgpu_tx_block *>(a->d_tx),
                          const_cast<xvcgpu_rdoq_params *>(a->d_rdoq_params), a->d_luma_tx_index,
                          a->n_cus, q->d_cu_qp, q->d_ctu_dqp);
}

// resolve, search, the form's launches, tail.  plan: null = xvcgpu_frame_pass; q: null = one
// QP, else xvcgpu_frame_pass_aqp: the QP map in front of the search, the records' QPs
// corrected in front of the tail
static xvcgpu_status frame_pass_impl(xvcgpu_ctx *ctx, const xvcgpu_frame_pass_args *a,
                                     int phases, const xvcgpu_me_plan *plan,
                                     const xvcgpu_aqp_args *q) {
  FramePassForm r;
  xvcgpu_status st = frame_pass_resolve(ctx, a, phases, plan, &r);
  if (st == XVCGPU_OK && q) st = fp_aqp_check(ctx, a, q, phases);
  if (st != XVCGPU_OK) return st;
  xvcgpu_picture *const rec = r.fused_tail ? a->scratch_rec : a->rec;
  hipStream_t main_stream = nullptr;   // set while the pass runs on ctx->hi_stream
  if (r.form) {
    if (q) {
      xvcgpu_me_block *const jobs[1] = {const_cast<xvcgpu_me_block *>(a->d_me)};
      st = fp_aqp_front(ctx, a, q, jobs, 1);
      if (st != XVCGPU_OK) return st;
    }
    st = fp_search(ctx, a, a->ref, a->d_me, a->d_results, plan);
    if (st != XVCGPU_OK) return st;   // (nothing behind a search that was refused)
    switch (r.form) {
      case XVC_FP_FORM_RECON_FROM_ME: st = fp_recon_from_me(ctx, a, rec); break;
      case XVC_FP_FORM_FWD_FROM_ME:
        st = fp_fwd_from_me(ctx, a, rec, r.tail_on_hi, &main_stream);
        break;
      default: st = fp_from_pred(ctx, a, rec, r.form); break;
    }
    if (st == XVCGPU_OK && q) st = xvcgpu_cu_info_set_qp(ctx, a->d_cus_own, q->d_cu_qp, a->n_cus);
  }
  if (st == XVCGPU_OK) st = fp_tail(ctx, a, phases, r.fused_tail, 0);
  if (main_stream) {   // every way out: the chain continues on its own stream, after the tail
    hipEventRecord(ctx->ev_hi_out, ctx->hi_stream);
    ctx->stream = main_stream;
    hipStreamWaitEvent(ctx->stream, ctx->ev_hi_out, 0);
  }
  return st;
}

xvcgpu_status xvcgpu_frame_pass(xvcgpu_ctx *ctx, const xvcgpu_frame_pass_args *a,
                                int phases) {
  return frame_pass_impl(ctx, a, phases, nullptr, nullptr);
}

// what a plan must be to serve a->d_me's search
static xvcgpu_status fp_plan_check(xvcgpu_ctx *ctx, const xvcgpu_frame_pass_args *a,
                                   const xvcgpu_me_plan *plan) {
  if (!ctx || !a || !plan || plan->n != a->n_cus || plan->d_blocks != a->d_me)
    return XVCGPU_INVALID_ARGUMENT;
  // (a plan of a smaller class would answer this pass's larger CUs as unsupported)
  if (plan->max_launched != me_class_of(a->max_block_size))
    return fail(ctx, XVCGPU_INVALID_ARGUMENT,
                "frame_pass_planned: the plan was made for another max_block_size class");
  return XVCGPU_OK;
}

xvcgpu_status xvcgpu_frame_pass_planned(xvcgpu_ctx *ctx, const xvcgpu_frame_pass_args *a,
                                        const xvcgpu_me_plan *plan, int phases) {
  const xvcgpu_status st = fp_plan_check(ctx, a, plan);
  return st != XVCGPU_OK ? st : frame_pass_impl(ctx, a, phases, plan, nullptr);
}

xvcgpu_status xvcgpu_frame_pass_aqp(xvcgpu_ctx *ctx, const xvcgpu_frame_pass_args *a,
                                    const xvcgpu_aqp_args *q, const xvcgpu_me_plan *plan,
                                    int phases) {
  if (!q) return XVCGPU_INVALID_ARGUMENT;
  const xvcgpu_status st = plan ? fp_plan_check(ctx, a, plan) : XVCGPU_OK;
  return st != XVCGPU_OK ? st : frame_pass_impl(ctx, a, phases, plan, q);
}

/* ---- the P frame pass with affine motion (k_fp_affine.h) ---- */
xvcgpu_status xvcgpu_fp_affine_boot(xvcgpu_ctx *ctx, const xvcgpu_me_result *d_results,
                                    const int32_t *d_order, int n_listed, int pic_w,
                                    int pic_h, xvcgpu_affine_me_block *d_affine) {
  if (!ctx || n_listed < 0 || pic_w <= 0 || pic_h <= 0 ||
      (n_listed && (!d_results || !d_order || !d_affine)))
    return XVCGPU_INVALID_ARGUMENT;
  if (n_listed == 0) return XVCGPU_OK;
  // (the caller's word that the list names jobs of d_affine: no bound but int's)
  hipLaunchKernelGGL(fp_affine_boot_kernel, dim3((n_listed + 255) / 256), dim3(256), 0,
                     ctx->stream, d_results, d_order, n_listed, 0x7fffffff, pic_w, pic_h,
                     d_affine);
  CHECK_LAUNCH(ctx, "fp_affine_boot");
  return XVCGPU_OK;
}

xvcgpu_status xvcgpu_affine_me_listed(xvcgpu_ctx *ctx, const xvcgpu_picture *orig,
                                      const xvcgpu_picture *ref,
                                      const xvcgpu_affine_me_block *d_blocks, int n,
                                      const int32_t *d_order, const int32_t n_class[3],
                                      xvcgpu_affine_me_result *d_results) {
  if (!ctx || !orig || !ref || n < 0 || !n_class) return XVCGPU_INVALID_ARGUMENT;
  if (orig->v.bd != ref->v.bd || orig->v.c[0].w != ref->v.c[0].w ||
      orig->v.c[0].h != ref->v.c[0].h)
    return XVCGPU_INVALID_ARGUMENT;
  long long listed = 0;
  for (int k = 0; k < 3; k++) {
    if (n_class[k] < 0) return fail(ctx, XVCGPU_INVALID_ARGUMENT, "affine_me_listed: n_class");
    listed += n_class[k];
  }
  if (listed > n) return fail(ctx, XVCGPU_INVALID_ARGUMENT, "affine_me_listed: n_class names more jobs than n");
  if (listed && (!d_blocks || !d_order || !d_results)) return XVCGPU_INVALID_ARGUMENT;
  // one instance per CU height (a wave per 8 rows of the block), over its run of the list
  int first = 0;
#define AFF_LISTED(NW, K)                                                                  \
  if (n_class[K]) {                                                                        \
    hipLaunchKernelGGL(affine_me_listed_kernel<NW>, dim3(n_class[K]), dim3(64 * NW), 0,    \
                       ctx->stream, orig->v.c[0], ref->v.c[0], ref->v.bd, d_blocks, n,     \
                       d_order + first, n_class[K], d_results);                            \
    first += n_class[K];                                                                   \
  }
  AFF_LISTED(2, 0)
  AFF_LISTED(4, 1)
  AFF_LISTED(8, 2)
#undef AFF_LISTED
  CHECK_LAUNCH(ctx, "affine_me_listed");
  return XVCGPU_OK;
}

xvcgpu_status xvcgpu_fp_affine_choice(xvcgpu_ctx *ctx, const xvcgpu_me_block *d_me,
                                      const xvcgpu_me_result *d_results, int n_cus,
                                      const xvcgpu_frame_pass_affine_args *f) {
  if (!ctx || !f || n_cus < 0) return XVCGPU_INVALID_ARGUMENT;
  if (n_cus && (!d_me || !d_results)) return XVCGPU_INVALID_ARGUMENT;
  if (n_cus && (!f->d_affine || !f->d_affine_results || !f->d_choice || !f->d_inter))
    return fail(ctx, XVCGPU_INVALID_ARGUMENT,
                "fp_affine_choice: d_affine, d_affine_results, d_choice and d_inter");
  if (n_cus == 0) return XVCGPU_OK;
  hipLaunchKernelGGL(fp_affine_choice_kernel, dim3((n_cus + 255) / 256), dim3(256), 0,
                     ctx->stream, d_me, d_results, n_cus, f->d_affine, f->d_affine_results,
                     f->side_bits, f->d_choice, f->d_inter);
  CHECK_LAUNCH(ctx, "fp_affine_choice");
  return XVCGPU_OK;
}

xvcgpu_status xvcgpu_cu_info_from_affine_choice(
    xvcgpu_ctx *ctx, const xvcgpu_me_block *d_me, const xvcgpu_fp_affine_result *d_choice,
    const int32_t *d_nnz, const int32_t *d_luma_tx_index, int n, int qp_y, int qp_c,
    int ref_poc, xvcgpu_cu_info *d_cus_own) {
  if (!ctx || n < 0 || (n && (!d_me || !d_choice || !d_nnz || !d_cus_own)))
    return XVCGPU_INVALID_ARGUMENT;
  if (n == 0) return XVCGPU_OK;
  hipLaunchKernelGGL(cu_info_from_affine_choice_kernel, dim3((n + 255) / 256), dim3(256), 0,
                     ctx->stream, d_me, d_choice, d_nnz, d_luma_tx_index, n, qp_y, qp_c,
                     ref_poc, d_cus_own);
  CHECK_LAUNCH(ctx, "cu_info_from_affine_choice");
  return XVCGPU_OK;
}

xvcgpu_status xvcgpu_frame_pass_affine(xvcgpu_ctx *ctx, const xvcgpu_frame_pass_args *a,
                                       const xvcgpu_frame_pass_affine_args *f,
                                       const xvcgpu_me_plan *plan, int phases) {
  if (!f) return XVCGPU_INVALID_ARGUMENT;
  xvcgpu_status st = plan ? fp_plan_check(ctx, a, plan) : XVCGPU_OK;
  FramePassForm r;
  if (st == XVCGPU_OK) st = frame_pass_resolve(ctx, a, phases, plan, &r);
  if (st != XVCGPU_OK) return st;
  const int n = a->n_cus;
  int listed = 0;
#define FPA_NEED(cond, what) \
  if (!(cond)) return fail(ctx, XVCGPU_INVALID_ARGUMENT, "frame_pass_affine: " what)
  FPA_NEED(phases & XVC_FP_ENCODE, "phases: the second search belongs to XVC_FP_ENCODE");
  FPA_NEED(n == a->n_cus_total && a->db_y_begin == 0 && a->db_y_end >= a->rec->h &&
               a->dbh_y_end >= a->rec->h && a->ssd_y_begin == 0 && a->ssd_y_end >= a->rec->h,
           "whole pictures only (no row shard)");
  if (n > 0) {
    FPA_NEED(a->form == XVC_FP_FORM_FWD_TRANSFORM || a->form == XVC_FP_FORM_RESIDUAL ||
                 a->form == XVC_FP_FORM_RESIDUAL_RDOQ,
             "the form must be one with a prediction picture: FWD_TRANSFORM, RESIDUAL or "
             "RESIDUAL_RDOQ");
    FPA_NEED(f->d_affine && f->d_affine_results && f->d_choice && f->d_inter,
             "d_affine, d_affine_results, d_choice and d_inter");
    FPA_NEED(f->n_class[0] >= 0 && f->n_class[1] >= 0 && f->n_class[2] >= 0 &&
                 (long long)f->n_class[0] + f->n_class[1] + f->n_class[2] <= n,
             "n_class: the d_order counts are negative or name more than n_cus CUs");
    listed = f->n_class[0] + f->n_class[1] + f->n_class[2];
    FPA_NEED(listed == 0 || f->d_order, "d_order");
    FPA_NEED(a->rec->w == a->orig->w && a->rec->h == a->orig->h && a->rec->bd == a->orig->bd &&
                 a->ref->w == a->orig->w && a->ref->h == a->orig->h && a->ref->bd == a->orig->bd,
             "ref and rec must be pictures of orig's size and depth");
    FPA_NEED(a->pred->w == a->orig->w && a->pred->h == a->orig->h && a->pred->bd == a->orig->bd,
             "pred must be a picture of orig's size and depth");
    FPA_NEED(!plan || plan->first[XVCGPU_ME_PLAN_UNSUPPORTED] == plan->first[XVCGPU_ME_PLAN_LIC16],
             "the plan holds LIC jobs");
  }
#undef FPA_NEED
  xvcgpu_picture *const rec = r.fused_tail ? a->scratch_rec : a->rec;
  if (r.form) {
    st = fp_search(ctx, a, a->ref, a->d_me, a->d_results, plan);
    if (st != XVCGPU_OK) return st;   // (nothing behind a search that was refused)
    if (listed) {
      hipLaunchKernelGGL(fp_affine_boot_kernel, dim3((listed + 255) / 256), dim3(256), 0,
                         ctx->stream, a->d_results, f->d_order, listed, n, a->orig->w,
                         a->orig->h, f->d_affine);
      CHECK_LAUNCH(ctx, "fp_affine_boot");
      st = xvcgpu_affine_me_listed(ctx, a->orig, a->ref, f->d_affine, n, f->d_order, f->n_class,
                                   f->d_affine_results);
    }
    if (st == XVCGPU_OK) st = xvcgpu_fp_affine_choice(ctx, a->d_me, a->d_results, n, f);
    // (the prediction reads its `rec` for LIC jobs only: there are none)
    const xvcgpu_picture *const refs[1] = {a->ref};
    if (st == XVCGPU_OK)
      st = xvcgpu_inter_pred_batch(ctx, refs, 1, a->rec, a->pred, f->d_inter, 3 * n);
    if (st == XVCGPU_OK) st = fp_residual(ctx, a, rec, r.form);
    if (st == XVCGPU_OK)
      st = xvcgpu_cu_info_from_affine_choice(ctx, a->d_me, f->d_choice, a->d_nnz,
                                             a->d_luma_tx_index, n, a->qp_y, a->qp_c, a->ref_poc,
                                             a->d_cus_own);
  }
  if (st == XVCGPU_OK) st = fp_tail(ctx, a, phases, r.fused_tail, 0);
  return st;
}

/* ---- the P frame pass with merge mode (k_fp_merge.h) ---- */
static bool fp_merge_args_ok(const xvcgpu_frame_pass_merge_args *m, int n_cus) {
  return m->n_listed >= 0 && m->n_listed <= n_cus;
}

xvcgpu_status xvcgpu_fp_merge_rank(xvcgpu_ctx *ctx, const xvcgpu_picture *orig,
                                   const xvcgpu_picture *ref, const xvcgpu_me_block *d_me,
                                   int n_cus, const xvcgpu_frame_pass_merge_args *m) {
  if (!ctx || !orig || !ref || !m || n_cus < 0) return XVCGPU_INVALID_ARGUMENT;
  if (orig->v.bd != ref->v.bd || orig->v.c[0].w != ref->v.c[0].w ||
      orig->v.c[0].h != ref->v.c[0].h)
    return fail(ctx, XVCGPU_INVALID_ARGUMENT, "fp_merge_rank: ref must be a picture of orig's size and depth");
  if (!fp_merge_args_ok(m, n_cus))
    return fail(ctx, XVCGPU_INVALID_ARGUMENT, "fp_merge_rank: n_listed outside [0, n_cus]");
  if (!(m->lambda_sqrt >= 0) || !std::isfinite(m->lambda_sqrt))
    return fail(ctx, XVCGPU_INVALID_ARGUMENT, "fp_merge_rank: lambda_sqrt");
  if (m->n_listed && (!d_me || !m->d_cands || !m->d_rank))
    return fail(ctx, XVCGPU_INVALID_ARGUMENT, "fp_merge_rank: d_me, d_cands and d_rank");
  if (m->n_listed == 0) return XVCGPU_OK;
  hipLaunchKernelGGL(fp_merge_rank_kernel, dim3((m->n_listed + 1) / 2), dim3(128), 0, ctx->stream,
                     orig->v.c[0], ref->v.c[0], ref->v.bd, d_me, m->d_cands, m->d_order,
                     m->n_listed, n_cus, m->lambda_sqrt, m->d_rank);
  CHECK_LAUNCH(ctx, "fp_merge_rank");
  return XVCGPU_OK;
}

xvcgpu_status xvcgpu_fp_merge_choice(xvcgpu_ctx *ctx, const xvcgpu_me_block *d_me,
                                     const xvcgpu_me_result *d_results, int n_cus,
                                     const xvcgpu_frame_pass_merge_args *m) {
  if (!ctx || !m || n_cus < 0) return XVCGPU_INVALID_ARGUMENT;
  if (n_cus && (!d_me || !d_results)) return XVCGPU_INVALID_ARGUMENT;
  if (!fp_merge_args_ok(m, n_cus))
    return fail(ctx, XVCGPU_INVALID_ARGUMENT, "fp_merge_choice: n_listed outside [0, n_cus]");
  if (n_cus && (!m->d_choice || !m->d_chosen || (m->n_listed && (!m->d_cands || !m->d_rank))))
    return fail(ctx, XVCGPU_INVALID_ARGUMENT,
                "fp_merge_choice: d_cands, d_rank, d_choice and d_chosen");
  if (n_cus == 0) return XVCGPU_OK;
  hipLaunchKernelGGL(fp_merge_choice_kernel, dim3((n_cus + 255) / 256), dim3(256), 0,
                     ctx->stream, d_me, d_results, n_cus, m->d_cands, m->d_order, m->n_listed,
                     m->d_rank, m->side_bits, m->merge_side_bits, m->d_choice, m->d_chosen);
  CHECK_LAUNCH(ctx, "fp_merge_choice");
  return XVCGPU_OK;
}

xvcgpu_status xvcgpu_fp_merge_skip(xvcgpu_ctx *ctx, const int32_t *d_nnz,
                                   const int32_t *d_luma_tx_index, int n_cus,
                                   xvcgpu_fp_merge_result *d_choice) {
  if (!ctx || n_cus < 0 || (n_cus && (!d_nnz || !d_choice))) return XVCGPU_INVALID_ARGUMENT;
  if (n_cus == 0) return XVCGPU_OK;
  hipLaunchKernelGGL(fp_merge_skip_kernel, dim3((n_cus + 255) / 256), dim3(256), 0, ctx->stream,
                     d_nnz, d_luma_tx_index, n_cus, d_choice);
  CHECK_LAUNCH(ctx, "fp_merge_skip");
  return XVCGPU_OK;
}

xvcgpu_status xvcgpu_frame_pass_merge(xvcgpu_ctx *ctx, const xvcgpu_frame_pass_args *a,
                                      const xvcgpu_frame_pass_merge_args *m,
                                      const xvcgpu_me_plan *plan, int phases) {
  if (!m) return XVCGPU_INVALID_ARGUMENT;
  xvcgpu_status st = plan ? fp_plan_check(ctx, a, plan) : XVCGPU_OK;
  FramePassForm r;
  if (st == XVCGPU_OK) st = frame_pass_resolve(ctx, a, phases, plan, &r);
  if (st != XVCGPU_OK) return st;
  const int n = a->n_cus;
#define FPM_NEED(cond, what) \
  if (!(cond)) return fail(ctx, XVCGPU_INVALID_ARGUMENT, "frame_pass_merge: " what)
  FPM_NEED(phases & XVC_FP_ENCODE, "phases: the merge stage belongs to XVC_FP_ENCODE");
  FPM_NEED(n == a->n_cus_total && a->db_y_begin == 0 && a->db_y_end >= a->rec->h &&
               a->dbh_y_end >= a->rec->h && a->ssd_y_begin == 0 && a->ssd_y_end >= a->rec->h,
           "whole pictures only (no row shard)");
  FPM_NEED(m->lambda_sqrt >= 0 && std::isfinite(m->lambda_sqrt),
           "lambda_sqrt must be finite and not below 0");
  if (n > 0) {
    FPM_NEED(m->n_listed >= 0 && m->n_listed <= n, "n_listed outside [0, n_cus]");
    FPM_NEED(m->d_cands && m->d_rank && m->d_choice && m->d_chosen,
             "d_cands, d_rank, d_choice and d_chosen");
    FPM_NEED(a->d_nnz, "d_nnz: the skip flag is read from it");
    FPM_NEED(a->rec->w == a->orig->w && a->rec->h == a->orig->h && a->rec->bd == a->orig->bd &&
                 a->ref->w == a->orig->w && a->ref->h == a->orig->h && a->ref->bd == a->orig->bd,
             "ref and rec must be pictures of orig's size and depth");
  }
#undef FPM_NEED
  xvcgpu_picture *const rec = r.fused_tail ? a->scratch_rec : a->rec;
  hipStream_t main_stream = nullptr;   // set while the pass runs on ctx->hi_stream
  if (r.form) {
    st = fp_search(ctx, a, a->ref, a->d_me, a->d_results, plan);
    if (st != XVCGPU_OK) return st;   // (nothing behind a search that was refused)
    st = xvcgpu_fp_merge_rank(ctx, a->orig, a->ref, a->d_me, n, m);
    if (st == XVCGPU_OK) st = xvcgpu_fp_merge_choice(ctx, a->d_me, a->d_results, n, m);
    if (st != XVCGPU_OK) return st;
    // everything behind the search reads d_me and d_results[i].mv_x / mv_y only: the chosen
    // results stand in for the search's
    xvcgpu_frame_pass_args c = *a;
    c.d_results = m->d_chosen;
    switch (r.form) {
      case XVC_FP_FORM_RECON_FROM_ME: st = fp_recon_from_me(ctx, &c, rec); break;
      case XVC_FP_FORM_FWD_FROM_ME:
        st = fp_fwd_from_me(ctx, &c, rec, r.tail_on_hi, &main_stream);
        break;
      default: st = fp_from_pred(ctx, &c, rec, r.form); break;
    }
    const bool from_me = r.form == XVC_FP_FORM_RECON_FROM_ME || r.form == XVC_FP_FORM_FWD_FROM_ME;
    if (st == XVCGPU_OK)
      st = xvcgpu_fp_merge_skip(ctx, a->d_nnz, from_me ? nullptr : a->d_luma_tx_index, n,
                                m->d_choice);
  }
  if (st == XVCGPU_OK) st = fp_tail(ctx, a, phases, r.fused_tail, 0);
  if (main_stream) {   // every way out: the chain continues on its own stream, after the tail
    hipEventRecord(ctx->ev_hi_out, ctx->hi_stream);
    ctx->stream = main_stream;
    hipStreamWaitEvent(ctx->stream, ctx->ev_hi_out, 0);
  }
  return st;
}

/* ---- several pictures per call: every kernel launched once for all of them ---- */
// Picture by picture.  The batched form runs everything on ctxs[0]'s stream; so that a
// caller sees ONE ordering rule either way, a picture whose context has another stream is
// fenced into that one: it starts after what it holds now, which continues only after it.
static xvcgpu_status frame_pass_each(xvcgpu_ctx *const *ctxs,
                                     const xvcgpu_frame_pass_args *const *args, int n,
                                     int phases) {
  xvcgpu_ctx *ctx = ctxs[0];
  for (int i = 0; i < n; i++) {
    if (!ctxs[i] || !args[i]) return XVCGPU_INVALID_ARGUMENT;
    const bool foreign = ctxs[i]->stream != ctx->stream;
    hipEvent_t before = nullptr, after = nullptr;
    // an event belongs to the device that was current when it was created and
    // can only be recorded on that device's streams: `before` is ctxs[0]'s,
    // `after` the picture's own (contexts on another device are exactly what
    // sends a call down this path); both are destroyed on every way out
    auto fence_in = [&]() -> hipError_t {
      hipError_t e = hipSetDevice(ctx->device);
      if (e == hipSuccess) e = hipEventCreateWithFlags(&before, hipEventDisableTiming);
      if (e == hipSuccess) e = hipEventRecord(before, ctx->stream);
      if (e == hipSuccess) e = hipSetDevice(ctxs[i]->device);
      if (e == hipSuccess) e = hipEventCreateWithFlags(&after, hipEventDisableTiming);
      if (e == hipSuccess) e = hipStreamWaitEvent(ctxs[i]->stream, before, 0);
      return e;
    };
    auto fence_out = [&]() -> hipError_t {
      hipError_t e = hipSetDevice(ctxs[i]->device);
      if (e == hipSuccess) e = hipEventRecord(after, ctxs[i]->stream);
      if (e == hipSuccess) e = hipSetDevice(ctx->device);
      if (e == hipSuccess) e = hipStreamWaitEvent(ctx->stream, after, 0);
      return e;
    };
    hipError_t herr = foreign ? fence_in() : hipSuccess;
    xvcgpu_status st = XVCGPU_OK;
    if (herr == hipSuccess) {
      st = xvcgpu_frame_pass(ctxs[i], args[i], phases);
      if (foreign && st == XVCGPU_OK) herr = fence_out();
    }
    if (before) hipEventDestroy(before);   // released when the recorded work has passed them
    if (after) hipEventDestroy(after);
    HIP_TRY(ctx, herr);
    if (st != XVCGPU_OK) return st;
  }
  return XVCGPU_OK;
}

xvcgpu_status xvcgpu_frame_pass_multi(xvcgpu_ctx *const *ctxs,
                                      const xvcgpu_frame_pass_args *const *args, int n,
                                      int phases) {
  if (!ctxs || !args || n < 1 || !ctxs[0]) return XVCGPU_INVALID_ARGUMENT;
  xvcgpu_ctx *ctx = ctxs[0];
  // the forms the launches below cover: whole pictures with the fused tail, every one
  // fwd_from_me or every one recon_from_me with QuantFast; anything else (a block its own
  // call would refuse too) runs picture by picture, each on its own context
  bool batched = n >= 2 && n <= XVC_MULTI_MAX;
  int form = 0;
  for (int i = 0; i < n && batched; i++) {
    const xvcgpu_frame_pass_args *a = args[i];
    FramePassForm r;
    if (!ctxs[i] || !a) return XVCGPU_INVALID_ARGUMENT;
    batched = frame_pass_resolve(ctxs[i], a, phases, nullptr, &r) == XVCGPU_OK && r.fused_tail &&
              (r.form == XVC_FP_FORM_FWD_FROM_ME ||
               (r.form == XVC_FP_FORM_RECON_FROM_ME && !a->d_rdoq_params)) &&
              (i == 0 || r.form == form) && a->rec->w == args[0]->rec->w &&
              a->rec->h == args[0]->rec->h && a->rec->bd == args[0]->rec->bd &&
              ctxs[i]->device == ctx->device &&
              // what the launches below dereference beyond the form's own fields (a picture
              // missing one goes to the single call, which refuses it)
              a->d_cus && a->d_cu_map && a->d_ssd && a->d_nnz && a->d_cus_own &&
              (r.form != XVC_FP_FORM_FWD_FROM_ME || a->d_luma_tx_index);
    form = r.form;
  }
  if (!batched) return frame_pass_each(ctxs, args, n, phases);
  const bool rdoq = form == XVC_FP_FORM_FWD_FROM_ME;
  int max_cus = 0, max_tx = 0;
  for (int i = 0; i < n; i++) {
    max_cus = std::max(max_cus, (int)args[i]->n_cus);
    max_tx = std::max(max_tx, (int)args[i]->n_tx);
  }
  const TxTableLayout lay = xvcgpu_tx_layout();
  typedef const xvcgpu_frame_pass_args *Args;
  // 1. the motion searches
  {
    const MultiArgs<MeMultiArgs> m = multi_args<MeMultiArgs>(
        ctxs, args, n, [](Args a, xvcgpu_ctx *c, MeMultiArgs &k) {
          k.orig = a->orig->v;
          k.ref = a->ref->v;
          k.blocks = a->d_me;
          k.n = a->n_cus;
          k.results = a->d_results;
          k.sched = me_sched_next(c);   // the picture's own rotation records
        });
    hipLaunchKernelGGL(me_search_multi_kernel, me2_grid(max_cus, ME2_WAVES(16), n),
                       dim3(64 * ME2_WAVES(16)), 0, ctx->stream, m, ctx->d_tz_pattern);
  }
  // 2. prediction + transform (RDOQ: forward half only, the quantiser follows)
  {
    const MultiArgs<ReconMultiArgs> m = multi_args<ReconMultiArgs>(
        ctxs, args, n, [rdoq](Args a, xvcgpu_ctx *, ReconMultiArgs &k) {
          k.orig = a->orig->v;
          k.ref = a->ref->v;
          k.rec = a->scratch_rec->v;   // (RDOQ: the prediction; the inverse half works in place)
          k.blocks = a->d_me;
          k.results = a->d_results;
          k.n_cus = a->n_cus;
          k.qp_y = rdoq ? 0 : a->qp_y;
          k.qp_c = rdoq ? 0 : a->qp_c;
          k.ref_poc = rdoq ? 0 : a->ref_poc;
          k.nnz_out = rdoq ? nullptr : a->d_nnz;
          k.cus = rdoq ? nullptr : a->d_cus_own;
          k.coeffs = rdoq ? a->d_coeffs : nullptr;
          k.coeff_off = rdoq ? a->d_level_off : nullptr;
        });
    const int n_wg = (2 * max_cus + 3) / 4;
    const dim3 grid((n_wg + 7) / 8 * 8, n);
    if (rdoq)
      hipLaunchKernelGGL(recon_from_me_multi_kernel<true>, grid, dim3(256), 0, ctx->stream, m,
                         ctx->d_tx_tables, ctx->d_tx_tables_t, lay);
    else
      hipLaunchKernelGGL(recon_from_me_multi_kernel<false>, grid, dim3(256), 0, ctx->stream, m,
                         ctx->d_tx_tables, ctx->d_tx_tables_t, lay);
  }
  if (rdoq) {
    // 3. the quantiser: classification, class lists, the walks
    for (int i = 0; i < n; i++) {
      const xvcgpu_status st = ensure_rdoq_scratch(ctxs[i], args[i]->n_tx);
      if (st != XVCGPU_OK) return st;
    }
    const MultiArgs<RdoqMultiArgs> q = multi_args<RdoqMultiArgs>(
        ctxs, args, n, [](Args a, xvcgpu_ctx *c, RdoqMultiArgs &k) {
          k.blocks = a->d_tx;
          k.n = a->n_tx;
          k.coeffs = a->d_coeffs;
          k.d_off = a->d_level_off;
          k.levels = a->d_levels;
          k.nnz_out = a->d_nnz;
          k.l = rdoq_lists_of(c);
          k.rq_ctx = a->d_rdoq_contexts;
          k.rq_prm = a->d_rdoq_params;
        });
    const int bd = args[0]->rec->bd;
    hipLaunchKernelGGL(rdoq_classify_multi_kernel, dim3((max_tx + 3) / 4, n), dim3(256), 0,
                       ctx->stream, q, bd);
    hipLaunchKernelGGL(rdoq_compact_multi_kernel, dim3(1, n), dim3(1024), 0, ctx->stream, q);
    const RdoqGrids g = rdoq_walk_grids(max_tx);
    hipLaunchKernelGGL(quant_rdo_packed4_multi_kernel, dim3(g.g16 + g.g4, n), dim3(64), 0,
                       ctx->stream, q, bd, g.g16);
    hipLaunchKernelGGL(quant_rdo_packed_multi_kernel, dim3(g.g64, n), dim3(64), 0,
                       ctx->stream, q, bd);
    // 4. dequantisation + inverse transform + reconstruction
    const MultiArgs<InvMultiArgs> v = multi_args<InvMultiArgs>(
        ctxs, args, n, [](Args a, xvcgpu_ctx *, InvMultiArgs &k) {
          k.pred = a->scratch_rec->v;
          k.rec = a->scratch_rec->v;
          k.blocks = a->d_tx;
          k.n = a->n_tx;
          k.levels = a->d_levels;
          k.level_off = a->d_level_off;
          k.nnz = a->d_nnz;
        });
    const int n_wg = (max_tx + TX2_WAVES - 1) / TX2_WAVES;
    hipLaunchKernelGGL(inv_wave_multi_kernel, dim3((n_wg + 7) / 8 * 8, n), dim3(64 * TX2_WAVES), 0,
                       ctx->stream, v, ctx->d_tx_tables, ctx->d_tx_tables_t, lay);
    hipLaunchKernelGGL(inv_general_multi_kernel, dim3((max_tx + TX_THREADS - 1) / TX_THREADS, n),
                       dim3(TX_THREADS), 0, ctx->stream, v, ctx->d_tx_tables, lay);
    // 5. the CUs' deblocking records
    const MultiArgs<CuInfoMultiArgs> u = multi_args<CuInfoMultiArgs>(
        ctxs, args, n, [](Args a, xvcgpu_ctx *, CuInfoMultiArgs &k) {
          k.blocks = a->d_me;
          k.results = a->d_results;
          k.nnz = a->d_nnz;
          k.luma_tx_index = a->d_luma_tx_index;
          k.n = a->n_cus;
          k.qp_y = a->qp_y;
          k.qp_c = a->qp_c;
          k.ref_poc = a->ref_poc;
          k.cus = a->d_cus_own;
        });
    hipLaunchKernelGGL(cu_info_multi_kernel, dim3((max_cus + 255) / 256, n), dim3(256), 0,
                       ctx->stream, u);
  }
  // 6. deblocking, border, SSD parts
  {
    const int tiles = tail_tiles(args[0]->rec->w, args[0]->rec->h);   // one size for all
    for (int i = 0; i < n; i++) {
      const xvcgpu_frame_pass_args *a = args[i];
      const xvcgpu_status st = ensure_tail(ctxs[i], tiles);
      if (st != XVCGPU_OK) return st;
      if (a->orig->w != a->rec->w || a->orig->h != a->rec->h || a->shift_bitdepth < 8)
        return XVCGPU_INVALID_ARGUMENT;
    }
    const MultiArgs<TailMultiArgs> t = multi_args<TailMultiArgs>(
        ctxs, args, n, [tiles](Args a, xvcgpu_ctx *c, TailMultiArgs &k) {
          k.d.bd = a->rec->bd;
          k.d.pic_w = a->rec->w;
          k.d.pic_h = a->rec->h;
          k.d.bipred = k.d.beta_off = k.d.tc_off = 0;
          k.d.sub = 4;
          k.d.y_begin = 0;
          k.d.y_end = a->rec->h;
          k.d.cus = a->d_cus;
          k.d.map = a->d_cu_map;
          k.d.map_stride = a->map_stride;
          k.d.map_rows = (a->rec->h + 3) / 4;
          k.d.comp_mask = 3;
          k.src = a->scratch_rec->v;
          k.dst = a->rec->v;
          k.orig = a->orig->v.c[0];
          k.shift = 2 * (a->shift_bitdepth - 8);
          k.tiles = tiles;
          k.part = c->d_tail_part;
          k.out = reinterpret_cast<unsigned long long *>(a->d_ssd);
        });
    hipLaunchKernelGGL(deblock_tail_multi_kernel, dim3((tiles + 7) / 8 * 8, n), dim3(256), 0,
                       ctx->stream, t);
    hipLaunchKernelGGL(picture_ssd_sum_multi_kernel, dim3(1, n), dim3(256), 0, ctx->stream, t);
  }
  CHECK_LAUNCH(ctx, "frame_pass_multi");
  return XVCGPU_OK;
}

xvcgpu_status xvcgpu_affine_me_batch(xvcgpu_ctx *ctx, const xvcgpu_picture *orig,
                                     const xvcgpu_picture *ref,
                                     const xvcgpu_picture *ref_other,
                                     const xvcgpu_affine_me_block *d_blocks, int n,
                                     xvcgpu_affine_me_result *d_results) {
  if (!ctx || !orig || !ref || n < 0 || (n && (!d_blocks || !d_results)))
    return XVCGPU_INVALID_ARGUMENT;
  if (!ref_other) ref_other = ref;
  if (orig->v.bd != ref->v.bd || orig->v.c[0].w != ref->v.c[0].w ||
      orig->v.c[0].h != ref->v.c[0].h || ref_other->v.bd != ref->v.bd ||
      ref_other->v.c[0].w != ref->v.c[0].w || ref_other->v.c[0].h != ref->v.c[0].h)
    return XVCGPU_INVALID_ARGUMENT;
  if (n == 0) return XVCGPU_OK;
  // one instance per CU height (a wave per 8 rows of the block)
  hipLaunchKernelGGL(affine_me_kernel<2>, dim3(n), dim3(128), 0, ctx->stream, orig->v.c[0],
                     ref->v.c[0], ref_other->v.c[0], ref->v.bd, d_blocks, n, d_results);
  hipLaunchKernelGGL(affine_me_kernel<4>, dim3(n), dim3(256), 0, ctx->stream, orig->v.c[0],
                     ref->v.c[0], ref_other->v.c[0], ref->v.bd, d_blocks, n, d_results);
  hipLaunchKernelGGL(affine_me_kernel<8>, dim3(n), dim3(512), 0, ctx->stream, orig->v.c[0],
                     ref->v.c[0], ref_other->v.c[0], ref->v.bd, d_blocks, n, d_results);
  CHECK_LAUNCH(ctx, "affine_me_batch");
  return XVCGPU_OK;
}

/* ---- the searches of one CU state into several reference pictures, one launch each ---
 * A CU state's SearchMotion runs the same step for every (list, picture) of the CU:
 * with the single-picture entry points that is one launch per picture, each with one
 * job, one after the other.  Here the pictures come as a table and every job names its
 * slot, so the step is ONE launch whose jobs run side by side; and the caller says
 * which block-size class its jobs are (a CU state's jobs all have the CU's size), so
 * only that class's instances are launched. */
static xvcgpu_status ref_table_of(xvcgpu_ctx *ctx, const xvcgpu_picture *orig,
                                  const xvcgpu_picture *const *refs, int n_refs, RefTable *t) {
  if (!refs || n_refs < 1 || n_refs > XVC_MAX_REF_SLOTS) return XVCGPU_INVALID_ARGUMENT;
  memset(t, 0, sizeof(*t));
  for (int i = 0; i < n_refs; i++) {
    if (!refs[i]) return XVCGPU_INVALID_ARGUMENT;
    if (refs[i]->w != orig->w || refs[i]->h != orig->h || refs[i]->bd != orig->bd)
      return fail(ctx, XVCGPU_INVALID_ARGUMENT, "reference picture mismatch");
    t->pic[i] = refs[i]->v;
  }
  t->n = n_refs;
  return XVCGPU_OK;
}

xvcgpu_status xvcgpu_me_search_refs(xvcgpu_ctx *ctx, const xvcgpu_picture *orig,
                                    const xvcgpu_picture *const *refs, int n_refs, int flags,
                                    const xvcgpu_me_block *d_blocks, const uint8_t *d_slots,
                                    int n, xvcgpu_me_result *d_results, int block_class) {
  if (!ctx || !orig || n < 0 || (n && (!d_blocks || !d_slots || !d_results)) ||
      !(flags & (XVCGPU_ME_FULLPEL | XVCGPU_ME_SUBPEL)) || (flags & XVCGPU_ME_LIC_JOBS) ||
      (block_class != 16 && block_class != 32 && block_class != 64))
    return XVCGPU_INVALID_ARGUMENT;
  RefTable t;
  const xvcgpu_status st = ref_table_of(ctx, orig, refs, n_refs, &t);
  if (st != XVCGPU_OK) return st;
  if (n == 0) return XVCGPU_OK;
  Me2Sched sched = {nullptr, nullptr, nullptr};
  if (flags & XVCGPU_ME_FULLPEL) sched = me_sched_next(ctx);
  auto wave = [&](auto inst) {
    typedef decltype(inst) I;
    hipLaunchKernelGGL((me_search_refs_kernel<I::MS, I::PH>), me2_grid(n, ME2_WAVES(I::MS)),
                       dim3(64 * ME2_WAVES(I::MS)), 0, ctx->stream, orig->v, t, d_slots,
                       d_blocks, n, d_results, ctx->d_tz_pattern, sched, block_class);
  };
  auto team = [&] {
    hipLaunchKernelGGL((me_subpel_team_refs_kernel<64, 4>), me_team_grid(n), dim3(256), 0,
                       ctx->stream, orig->v, t, d_slots, d_blocks, n, d_results);
  };
  me_launches<false>(block_class, flags & 3, wave, team);
  CHECK_LAUNCH(ctx, "me_search_refs");
  return XVCGPU_OK;
}

xvcgpu_status xvcgpu_bipred_search_refs(xvcgpu_ctx *ctx, const xvcgpu_picture *orig,
                                        const xvcgpu_picture *const *refs, int n_refs,
                                        const xvcgpu_bi_block *d_jobs, const uint8_t *d_slots,
                                        int n, xvcgpu_me_result *d_results, int block_class) {
  if (!ctx || !orig || n < 0 || (n && (!d_jobs || !d_slots || !d_results)) ||
      (block_class != 16 && block_class != 32 && block_class != 64))
    return XVCGPU_INVALID_ARGUMENT;
  RefTable t;
  const xvcgpu_status st = ref_table_of(ctx, orig, refs, n_refs, &t);
  if (st != XVCGPU_OK) return st;
  if (n == 0) return XVCGPU_OK;
  const dim3 grid((n + 7) / 8 * 8);
#define BI_REFS(MS)                                                                          \
  hipLaunchKernelGGL((bipred_search_refs_kernel<MS>), grid, dim3(64 * BI_WAVES(MS)), 0,      \
                     ctx->stream, orig->v.c[0], t, d_slots, orig->bd, d_jobs, n, d_results,  \
                     block_class)
  if (block_class == 16) BI_REFS(16);
  else if (block_class == 32) BI_REFS(32);
  else BI_REFS(64);
#undef BI_REFS
  CHECK_LAUNCH(ctx, "bipred_search_refs");
  return XVCGPU_OK;
}

xvcgpu_status xvcgpu_bipred_search_refs_planned(xvcgpu_ctx *ctx, const xvcgpu_picture *orig,
                                                const xvcgpu_picture *const *refs, int n_refs,
                                                const xvcgpu_me_plan *plan, int jobs_per_cu,
                                                const xvcgpu_bi_block *d_jobs,
                                                const uint8_t *d_slots,
                                                xvcgpu_me_result *d_results) {
  if (!ctx || !orig || !plan || jobs_per_cu < 1 || jobs_per_cu > XVC_CS_MAX_REFS ||
      (plan->n && (!d_jobs || !d_slots || !d_results)))
    return XVCGPU_INVALID_ARGUMENT;
  RefTable t;
  const xvcgpu_status st = ref_table_of(ctx, orig, refs, n_refs, &t);
  if (st != XVCGPU_OK) return st;
  const int *first = plan->first;
  if (first[XVCGPU_ME_PLAN_UNSUPPORTED] != first[XVCGPU_ME_PLAN_LIC16])
    return fail(ctx, XVCGPU_INVALID_ARGUMENT, "bipred_search_refs_planned: the plan holds LIC jobs");
  if (plan->n == 0) return XVCGPU_OK;
  // a class = a run of adjacent bins = a run of the plan's list
#define BI_PLANNED(MS, FROM, TO)                                                             \
  do {                                                                                       \
    const int n_wg = (first[TO] - first[FROM]) * jobs_per_cu;                                \
    if (n_wg > 0)                                                                            \
      hipLaunchKernelGGL((bipred_search_refs_planned_kernel<MS>), dim3(n_wg),                \
                         dim3(64 * BI_WAVES(MS)), 0, ctx->stream, orig->v.c[0], t, d_slots,  \
                         orig->bd, d_jobs, plan->d_order + first[FROM], n_wg, jobs_per_cu,   \
                         d_results, plan->max_launched);                                     \
  } while (0)
  BI_PLANNED(16, XVCGPU_ME_PLAN_16X16, XVCGPU_ME_PLAN_C32);
  BI_PLANNED(32, XVCGPU_ME_PLAN_C32, XVCGPU_ME_PLAN_C64_TEAM);
  BI_PLANNED(64, XVCGPU_ME_PLAN_C64_TEAM, XVCGPU_ME_PLAN_LIC16);
#undef BI_PLANNED
  const int bad = (first[XVCGPU_ME_PLAN_BINS] - first[XVCGPU_ME_PLAN_UNSUPPORTED]) * jobs_per_cu;
  if (bad > 0)
    hipLaunchKernelGGL(bipred_refs_planned_unsupported_kernel, dim3((bad + 255) / 256), dim3(256),
                       0, ctx->stream, plan->d_order + first[XVCGPU_ME_PLAN_UNSUPPORTED], bad,
                       jobs_per_cu, d_slots, n_refs, d_results);
  CHECK_LAUNCH(ctx, "bipred_search_refs_planned");
  return XVCGPU_OK;
}

/* ---- the frame pass of a B picture (k_fp_bi_refs.h) ---- */
// The tables of the args block checked (*what names the field of a refusal) and turned into
// the kernels' form.  back: the entries of k_fp_bi_back.h, which run the rule of a picture
// with only back references and take no other block
static bool fp_bi_refs_tables(const xvcgpu_frame_pass_bi_refs_args *b, FpBiRefsDev *t,
                              const char **what, bool back = false) {
#define FPR_NEED(cond, text) \
  if (!(cond)) {             \
    *what = text;            \
    return false;            \
  }
  memset(t, 0, sizeof(*t));
  for (int l = 0; l < 2; l++)
    FPR_NEED(b->num_ref[l] >= 1 && b->num_ref[l] <= XVC_CS_MAX_REFS,
             "num_ref must be 1 .. XVC_CS_MAX_REFS per list");
  FPR_NEED(back || !b->force_l1_mvd_zero,
           "force_l1_mvd_zero: pictures with only back references are out of scope");
  FPR_NEED(!back || b->force_l1_mvd_zero == 1,
           "force_l1_mvd_zero must be 1: this entry runs the rule of a picture with only back "
           "references");
  FPR_NEED(b->n_refs >= 1 && b->n_refs <= XVC_FP_BI_MAX_REF_PICS,
           "n_refs must be 1 .. XVC_FP_BI_MAX_REF_PICS");
  for (int r = 0; r < b->num_ref[1]; r++) {
    const int s = b->same_poc_in_l0[r];
    FPR_NEED(s < b->num_ref[0], "same_poc_in_l0 names no picture of list 0");
    if (s >= 0) {
      FPR_NEED(b->slot[1][r] == b->slot[0][s], "slot of a re-used picture differs from its twin's");
      FPR_NEED(b->ref_poc[1][r] == b->ref_poc[0][s],
               "ref_poc of a re-used picture differs from its twin's");
    }
  }
  for (int l = 0; l < 2; l++)
    for (int r = 0; r < b->num_ref[l]; r++) {
      const int same = l == 1 ? b->same_poc_in_l0[r] : -1;
      FPR_NEED(b->slot[l][r] < b->n_refs, "slot is not below n_refs");
      FPR_NEED(b->d_me[l][r], "d_me is missing for a picture of a list");
      FPR_NEED(same >= 0 || b->d_results[l][r], "d_results is missing for a searched picture");
      t->me[l][r] = b->d_me[l][r];
      t->res[l][r] = same >= 0 ? b->d_results[0][same] : b->d_results[l][r];
      t->slot[l][r] = b->slot[l][r];
      t->ref_poc[l][r] = b->ref_poc[l][r];
      if (l == 1) t->same[r] = same;
    }
  FPR_NEED(b->d_bi_jobs && b->d_bi_results && b->d_bi_slots && b->d_choice && b->d_inter,
           "d_bi_jobs, d_bi_results, d_bi_slots, d_choice and d_inter");
#undef FPR_NEED
  t->num_ref[0] = b->num_ref[0];
  t->num_ref[1] = b->num_ref[1];
  t->side_uni[0] = b->side_bits_uni[0];
  t->side_uni[1] = b->side_bits_uni[1];
  t->side_bi = b->side_bits_bi;
  t->rmax = b->num_ref[0] > b->num_ref[1] ? b->num_ref[0] : b->num_ref[1];
  return true;
}

xvcgpu_status xvcgpu_fp_bi_refs_uni_fold(xvcgpu_ctx *ctx,
                                         const xvcgpu_frame_pass_bi_refs_args *b) {
  if (!ctx || !b || b->p.n_cus < 0) return XVCGPU_INVALID_ARGUMENT;
  FpBiRefsDev t;
  const char *what = nullptr;
  if (!fp_bi_refs_tables(b, &t, &what)) return fail(ctx, XVCGPU_INVALID_ARGUMENT, what);
  const int n = b->p.n_cus;
  if (n == 0) return XVCGPU_OK;
  hipLaunchKernelGGL(fp_bi_refs_uni_fold_kernel, dim3((n + 255) / 256), dim3(256), 0,
                     ctx->stream, t, n, b->d_bi_jobs, b->d_bi_slots, b->d_choice);
  CHECK_LAUNCH(ctx, "fp_bi_refs_uni_fold");
  return XVCGPU_OK;
}

xvcgpu_status xvcgpu_fp_bi_refs_choice(xvcgpu_ctx *ctx,
                                       const xvcgpu_frame_pass_bi_refs_args *b) {
  if (!ctx || !b || b->p.n_cus < 0) return XVCGPU_INVALID_ARGUMENT;
  FpBiRefsDev t;
  const char *what = nullptr;
  if (!fp_bi_refs_tables(b, &t, &what)) return fail(ctx, XVCGPU_INVALID_ARGUMENT, what);
  const int n = b->p.n_cus;
  if (n == 0) return XVCGPU_OK;
  hipLaunchKernelGGL(fp_bi_refs_choice_kernel, dim3((n + 255) / 256), dim3(256), 0, ctx->stream,
                     t, n, b->d_bi_results, b->d_choice, b->d_inter);
  CHECK_LAUNCH(ctx, "fp_bi_refs_choice");
  return XVCGPU_OK;
}

xvcgpu_status xvcgpu_cu_info_from_choice_refs(xvcgpu_ctx *ctx,
                                              const xvcgpu_frame_pass_bi_refs_args *b) {
  if (!ctx || !b || b->p.n_cus < 0) return XVCGPU_INVALID_ARGUMENT;
  const xvcgpu_frame_pass_args *a = &b->p;
  const int n = a->n_cus;
  if (n && (!b->d_me[0][0] || !b->d_choice || !a->d_nnz || !a->d_cus_own))
    return XVCGPU_INVALID_ARGUMENT;
  if (n == 0) return XVCGPU_OK;
  FpBiRefsPocs pocs;
  memcpy(pocs.poc, b->ref_poc, sizeof(pocs.poc));
  hipLaunchKernelGGL(cu_info_from_choice_refs_kernel, dim3((n + 255) / 256), dim3(256), 0,
                     ctx->stream, b->d_me[0][0], b->d_choice, a->d_nnz, a->d_luma_tx_index, n,
                     a->qp_y, a->qp_c, pocs, a->d_cus_own);
  CHECK_LAUNCH(ctx, "cu_info_from_choice_refs");
  return XVCGPU_OK;
}

/* ---- the B frame pass with affine motion (k_fp_bi_affine.h) ---- */
// What is wrong with the affine run's block for n CUs, or null
static const char *fp_bi_affine_check(const xvcgpu_frame_pass_bi_affine_args *f, int n) {
  if (!f->d_uni || !f->d_uni_results || !f->d_uni_slots)
    return "affine: d_uni, d_uni_results and d_uni_slots";
  if (!f->d_bi || !f->d_bi_results || !f->d_bi_slots)
    return "affine: d_bi, d_bi_results and d_bi_slots";
  if (!f->d_choice) return "affine: d_choice";
  if (f->n_class[0] < 0 || f->n_class[1] < 0 || f->n_class[2] < 0 ||
      (long long)f->n_class[0] + f->n_class[1] + f->n_class[2] > n)
    return "affine: n_class: the d_order counts are negative or name more than n_cus CUs";
  if (f->n_class[0] + f->n_class[1] + f->n_class[2] > 0 && !f->d_order) return "affine: d_order";
  return nullptr;
}

// The tables and arrays of both blocks as the small kernels read them
static xvcgpu_status fp_bi_affine_dev(xvcgpu_ctx *ctx, const xvcgpu_frame_pass_bi_refs_args *b,
                                      const xvcgpu_frame_pass_bi_affine_args *f, FpBiRefsDev *t,
                                      FpBiAffineDev *d) {
  if (!ctx || !b || !f || b->p.n_cus < 0) return XVCGPU_INVALID_ARGUMENT;
  const char *what = nullptr;
  if (!fp_bi_refs_tables(b, t, &what)) return fail(ctx, XVCGPU_INVALID_ARGUMENT, what);
  what = fp_bi_affine_check(f, b->p.n_cus);
  if (what) return fail(ctx, XVCGPU_INVALID_ARGUMENT, what);
  d->uni = f->d_uni;
  d->uni_res = f->d_uni_results;
  d->uni_slots = f->d_uni_slots;
  d->bi = f->d_bi;
  d->bi_res = f->d_bi_results;
  d->bi_slots = f->d_bi_slots;
  d->choice = f->d_choice;
  return XVCGPU_OK;
}

xvcgpu_status xvcgpu_fp_bi_affine_boot(xvcgpu_ctx *ctx, const xvcgpu_frame_pass_bi_refs_args *b,
                                       const xvcgpu_frame_pass_bi_affine_args *f) {
  FpBiRefsDev t;
  FpBiAffineDev d;
  const xvcgpu_status st = fp_bi_affine_dev(ctx, b, f, &t, &d);
  if (st != XVCGPU_OK) return st;
  if (!b->p.orig) return fail(ctx, XVCGPU_INVALID_ARGUMENT, "fp_bi_affine_boot: p.orig");
  const int listed = f->n_class[0] + f->n_class[1] + f->n_class[2];
  if (listed == 0) return XVCGPU_OK;
  const long long threads = (long long)listed * 2 * t.rmax;
  hipLaunchKernelGGL(fp_bi_affine_boot_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256),
                     0, ctx->stream, t, d, f->d_order, listed, b->p.n_cus, b->p.orig->w,
                     b->p.orig->h);
  CHECK_LAUNCH(ctx, "fp_bi_affine_boot");
  return XVCGPU_OK;
}

xvcgpu_status xvcgpu_affine_me_listed_refs(xvcgpu_ctx *ctx, const xvcgpu_picture *orig,
                                           const xvcgpu_picture *const *refs, int n_refs,
                                           const xvcgpu_affine_me_block *d_blocks,
                                           const uint8_t *d_slots, int n_cus, int per_cu,
                                           const int32_t *d_order, const int32_t n_class[3],
                                           xvcgpu_affine_me_result *d_results) {
  if (!ctx || !orig || n_cus < 0 || !n_class || per_cu < 1 || per_cu > 2 * XVC_CS_MAX_REFS)
    return XVCGPU_INVALID_ARGUMENT;
  long long listed = 0;
  for (int k = 0; k < 3; k++) {
    if (n_class[k] < 0) return fail(ctx, XVCGPU_INVALID_ARGUMENT, "affine_me_listed_refs: n_class");
    listed += n_class[k];
  }
  if (listed > n_cus)
    return fail(ctx, XVCGPU_INVALID_ARGUMENT,
                "affine_me_listed_refs: n_class names more CUs than n_cus");
  if ((long long)n_cus * per_cu > 0x7fffffff) return XVCGPU_INVALID_ARGUMENT;
  if (listed && (!d_blocks || !d_slots || !d_order || !d_results)) return XVCGPU_INVALID_ARGUMENT;
  RefTable t;
  const xvcgpu_status st = ref_table_of(ctx, orig, refs, n_refs, &t);
  if (st != XVCGPU_OK) return st;
  // one instance per CU height over its run of the list, every picture of a CU in the launch
  int first = 0;
#define AFF_LISTED_REFS(NW, K)                                                               \
  if (n_class[K]) {                                                                          \
    hipLaunchKernelGGL(affine_me_listed_refs_kernel<NW>, dim3(n_class[K] * per_cu),          \
                       dim3(64 * NW), 0, ctx->stream, orig->v.c[0], t, d_slots, orig->bd,    \
                       d_blocks, d_order + first, n_class[K] * per_cu, per_cu, n_cus,        \
                       d_results);                                                           \
    first += n_class[K];                                                                     \
  }
  AFF_LISTED_REFS(2, 0)
  AFF_LISTED_REFS(4, 1)
  AFF_LISTED_REFS(8, 2)
#undef AFF_LISTED_REFS
  CHECK_LAUNCH(ctx, "affine_me_listed_refs");
  return XVCGPU_OK;
}

xvcgpu_status xvcgpu_fp_bi_affine_uni_fold(xvcgpu_ctx *ctx,
                                           const xvcgpu_frame_pass_bi_refs_args *b,
                                           const xvcgpu_frame_pass_bi_affine_args *f) {
  FpBiRefsDev t;
  FpBiAffineDev d;
  const xvcgpu_status st = fp_bi_affine_dev(ctx, b, f, &t, &d);
  if (st != XVCGPU_OK) return st;
  const int n = b->p.n_cus;
  if (n == 0) return XVCGPU_OK;
  hipLaunchKernelGGL(fp_bi_affine_uni_fold_kernel, dim3((n + 255) / 256), dim3(256), 0,
                     ctx->stream, t, d, n);
  CHECK_LAUNCH(ctx, "fp_bi_affine_uni_fold");
  return XVCGPU_OK;
}

xvcgpu_status xvcgpu_fp_bi_affine_choice(xvcgpu_ctx *ctx,
                                         const xvcgpu_frame_pass_bi_refs_args *b,
                                         const xvcgpu_frame_pass_bi_affine_args *f) {
  FpBiRefsDev t;
  FpBiAffineDev d;
  const xvcgpu_status st = fp_bi_affine_dev(ctx, b, f, &t, &d);
  if (st != XVCGPU_OK) return st;
  const int n = b->p.n_cus;
  if (n == 0) return XVCGPU_OK;
  hipLaunchKernelGGL(fp_bi_affine_choice_kernel, dim3((n + 255) / 256), dim3(256), 0,
                     ctx->stream, t, d, n, b->d_choice, b->d_inter);
  CHECK_LAUNCH(ctx, "fp_bi_affine_choice");
  return XVCGPU_OK;
}

xvcgpu_status xvcgpu_cu_info_from_bi_affine_choice(xvcgpu_ctx *ctx,
                                                   const xvcgpu_frame_pass_bi_refs_args *b,
                                                   const xvcgpu_frame_pass_bi_affine_args *f) {
  if (!ctx || !b || !f || b->p.n_cus < 0) return XVCGPU_INVALID_ARGUMENT;
  const xvcgpu_frame_pass_args *a = &b->p;
  const int n = a->n_cus;
  if (n && (!b->d_me[0][0] || !f->d_choice || !a->d_nnz || !a->d_cus_own))
    return XVCGPU_INVALID_ARGUMENT;
  if (n == 0) return XVCGPU_OK;
  FpBiRefsPocs pocs;
  memcpy(pocs.poc, b->ref_poc, sizeof(pocs.poc));
  hipLaunchKernelGGL(cu_info_from_bi_affine_choice_kernel, dim3((n + 255) / 256), dim3(256), 0,
                     ctx->stream, b->d_me[0][0], f->d_choice, a->d_nnz, a->d_luma_tx_index, n,
                     a->qp_y, a->qp_c, pocs, a->d_cus_own);
  CHECK_LAUNCH(ctx, "cu_info_from_bi_affine_choice");
  return XVCGPU_OK;
}

// Launches 5-9 of the pass, behind the plain run's choice
static xvcgpu_status fp_bi_affine_run(xvcgpu_ctx *ctx, const xvcgpu_frame_pass_bi_refs_args *b,
                                      const xvcgpu_frame_pass_bi_affine_args *f, int rmax) {
  const int n = b->p.n_cus;
  xvcgpu_status st = xvcgpu_fp_bi_affine_boot(ctx, b, f);
  if (st == XVCGPU_OK)
    st = xvcgpu_affine_me_listed_refs(ctx, b->p.orig, b->refs, b->n_refs, f->d_uni,
                                      f->d_uni_slots, n, 2 * rmax, f->d_order, f->n_class,
                                      f->d_uni_results);
  if (st == XVCGPU_OK) st = xvcgpu_fp_bi_affine_uni_fold(ctx, b, f);
  if (st == XVCGPU_OK)
    st = xvcgpu_affine_me_listed_refs(ctx, b->p.orig, b->refs, b->n_refs, f->d_bi, f->d_bi_slots,
                                      n, rmax, f->d_order, f->n_class, f->d_bi_results);
  if (st == XVCGPU_OK) st = xvcgpu_fp_bi_affine_choice(ctx, b, f);
  return st;
}

/* ---- the B frame pass with merge mode (k_fp_bi_merge.h) ---- */
// What is wrong with the merge stage's block for n CUs beside the B block's plain choice
// array, or null
static const char *fp_bi_merge_check(const xvcgpu_frame_pass_bi_merge_args *m, int n,
                                     const xvcgpu_fp_bi_refs_result *d_plain) {
  if (m->n_listed < 0 || m->n_listed > n) return "merge: n_listed outside [0, n_cus]";
  if (!(m->lambda_sqrt >= 0) || !std::isfinite(m->lambda_sqrt))
    return "merge: lambda_sqrt must be finite and not below 0";
  if (n > 0 && (!m->d_cands || !m->d_rank || !m->d_choice || !m->d_chosen))
    return "merge: d_cands, d_rank, d_choice and d_chosen";
  // (the stage reads the plain records and leaves them as they are)
  if (n > 0 && d_plain &&
      (m->d_chosen == d_plain || static_cast<const void *>(m->d_choice) == d_plain))
    return "merge: d_chosen and d_choice must not be the plain pass's d_choice";
  if (n > 0 && static_cast<const void *>(m->d_choice) == m->d_chosen)
    return "merge: d_choice and d_chosen must be two arrays";
  return nullptr;
}

// The tables of both blocks checked, as the stage's kernels read them
static xvcgpu_status fp_bi_merge_dev(xvcgpu_ctx *ctx, const xvcgpu_frame_pass_bi_refs_args *b,
                                     const xvcgpu_frame_pass_bi_merge_args *m, const char *entry,
                                     FpBiRefsDev *t) {
  if (!ctx || !b || !m || b->p.n_cus < 0) return XVCGPU_INVALID_ARGUMENT;
  const char *what = nullptr;
  if (!fp_bi_refs_tables(b, t, &what)) return fail(ctx, XVCGPU_INVALID_ARGUMENT, what);
  what = fp_bi_merge_check(m, b->p.n_cus, b->d_choice);
  if (what) {
    char msg[240];
    snprintf(msg, sizeof(msg), "%s: %s", entry, what);
    return fail(ctx, XVCGPU_INVALID_ARGUMENT, msg);
  }
  return XVCGPU_OK;
}

xvcgpu_status xvcgpu_fp_bi_merge_rank(xvcgpu_ctx *ctx, const xvcgpu_frame_pass_bi_refs_args *b,
                                      const xvcgpu_frame_pass_bi_merge_args *m) {
  FpBiRefsDev t;
  xvcgpu_status st = fp_bi_merge_dev(ctx, b, m, "fp_bi_merge_rank", &t);
  if (st != XVCGPU_OK) return st;
  if (!b->p.orig) return fail(ctx, XVCGPU_INVALID_ARGUMENT, "fp_bi_merge_rank: p.orig");
  RefTable refs;
  st = ref_table_of(ctx, b->p.orig, b->refs, b->n_refs, &refs);
  if (st != XVCGPU_OK) return st;
  if (m->n_listed == 0) return XVCGPU_OK;
  hipLaunchKernelGGL(fp_bi_merge_rank_kernel, dim3((m->n_listed + 1) / 2), dim3(128), 0,
                     ctx->stream, b->p.orig->v.c[0], refs, t, b->p.orig->bd, m->d_cands,
                     m->d_order, m->n_listed, b->p.n_cus, m->lambda_sqrt, m->d_rank);
  CHECK_LAUNCH(ctx, "fp_bi_merge_rank");
  return XVCGPU_OK;
}

xvcgpu_status xvcgpu_fp_bi_merge_choice(xvcgpu_ctx *ctx, const xvcgpu_frame_pass_bi_refs_args *b,
                                        const xvcgpu_frame_pass_bi_merge_args *m) {
  FpBiRefsDev t;
  const xvcgpu_status st = fp_bi_merge_dev(ctx, b, m, "fp_bi_merge_choice", &t);
  if (st != XVCGPU_OK) return st;
  const int n = b->p.n_cus;
  if (n == 0) return XVCGPU_OK;
  hipLaunchKernelGGL(fp_bi_merge_choice_kernel, dim3((n + 255) / 256), dim3(256), 0, ctx->stream,
                     t, b->n_refs, n, b->d_choice, m->d_cands, m->d_order, m->n_listed, m->d_rank,
                     m->merge_side_bits, m->d_choice, m->d_chosen, b->d_inter);
  CHECK_LAUNCH(ctx, "fp_bi_merge_choice");
  return XVCGPU_OK;
}

xvcgpu_status xvcgpu_fp_bi_merge_skip(xvcgpu_ctx *ctx, const int32_t *d_nnz,
                                      const int32_t *d_luma_tx_index, int n_cus,
                                      xvcgpu_fp_bi_merge_result *d_choice) {
  if (!ctx || n_cus < 0 || (n_cus && (!d_nnz || !d_choice))) return XVCGPU_INVALID_ARGUMENT;
  if (n_cus == 0) return XVCGPU_OK;
  hipLaunchKernelGGL(fp_bi_merge_skip_kernel, dim3((n_cus + 255) / 256), dim3(256), 0,
                     ctx->stream, d_nnz, d_luma_tx_index, n_cus, d_choice);
  CHECK_LAUNCH(ctx, "fp_bi_merge_skip");
  return XVCGPU_OK;
}

// q: null = one QP (xvcgpu_frame_pass_bi_refs), else xvcgpu_frame_pass_bi_refs_aqp.
// entry: the name in front of a refusal.  back: xvcgpu_frame_pass_bi_back - the folds of
// k_fp_bi_back.h, with the predictor-cost launch into d_l1_mvp_cost in front of them.
// m: xvcgpu_frame_pass_bi_refs_merge - the merge stage behind the choice; what follows reads
// m->d_chosen.
static xvcgpu_status frame_pass_bi_refs_impl(xvcgpu_ctx *ctx,
                                             const xvcgpu_frame_pass_bi_refs_args *b,
                                             const xvcgpu_me_plan *const plans[2][XVC_CS_MAX_REFS],
                                             int phases, const xvcgpu_aqp_args *q,
                                             const char *entry = "frame_pass_bi_refs",
                                             bool back = false,
                                             uint32_t *d_l1_mvp_cost = nullptr,
                                             const xvcgpu_frame_pass_bi_affine_args *f = nullptr,
                                             const xvcgpu_frame_pass_bi_merge_args *m = nullptr) {
  if (!ctx || !b || !b->p.rec) return XVCGPU_INVALID_ARGUMENT;
  // the P pass's block with list 0's first picture in the fields the shared helpers read
  xvcgpu_frame_pass_args pa = b->p;
  const xvcgpu_frame_pass_args *a = &pa;
  const int n = a->n_cus;
  FpBiRefsDev t;
  const xvcgpu_me_plan *plan0 = nullptr;
#define FPB_NEED(cond, what)                               \
  if (!(cond)) {                                           \
    char msg_[240];                                        \
    snprintf(msg_, sizeof(msg_), "%s: %s", entry, what);   \
    return fail(ctx, XVCGPU_INVALID_ARGUMENT, msg_);       \
  }
  FPB_NEED(n == a->n_cus_total && a->db_y_begin == 0 && a->db_y_end >= a->rec->h &&
               a->dbh_y_end >= a->rec->h && a->ssd_y_begin == 0 && a->ssd_y_end >= a->rec->h,
           "whole pictures only (no row shard)");
  if (m) {
    const char *bad = fp_bi_merge_check(m, n, b->d_choice);
    FPB_NEED(!bad, bad);
  }
  if ((phases & XVC_FP_ENCODE) && n > 0) {
    FPB_NEED(a->form == XVC_FP_FORM_FWD_TRANSFORM || a->form == XVC_FP_FORM_RESIDUAL ||
                 a->form == XVC_FP_FORM_RESIDUAL_RDOQ,
             "the form must be one with a prediction picture: FWD_TRANSFORM, RESIDUAL or "
             "RESIDUAL_RDOQ");
    const char *what = nullptr;
    if (!fp_bi_refs_tables(b, &t, &what, back)) {
      char msg[240];
      snprintf(msg, sizeof(msg), "%s: %s", entry, what);
      return fail(ctx, XVCGPU_INVALID_ARGUMENT, msg);
    }
    FPB_NEED(!back || d_l1_mvp_cost, "d_l1_mvp_cost");
    if (f) {
      const char *bad = fp_bi_affine_check(f, n);
      FPB_NEED(!bad, bad);
    }
    FPB_NEED(!m || a->d_nnz, "d_nnz: the skip flag is read from it");
    FPB_NEED(a->orig, "orig");
    for (int k = 0; k < b->n_refs; k++)
      FPB_NEED(b->refs[k] && b->refs[k]->w == a->orig->w && b->refs[k]->h == a->orig->h &&
                   b->refs[k]->bd == a->orig->bd,
               "refs holds a missing picture or one not of orig's size and depth");
    FPB_NEED(a->rec->w == a->orig->w && a->rec->h == a->orig->h && a->rec->bd == a->orig->bd,
             "rec is not a picture of orig's size and depth");
    int given = 0, searched = 0;
    for (int l = 0; l < 2; l++)
      for (int r = 0; r < b->num_ref[l]; r++) {
        if (l == 1 && b->same_poc_in_l0[r] >= 0) continue;
        searched++;
        const xvcgpu_me_plan *p = plans ? plans[l][r] : nullptr;
        if (!p) continue;
        given++;
        FPB_NEED(p->n == n && p->d_blocks == b->d_me[l][r], "a plan was not made from its d_me");
        FPB_NEED(p->max_launched == me_class_of(a->max_block_size),
                 "a plan was made for another max_block_size class");
        if (!plan0) plan0 = p;
        for (int k = 0; k <= XVCGPU_ME_PLAN_BINS + 1; k++)
          FPB_NEED(p->first[k] == plan0->first[k], "the plans' bin counts differ");
      }
    FPB_NEED(given == 0 || given == searched, "plans for every searched picture or for none");
    FPB_NEED(!plan0 || plan0->first[XVCGPU_ME_PLAN_UNSUPPORTED] == plan0->first[XVCGPU_ME_PLAN_LIC16],
             "the plans hold LIC jobs");
    pa.ref = b->refs[b->slot[0][0]];
    pa.d_me = b->d_me[0][0];
    pa.d_results = b->d_results[0][0];
    pa.ref_poc = b->ref_poc[0][0];
  }
#undef FPB_NEED
  FramePassForm r;
  xvcgpu_status st = frame_pass_resolve(ctx, a, phases, plan0, &r);
  if (st == XVCGPU_OK && q) st = fp_aqp_check(ctx, a, q, phases);
  if (st != XVCGPU_OK) return st;
  xvcgpu_picture *const rec = r.fused_tail ? a->scratch_rec : a->rec;
  if (r.form) {
    if (q) {   // every (list, picture)'s jobs, the re-used entries' too: they price list 1
      xvcgpu_me_block *jobs[2 * XVC_CS_MAX_REFS];
      int n_me = 0;
      for (int l = 0; l < 2; l++)
        for (int k = 0; k < b->num_ref[l]; k++)
          jobs[n_me++] = const_cast<xvcgpu_me_block *>(b->d_me[l][k]);
      st = fp_aqp_front(ctx, a, q, jobs, n_me);
      if (st != XVCGPU_OK) return st;
    }
    for (int l = 0; l < 2 && st == XVCGPU_OK; l++)
      for (int q = 0; q < b->num_ref[l] && st == XVCGPU_OK; q++) {
        if (l == 1 && b->same_poc_in_l0[q] >= 0) continue;   // :536-542: list 0 searched it
        st = fp_search(ctx, a, b->refs[b->slot[l][q]], b->d_me[l][q], b->d_results[l][q],
                       plan0 ? plans[l][q] : nullptr);
      }
    if (st == XVCGPU_OK && back) st = xvcgpu_fp_bi_back_mvp_cost(ctx, b, d_l1_mvp_cost);
    if (st == XVCGPU_OK)
      st = back ? xvcgpu_fp_bi_back_uni_fold(ctx, b, d_l1_mvp_cost)
                : xvcgpu_fp_bi_refs_uni_fold(ctx, b);
    // SearchBiIterative's one step of every CU into every picture of its searched list
    if (st == XVCGPU_OK && plan0)
      st = xvcgpu_bipred_search_refs_planned(ctx, a->orig, b->refs, b->n_refs, plan0, t.rmax,
                                             b->d_bi_jobs, b->d_bi_slots, b->d_bi_results);
    for (int cls = 16; !plan0 && cls <= me_class_of(a->max_block_size) && st == XVCGPU_OK;
         cls *= 2)
      st = xvcgpu_bipred_search_refs(ctx, a->orig, b->refs, b->n_refs, b->d_bi_jobs,
                                     b->d_bi_slots, n * t.rmax, b->d_bi_results, cls);
    if (st == XVCGPU_OK)
      st = back ? xvcgpu_fp_bi_back_choice(ctx, b) : xvcgpu_fp_bi_refs_choice(ctx, b);
    if (st == XVCGPU_OK && f && n > 0) st = fp_bi_affine_run(ctx, b, f, t.rmax);
    // the merge stage; the CU records behind it read the chosen records (the prediction
    // reads d_inter, which the stage rewrites for its winners)
    xvcgpu_frame_pass_bi_refs_args chosen = *b;
    if (m && n > 0) {
      if (st == XVCGPU_OK) st = xvcgpu_fp_bi_merge_rank(ctx, b, m);
      if (st == XVCGPU_OK) st = xvcgpu_fp_bi_merge_choice(ctx, b, m);
      chosen.d_choice = m->d_chosen;
    }
    // (the prediction reads its `rec` for LIC jobs only: there are none)
    if (st == XVCGPU_OK)
      st = xvcgpu_inter_pred_batch(ctx, b->refs, b->n_refs, a->rec, a->pred, b->d_inter, 3 * n);
    if (st == XVCGPU_OK) st = fp_residual(ctx, a, rec, r.form);
    if (st == XVCGPU_OK)
      st = f ? xvcgpu_cu_info_from_bi_affine_choice(ctx, b, f)
             : xvcgpu_cu_info_from_choice_refs(ctx, &chosen);
    if (st == XVCGPU_OK && m && n > 0)
      st = xvcgpu_fp_bi_merge_skip(ctx, a->d_nnz, a->d_luma_tx_index, n, m->d_choice);
    if (st == XVCGPU_OK && q) st = xvcgpu_cu_info_set_qp(ctx, a->d_cus_own, q->d_cu_qp, n);
  }
  if (st == XVCGPU_OK) st = fp_tail(ctx, a, phases, r.fused_tail, 1);
  return st;
}

xvcgpu_status xvcgpu_frame_pass_bi_refs(xvcgpu_ctx *ctx, const xvcgpu_frame_pass_bi_refs_args *b,
                                        const xvcgpu_me_plan *const plans[2][XVC_CS_MAX_REFS],
                                        int phases) {
  return frame_pass_bi_refs_impl(ctx, b, plans, phases, nullptr);
}

xvcgpu_status xvcgpu_frame_pass_bi_refs_affine(
    xvcgpu_ctx *ctx, const xvcgpu_frame_pass_bi_refs_args *b,
    const xvcgpu_frame_pass_bi_affine_args *f,
    const xvcgpu_me_plan *const plans[2][XVC_CS_MAX_REFS], int phases) {
  if (!ctx || !f) return XVCGPU_INVALID_ARGUMENT;
  if (!(phases & XVC_FP_ENCODE))
    return fail(ctx, XVCGPU_INVALID_ARGUMENT,
                "frame_pass_bi_refs_affine: phases: the second run belongs to XVC_FP_ENCODE");
  return frame_pass_bi_refs_impl(ctx, b, plans, phases, nullptr, "frame_pass_bi_refs_affine",
                                 false, nullptr, f);
}

xvcgpu_status xvcgpu_frame_pass_bi_refs_merge(
    xvcgpu_ctx *ctx, const xvcgpu_frame_pass_bi_refs_args *b,
    const xvcgpu_frame_pass_bi_merge_args *m,
    const xvcgpu_me_plan *const plans[2][XVC_CS_MAX_REFS], int phases) {
  if (!ctx || !m) return XVCGPU_INVALID_ARGUMENT;
  if (!(phases & XVC_FP_ENCODE))
    return fail(ctx, XVCGPU_INVALID_ARGUMENT,
                "frame_pass_bi_refs_merge: phases: the merge stage belongs to XVC_FP_ENCODE");
  return frame_pass_bi_refs_impl(ctx, b, plans, phases, nullptr, "frame_pass_bi_refs_merge",
                                 false, nullptr, nullptr, m);
}

xvcgpu_status xvcgpu_frame_pass_bi_refs_aqp(
    xvcgpu_ctx *ctx, const xvcgpu_frame_pass_bi_refs_args *b, const xvcgpu_aqp_args *q,
    const xvcgpu_me_plan *const plans[2][XVC_CS_MAX_REFS], int phases) {
  if (!q) return XVCGPU_INVALID_ARGUMENT;
  return frame_pass_bi_refs_impl(ctx, b, plans, phases, q);
}

/* ---- the frame pass of a B picture with only back references (k_fp_bi_back.h) ---- */
xvcgpu_status xvcgpu_fp_bi_back_mvp_cost(xvcgpu_ctx *ctx,
                                         const xvcgpu_frame_pass_bi_refs_args *b,
                                         uint32_t *d_l1_mvp_cost) {
  if (!ctx || !b || b->p.n_cus < 0) return XVCGPU_INVALID_ARGUMENT;
  FpBiRefsDev t;
  const char *what = nullptr;
  if (!fp_bi_refs_tables(b, &t, &what, true)) return fail(ctx, XVCGPU_INVALID_ARGUMENT, what);
  if (!d_l1_mvp_cost || !b->p.orig)
    return fail(ctx, XVCGPU_INVALID_ARGUMENT, "fp_bi_back_mvp_cost: d_l1_mvp_cost and p.orig");
  RefTable refs;
  const xvcgpu_status st = ref_table_of(ctx, b->p.orig, b->refs, b->n_refs, &refs);
  if (st != XVCGPU_OK) return st;
  const int n = b->p.n_cus;
  if (n == 0) return XVCGPU_OK;
  FpBiBackL1 l1;
  memset(&l1, 0, sizeof(l1));
  l1.num_ref = t.num_ref[1];
  for (int r = 0; r < t.num_ref[1]; r++) {
    l1.me[r] = t.me[1][r];
    l1.slot[r] = t.slot[1][r];
  }
  const int waves = n * l1.num_ref;
  hipLaunchKernelGGL(fp_bi_back_mvp_cost_kernel, dim3((waves + 1) / 2), dim3(128), 0, ctx->stream,
                     b->p.orig->v.c[0], refs, l1, b->p.orig->bd, n, d_l1_mvp_cost);
  CHECK_LAUNCH(ctx, "fp_bi_back_mvp_cost");
  return XVCGPU_OK;
}

xvcgpu_status xvcgpu_fp_bi_back_uni_fold(xvcgpu_ctx *ctx,
                                         const xvcgpu_frame_pass_bi_refs_args *b,
                                         const uint32_t *d_l1_mvp_cost) {
  if (!ctx || !b || b->p.n_cus < 0) return XVCGPU_INVALID_ARGUMENT;
  FpBiRefsDev t;
  const char *what = nullptr;
  if (!fp_bi_refs_tables(b, &t, &what, true)) return fail(ctx, XVCGPU_INVALID_ARGUMENT, what);
  if (!d_l1_mvp_cost)
    return fail(ctx, XVCGPU_INVALID_ARGUMENT, "fp_bi_back_uni_fold: d_l1_mvp_cost");
  const int n = b->p.n_cus;
  if (n == 0) return XVCGPU_OK;
  hipLaunchKernelGGL(fp_bi_back_uni_fold_kernel, dim3((n + 255) / 256), dim3(256), 0,
                     ctx->stream, t, n, d_l1_mvp_cost, b->d_bi_jobs, b->d_bi_slots, b->d_choice);
  CHECK_LAUNCH(ctx, "fp_bi_back_uni_fold");
  return XVCGPU_OK;
}

xvcgpu_status xvcgpu_fp_bi_back_choice(xvcgpu_ctx *ctx,
                                       const xvcgpu_frame_pass_bi_refs_args *b) {
  if (!ctx || !b || b->p.n_cus < 0) return XVCGPU_INVALID_ARGUMENT;
  FpBiRefsDev t;
  const char *what = nullptr;
  if (!fp_bi_refs_tables(b, &t, &what, true)) return fail(ctx, XVCGPU_INVALID_ARGUMENT, what);
  const int n = b->p.n_cus;
  if (n == 0) return XVCGPU_OK;
  hipLaunchKernelGGL(fp_bi_back_choice_kernel, dim3((n + 255) / 256), dim3(256), 0, ctx->stream,
                     t, n, b->d_bi_results, b->d_choice, b->d_inter);
  CHECK_LAUNCH(ctx, "fp_bi_back_choice");
  return XVCGPU_OK;
}

xvcgpu_status xvcgpu_frame_pass_bi_back(xvcgpu_ctx *ctx, const xvcgpu_frame_pass_bi_refs_args *b,
                                        uint32_t *d_l1_mvp_cost, const xvcgpu_aqp_args *q,
                                        const xvcgpu_me_plan *const plans[2][XVC_CS_MAX_REFS],
                                        int phases) {
  return frame_pass_bi_refs_impl(ctx, b, plans, phases, q, "frame_pass_bi_back", true,
                                 d_l1_mvp_cost);
}

xvcgpu_status xvcgpu_mc_metric_batch_refs(xvcgpu_ctx *ctx, const xvcgpu_picture *orig,
                                          const xvcgpu_picture *const *refs, int n_refs,
                                          int structural_strength,
                                          const xvcgpu_mc_metric_cand *d_cands,
                                          const uint8_t *d_slots, int n, uint64_t *d_out) {
  if (!ctx || !orig || n < 0 || (n && (!d_cands || !d_slots || !d_out)))
    return XVCGPU_INVALID_ARGUMENT;
  RefTable t;
  const xvcgpu_status st = ref_table_of(ctx, orig, refs, n_refs, &t);
  if (st != XVCGPU_OK) return st;
  if (n == 0) return XVCGPU_OK;
  hipLaunchKernelGGL(mc_metric_refs_kernel, dim3((n + 1) / 2), dim3(128), 0, ctx->stream,
                     orig->v.c[0], t, d_slots, orig->bd, structural_strength, d_cands, n, d_out);
  CHECK_LAUNCH(ctx, "mc_metric_batch_refs");
  return XVCGPU_OK;
}

xvcgpu_status xvcgpu_affine_me_batch_refs(xvcgpu_ctx *ctx, const xvcgpu_picture *orig,
                                          const xvcgpu_picture *const *refs, int n_refs,
                                          const xvcgpu_affine_me_block *d_blocks,
                                          const uint8_t *d_slots, int n,
                                          xvcgpu_affine_me_result *d_results, int cu_height) {
  if (!ctx || !orig || n < 0 || (n && (!d_blocks || !d_slots || !d_results)) ||
      (cu_height != 16 && cu_height != 32 && cu_height != 64))
    return XVCGPU_INVALID_ARGUMENT;
  RefTable t;
  const xvcgpu_status st = ref_table_of(ctx, orig, refs, n_refs, &t);
  if (st != XVCGPU_OK) return st;
  if (n == 0) return XVCGPU_OK;
#define AFF_REFS(NW)                                                                      \
  hipLaunchKernelGGL(affine_me_refs_kernel<NW>, dim3(n), dim3(64 * NW), 0, ctx->stream,   \
                     orig->v.c[0], t, d_slots, orig->bd, d_blocks, n, d_results)
  if (cu_height == 16) AFF_REFS(2);
  else if (cu_height == 32) AFF_REFS(4);
  else AFF_REFS(8);
#undef AFF_REFS
  CHECK_LAUNCH(ctx, "affine_me_batch_refs");
  return XVCGPU_OK;
}

xvcgpu_status xvcgpu_copy_segments(xvcgpu_ctx *ctx, const xvcgpu_copy_segment *d_segments,
                                   int n) {
  if (!ctx || n < 0 || (n && !d_segments)) return XVCGPU_INVALID_ARGUMENT;
  if (n == 0) return XVCGPU_OK;
  hipLaunchKernelGGL(copy_segments_kernel, dim3(32, n), dim3(256), 0, ctx->stream, d_segments,
                     n);
  CHECK_LAUNCH(ctx, "copy_segments");
  return XVCGPU_OK;
}


/* ---- many chains' steps in one launch (k_cs_engine.h) --------------------------- */
struct xvcgpu_cs_env {
  xvcgpu_ctx *ctx;
  CsEnvDev *dev;
};

xvcgpu_status xvcgpu_cs_env_create(xvcgpu_ctx *ctx, const xvcgpu_picture *orig,
                                   const xvcgpu_picture *const *refs, int n_refs,
                                   xvcgpu_picture *s_orig, xvcgpu_picture *s_pred,
                                   xvcgpu_picture *s_rec, int16_t *d_levels,
                                   xvcgpu_cs_result *d_results, xvcgpu_cs_env **out) {
  if (!ctx || !orig || !s_orig || !s_pred || !s_rec || !out) return XVCGPU_INVALID_ARGUMENT;
  if (s_pred->bd != orig->bd || s_rec->bd != orig->bd || s_orig->bd != orig->bd ||
      s_rec->w != s_pred->w || s_rec->h != s_pred->h)
    return fail(ctx, XVCGPU_INVALID_ARGUMENT, "picture mismatch");
  CsEnvDev h;
  memset(&h, 0, sizeof(h));
  const xvcgpu_status st = ref_table_of(ctx, orig, refs, n_refs, &h.refs);
  if (st != XVCGPU_OK) return st;
  h.orig = orig->v;
  h.s_orig = s_orig->v;
  h.s_pred = s_pred->v;
  h.s_rec = s_rec->v;
  h.levels = d_levels;
  h.results = d_results;
  h.pic_w = orig->w;
  h.pic_h = orig->h;
  xvcgpu_cs_env *e = new (std::nothrow) xvcgpu_cs_env();
  if (!e) return XVCGPU_OUT_OF_MEMORY;
  e->ctx = ctx;
  e->dev = nullptr;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (hipMalloc(reinterpret_cast<void **>(&e->dev), sizeof(CsEnvDev)) != hipSuccess) {
    delete e;
    return fail(ctx, XVCGPU_OUT_OF_MEMORY, "cs_env");
  }
  if (hipMemcpy(e->dev, &h, sizeof(h), hipMemcpyHostToDevice) != hipSuccess) {
    hipFree(e->dev);
    delete e;
    return fail(ctx, XVCGPU_DEVICE_ERROR, "cs_env upload");
  }
  *out = e;
  return XVCGPU_OK;
}

void xvcgpu_cs_env_destroy(xvcgpu_cs_env *env) {
  if (!env) return;
  if (env->dev) hipFree(env->dev);
  delete env;
}

#define CS_SEG_RING_HALF (4u << 20)
// room for n segment records in the context's ring (see xvcgpu_internal.h)
static CsSegDev *seg_ring_take(xvcgpu_ctx *ctx, int n) {
  const size_t bytes = (sizeof(CsSegDev) * (size_t)n + 255) & ~(size_t)255;
  if (bytes > CS_SEG_RING_HALF) return nullptr;
  if (!ctx->h_seg_ring) {
    if (hipHostMalloc(reinterpret_cast<void **>(&ctx->h_seg_ring), 2 * CS_SEG_RING_HALF,
                      hipHostMallocDefault) != hipSuccess ||
        hipEventCreateWithFlags(&ctx->seg_ring_ev[0], hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&ctx->seg_ring_ev[1], hipEventDisableTiming) != hipSuccess) {
      (void)hipGetLastError();
      ctx->h_seg_ring = nullptr;
      return nullptr;
    }
  }
  if (ctx->seg_ring_pos + bytes > CS_SEG_RING_HALF) {
    // this half is full: what read it is behind this event; the other half is free once
    // the launches that read IT have passed
    const int h = ctx->seg_ring_half;
    hipEventRecord(ctx->seg_ring_ev[h], ctx->stream);
    ctx->seg_ring_used[h] = true;
    ctx->seg_ring_half = 1 - h;
    if (ctx->seg_ring_used[1 - h]) hipEventSynchronize(ctx->seg_ring_ev[1 - h]);
    ctx->seg_ring_pos = 0;
  }
  CsSegDev *out = reinterpret_cast<CsSegDev *>(ctx->h_seg_ring + ctx->seg_ring_half * CS_SEG_RING_HALF +
                                              ctx->seg_ring_pos);
  ctx->seg_ring_pos += bytes;
  return out;
}

xvcgpu_status xvcgpu_cs_segs_launch(xvcgpu_ctx *ctx, int kind, const xvcgpu_cs_seg *segs,
                                    int n_segs) {
  if (!ctx || n_segs < 0 || (n_segs && !segs) || kind < 0 || kind >= XVC_CS_SEG_KINDS)
    return XVCGPU_INVALID_ARGUMENT;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const int kChunk = 16384;          // segments per launch (grid y)
  for (int first = 0; first < n_segs; first += kChunk) {
    const int cnt = std::min(kChunk, n_segs - first);
    CsSegDev *a = seg_ring_take(ctx, cnt);
    if (!a) return fail(ctx, XVCGPU_OUT_OF_MEMORY, "cs_segs_launch: segment ring");
    int max_n = 0, max_nh = 0;
    const int key = segs[first].i0;
    for (int i = 0; i < cnt; i++) {
      const xvcgpu_cs_seg &g = segs[first + i];
      if (g.n < 0 || (kind != XVC_CS_SEG_FETCH && (!g.env || g.env->ctx->device != ctx->device)))
        return XVCGPU_INVALID_ARGUMENT;
      if ((kind == XVC_CS_SEG_ME_REFS || kind == XVC_CS_SEG_BI_REFS ||
           kind == XVC_CS_SEG_AFFINE_REFS) && g.i0 != key)
        return fail(ctx, XVCGPU_INVALID_ARGUMENT, "cs_segs_launch: one kernel instance per call");
      CsSegDev &d = a[i];
      d.n = g.n;
      d.i0 = g.i0;
      d.r0 = g.r0;
      d.r1 = g.r1;
      for (int k = 0; k < 8; k++) d.p[k] = reinterpret_cast<const void *>(g.p[k]);
      d.env = g.env ? g.env->dev : nullptr;
      max_n = std::max(max_n, g.n);
      max_nh = std::max(max_nh, g.n + (g.p[6] ? g.r0 : 0));
    }
    if (max_n == 0) continue;
    const unsigned gy = (unsigned)cnt;
    hipStream_t st = ctx->stream;
    switch (kind) {
      case XVC_CS_SEG_MC_METRIC_REFS:
        hipLaunchKernelGGL(cs_seg_mc_metric_kernel, dim3((max_n + 1) / 2, gy), dim3(128), 0, st, a);
        break;
      case XVC_CS_SEG_START_FOLD:
        hipLaunchKernelGGL(cs_seg_start_fold_kernel, dim3(max_n, gy), dim3(64), 0, st, a);
        break;
      case XVC_CS_SEG_UNI_FOLD:
        hipLaunchKernelGGL(cs_seg_uni_fold_kernel, dim3(max_n, gy), dim3(64), 0, st, a);
        break;
      case XVC_CS_SEG_BI_FOLD:
        hipLaunchKernelGGL(cs_seg_bi_fold_kernel, dim3(max_n, gy), dim3(64), 0, st, a);
        break;
      case XVC_CS_SEG_MERGE_FOLD:
        hipLaunchKernelGGL(cs_seg_merge_fold_kernel, dim3((max_n + 63) / 64, gy), dim3(64), 0, st, a);
        break;
      case XVC_CS_SEG_ME_REFS: {
        const Me2Sched sched = me_sched_next(ctx);
        if (key != 16 && key != 32 && key != 64) return XVCGPU_INVALID_ARGUMENT;
        auto wave = [&](auto inst) {
          typedef decltype(inst) I;
          hipLaunchKernelGGL((cs_seg_me_kernel<I::MS, I::PH>), me2_grid(max_n, ME2_WAVES(I::MS), gy),
                             dim3(64 * ME2_WAVES(I::MS)), 0, st, a, ctx->d_tz_pattern, sched);
        };
        auto team = [&] {
          hipLaunchKernelGGL(cs_seg_me_team_kernel, me_team_grid(max_n, gy), dim3(256), 0, st, a);
        };
        me_launches_of<3, false>(key, wave, team);   // both phases, always
        break;
      }
      case XVC_CS_SEG_BI_REFS: {
        const dim3 grid((max_n + 7) / 8 * 8, gy);
        if (key == 16) hipLaunchKernelGGL(cs_seg_bi_kernel<16>, grid, dim3(64 * BI_WAVES(16)), 0, st, a);
        else if (key == 32) hipLaunchKernelGGL(cs_seg_bi_kernel<32>, grid, dim3(64 * BI_WAVES(32)), 0, st, a);
        else if (key == 64) hipLaunchKernelGGL(cs_seg_bi_kernel<64>, grid, dim3(64 * BI_WAVES(64)), 0, st, a);
        else return XVCGPU_INVALID_ARGUMENT;
        break;
      }
      case XVC_CS_SEG_AFFINE_REFS:
        if (key == 16) hipLaunchKernelGGL(cs_seg_affine_kernel<2>, dim3(max_n, gy), dim3(128), 0, st, a);
        else if (key == 32) hipLaunchKernelGGL(cs_seg_affine_kernel<4>, dim3(max_n, gy), dim3(256), 0, st, a);
        else if (key == 64) hipLaunchKernelGGL(cs_seg_affine_kernel<8>, dim3(max_n, gy), dim3(512), 0, st, a);
        else return XVCGPU_INVALID_ARGUMENT;
        break;
      case XVC_CS_SEG_INTER_PRED:
        hipLaunchKernelGGL(cs_seg_inter_pred_kernel, dim3(max_n, gy), dim3(256), 0, st, a);
        break;
      case XVC_CS_SEG_RESIDUAL_AT:
        // as xvcgpu_residual_rdoq_batch_at checks a single call: <= 64 blocks, the arrays
        // of the blocks, 0 ... 64 head candidates, candidates and their output both or neither
        for (int i = 0; i < cnt; i++) {
          const xvcgpu_cs_seg &g = segs[first + i];
          if (g.n > 64 || !g.p[5] || g.r0 < 0 || g.r0 > 64 || (g.p[6] != 0) != (g.p[7] != 0) ||
              (g.n && (!g.p[0] || !g.p[1] || !g.p[2] || !g.p[3] || !g.p[4])))
            return fail(ctx, XVCGPU_INVALID_ARGUMENT, "cs_segs_launch: residual segment");
        }
        hipLaunchKernelGGL(cs_seg_residual_kernel, dim3(max_nh, gy), dim3(TX_THREADS), 0, st, a,
                           ctx->d_tx_tables, ctx->d_tx_tables_t, xvcgpu_tx_layout());
        break;
      case XVC_CS_SEG_EVAL_DIST:
        hipLaunchKernelGGL(cs_seg_eval_dist_kernel, dim3((max_n + 3) / 4, gy), dim3(256), 0, st, a);
        break;
      case XVC_CS_SEG_FETCH:
        for (int i = 0; i < cnt; i++)
          if ((segs[first + i].n & 3) || ((segs[first + i].p[0] | segs[first + i].p[1]) & 3))
            return XVCGPU_INVALID_ARGUMENT;
        hipLaunchKernelGGL(cs_seg_fetch_kernel, dim3(8, gy), dim3(256), 0, st, a);
        break;
      default:
        return XVCGPU_INVALID_ARGUMENT;
    }
    CHECK_LAUNCH(ctx, "cs_segs_launch");
  }
  return XVCGPU_OK;
}

/* ---- the folds of one SearchMotion chain (k_cu_state.h) ----------------------- */
xvcgpu_status xvcgpu_cs_start_fold(xvcgpu_ctx *ctx, const xvcgpu_cs_pass *d_passes, int first,
    int n,
                                   const uint64_t *d_start_dist, xvcgpu_me_block *d_me_jobs,
                                   const xvcgpu_me_result *d_me_res,
                                   xvcgpu_affine_me_block *d_aff_jobs,
                                   xvcgpu_cs_result *d_results, int pic_w, int pic_h) {
  if (!ctx || n < 0 || first < 0 || (n && (!d_passes || !d_start_dist || !d_results)))
    return XVCGPU_INVALID_ARGUMENT;
  if (!n) return XVCGPU_OK;
  hipLaunchKernelGGL(cs_start_fold_kernel, dim3(n), dim3(64), 0, ctx->stream, d_passes,
                     first, n, d_start_dist, d_me_jobs, d_me_res, d_aff_jobs, d_results, pic_w, pic_h);
  CHECK_LAUNCH(ctx, "cs_start_fold");
  return XVCGPU_OK;
}

xvcgpu_status xvcgpu_cs_merge_fold(xvcgpu_ctx *ctx, const xvcgpu_cs_merge *d_merges, int first,
                                   int n, const uint64_t *d_dist,
                                   const xvcgpu_inter_block *d_cands,
                                   xvcgpu_cs_merge_result *d_results,
                                   xvcgpu_inter_block *d_ev_inter) {
  if (!ctx || n < 0 || first < 0 || (n && (!d_merges || !d_dist || !d_cands || !d_results)))
    return XVCGPU_INVALID_ARGUMENT;
  if (!n) return XVCGPU_OK;
  hipLaunchKernelGGL(cs_merge_fold_kernel, dim3((n + 63) / 64), dim3(64), 0, ctx->stream,
                     d_merges, first, n, d_dist, d_cands, d_results, d_ev_inter);
  CHECK_LAUNCH(ctx, "cs_merge_fold");
  return XVCGPU_OK;
}

xvcgpu_status xvcgpu_cs_uni_fold(xvcgpu_ctx *ctx, const xvcgpu_cs_pass *d_passes, int first,
    int n,
                                 const xvcgpu_me_result *d_me_res,
                                 const xvcgpu_affine_me_result *d_aff_res,
                                 xvcgpu_cs_result *d_results, xvcgpu_bi_block *d_bi_jobs,
                                 xvcgpu_affine_me_block *d_aff_jobs) {
  if (!ctx || n < 0 || (n && (!d_passes || !d_results))) return XVCGPU_INVALID_ARGUMENT;
  if (!n) return XVCGPU_OK;
  hipLaunchKernelGGL(cs_uni_fold_kernel, dim3(n), dim3(64), 0, ctx->stream, d_passes, first, n,
                     d_me_res, d_aff_res, d_results, d_bi_jobs, d_aff_jobs);
  CHECK_LAUNCH(ctx, "cs_uni_fold");
  return XVCGPU_OK;
}

xvcgpu_status xvcgpu_cs_bi_fold(xvcgpu_ctx *ctx, const xvcgpu_cs_pass *d_passes, int first,
    int n,
                                const xvcgpu_me_result *d_bi_res,
                                const xvcgpu_affine_me_result *d_aff_res,
                                xvcgpu_cs_result *d_results, xvcgpu_inter_block *d_ev_inter) {
  if (!ctx || n < 0 || (n && (!d_passes || !d_results))) return XVCGPU_INVALID_ARGUMENT;
  if (!n) return XVCGPU_OK;
  hipLaunchKernelGGL(cs_bi_fold_kernel, dim3(n), dim3(64), 0, ctx->stream, d_passes, first, n,
                     d_bi_res, d_aff_res, d_results, d_ev_inter);
  CHECK_LAUNCH(ctx, "cs_bi_fold");
  return XVCGPU_OK;
}

xvcgpu_status xvcgpu_eval_dist_batch(xvcgpu_ctx *ctx, const xvcgpu_picture *orig,
                                     const xvcgpu_picture *pred, const xvcgpu_picture *rec,
                                     int structural_strength, const xvcgpu_eval_cand *d_cands,
                                     int n, uint64_t *d_out) {
  if (!ctx || !orig || !pred || !rec || n < 0 || (n && (!d_cands || !d_out)))
    return XVCGPU_INVALID_ARGUMENT;
  if (orig->bd != pred->bd || orig->bd != rec->bd)
    return fail(ctx, XVCGPU_INVALID_ARGUMENT, "picture mismatch");
  if (n == 0) return XVCGPU_OK;
  hipLaunchKernelGGL(eval_dist_kernel, dim3((n + 3) / 4), dim3(256), 0, ctx->stream, orig->v,
                     pred->v, rec->v, structural_strength, d_cands, n, d_out);
  CHECK_LAUNCH(ctx, "eval_dist_batch");
  return XVCGPU_OK;
}

}  // extern "C"
