// k_interp.h -- I1 / I2: InterPrediction::MotionCompUniPred of one block
// (inter_prediction.cc:1138-1172; FilterLuma / FilterChroma :1387-1448, C
// kernels :1207-1385, Filter*Bipred / FilterCopyBipred :1450-1538, shift/offset
// rules inter_prediction.h:218-254) as ONE cooperative device function,
// mc_filter_block<CHROMA, TEAM, OUT>, and what its callers do around it: the
// block setup of MotionCompensationMv (McBlock), the run-time component ->
// CHROMA dispatch (mc_filter) and AddAvgBi (wg_add_avg_bi).
//
//   TEAM  who runs the loops: McWorkgroup (threadIdx.x of blockDim.x lanes,
//         __syncthreads) or McWave (one wave's 64 lanes, wave_sync).  All lanes
//         of the team call with uniform arguments.
//   OUT   what a sample becomes and where it goes: McOut<INT14 = false, ...> the
//         Sample clipped to the bit depth, McOut<true, ...> the 14-bit int16
//         with the offset removed; STRIDED = true stores to dst[y * ds + x] (a
//         picture), false to dst[i] (a dense w x h block in LDS: no index
//         arithmetic per sample).
//
// The horizontal pass reads the reference window from global memory (L1/L2
// resident: neighbouring CUs and the sub-pel candidates of one CU hit the same
// lines) and writes the 14-bit intermediate to `tmp`; the vertical pass reads
// its columns.
#ifndef XVCGPU_K_INTERP_H_
#define XVCGPU_K_INTERP_H_

#include <type_traits>

#include "dev_common.h"
#include "dev_tables.h"
#include "xvcgpu_internal.h"

struct McWorkgroup {
  static __device__ __forceinline__ int lane() { return threadIdx.x; }
  static __device__ __forceinline__ int lanes() { return blockDim.x; }
  static __device__ __forceinline__ void sync() { __syncthreads(); }
};
struct McWave {
  static __device__ __forceinline__ int lane() { return threadIdx.x & 63; }
  static __device__ __forceinline__ int lanes() { return 64; }
  static __device__ __forceinline__ void sync() { wave_sync(); }
};

template <bool INT14, bool STRIDED>
struct McOut {
  static constexpr bool kInt14 = INT14;
  typedef typename std::conditional<INT14, int16_t, uint16_t>::type T;
  T *dst;
  int ds;  // row stride (STRIDED only)
  __device__ __forceinline__ void put(int i, int y, int x, int v) const {
    dst[STRIDED ? y * ds + x : i] = (T)v;
  }
};
typedef McOut<false, true> McSampleStrided;
typedef McOut<false, false> McSampleDense;
typedef McOut<true, false> McInt14Dense;

// sum of N taps over s[0], s[step], ...
template <int N, typename T, typename S>
__device__ __forceinline__ int d_tap_sum(const T *s, S step, const int16_t *f) {
  int sum = 0;
#pragma unroll
  for (int k = 0; k < N; k++) sum += (int)s[k * step] * f[k];
  return sum;
}

// tmp must hold w * (h + 7) int16 (chroma: h + 3).  Contains TEAM::sync(): call uniformly.
template <bool CHROMA, typename TEAM, typename OUT>
__device__ __forceinline__ void mc_filter_block(int bd, int w, int h, int fx, int fy,
                                                const uint16_t *ref, int rs, int16_t *tmp,
                                                const OUT out) {
  constexpr int N = CHROMA ? 4 : 8;
  constexpr int BACK = N / 2 - 1;
  constexpr bool INT14 = OUT::kInt14;
  const int lane = TEAM::lane(), nt = TEAM::lanes();
  const int smax = (1 << bd) - 1, head = 14 - bd;
  const int lw = 31 - __clz(w);
  const int16_t *fh = CHROMA ? kChromaTaps[fx] : kLumaTaps[fx];
  const int16_t *fv = CHROMA ? kChromaTaps[fy] : kLumaTaps[fy];
  const int sh1 = 6 - head, off1 = -(8192 << sh1);  // Sample -> 14-bit int16
  if (fx == 0 && fy == 0) {  // CopyFrom / FilterCopyBipred
    for (int i = lane; i < w * h; i += nt) {
      const int y = i >> lw, x = i & (w - 1);
      const uint16_t v = ref[(ptrdiff_t)y * rs + x];
      out.put(i, y, x, INT14 ? (int16_t)((int16_t)(v << head) - (int16_t)8192) : v);
    }
    return;
  }
  if (fy == 0) {  // FilterHorSampleSample / FilterHorSampleShort
    for (int i = lane; i < w * h; i += nt) {
      const int y = i >> lw, x = i & (w - 1);
      const int sum = d_tap_sum<N>(ref + (ptrdiff_t)y * rs + x - BACK, 1, fh);
      out.put(i, y, x, INT14 ? (int16_t)((sum + off1) >> sh1) : d_clip_bd((sum + 32) >> 6, smax));
    }
    return;
  }
  if (fx == 0) {  // FilterVerSampleSample (narrows to int16 before the clip) / ...SampleShort
    for (int i = lane; i < w * h; i += nt) {
      const int y = i >> lw, x = i & (w - 1);
      const int sum = d_tap_sum<N>(ref + (ptrdiff_t)(y - BACK) * rs + x, (ptrdiff_t)rs, fv);
      out.put(i, y, x, INT14 ? (int16_t)((sum + off1) >> sh1)
                             : d_clip_bd((int16_t)((sum + 32) >> 6), smax));
    }
    return;
  }
  // FilterHorSampleShort over h + N - 1 rows, then FilterVerShortSample / ...ShortShort
  for (int i = lane; i < w * (h + N - 1); i += nt) {
    const int y = i >> lw, x = i & (w - 1);
    const int sum = d_tap_sum<N>(ref + (ptrdiff_t)(y - BACK) * rs + x - BACK, 1, fh);
    tmp[i] = (int16_t)((sum + off1) >> sh1);
  }
  TEAM::sync();
  const int sh2 = 6 + head, off2 = (8192 << 6) + (1 << (sh2 - 1));  // int16 -> Sample
  for (int i = lane; i < w * h; i += nt) {
    const int sum = d_tap_sum<N>(tmp + i, w, fv);
    out.put(i, i >> lw, i & (w - 1), INT14 ? (int16_t)(sum >> 6)  // int16 -> int16: shift 6, offset 0
                                           : d_clip_bd((int16_t)((sum + off2) >> sh2), smax));
  }
}

// The block setup of MotionCompensationMv (inter_prediction.cc:740-758, ClipMv,
// GetFullpelRef :1174-1205, 4:2:0) for component `comp` of the CU at luma (x, y),
// w x h: the clipped vector, the component's block, the filter phases (chroma:
// frac = (mv & mask) << (1 - size_shift) = << 0) and the reference samples under
// the block at the vector's full-pel part.  row0, h: a slab of the block - rows
// [row0, row0 + h) of the component - instead of the whole.
struct McBlock {
  int mx, my;  // clipped, 1/16 pel
  int cx, cy, cw, ch, fx, fy;
  const uint16_t *ref;
  int rs;
  __device__ __forceinline__ McBlock(int x, int y, int w, int h, int comp, int mv_x, int mv_y,
                                     const PlaneView &pr, int pic_w, int pic_h, int row0 = 0)
      : mx(mv_x), my(mv_y) {
    d_clip_mv(x, y, pic_w, pic_h, mx, my);
    const int cs = comp ? 1 : 0, shift = 4 + cs;
    cx = x >> cs, cy = (y >> cs) + row0, cw = w >> cs, ch = h >> cs;
    fx = mx & ((1 << shift) - 1), fy = my & ((1 << shift) - 1);
    ref = pr.p + (ptrdiff_t)(cy + (my >> shift)) * pr.stride + cx + (mx >> shift);
    rs = pr.stride;
  }
};

// mc_filter_block of that block, the run-time component as the CHROMA argument
template <typename TEAM, typename OUT>
__device__ __forceinline__ void mc_filter(int bd, int comp, const McBlock &m, int16_t *tmp,
                                          const OUT out) {
  if (comp)
    mc_filter_block<true, TEAM>(bd, m.cw, m.ch, m.fx, m.fy, m.ref, m.rs, tmp, out);
  else
    mc_filter_block<false, TEAM>(bd, m.cw, m.ch, m.fx, m.fy, m.ref, m.rs, tmp, out);
}

// AddAvgBi (inter_prediction.cc:1545-1547) of two dense 14-bit cw x ch blocks by a workgroup of 256.
__device__ __forceinline__ void wg_add_avg_bi(int bd, int cw, int ch, const int16_t *p0,
                                              const int16_t *p1, uint16_t *dst, int ds) {
  const int head = 14 - bd;
  const int sh = (head > 2 ? head : 2) + 1;
  const int off = (1 << (sh - 1)) + 2 * 8192;
  const int smax = (1 << bd) - 1;
  const int lw = 31 - __clz(cw);
  for (int i = threadIdx.x; i < cw * ch; i += 256)
    dst[(ptrdiff_t)(i >> lw) * ds + (i & (cw - 1))] =
        d_clip_bd(((int)p0[i] + (int)p1[i] + off) >> sh, smax);
}

#endif  // XVCGPU_K_INTERP_H_
