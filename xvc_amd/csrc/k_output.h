// Decoder output formats (Resampler::ConvertTo, xvc_common_lib/resample.cc:94-148):
// the per-plane dispatch of CopyToWithResize (:340-393) - a plain depth shift
// (CopyToBytesWithShift :304-338), the exact-2x bilinear chroma path
// (resample::BilinearResample :891-930) or the separable 8-tap up / 12-tap down
// filter (resample::Resample :741-856) - and the matrix of ConvertColorSpace
// (:396-474) for interleaved ARGB.  Arithmetic, clips and the uint16 clip of
// the horizontal pass are the reference's.
//
// Edge rule: a sample position outside the picture is clamped to the picture's
// internal size (PlaneView w/h), which is what YuvPicture::PadBorder replicates
// from.  The conversion therefore reads the picture as if it were padded; it
// never reads the device border and never writes to the picture.
//
// The work is HBM-bound, so a workgroup owns an output tile of XVC_OUT_TW
// columns x tile_rows rows, filters the source rows it needs horizontally into
// LDS and filters vertically from there: no full-picture temporary.  All planes
// of an output go in one launch (a plane table; the ARGB kernel computes the
// three 12-bit components of its tile into LDS and applies the matrix).
#ifndef XVCGPU_K_OUTPUT_H_
#define XVCGPU_K_OUTPUT_H_

#include "dev_common.h"
#include "xvcgpu_internal.h"
#include "k_stats.h"  // StU8x8 / StU16x8; the dither carries come from its export kernels

#define XVC_OUT_TW 64          // output columns per tile
#define XVC_OUT_MAX_TR 32      // output rows per tile, at most (resample)
#define XVC_OUT_POINT_TR 8     // output rows per tile without the filter (shift / bilinear)
#define XVC_OUT_TMP_ROWS 256   // horizontally filtered source rows a tile may hold
#define XVC_OUT_SCALE_ONE (1 << 15)  // resample.cc kScaleFactor

// resample.cc kUpsampleFilter / kDownsampleFilters: [sub-pel phase][tap], taps
// at offsets -3..4 (up, sum 64) and -5..6 (down, sum 128).
__constant__ int16_t kOutUpFilter[16][8] = {
    {  0,   0,   0,  64,   0,   0,   0,   0},
    {  0,   1,  -3,  63,   4,  -2,   1,   0},
    { -1,   2,  -5,  62,   8,  -3,   1,   0},
    { -1,   3,  -8,  60,  13,  -4,   1,   0},
    { -1,   4, -10,  58,  17,  -5,   1,   0},
    { -1,   4, -11,  52,  26,  -8,   3,  -1},
    { -1,   3,  -9,  47,  31, -10,   4,  -1},
    { -1,   4, -11,  45,  34, -10,   4,  -1},
    { -1,   4, -11,  40,  40, -11,   4,  -1},
    { -1,   4, -10,  34,  45, -11,   4,  -1},
    { -1,   4, -10,  31,  47,  -9,   3,  -1},
    { -1,   3,  -8,  26,  52, -11,   4,  -1},
    {  0,   1,  -5,  17,  58, -10,   4,  -1},
    {  0,   1,  -4,  13,  60,  -8,   3,  -1},
    {  0,   1,  -3,   8,  62,  -5,   2,  -1},
    {  0,   1,  -2,   4,  63,  -3,   1,   0},
};
__constant__ int16_t kOutDownFilter[8][16][12] = {
    {
        {  0,   0,   0,   0,   0, 128,   0,   0,   0,   0,   0,   0},
        {  0,   0,   0,   2,  -6, 127,   7,  -2,   0,   0,   0,   0},
        {  0,   0,   0,   3, -12, 125,  16,  -5,   1,   0,   0,   0},
        {  0,   0,   0,   4, -16, 120,  26,  -7,   1,   0,   0,   0},
        {  0,   0,   0,   5, -18, 114,  36, -10,   1,   0,   0,   0},
        {  0,   0,   0,   5, -20, 107,  46, -12,   2,   0,   0,   0},
        {  0,   0,   0,   5, -21,  99,  57, -15,   3,   0,   0,   0},
        {  0,   0,   0,   5, -20,  89,  68, -18,   4,   0,   0,   0},
        {  0,   0,   0,   4, -19,  79,  79, -19,   4,   0,   0,   0},
        {  0,   0,   0,   4, -18,  68,  89, -20,   5,   0,   0,   0},
        {  0,   0,   0,   3, -15,  57,  99, -21,   5,   0,   0,   0},
        {  0,   0,   0,   2, -12,  46, 107, -20,   5,   0,   0,   0},
        {  0,   0,   0,   1, -10,  36, 114, -18,   5,   0,   0,   0},
        {  0,   0,   0,   1,  -7,  26, 120, -16,   4,   0,   0,   0},
        {  0,   0,   0,   1,  -5,  16, 125, -12,   3,   0,   0,   0},
        {  0,   0,   0,   0,  -2,   7, 127,  -6,   2,   0,   0,   0},
    },
    {
        {  0,   2,   0, -14,  33,  86,  33, -14,   0,   2,   0,   0},
        {  0,   1,   1, -14,  29,  85,  38, -13,  -1,   2,   0,   0},
        {  0,   1,   2, -14,  24,  84,  43, -12,  -2,   2,   0,   0},
        {  0,   1,   2, -13,  19,  83,  48, -11,  -3,   2,   0,   0},
        {  0,   0,   3, -13,  15,  81,  53, -10,  -4,   3,   0,   0},
        {  0,   0,   3, -12,  11,  79,  57,  -8,  -5,   3,   0,   0},
        {  0,   0,   3, -11,   7,  76,  62,  -5,  -7,   3,   0,   0},
        {  0,   0,   3, -10,   3,  73,  65,  -2,  -7,   3,   0,   0},
        {  0,   0,   3,  -9,   0,  70,  70,   0,  -9,   3,   0,   0},
        {  0,   0,   3,  -7,  -2,  65,  73,   3, -10,   3,   0,   0},
        {  0,   0,   3,  -7,  -5,  62,  76,   7, -11,   3,   0,   0},
        {  0,   0,   3,  -5,  -8,  57,  79,  11, -12,   3,   0,   0},
        {  0,   0,   3,  -4, -10,  53,  81,  15, -13,   3,   0,   0},
        {  0,   0,   2,  -3, -11,  48,  83,  19, -13,   2,   1,   0},
        {  0,   0,   2,  -2, -12,  43,  84,  24, -14,   2,   1,   0},
        {  0,   0,   2,  -1, -13,  38,  85,  29, -14,   1,   1,   0},
    },
    {
        {  0,   5,  -6, -10,  37,  76,  37, -10,  -6,   5,   0,   0},
        {  0,   5,  -4, -11,  33,  76,  40,  -9,  -7,   5,   0,   0},
        { -1,   5,  -3, -12,  29,  75,  45,  -7,  -8,   5,   0,   0},
        { -1,   4,  -2, -13,  25,  75,  48,  -5,  -9,   5,   1,   0},
        { -1,   4,  -1, -13,  22,  73,  52,  -3, -10,   4,   1,   0},
        { -1,   4,   0, -13,  18,  72,  55,  -1, -11,   4,   2,  -1},
        { -1,   4,   1, -13,  14,  70,  59,   2, -12,   3,   2,  -1},
        { -1,   3,   1, -13,  11,  68,  62,   5, -12,   3,   2,  -1},
        { -1,   3,   2, -13,   8,  65,  65,   8, -13,   2,   3,  -1},
        { -1,   2,   3, -12,   5,  62,  68,  11, -13,   1,   3,  -1},
        { -1,   2,   3, -12,   2,  59,  70,  14, -13,   1,   4,  -1},
        { -1,   2,   4, -11,  -1,  55,  72,  18, -13,   0,   4,  -1},
        {  0,   1,   4, -10,  -3,  52,  73,  22, -13,  -1,   4,  -1},
        {  0,   1,   5,  -9,  -5,  48,  75,  25, -13,  -2,   4,  -1},
        {  0,   0,   5,  -8,  -7,  45,  75,  29, -12,  -3,   5,  -1},
        {  0,   0,   5,  -7,  -9,  40,  76,  33, -11,  -4,   5,   0},
    },
    {
        {  2,  -3,  -9,   6,  39,  58,  39,   6,  -9,  -3,   2,   0},
        {  2,  -3,  -9,   4,  38,  58,  43,   7,  -9,  -4,   1,   0},
        {  2,  -2,  -9,   2,  35,  58,  44,   9,  -8,  -4,   1,   0},
        {  1,  -2,  -9,   1,  34,  58,  46,  11,  -8,  -5,   1,   0},
        {  1,  -1,  -8,  -1,  31,  57,  47,  13,  -7,  -5,   1,   0},
        {  1,  -1,  -8,  -2,  29,  56,  49,  15,  -7,  -6,   1,   1},
        {  1,   0,  -8,  -3,  26,  55,  51,  17,  -7,  -6,   1,   1},
        {  1,   0,  -7,  -4,  24,  54,  52,  19,  -6,  -7,   1,   1},
        {  1,   0,  -7,  -5,  22,  53,  53,  22,  -5,  -7,   0,   1},
        {  1,   1,  -7,  -6,  19,  52,  54,  24,  -4,  -7,   0,   1},
        {  1,   1,  -6,  -7,  17,  51,  55,  26,  -3,  -8,   0,   1},
        {  1,   1,  -6,  -7,  15,  49,  56,  29,  -2,  -8,  -1,   1},
        {  0,   1,  -5,  -7,  13,  47,  57,  31,  -1,  -8,  -1,   1},
        {  0,   1,  -5,  -8,  11,  46,  58,  34,   1,  -9,  -2,   1},
        {  0,   1,  -4,  -8,   9,  44,  58,  35,   2,  -9,  -2,   2},
        {  0,   1,  -4,  -9,   7,  43,  58,  38,   4,  -9,  -3,   2},
    },
    {
        { -2,  -7,   0,  17,  35,  43,  35,  17,   0,  -7,  -5,   2},
        { -2,  -7,  -1,  16,  34,  43,  36,  18,   1,  -7,  -5,   2},
        { -1,  -7,  -1,  14,  33,  43,  36,  19,   1,  -6,  -5,   2},
        { -1,  -7,  -2,  13,  32,  42,  37,  20,   3,  -6,  -5,   2},
        {  0,  -7,  -3,  12,  31,  42,  38,  21,   3,  -6,  -5,   2},
        {  0,  -7,  -3,  11,  30,  42,  39,  23,   4,  -6,  -6,   1},
        {  0,  -7,  -4,  10,  29,  42,  40,  24,   5,  -6,  -6,   1},
        {  1,  -7,  -4,   9,  27,  41,  40,  25,   6,  -5,  -6,   1},
        {  1,  -6,  -5,   7,  26,  41,  41,  26,   7,  -5,  -6,   1},
        {  1,  -6,  -5,   6,  25,  40,  41,  27,   9,  -4,  -7,   1},
        {  1,  -6,  -6,   5,  24,  40,  42,  29,  10,  -4,  -7,   0},
        {  1,  -6,  -6,   4,  23,  39,  42,  30,  11,  -3,  -7,   0},
        {  2,  -5,  -6,   3,  21,  38,  42,  31,  12,  -3,  -7,   0},
        {  2,  -5,  -6,   3,  20,  37,  42,  32,  13,  -2,  -7,  -1},
        {  2,  -5,  -6,   1,  19,  36,  43,  33,  14,  -1,  -7,  -1},
        {  2,  -5,  -7,   1,  18,  36,  43,  34,  16,  -1,  -7,  -2},
    },
    {
        { -6,  -3,   5,  19,  31,  36,  31,  19,   5,  -3,  -6,   0},
        { -6,  -4,   4,  18,  31,  37,  32,  20,   6,  -3,  -6,  -1},
        { -6,  -4,   4,  17,  30,  36,  33,  21,   7,  -3,  -6,  -1},
        { -5,  -5,   3,  16,  30,  36,  33,  22,   8,  -2,  -6,  -2},
        { -5,  -5,   2,  15,  29,  36,  34,  23,   9,  -2,  -6,  -2},
        { -5,  -5,   2,  15,  28,  36,  34,  24,  10,  -2,  -6,  -3},
        { -4,  -5,   1,  14,  27,  36,  35,  24,  10,  -1,  -6,  -3},
        { -4,  -5,   0,  13,  26,  35,  35,  25,  11,   0,  -5,  -3},
        { -4,  -6,   0,  12,  26,  36,  36,  26,  12,   0,  -6,  -4},
        { -3,  -5,   0,  11,  25,  35,  35,  26,  13,   0,  -5,  -4},
        { -3,  -6,  -1,  10,  24,  35,  36,  27,  14,   1,  -5,  -4},
        { -3,  -6,  -2,  10,  24,  34,  36,  28,  15,   2,  -5,  -5},
        { -2,  -6,  -2,   9,  23,  34,  36,  29,  15,   2,  -5,  -5},
        { -2,  -6,  -2,   8,  22,  33,  36,  30,  16,   3,  -5,  -5},
        { -1,  -6,  -3,   7,  21,  33,  36,  30,  17,   4,  -4,  -6},
        { -1,  -6,  -3,   6,  20,  32,  37,  31,  18,   4,  -4,  -6},
    },
    {
        { -9,   0,   9,  20,  28,  32,  28,  20,   9,   0,  -9,   0},
        { -9,   0,   8,  19,  28,  32,  29,  20,  10,   0,  -4,  -5},
        { -9,  -1,   8,  18,  28,  32,  29,  21,  10,   1,  -4,  -5},
        { -9,  -1,   7,  18,  27,  32,  30,  22,  11,   1,  -4,  -6},
        { -8,  -2,   6,  17,  27,  32,  30,  22,  12,   2,  -4,  -6},
        { -8,  -2,   6,  16,  26,  32,  31,  23,  12,   2,  -4,  -6},
        { -8,  -2,   5,  16,  26,  31,  31,  23,  13,   3,  -3,  -7},
        { -8,  -3,   5,  15,  25,  31,  31,  24,  14,   4,  -3,  -7},
        { -7,  -3,   4,  14,  25,  31,  31,  25,  14,   4,  -3,  -7},
        { -7,  -3,   4,  14,  24,  31,  31,  25,  15,   5,  -3,  -8},
        { -7,  -3,   3,  13,  23,  31,  31,  26,  16,   5,  -2,  -8},
        { -6,  -4,   2,  12,  23,  31,  32,  26,  16,   6,  -2,  -8},
        { -6,  -4,   2,  12,  22,  30,  32,  27,  17,   6,  -2,  -8},
        { -6,  -4,   1,  11,  22,  30,  32,  27,  18,   7,  -1,  -9},
        { -5,  -4,   1,  10,  21,  29,  32,  28,  18,   8,  -1,  -9},
        { -5,  -4,   0,  10,  20,  29,  32,  28,  19,   8,   0,  -9},
    },
    {
        { -8,   7,  13,  18,  22,  24,  22,  18,  13,   7,   2, -10},
        { -8,   7,  13,  18,  22,  23,  22,  19,  13,   7,   2, -10},
        { -8,   6,  12,  18,  22,  23,  22,  19,  14,   8,   2, -10},
        { -9,   6,  12,  17,  22,  23,  23,  19,  14,   8,   3, -10},
        { -9,   6,  12,  17,  21,  23,  23,  19,  14,   9,   3, -10},
        { -9,   5,  11,  17,  21,  23,  23,  20,  15,   9,   3, -10},
        { -9,   5,  11,  16,  21,  23,  23,  20,  15,   9,   4, -10},
        { -9,   5,  10,  16,  21,  23,  23,  20,  15,  10,   4, -10},
        {-10,   5,  10,  16,  20,  23,  23,  20,  16,  10,   5, -10},
        {-10,   4,  10,  15,  20,  23,  23,  21,  16,  10,   5,  -9},
        {-10,   4,   9,  15,  20,  23,  23,  21,  16,  11,   5,  -9},
        {-10,   3,   9,  15,  20,  23,  23,  21,  17,  11,   5,  -9},
        {-10,   3,   9,  14,  19,  23,  23,  21,  17,  12,   6,  -9},
        {-10,   3,   8,  14,  19,  23,  23,  22,  17,  12,   6,  -9},
        {-10,   2,   8,  14,  19,  22,  23,  22,  18,  12,   6,  -8},
        {-10,   2,   7,  13,  19,  22,  23,  22,  18,  13,   7,  -8},
    },
};

enum { kOutShift = 0, kOutBilinear = 1, kOutResample = 2 };

struct OutPlane {
  int kind;
  int src_c;            // source plane
  int dw, dh;           // output plane size
  int iw, ih;           // source plane internal size: positions clamp here
  int scale_x, scale_y; // resample: source step per output sample, 1.15 fixed point
  int filt_x, filt_y;   // resample: GetFilterFromScale when downsampling
  int shift_hor, shift_ver;
  int mode;             // shift: 0 copy / up-shift, 1 rounding down-shift, 2 dither
  int shift;            // shift: depth difference; bilinear: out - in depth
  int tile_rows;        // bilinear / resample: output rows per workgroup
  int tiles_x;
  int blocks;           // workgroups of this plane
  int row_base;         // shift mode 2: the plane's first row in row_carry
  size_t dst_off;       // byte offset of the plane in the output (planar)
};

struct OutArgs {
  OutPlane p[3];
  int np;
  int wide;             // planar: 16-bit output samples
  int smax;             // max at the depth the planes are produced at
  uint8_t *dst;
  const uint32_t *row_carry;  // shift mode 2: remainder entering each row
  // ARGB (ConvertColorSpace): out depth, its max, the right shift, the matrix
  int argb_wide, argb_max, argb_shift;
  int m[3][3];
};

__device__ __forceinline__ int out_pel(const PlaneView &s, int x, int y) {
  return s.p[(ptrdiff_t)d_clip3(y, 0, s.h - 1) * s.stride + d_clip3(x, 0, s.w - 1)];
}

// FilterHor / FilterVer: the taps of one position, 1-D, `at(k)` = sample k away
template <typename At>
__device__ __forceinline__ int out_filter(int scale, int filt, int sub, At at) {
  int sum = 0;
  if (scale < XVC_OUT_SCALE_ONE) {
#pragma unroll
    for (int k = 0; k < 8; k++) sum += at(k - 3) * kOutUpFilter[sub][k];
  } else if (scale == XVC_OUT_SCALE_ONE) {
    sum = at(0) << 6;
  } else {
#pragma unroll
    for (int k = 0; k < 12; k++) sum += at(k - 5) * kOutDownFilter[filt][sub][k];
    sum >>= 1;
  }
  return sum;
}

// One tile of one plane: sink(tile row, tile column, y, x, value) for every
// output sample of the tile.  The value is at the production depth, truncated
// to its sample type as the reference's static_cast does.  Uniform over the
// workgroup; ends with a barrier, so LDS may be reused right after.
template <typename Sink>
__device__ void out_tile(const OutPlane &q, const PlaneView &s, int src_bd, int wide,
                         int smax, int tx, int ty, uint16_t (*tmp)[XVC_OUT_TW], int tmp_rows,
                         Sink sink) {
  const int x0 = tx * XVC_OUT_TW, y0 = ty * q.tile_rows;
  const int n = q.tile_rows * XVC_OUT_TW;
  const uint32_t tmask = wide ? 0xffffu : 0xffu;
  if (q.kind == kOutShift) {  // no dither here (the host keeps mode 2 to out_shift_row)
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
      const int ly = i / XVC_OUT_TW, lx = i % XVC_OUT_TW, y = y0 + ly, x = x0 + lx;
      if (y >= q.dh || x >= q.dw) continue;
      const uint32_t v = s.p[(ptrdiff_t)y * s.stride + x];
      uint32_t o;
      if (q.mode == 0) {
        o = wide ? (v << q.shift) & 0xffffu : v & 0xffu;
      } else {
        const uint32_t r = (v + (1u << (q.shift - 1))) >> q.shift;
        o = r > (uint32_t)smax ? smax : r;
      }
      sink(ly, lx, y, x, o);
    }
  } else if (q.kind == kOutBilinear) {
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
      const int ly = i / XVC_OUT_TW, lx = i % XVC_OUT_TW, y = y0 + ly, x = x0 + lx;
      if (y >= q.dh || x >= q.dw) continue;
      const int sx = x >> 1, sy = y >> 1, ph = (x & 1) + 2 * (y & 1);
      const int a = out_pel(s, sx, sy);
      int v, sh;  // sh: the shift of the phase for out - in depth > 1 (left)
      if (ph == 0) { v = a; sh = 0; }
      else if (ph == 1) { v = a + out_pel(s, sx + 1, sy); sh = 1; }
      else if (ph == 2) { v = a + out_pel(s, sx, sy + 1); sh = 1; }
      else {
        v = a + out_pel(s, sx + 1, sy) + out_pel(s, sx, sy + 1) +
            out_pel(s, sx + 1, sy + 1) + 2;
        sh = 2;
      }
      const uint32_t o = q.shift > 1 ? (uint32_t)v << (q.shift - sh)
                                     : (uint32_t)v >> (-q.shift + sh);
      sink(ly, lx, y, x, o & tmask);
    }
  } else {
    const int y1 = min(y0 + q.tile_rows, q.dh) - 1;
    const int f0 = (y0 * q.scale_y) >> 15, f1 = (y1 * q.scale_y) >> 15;
    const int r0 = f0 - 5, nrows = f1 - f0 + 12;
    if (nrows > tmp_rows) return;  // the host sizes tile_rows (and tmp) so this never holds
    for (int i = threadIdx.x; i < nrows * XVC_OUT_TW; i += blockDim.x) {
      const int r = i / XVC_OUT_TW, lx = i % XVC_OUT_TW, x = x0 + lx;
      if (x >= q.dw) continue;
      const uint16_t *row = s.p + (ptrdiff_t)d_clip3(r0 + r, 0, s.h - 1) * s.stride;
      const int pos = (x * q.scale_x) >> 11, fx = pos >> 4, wmax = s.w - 1;
      const int sum = out_filter(q.scale_x, q.filt_x, pos & 15,
                                 [&](int k) { return (int)row[d_clip3(fx + k, 0, wmax)]; });
      tmp[r][lx] = (uint16_t)d_clip3(sum >> q.shift_hor, 0, 0xffff);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
      const int ly = i / XVC_OUT_TW, lx = i % XVC_OUT_TW, y = y0 + ly, x = x0 + lx;
      if (y >= q.dh || x >= q.dw) continue;
      const int pos = (y * q.scale_y) >> 11, b = (pos >> 4) - r0;
      const int sum = out_filter(q.scale_y, q.filt_y, pos & 15,
                                 [&](int k) { return (int)tmp[b + k][lx]; });
      sink(ly, lx, y, x, (uint32_t)d_clip3(sum >> q.shift_ver, 0, smax));
    }
  }
  __syncthreads();
}

// The plain shift of one output row (CopyToBytesWithShift), the row scheme of
// picture_export_kernel: mode 2 takes the remainder entering the row from
// row_carry (export_row_sums_kernel + export_row_scan_kernel) and scans the row.
__device__ void out_shift_row(const OutPlane &q, const PlaneView &s, const OutArgs &a,
                              int y) {
  __shared__ uint32_t wave_tot[4];
  __shared__ uint32_t carry_s;
  const int w = q.dw;
  const uint16_t *row = s.p + (ptrdiff_t)y * s.stride;
  uint8_t *out8 = a.dst + q.dst_off + (size_t)y * w * (a.wide ? 2 : 1);
  uint16_t *out16 = reinterpret_cast<uint16_t *>(out8);
  const uint32_t mask = (1u << q.shift) - 1;
  if (q.mode == 2 && threadIdx.x == 0) carry_s = a.row_carry[q.row_base + y];
  for (int base = 0; base < w; base += 256 * 8) {
    const int x0 = base + threadIdx.x * 8;
    uint32_t v[8], o[8];
#pragma unroll
    for (int k = 0; k < 8; k++) v[k] = x0 + k < w ? row[x0 + k] : 0;
    if (q.mode == 0) {
#pragma unroll
      for (int k = 0; k < 8; k++) o[k] = a.wide ? (v[k] << q.shift) & 0xffffu : v[k] & 0xffu;
    } else if (q.mode == 1) {
#pragma unroll
      for (int k = 0; k < 8; k++) {
        const uint32_t r = (v[k] + (1u << (q.shift - 1))) >> q.shift;
        o[k] = r > (uint32_t)a.smax ? a.smax : r;
      }
    } else {
      uint32_t t = 0;
#pragma unroll
      for (int k = 0; k < 8; k++) t += v[k];
      uint32_t inc = t;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const uint32_t u = __shfl_up(inc, d, XVC_WAVE);
        if ((int)(threadIdx.x & 63) >= d) inc += u;
      }
      __syncthreads();  // carry_s / wave_tot of the previous sweep consumed
      if ((threadIdx.x & 63) == 63) wave_tot[threadIdx.x >> 6] = inc;
      __syncthreads();
      uint32_t before = carry_s + inc - t;
      for (int w4 = 0; w4 < (int)(threadIdx.x >> 6); w4++) before += wave_tot[w4];
      uint32_t carry = before & mask;
#pragma unroll
      for (int k = 0; k < 8; k++) {
        carry += v[k];
        const uint32_t r = carry >> q.shift;
        o[k] = r > (uint32_t)a.smax ? a.smax : r;
        carry &= mask;
      }
      __syncthreads();
      if (threadIdx.x == 255) carry_s = carry;  // remainder after the sweep's last sample
    }
    if (x0 + 8 <= w) {
      if (a.wide) {
        StU16x8 t;
#pragma unroll
        for (int k = 0; k < 8; k++) t.v[k] = (uint16_t)o[k];
        *reinterpret_cast<StU16x8 *>(out16 + x0) = t;
      } else {
        StU8x8 t;
#pragma unroll
        for (int k = 0; k < 8; k++) t.v[k] = (uint8_t)o[k];
        *reinterpret_cast<StU8x8 *>(out8 + x0) = t;
      }
    } else {
      for (int k = 0; x0 + k < w; k++) {
        if (a.wide) out16[x0 + k] = (uint16_t)o[k];
        else out8[x0 + k] = (uint8_t)o[k];
      }
    }
  }
}

// Planar output: grid = the sum of the planes' workgroups (one row per
// workgroup for a shift plane, one tile otherwise); block 256.
template <bool kFilter>  // a plane is resampled: the LDS rows of the filter
__global__ void __launch_bounds__(256)
output_planar_kernel(PicView src, OutArgs a) {
  constexpr int kTmpRows = kFilter ? XVC_OUT_TMP_ROWS : 1;
  __shared__ uint16_t tmp[kTmpRows][XVC_OUT_TW];
  int b = blockIdx.x, c = 0;
  while (c + 1 < a.np && b >= a.p[c].blocks) b -= a.p[c++].blocks;
  const OutPlane &q = a.p[c];
  const PlaneView &s = src.c[q.src_c];
  if (q.kind == kOutShift) {
    out_shift_row(q, s, a, b);
    return;
  }
  uint8_t *dst = a.dst + q.dst_off;
  const int wide = a.wide;
  out_tile(q, s, src.bd, wide, a.smax, b % q.tiles_x, b / q.tiles_x, tmp, kTmpRows,
           [&](int, int, int y, int x, uint32_t v) {
             const size_t o = (size_t)y * q.dw + x;
             if (wide) reinterpret_cast<uint16_t *>(dst)[o] = (uint16_t)v;
             else dst[o] = (uint8_t)v;
           });
}

// ARGB: grid = tiles of the picture (all three planes have the output size);
// block 256.  The 12-bit intermediate (kColorConversionBitdepth) of the three
// components stays in LDS; one lane writes one pixel's four values (4 or 8 bytes).
template <bool kFilter>  // a component is resampled: the LDS rows of the filter
__global__ void __launch_bounds__(256)
output_argb_kernel(PicView src, OutArgs a) {
  constexpr int kTmpRows = kFilter ? XVC_OUT_TMP_ROWS : 1;
  __shared__ uint16_t tmp[kTmpRows][XVC_OUT_TW];
  __shared__ uint16_t comp[3][XVC_OUT_MAX_TR][XVC_OUT_TW];
  const OutPlane &q0 = a.p[0];
  const int tx = blockIdx.x % q0.tiles_x, ty = blockIdx.x / q0.tiles_x;
  for (int c = 0; c < 3; c++) {
    out_tile(a.p[c], src.c[a.p[c].src_c], src.bd, 1, a.smax, tx, ty, tmp, kTmpRows,
             [&](int ly, int lx, int, int, uint32_t v) { comp[c][ly][lx] = (uint16_t)v; });
  }
  const int n = q0.tile_rows * XVC_OUT_TW;
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    const int ly = i / XVC_OUT_TW, lx = i % XVC_OUT_TW;
    const int y = ty * q0.tile_rows + ly, x = tx * XVC_OUT_TW + lx;
    if (y >= q0.dh || x >= q0.dw) continue;
    const int cy = comp[0][ly][lx] - (16 << 4);
    const int d = comp[1][ly][lx] - (128 << 4);
    const int e = comp[2][ly][lx] - (128 << 4);
    const uint32_t r = d_clip_bd((a.m[0][0] * cy + a.m[0][2] * e) >> a.argb_shift, a.argb_max);
    const uint32_t g = d_clip_bd((a.m[1][0] * cy + a.m[1][1] * d + a.m[1][2] * e) >> a.argb_shift,
                                 a.argb_max);
    const uint32_t bl = d_clip_bd((a.m[2][0] * cy + a.m[2][1] * d) >> a.argb_shift, a.argb_max);
    const uint32_t al = a.argb_max;
    const size_t o = (size_t)y * q0.dw + x;
    if (a.argb_wide) {
      reinterpret_cast<uint2 *>(a.dst)[o] = make_uint2(r | (g << 16), bl | (al << 16));
    } else {
      reinterpret_cast<uint32_t *>(a.dst)[o] = r | (g << 8) | (bl << 16) | (al << 24);
    }
  }
}

#endif  // XVCGPU_K_OUTPUT_H_
