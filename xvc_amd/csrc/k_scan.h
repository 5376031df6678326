// k_scan.h -- the coefficient scans (TransformHelper, transform.cc:65-76,
// :1639-1683) and the sign-data hiding of QuantFast that walks them.
#ifndef XVCGPU_K_SCAN_H_
#define XVCGPU_K_SCAN_H_

#include "dev_common.h"

// ---- sign-data hiding: RdoQuant::CoeffSignHideFast (rdo_quant.cc:448-573) --
// Scan position k of a 4x4 sub-block as y*4 + x (TransformHelper::
// kScanCoeff4x4, transform.cc:72-76): order 0 walks the anti-diagonals from
// bottom-left to top-right, 1 is raster, 2 is column-major.
constexpr unsigned long long tx_pack_scan4(int order) {
  unsigned long long t = 0;
  int k = 0;
  if (order == 0) {
    for (int s = 0; s < 7; s++)
      for (int y = (s < 4 ? s : 3); y >= 0 && s - y < 4; y--, k++)
        t |= (unsigned long long)((y << 2) | (s - y)) << (4 * k);
  } else {
    for (k = 0; k < 16; k++)
      t |= (unsigned long long)(order == 1 ? k : (((k & 3) << 2) | (k >> 2))) << (4 * k);
  }
  return t;
}
// 16 nibbles: scan position k -> y*4 + x
__device__ __forceinline__ unsigned long long d_scan4_table(int order) {
  constexpr unsigned long long t0 = tx_pack_scan4(0), t1 = tx_pack_scan4(1),
                               t2 = tx_pack_scan4(2);
  return order == 0 ? t0 : (order == 1 ? t1 : t2);
}
// Index of sub-block (sx, sy) in the scan over a gw x gh grid of sub-blocks
// (TransformHelper::DeriveSubblockScan, transform.cc:1639-1683).
// (constexpr: also evaluated at compile time, rq_pack_sb_scan below)
__attribute__((always_inline)) constexpr int sb_scan_index(int order, int gw, int gh, int sx, int sy) {
  if (order == 1) return sy * gw + sx;
  if (order == 2) return sx * gh + sy;
  const int s = sx + sy;
  int idx = 0;
  for (int d = 0; d < s; d++) {
    int c = d < gw - 1 ? d : gw - 1;
    c = c < gh - 1 ? c : gh - 1;
    c = c < gw + gh - 2 - d ? c : gw + gh - 2 - d;
    idx += c + 1;
  }
  return idx + ((s < gh - 1 ? s : gh - 1) - sy);
}
__device__ __forceinline__ int d_sb_scan_index(int order, int gw, int gh, int sx, int sy) {
  return sb_scan_index(order, gw, gh, sx, sy);
}
// The diagonal scan's index of every sub-block of a gw x gh grid of at most sixteen, as
// nibbles: sub-block (sx, sy) at nibble sy * gw + sx.
constexpr unsigned long long rq_pack_sb_scan(int gw, int gh) {
  unsigned long long r = 0;
  for (int sy = 0; sy < gh; sy++)
    for (int sx = 0; sx < gw; sx++)
      r |= (unsigned long long)sb_scan_index(0, gw, gh, sx, sy) << (4 * (sy * gw + sx));
  return r;
}

// One 4x4 sub-block, by one thread.  IDX(x, y) maps a coefficient position
// to the index used by the three arrays (levels in/out, remainders, the
// unquantised coefficients).  Returns the change of the non-zero count.
template <typename IDX>
__device__ __forceinline__ int d_sign_hide_subblock(int order, int px, int py,
                                                    bool is_last_sb, int16_t *lev,
                                                    const int16_t *dl, const int16_t *cf,
                                                    IDX idx) {
  const unsigned long long tab = d_scan4_table(order);
  auto at = [&](int k) {
    const int p = (int)((tab >> (4 * k)) & 15ull);
    return idx(px + (p & 3), py + (p >> 2));
  };
  int last = -1, first = 16, sum = 0;
  for (int k = 0; k < 16; k++) {
    const int c = lev[at(k)];
    if (c) {
      first = k < first ? k : first;
      last = k;
      sum += c;
    }
  }
  if (last - first <= 3) return 0;
  const int sign = lev[at(first)] > 0 ? 0 : 1;
  if (sign == (sum & 1)) return 0;
  int curr_cost = 32767, curr_change = 0, min_cost = 32767, min_change = 0, min_index = 0;
  for (int k = is_last_sb ? last : 15; k >= 0; k--) {
    const int p = at(k);
    const int l = lev[p], d = dl[p];
    if (l != 0) {
      if (d > 0) { curr_cost = -d; curr_change = 1; }
      else if (k == first && d_abs(l) == 1) curr_cost = 32767;
      else { curr_cost = d; curr_change = -1; }
    } else if (k < first && (cf[p] >= 0 ? 0 : 1) != sign) {
      curr_cost = 32767;
    } else {
      curr_cost = -d;
      curr_change = 1;
    }
    if (curr_cost < min_cost) { min_cost = curr_cost; min_change = curr_change; min_index = k; }
  }
  const int p = at(min_index);
  const int before = lev[p];
  if (before == -32768 || before == 32767) min_change = -1;
  const int after = (int16_t)(before + (cf[p] >= 0 ? min_change : -min_change));
  lev[p] = (int16_t)after;
  return (after != 0) - (before != 0);
}

// the inverse of the 4x4 scan: position y * 4 + x -> scan offset, 16 nibbles
constexpr unsigned long long rq_pack_scan4_inv(int order) {
  const unsigned long long t = tx_pack_scan4(order);
  unsigned long long r = 0;
  for (int k = 0; k < 16; k++) r |= (unsigned long long)k << (4 * (int)((t >> (4 * k)) & 15ull));
  return r;
}

#endif  // XVCGPU_K_SCAN_H_
