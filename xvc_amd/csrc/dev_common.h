// dev_common.h -- device helpers (gfx950, wave64).
#ifndef XVCGPU_DEV_COMMON_H_
#define XVCGPU_DEV_COMMON_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

#define XVC_WAVE 64

__device__ __forceinline__ int d_clip3(int v, int lo, int hi) {
  return v < lo ? lo : (v > hi ? hi : v);
}
__device__ __forceinline__ int d_abs(int v) { return v < 0 ? -v : v; }
__device__ __forceinline__ int d_log2_size(int size) {  // util::SizeToLog2
  int l = 1;
  while ((1 << l) < size) l++;
  return l;
}
__device__ __forceinline__ uint16_t d_clip_bd(int v, int smax) {
  return (uint16_t)(v < 0 ? 0 : (v > smax ? smax : v));
}

// Sum over a group of `G` consecutive lanes (G power of two <= 64); every lane
// of the group receives the total.
template <int G, typename T>
__device__ __forceinline__ T group_sum(T v) {
#pragma unroll
  for (int s = 1; s < G; s <<= 1) v += __shfl_xor(v, s, XVC_WAVE);
  return v;
}

// Orders LDS traffic between the lanes of ONE wave (jobs never share data
// across waves, so no workgroup barrier is ever needed): LDS requests of a
// wave are serviced in issue order; this only stops compiler reordering and
// drains outstanding LDS returns.
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// for (i = first; i < n; i += STEP) body(i) over the lanes of a wave, first < STEP.  N > 0:
// n is the constant N - the trips are unrolled and carry no compare, mask update or branch
// (a bound test only in a last, partial trip); N == 0: the loop as written, n at run time.
template <int N, int STEP, typename F>
__device__ __forceinline__ void lane_loop(int first, int n, F body) {
  if constexpr (N > 0) {
    constexpr int TRIPS = (N + STEP - 1) / STEP;
#pragma unroll
    for (int k = 0; k < TRIPS; k++) {
      const int i = first + k * STEP;
      if (N % STEP != 0 && k == TRIPS - 1 && i >= N) break;
      body(i);
    }
  } else {
    for (int i = first; i < n; i += STEP) body(i);
  }
}

// Arguments of one kernel for up to XVC_MULTI_MAX pictures, passed by value: a
// "multi" kernel is the single-picture kernel's body run with the arguments of
// picture blockIdx.y (xvcgpu_frame_pass_multi: kernels of the same kind run well
// beside each other, kernels of different kinds do not - profiles/ARCHIVE_r01_r04_design_measured.md section 6b).
#define XVC_MULTI_MAX 4
template <typename A>
struct MultiArgs {
  A a[XVC_MULTI_MAX];
};

// ClipMv, inter_prediction.cc:769-782 (1/16-pel units).
__device__ __forceinline__ void d_clip_mv(int pos_x, int pos_y, int pic_w,
                                          int pic_h, int &mx, int &my) {
  const int min_x = -((64 + 8 + pos_x - 1) << 4);
  const int min_y = -((64 + 8 + pos_y - 1) << 4);
  const int max_x = (pic_w + 8 - pos_x - 1) << 4;
  const int max_y = (pic_h + 8 - pos_y - 1) << 4;
  mx = d_clip3(mx, min_x, max_x);
  my = d_clip3(my, min_y, max_y);
}

// GetNumExpGolombBits, inter_search.cc:1179-1188 (closed form: the loop adds
// 2 per halving until 1 => 2*floor(log2(u)) + 1).
__device__ __forceinline__ uint32_t d_eg_bits(int mvd) {
  // u = mvd <= 0 ? (-mvd << 1) + 1 : mvd << 1; for mvd > 0, 2 mvd and 2 mvd + 1 have the
  // same leading bit, so (|mvd| << 1) | 1 serves both signs
  const uint32_t u = ((uint32_t)(mvd < 0 ? -mvd : mvd) << 1) | 1u;
  return 63u - 2u * (uint32_t)__clz((int)u);
}
// GetMvdBitsFullpel, inter_search.cc:1166-1177
__device__ __forceinline__ uint32_t d_mvd_bits_fullpel(int mvp_x, int mvp_y,
                                                       int fx, int fy,
                                                       int down) {
  down += 2;
  return d_eg_bits(((fx * 16) - mvp_x) >> down) +
         d_eg_bits(((fy * 16) - mvp_y) >> down);
}
// GetMvdBits, inter_search.cc:1150-1159
__device__ __forceinline__ uint32_t d_mvd_bits(int mvp_x, int mvp_y, int mx,
                                               int my, int down) {
  return d_eg_bits((mx - mvp_x) >> (2 + down)) +
         d_eg_bits((my - mvp_y) >> (2 + down));
}

// XCD-aware job index (MI355X: 8 XCDs, each with a private 4 MiB L2; workgroup
// b is observed to run on XCD b % 8).  Jobs are laid out in picture raster
// order, so giving XCD k the k-th contiguous eighth of the job list keeps each
// L2's working set to one horizontal band of the pictures instead of all of
// them.  Launch ceil(n/8)*8 workgroups; returns -1 for the padding ones.
// Placement only affects speed, never results.
__device__ __forceinline__ int xcd_job_index(int block, int n) {
  const int chunk = (n + 7) >> 3;
  const int job = (block & 7) * chunk + (block >> 3);
  return ((block >> 3) < chunk && job < n) ? job : -1;
}

// The same for kernels whose jobs come in pairs that belong together (job 2 * cu the
// luma wave of a CU, job 2 * cu + 1 its chroma wave) and whose workgroups are W waves
// (1, 2 or 4), one job per wave.  What xcd_job_index spreads over the XCDs is the unit
// of max(W, 2) jobs, so a pair never straddles two XCDs: with W = 1 a unit is two
// workgroups, 8 apart in the grid (both on XCD block % 8).  W = 4 is xcd_job_index
// over workgroups.  Returns the first job of workgroup `block` (its wave v takes that
// + v), -1 for a padding workgroup; n jobs in all.
template <int W>
struct XcdPairJobs {
  static_assert(W == 1 || W == 2 || W == 4, "waves per workgroup");
  static constexpr int UNIT = W > 2 ? W : 2;   // jobs per unit
  static constexpr int WGS = UNIT / W;         // workgroups per unit
  // workgroups to launch for n jobs (a multiple of 8)
  __host__ __device__ static constexpr int grid(int n) {
    return ((n + UNIT - 1) / UNIT + 7) / 8 * 8 * WGS;
  }
  __device__ __forceinline__ static int first_job(int block, int n) {
    const int slot = block >> 3;
    const int unit = xcd_job_index(((slot / WGS) << 3) | (block & 7), (n + UNIT - 1) / UNIT);
    return unit < 0 ? -1 : unit * UNIT + (slot % WGS) * W;
  }
};

#endif  // XVCGPU_DEV_COMMON_H_
