// k_me_plan.h -- the motion search of a job list through a plan: the jobs sorted once, on
// the device, into the bins that have a kernel instance of their own; a search then is one
// launch per non-empty bin over that bin's jobs only (xvcgpu_me_plan_create,
// xvcgpu_me_search_planned).  gfx950, wave64.
//
// xvcgpu_me_search_sized launches every class kernel over the whole list and each wave
// leaves when its job belongs to another class; its exact-shape kernel can only be chosen
// for the whole 16 class.  A real CU partition (64x64 beside 8x4 beside 16x16 ...) pays
// for that with up to six launches of one wave per job of the whole list, and with the
// 64-jobs-per-wave leftover kernel for everything of the 16 class that is not 16x16 / 16x8.
// A pass's descriptors are fixed when the pass is built, so they are sorted then.
//
// Bins (XVCGPU_ME_PLAN_*, xvcgpu_types.h), their instances and launches: the table of
// DESIGN.md section 8.  The classification is me2_job_class's (k_me2.h).
//
// The instances are me2_search_job's (k_me2.h); new here: the entry that reads its job
// through the bin's list (after me2_wave_entry, the wave entry it shares with the sized
// form), the 8x8 exact-shape instance and the kernel that answers the last bin.
// Resources of the exact-shape instances (both phases, one wave per workgroup, launch
// bound 5 waves per SIMD as me_search_sq16_kernel; hipcc
// -Rpass-analysis=kernel-resource-usage, gfx950):
//   me_plan_kernel<16, 3, false, 16, 16>  96 VGPRs, 5 waves / SIMD, 6864 B LDS, scratch 152 B / lane
//   me_plan_kernel<16, 3, false, 16, 8>   96 VGPRs, 5 waves / SIMD, 6864 B LDS, scratch 148 B / lane
//   me_plan_kernel<16, 3, false, 8, 8>    96 VGPRs, 5 waves / SIMD, 6864 B LDS, scratch  36 B / lane
//   me_plan_kernel<16, 3, false, 0, 0>   128 VGPRs, 4 waves / SIMD, 6864 B LDS, scratch  12 B / lane
// The scratch is not 0 (37 / 36 / 8 / 2 spilled VGPRs).  me_search_sq16_kernel, with the same
// job function under the same cap, has 164 B / lane, and k_me2.h places its spills in the
// step-5 grid loop, which one job in thousands runs; that the new instances spill in the
// same place is assumed from that, it has not been read off their ISA.
// The 8x8 bin runs one job per wave.  Not measured: the lane use of an 8x8 job, and two
// or four 8x8 jobs per wave against one - the choice is the simplest form, not a finding.
#ifndef XVCGPU_K_ME_PLAN_H_
#define XVCGPU_K_ME_PLAN_H_

#include "k_me2.h"

// The bin of a job: who takes it is me_search_wave_take's own test (me2_job_class, with
// the LIC jobs announced - whether they are is a flag of the search, not of the plan).
__device__ __forceinline__ int me_plan_bin(const xvcgpu_me_block &b, int max_launched) {
  const Me2JobClass jc = me2_job_class(b, max_launched, true);
  if (!jc.valid) return XVCGPU_ME_PLAN_UNSUPPORTED;
  const int w = b.w, h = b.h;
  const int cls = jc.mx <= 16 ? 0 : (jc.mx <= 32 ? 1 : 2);
  if (jc.lic) return XVCGPU_ME_PLAN_LIC16 + cls;
  if (cls == 1) return XVCGPU_ME_PLAN_C32;
  if (cls == 2) return (w >= 8 && h >= 8) ? XVCGPU_ME_PLAN_C64_TEAM : XVCGPU_ME_PLAN_C64_WAVE;
  if (w == 16 && h == 16) return XVCGPU_ME_PLAN_16X16;
  if (w == 16 && h == 8) return XVCGPU_ME_PLAN_16X8;
  if (w == 8 && h == 8) return XVCGPU_ME_PLAN_8X8;
  return XVCGPU_ME_PLAN_OTHER16;
}

// One workgroup of ME_PLAN_THREADS walks the list twice, ME_PLAN_THREADS jobs a step:
// first the counts per bin, then - the bins' first slots known - the scatter.  A job's
// slot is its bin's base + the jobs of that bin in earlier waves of the step (a table of
// wave x bin ballot counts in LDS) + those in lower lanes of its wave: list order inside
// every bin, the same plan on every run, no atomic whose order decides an index.
// offsets[XVCGPU_ME_PLAN_BINS + 2]: first slot of every bin in order[n], n, and the number
// of jobs with a side below 8 (the kernels that take a CU whole need 8: xvcgpu_frame_pass_planned).
#define ME_PLAN_THREADS 1024
__global__ void __launch_bounds__(ME_PLAN_THREADS)
me_plan_kernel_build(const xvcgpu_me_block *blocks, int n, int max_launched, int *order,
                     int *offsets) {
  constexpr int NW = ME_PLAN_THREADS / 64, NB = XVCGPU_ME_PLAN_BINS;
  __shared__ int s_cnt[NW][NB + 1];   // column NB: jobs with a side below 8
  __shared__ int s_base[NB + 1];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  if (tid <= NB) s_base[tid] = 0;
  __syncthreads();
  for (int pass = 0; pass < 2; pass++) {
    for (int i0 = 0; i0 < n; i0 += ME_PLAN_THREADS) {
      const int i = i0 + tid;
      int bin = -1;
      bool small = false;
      if (i < n) {
        const xvcgpu_me_block b = blocks[i];
        bin = me_plan_bin(b, max_launched);
        small = b.w < 8 || b.h < 8;
      }
      int before = 0;   // jobs of my bin in lower lanes of my wave
      for (int k = 0; k < NB; k++) {
        const unsigned long long m = __ballot(bin == k);
        if (lane == 0) s_cnt[wave][k] = __popcll(m);
        if (bin == k) before = __popcll(m & ((1ull << lane) - 1ull));
      }
      {
        const unsigned long long m = __ballot(small);
        if (lane == 0) s_cnt[wave][NB] = __popcll(m);
      }
      __syncthreads();
      if (pass == 1 && bin >= 0) {
        int slot = s_base[bin] + before;
        for (int wv = 0; wv < wave; wv++) slot += s_cnt[wv][bin];
        order[slot] = i;
      }
      __syncthreads();
      if (tid < NB || (tid == NB && pass == 0)) {
        int t = 0;
        for (int wv = 0; wv < NW; wv++) t += s_cnt[wv][tid];
        s_base[tid] += t;
      }
      __syncthreads();
    }
    if (pass == 0) {   // counts -> first slots
      if (tid == 0) {
        int at = 0;
        for (int k = 0; k < NB; k++) {
          const int c = s_base[k];
          s_base[k] = at;
          offsets[k] = at;
          at += c;
        }
        offsets[NB] = at;
        offsets[NB + 1] = s_base[NB];
      }
      __syncthreads();
    }
  }
}

// Slots [0, n) of `order` by one wave each (me2_wave_entry over the bin's own count): the
// job index read through the list, the class and the shape are the plan's word (no test).
// FW, FH > 0: the exact-shape instance.
template <int MS, int PH, bool LIC, int FW, int FH>
__device__ __forceinline__ void
me_plan_wave_body(const PicView &orig, const PicView &ref, const xvcgpu_me_block *blocks,
                  const int *order, int n, xvcgpu_me_result *results, const TzCand *tz_pattern,
                  Me2Sched sched) {
  Me2SharedT<MS, (PH & XVCGPU_ME_SUBPEL) != 0> *s;
  int slot, chunk, local;
  if (!me2_wave_entry<MS, PH, LIC>(n, sched, s, slot, chunk, local)) return;
  // wave-uniform: the descriptor and what derives from it stay in scalar registers
  const int bi = __builtin_amdgcn_readfirstlane(order[slot]);
  const xvcgpu_me_block b = blocks[bi];
  me2_search_job<MS, PH, LIC, FW, FH>(*s, orig, ref, b, bi, results, tz_pattern, sched, chunk,
                                      local, nullptr, nullptr);
}

template <int MS, int PH, bool LIC, int FW, int FH>
__global__ void
__launch_bounds__(64 * ME2_WAVES(MS), FW > 0 ? ME2_SQ16_MIN_WAVES : ME2_MIN_WAVES(MS))
me_plan_kernel(PicView orig, PicView ref, const xvcgpu_me_block *blocks, const int *order, int n,
               xvcgpu_me_result *results, const TzCand *tz_pattern, Me2Sched sched) {
  me_plan_wave_body<MS, PH, LIC, FW, FH>(orig, ref, blocks, order, n, results, tz_pattern, sched);
}

// The sub-pel team (me_subpel_team_body) over the slots of its bin.
template <int MS, int NW>
__global__ void __launch_bounds__(64 * NW)
me_plan_team_kernel(PicView orig, PicView ref, const xvcgpu_me_block *blocks, const int *order,
                    int n, xvcgpu_me_result *results) {
  me_subpel_team_body<MS, NW>(orig, ref, blocks, n, results, nullptr, nullptr, order);
}

// The jobs no instance takes: the XVCGPU_ME_UNSUPPORTED record.  One job per thread.
__global__ void __launch_bounds__(256)
me_plan_unsupported_kernel(const int *order, int n, xvcgpu_me_result *results) {
  const int slot = (int)(blockIdx.x * 256 + threadIdx.x);
  if (slot >= n) return;
  results[order[slot]] = me2_unsupported_record();
}

#endif  // XVCGPU_K_ME_PLAN_H_
