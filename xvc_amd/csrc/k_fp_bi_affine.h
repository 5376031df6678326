// k_fp_bi_affine.h -- the second SearchMotion run of InterSearch::CompressInter
// (inter_search.cc:74-99) for a whole B picture, behind the plain run of
// xvcgpu_frame_pass_bi_refs (xvcgpu_frame_pass_bi_refs_affine): fp_bi_affine_boot_kernel ->
// the affine search of every (list, picture) of the capable CUs (affine_me_listed_refs_kernel)
// -> fp_bi_affine_uni_fold_kernel -> the SearchBiIterative step on affine vectors into every
// picture of the list that lost (the same instance over the refinement jobs) ->
// fp_bi_affine_choice_kernel -> the prediction (k_inter_pred.h) -> residual pipeline ->
// cu_info_from_bi_affine_choice_kernel -> the B tail.
// Host twin: the CU-state walk (k_cu_state.h and its host driver), one CU at a time.
//
// The small kernels: one thread per CU (boot: per listed job), 256-thread workgroups, plain
// loads and stores, no LDS, no atomics.  A job's mvp stands for both AMVP entries, as in
// k_fp_bi_refs.h and k_fp_affine.h, whose prices these are: fp_bi_cost, fp_bi_ref_idx_bits,
// fp_affine_mvd_bits.
//
// Job layout.  E = 2 * Rmax uni-directional jobs per CU: [i * E + l * Rmax + r]; Rmax
// refinement jobs per CU: [i * Rmax + k].  Two slot bytes per job {searched, other}; a first
// byte of XVC_FP_BI_NO_JOB: no job.  A re-used list-1 entry (same_poc_in_l0[r] >= 0) has no
// job of its own: its distortion and vectors are list 0's of its twin (:536-542).
//
// The listed instance is affine_me_body with the job index and the slot bytes handed in: it
// adds scalar loads of the index, the first slot byte and the job's flag byte in front and
// leaves the body's budget as it is.  hipcc -Rpass-analysis=kernel-resource-usage, gfx950,
// affine_me_refs_kernel<NW> beside affine_me_listed_refs_kernel<NW>:
//   <2>  refs   132 VGPRs, 104 SGPRs, 32 B / lane scratch, LDS 11024 B, 3 waves / SIMD
//        listed 132 VGPRs, 104 SGPRs, 32 B / lane scratch, LDS 11024 B, 3 waves / SIMD
//   <4>  refs   136 VGPRs, 104 SGPRs, 32 B / lane scratch, LDS 22048 B, 3 waves / SIMD
//        listed 136 VGPRs, 104 SGPRs, 32 B / lane scratch, LDS 22048 B, 3 waves / SIMD
//   <8>  refs   144 VGPRs, 104 SGPRs, 32 B / lane scratch, LDS 44096 B, 3 waves / SIMD
//        listed 144 VGPRs, 104 SGPRs, 32 B / lane scratch, LDS 44096 B, 3 waves / SIMD
// (the scratch is affine_solve's, as in every instance of the body; the compiler parks 111 /
// 108 / 107 SGPRs of the refs instances in VGPR lanes and 113 / 112 / 112 of the listed ones:
// the index and the slot bytes).  The folds: boot 10 VGPRs, uni fold 74, CU records 36, none
// with scratch; choice 118 VGPRs and 84 B / lane of scratch (the record it builds is indexed
// by the CU's own lists, as fp_bi_refs_choice_kernel's tables are); a few workgroups a picture.
#ifndef XVCGPU_K_FP_BI_AFFINE_H_
#define XVCGPU_K_FP_BI_AFFINE_H_

#include "dev_common.h"
#include "k_affine_me.h"
#include "k_fp_affine.h"
#include "k_fp_bi_refs.h"
#include "xvcgpu_internal.h"

// The affine run's arrays (xvcgpu_frame_pass_bi_affine_args) as the kernels read them
struct FpBiAffineDev {
  xvcgpu_affine_me_block *uni;
  const xvcgpu_affine_me_result *uni_res;
  const uint8_t *uni_slots;
  xvcgpu_affine_me_block *bi;
  const xvcgpu_affine_me_result *bi_res;
  uint8_t *bi_slots;
  xvcgpu_fp_bi_affine_result *choice;
};

__device__ __forceinline__ int fp_bi_affine_num_ref(const FpBiRefsDev &t, int l) {
  return l ? t.num_ref[1] : t.num_ref[0];
}

// The job of the CU's E whose result stands for (l, r): its own, or list 0's twin of a
// re-used list-1 entry
__device__ __forceinline__ int fp_bi_affine_src(const FpBiRefsDev &t, int l, int r) {
  int e = l * t.rmax + r;
#pragma unroll
  for (int rr = 0; rr < XVC_CS_MAX_REFS; rr++)
    if (l == 1 && r == rr && t.same[rr] >= 0) e = t.same[rr];
  return e;
}

// The plain result of (l, r) of CU i; r < num_ref[l]
__device__ __forceinline__ xvcgpu_me_result fp_bi_affine_plain(const FpBiRefsDev &t, int l, int r,
                                                               int i) {
  xvcgpu_me_result q = me2_unsupported_record();
#pragma unroll
  for (int ll = 0; ll < 2; ll++)
#pragma unroll
    for (int rr = 0; rr < XVC_CS_MAX_REFS; rr++)
      if (ll == l && rr == r && rr < t.num_ref[ll]) q = t.res[ll][rr][i];
  return q;
}

// A CU the affine run searched: capable (fp_affine_capable on list 0's first job) and every
// one of its jobs that names a picture carries the boot kernel's flag
__device__ __forceinline__ bool fp_bi_affine_searched(const FpBiRefsDev &t, const FpBiAffineDev &d,
                                                      const xvcgpu_me_block &b00, int i) {
  if (!fp_affine_capable(b00)) return false;
  const size_t at = (size_t)i * 2 * t.rmax;
  bool ok = true;
  for (int e = 0; e < 2 * t.rmax; e++)
    if (d.uni_slots[2 * (at + e)] != XVC_FP_BI_NO_JOB)
      ok = ok && (d.uni[at + e].flags & XVC_AFFINE_ME_HAS_BOOTSTRAP);
  return ok;
}

// :525-531 per (list, picture): the bootstrap of job [i * E + e] = the plain result's vector
// of (l, r) through ClipMv at all three corners, flags = HAS_BOOTSTRAP; an unsupported plain
// result: XVC_AFFINE_ME_NO_JOB.  A job whose first slot byte is XVC_FP_BI_NO_JOB is not
// touched.  grid: ceil(n_listed * E / 256); block: 256.
__global__ void __launch_bounds__(256)
fp_bi_affine_boot_kernel(FpBiRefsDev t, FpBiAffineDev d, const int32_t *order, int n_listed,
                         int n_cus, int pic_w, int pic_h) {
  const int g = blockIdx.x * 256 + threadIdx.x;
  const int per_cu = 2 * t.rmax;
  if (g >= n_listed * per_cu) return;
  const int i = order[g / per_cu], e = g % per_cu;
  if (i < 0 || i >= n_cus) return;
  const size_t at = (size_t)i * per_cu + e;
  if (d.uni_slots[2 * at] == XVC_FP_BI_NO_JOB) return;
  const int l = e / t.rmax, r = e % t.rmax;
  if (r >= fp_bi_affine_num_ref(t, l)) return;
  const xvcgpu_me_result q = fp_bi_affine_plain(t, l, r, i);
  xvcgpu_affine_me_block *j = &d.uni[at];
  int mx = 0, my = 0;
  uint8_t flags = XVC_AFFINE_ME_NO_JOB;
  if (q.subpel_dist != XVCGPU_ME_UNSUPPORTED) {
    mx = q.mv_x;
    my = q.mv_y;
    d_clip_mv(j->x, j->y, pic_w, pic_h, mx, my);
    flags = XVC_AFFINE_ME_HAS_BOOTSTRAP;
  }
#pragma unroll
  for (int k = 0; k < 3; k++) {
    j->bootstrap[k][0] = mx;
    j->bootstrap[k][1] = my;
  }
  j->flags = flags;
}

// The affine search of one class's CUs, all their pictures in one launch: workgroup g takes
// job order[g / per_cu] * per_cu + g % per_cu (wave-uniform), the searched plane from the
// table by the job's first slot byte, with BIPRED the other list's by the second.  A first
// slot byte that names no picture (XVC_FP_BI_NO_JOB) or XVC_AFFINE_ME_NO_JOB: nothing is
// loaded or written.  grid: n_wg; block: 64 * NW.
template <int NW>
__global__ void __launch_bounds__(64 * NW)
affine_me_listed_refs_kernel(PlaneView orig, RefTable refs, const uint8_t *slots, int bd,
                             const xvcgpu_affine_me_block *blocks, const int32_t *order,
                             int n_wg, int per_cu, int n_cus, xvcgpu_affine_me_result *out) {
  const int g = (int)blockIdx.x;
  if (g >= n_wg) return;
  const int cu = __builtin_amdgcn_readfirstlane(order[g / per_cu]);
  if (cu < 0 || cu >= n_cus) return;
  const int job = cu * per_cu + g % per_cu;
  if (slots[2 * job] >= refs.n) return;
  if (blocks[job].flags & XVC_AFFINE_ME_NO_JOB) return;
  affine_me_body<NW>(orig, orig, orig, bd, blocks, n_cus * per_cu, out, &refs, slots, job);
}

// SearchRefIdx<true> over both lists (:484-572) and the jobs of SearchBiIterative (:394-435)
// for every searched CU: prices every (list, picture) in index order, keeps the best per list
// on strict < and the best of list 1's unique pictures, search_list = cost_0 <= cost_1 ? 1 :
// 0, and writes the CU's Rmax refinement jobs: the (s, k) job's geometry, lambda and mvp,
// bootstrap = the affine vectors of (s, k) (the twin's for a re-used entry), other_mv = the
// winner of list 1 - s, flags HAS_BOOTSTRAP | BIPRED, slot bytes {slot[s][k],
// slot[1-s][best_ref[1-s]]}.  choice: the fold's fields, the rest zero until
// fp_bi_affine_choice_kernel.  A CU that was not searched: no-job slots, its record is left
// to the choice kernel.  grid: ceil(n / 256); block: 256.
__global__ void __launch_bounds__(256)
fp_bi_affine_uni_fold_kernel(FpBiRefsDev t, FpBiAffineDev d, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const xvcgpu_me_block b00 = t.me[0][0][i];
  const size_t at = (size_t)i * t.rmax, ue = (size_t)i * 2 * t.rmax;
  if (!fp_bi_affine_searched(t, d, b00, i)) {
    for (int k = 0; k < t.rmax; k++)
      d.bi_slots[2 * (at + k)] = d.bi_slots[2 * (at + k) + 1] = XVC_FP_BI_NO_JOB;
    return;
  }
  xvcgpu_fp_bi_affine_result c;
  memset(&c, 0, sizeof(c));
  uint32_t best_cost[2] = {0xffffffffu, 0xffffffffu}, unique_cost = 0xffffffffu;
  // (a cost is below UINT32_MAX: picture 0 stands only until the first one is priced)
  int best[2] = {0, 0}, best_unique = -1;
#pragma unroll
  for (int l = 0; l < 2; l++)
#pragma unroll
    for (int r = 0; r < XVC_CS_MAX_REFS; r++) {
      c.cost_uni[l][r] = 0xffffffffu;
      if (r >= t.num_ref[l]) continue;
      const xvcgpu_affine_me_block j = d.uni[ue + l * t.rmax + r];
      const xvcgpu_affine_me_result q = d.uni_res[ue + fp_bi_affine_src(t, l, r)];
      const uint32_t bits = t.side_uni[l] + fp_bi_ref_idx_bits(t.num_ref[l], r) + 1 +
                            fp_affine_mvd_bits(j.mvp, q.mv);
      const uint32_t cost = fp_bi_cost(q.dist, bits, j.lambda16);
      c.cost_uni[l][r] = cost;
      if (cost < best_cost[l]) {
        best_cost[l] = cost;
        best[l] = r;
      }
      if (l == 1 && t.same[r] < 0 && cost < unique_cost) {
        unique_cost = cost;
        best_unique = r;
      }
    }
  const int s = best_cost[0] <= best_cost[1] ? 1 : 0, o = 1 - s;
  const int nr_s = fp_bi_affine_num_ref(t, s);
  const int oe = fp_bi_affine_src(t, o, o ? best[1] : best[0]);
  const xvcgpu_affine_me_result qo = d.uni_res[ue + oe];
  const uint8_t oslot = d.uni_slots[2 * (ue + oe)];
  for (int k = 0; k < t.rmax; k++) {
    if (k >= nr_s) {
      d.bi_slots[2 * (at + k)] = d.bi_slots[2 * (at + k) + 1] = XVC_FP_BI_NO_JOB;
      continue;
    }
    const int se = fp_bi_affine_src(t, s, k);
    xvcgpu_affine_me_block j = d.uni[ue + s * t.rmax + k];
    const xvcgpu_affine_me_result qs = d.uni_res[ue + se];
#pragma unroll
    for (int p = 0; p < 3; p++) {
      j.bootstrap[p][0] = qs.mv[p][0];
      j.bootstrap[p][1] = qs.mv[p][1];
      j.other_mv[p][0] = qo.mv[p][0];
      j.other_mv[p][1] = qo.mv[p][1];
    }
    j.flags = XVC_AFFINE_ME_HAS_BOOTSTRAP | XVC_AFFINE_ME_BIPRED;
    j.reserved = 0;
    d.bi[at + k] = j;
    d.bi_slots[2 * (at + k)] = d.uni_slots[2 * (ue + se)];
    d.bi_slots[2 * (at + k) + 1] = oslot;
  }
  c.search_list = s;
  c.cost_list[0] = best_cost[0];
  c.cost_list[1] = best_cost[1];
  c.cost_l1_unique = unique_cost;
  c.best_ref[0] = best[0];
  c.best_ref[1] = best[1];
  c.best_ref_l1_unique = best_unique;
  d.choice[i] = c;
}

// A list's picture, table slot and three corners into a record and a prediction job
__device__ __forceinline__ void fp_bi_affine_set(xvcgpu_fp_bi_affine_result &c,
                                                 xvcgpu_inter_block &p, int l, int ref_idx,
                                                 int slot, const int32_t mv[3][2]) {
#pragma unroll
  for (int ll = 0; ll < 2; ll++)
    if (ll == l) {
      c.ref_idx[ll] = ref_idx;
      p.ref[ll] = (int8_t)slot;
#pragma unroll
      for (int k = 0; k < 3; k++) {
        c.mv[ll][k][0] = p.mv[ll][k][0] = mv[k][0];
        c.mv[ll][k][1] = p.mv[ll][k][1] = mv[k][1];
      }
    }
}

// Prices the CU's refined pairs in picture order from UINT32_MAX on strict < (bits =
// side_bits_bi + for both lists RefIdxBits + 1 + the corner bits against that (l, r) job's
// mvp, :1108-1128; the refinement's dist is halved by the search), ChooseUniOrBi(cost_l0,
// cost_l1_unique, cost_bi) as fp_bi_refs_choice_kernel, and :90: the affine state only where
// cost_affine < plain[i].cost.  Writes choice[i]; where affine wins rewrites the CU's three
// prediction jobs (XVC_INTER_AFFINE, ref[l] = the slot or -1, three corners per used list),
// otherwise leaves the plain choice's.  grid: ceil(n / 256); block: 256.
__global__ void __launch_bounds__(256)
fp_bi_affine_choice_kernel(FpBiRefsDev t, FpBiAffineDev d, int n,
                           const xvcgpu_fp_bi_refs_result *plain, xvcgpu_inter_block *inter) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const xvcgpu_me_block b00 = t.me[0][0][i];
  const xvcgpu_fp_bi_refs_result pl = plain[i];
  xvcgpu_fp_bi_affine_result c;
  if (pl.inter_dir < 0 || pl.inter_dir > 2) {   // (the plain search had no instance)
    memset(&c, 0xff, sizeof(c));
    d.choice[i] = c;
    return;
  }
  memset(&c, 0, sizeof(c));
  c.cost_plain = pl.cost;
  c.cost_affine = c.cost_l1_unique = c.cost_bi = 0xffffffffu;
  c.cost_list[0] = c.cost_list[1] = 0xffffffffu;
  c.search_list = c.best_ref[0] = c.best_ref[1] = c.best_ref_l1_unique = -1;
#pragma unroll
  for (int r = 0; r < XVC_CS_MAX_REFS; r++)
    c.cost_uni[0][r] = c.cost_uni[1][r] = c.bi_cost[r] = 0xffffffffu;
  if (fp_bi_affine_searched(t, d, b00, i)) {
    const xvcgpu_fp_bi_affine_result f = d.choice[i];
    const size_t at = (size_t)i * t.rmax, ue = (size_t)i * 2 * t.rmax;
    // (the fold's indices bound: a record nobody folded must not lead outside the arrays)
    const int s = f.search_list & 1, o = 1 - s;
    const int nr_s = fp_bi_affine_num_ref(t, s), nr_o = fp_bi_affine_num_ref(t, o);
    c.search_list = s;
    c.cost_list[0] = f.cost_list[0];
    c.cost_list[1] = f.cost_list[1];
    c.cost_l1_unique = f.cost_l1_unique;
    c.best_ref[0] = f.best_ref[0];
    c.best_ref[1] = f.best_ref[1];
    c.best_ref_l1_unique = f.best_ref_l1_unique;
#pragma unroll
    for (int r = 0; r < XVC_CS_MAX_REFS; r++) {
      c.cost_uni[0][r] = f.cost_uni[0][r];
      c.cost_uni[1][r] = f.cost_uni[1][r];
    }
    const int bo = d_clip3(s ? f.best_ref[0] : f.best_ref[1], 0, nr_o - 1);
    const int bs = d_clip3(s ? f.best_ref[1] : f.best_ref[0], 0, nr_s - 1);
    const int oe = fp_bi_affine_src(t, o, bo);
    const xvcgpu_affine_me_block jo = d.uni[ue + o * t.rmax + bo];
    const xvcgpu_affine_me_result qo = d.uni_res[ue + oe];
    const uint32_t bits_o =
        t.side_bi + fp_bi_ref_idx_bits(nr_o, bo) + 1 + fp_affine_mvd_bits(jo.mvp, qo.mv);
    uint32_t cost_bi = 0xffffffffu;
    int best_k = -1;
#pragma unroll
    for (int k = 0; k < XVC_CS_MAX_REFS; k++) {
      if (k >= nr_s) continue;
      const xvcgpu_affine_me_result r = d.bi_res[at + k];
      const xvcgpu_affine_me_block j = d.uni[ue + s * t.rmax + k];
      const uint32_t cost = fp_bi_cost(
          r.dist, bits_o + fp_bi_ref_idx_bits(nr_s, k) + 1 + fp_affine_mvd_bits(j.mvp, r.mv),
          j.lambda16);
      c.bi_cost[k] = cost;
      if (cost < cost_bi) {
        cost_bi = cost;
        best_k = k;
      }
    }
    c.cost_bi = cost_bi;
    const uint32_t cost0 = c.cost_list[0], cost1u = c.cost_l1_unique;
    const int dir = (cost_bi <= cost0 && cost_bi <= cost1u) ? 2 : (cost0 <= cost1u ? 0 : 1);
    c.cost_affine = dir == 2 ? cost_bi : (dir == 0 ? cost0 : cost1u);
    if (c.cost_affine < c.cost_plain) {   // (:90: the first run's state on a tie)
      xvcgpu_inter_block p;
      memset(&p, 0, sizeof(p));
      p.x = b00.x;
      p.y = b00.y;
      p.w = b00.w;
      p.h = b00.h;
      p.flags = XVC_INTER_AFFINE;
      p.ref[0] = p.ref[1] = -1;
      c.use_affine = 1;
      c.inter_dir = dir;
      c.ref_idx[0] = c.ref_idx[1] = -1;
      c.cost = c.cost_affine;
      if (dir == 2) {
        // (no step priced below UINT32_MAX: the pair stays the uni-directional one)
        const int ks = best_k < 0 ? bs : best_k;
        const int se = fp_bi_affine_src(t, s, ks);
        const xvcgpu_affine_me_result qs = best_k < 0 ? d.uni_res[ue + se] : d.bi_res[at + ks];
        fp_bi_affine_set(c, p, s, ks, d.uni_slots[2 * (ue + se)], qs.mv);
        fp_bi_affine_set(c, p, o, bo, d.uni_slots[2 * (ue + oe)], qo.mv);
      } else {
        const int r = d_clip3(dir == 0 ? f.best_ref[0] : f.best_ref_l1_unique, 0,
                              fp_bi_affine_num_ref(t, dir) - 1);
        const int e = fp_bi_affine_src(t, dir, r);
        const xvcgpu_affine_me_result q = d.uni_res[ue + e];
        fp_bi_affine_set(c, p, dir, r, d.uni_slots[2 * (ue + e)], q.mv);
      }
      for (int comp = 0; comp < 3; comp++) {
        p.comp = (uint8_t)comp;
        inter[3 * i + comp] = p;
      }
    }
  }
  if (!c.use_affine) {
    c.inter_dir = pl.inter_dir;
    c.cost = pl.cost;
#pragma unroll
    for (int l = 0; l < 2; l++) {
      c.ref_idx[l] = pl.ref_idx[l];
#pragma unroll
      for (int k = 0; k < 3; k++) {
        c.mv[l][k][0] = pl.mv[l][0];
        c.mv[l][k][1] = pl.mv[l][1];
      }
    }
  }
  d.choice[i] = c;
}

// cu_info_from_choice_refs_kernel with corners: a used list of an affine CU gets UL, UR, DL
// and DR = UR + DL - UL, a used list of a plain CU its vector four times, an unused list
// zeros with ref_poc -1.  grid: ceil(n / 256); block: 256.
__global__ void __launch_bounds__(256)
cu_info_from_bi_affine_choice_kernel(const xvcgpu_me_block *blocks,
                                     const xvcgpu_fp_bi_affine_result *choice,
                                     const int32_t *nnz, const int32_t *luma_tx_index, int n,
                                     int qp_y, int qp_c, FpBiRefsPocs pocs,
                                     xvcgpu_cu_info *cus) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const xvcgpu_me_block b = blocks[i];
  const xvcgpu_fp_bi_affine_result ch = choice[i];
  const bool used[2] = {ch.inter_dir == 0 || ch.inter_dir == 2,
                        ch.inter_dir == 1 || ch.inter_dir == 2};
  int poc[2] = {-1, -1};
#pragma unroll
  for (int l = 0; l < 2; l++)
#pragma unroll
    for (int r = 0; r < XVC_CS_MAX_REFS; r++)
      if (used[l] && ch.ref_idx[l] == r) poc[l] = pocs.poc[l][r];
  xvcgpu_cu_info c;
  c.x = (uint16_t)b.x;
  c.y = (uint16_t)b.y;
  c.w = b.w;
  c.h = b.h;
  c.intra = 0;
  c.cbf_luma = nnz[luma_tx_index ? luma_tx_index[i] : i] != 0;
  c.qp_y = (int8_t)qp_y;
  c.qp_c = (int8_t)qp_c;
  c.ref_idx0 = used[0] ? (int8_t)ch.ref_idx[0] : -1;
  c.reserved = 0;
  const bool affine = ch.use_affine == 1;
#pragma unroll
  for (int l = 0; l < 2; l++) {
    c.ref_poc[l] = poc[l];
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const int s = affine && k < 3 ? k : 0;
      c.mv[l][k][0] = used[l] ? ch.mv[l][s][0] : 0;
      c.mv[l][k][1] = used[l] ? ch.mv[l][s][1] : 0;
    }
    if (affine && used[l]) {
      c.mv[l][XVC_CORNER_DR][0] = ch.mv[l][1][0] + ch.mv[l][2][0] - ch.mv[l][0][0];
      c.mv[l][XVC_CORNER_DR][1] = ch.mv[l][1][1] + ch.mv[l][2][1] - ch.mv[l][0][1];
    }
  }
  cus[i] = c;
}

#endif  // XVCGPU_K_FP_BI_AFFINE_H_
