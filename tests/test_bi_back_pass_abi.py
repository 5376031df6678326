"""CPU-side checks of the low-delay B pass's boundary: what pipeline.BiRefsFramePass(
low_delay=True) hands to xvcgpu_frame_pass_bi_back - the args block's tables and the sizes of
the work arrays - against what xvc_gpu::FramePassBiRefs with RefLists::low_delay hands to it,
the C++ class running in a plain g++ program over a stand-in for the C ABI that records the
allocations and the call (no GPU, no library), the Python class over a stand-in context."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
HOST = os.path.join(ROOT, "xvc_amd", "host")
W, H, BD, QP, CUR_POC = 104, 72, 10, 32, 20
LISTS = ((16, 12), (12, 4, 0))

_PROGRAM = r'''
#include <cstdio>
#include <cstdlib>
#include <map>
#include "xvc_frame_pass.h"

static std::map<const void *, size_t> g_size;
static size_t size_of(const void *p) { return p ? g_size[p] : 0; }
extern "C" {
xvcgpu_status xvcgpu_malloc(xvcgpu_ctx *, size_t bytes, void **out) {
  *out = std::malloc(bytes ? bytes : 1);
  g_size[*out] = bytes;
  return XVCGPU_OK;
}
xvcgpu_status xvcgpu_free(xvcgpu_ctx *, void *p) {
  std::free(p);
  return XVCGPU_OK;
}
void xvcgpu_destroy(xvcgpu_ctx *) {}
const char *xvcgpu_last_error(const xvcgpu_ctx *) { return ""; }
xvcgpu_status xvcgpu_memcpy_h2d(xvcgpu_ctx *, void *, const void *, size_t) { return XVCGPU_OK; }
xvcgpu_status xvcgpu_memset(xvcgpu_ctx *, void *, int, size_t) { return XVCGPU_OK; }
xvcgpu_status xvcgpu_picture_create(xvcgpu_ctx *, int, int, int, xvcgpu_picture **out) {
  *out = reinterpret_cast<xvcgpu_picture *>(std::malloc(1));
  return XVCGPU_OK;
}
void xvcgpu_picture_destroy(xvcgpu_picture *p) { std::free(p); }
xvcgpu_status xvcgpu_me_plan_create(xvcgpu_ctx *, const xvcgpu_me_block *, int, int,
                                    xvcgpu_me_plan **) { return XVCGPU_UNSUPPORTED; }
xvcgpu_status xvcgpu_me_plan_counts(const xvcgpu_me_plan *, int32_t *) { return XVCGPU_UNSUPPORTED; }
void xvcgpu_me_plan_destroy(xvcgpu_ctx *, xvcgpu_me_plan *) {}
xvcgpu_status xvcgpu_frame_pass_bi_refs(xvcgpu_ctx *, const xvcgpu_frame_pass_bi_refs_args *,
                                        const xvcgpu_me_plan *const[2][XVC_CS_MAX_REFS], int) {
  std::printf("entry bi_refs\n");
  return XVCGPU_OK;
}
xvcgpu_status xvcgpu_frame_pass_bi_refs_aqp(xvcgpu_ctx *, const xvcgpu_frame_pass_bi_refs_args *,
                                            const xvcgpu_aqp_args *,
                                            const xvcgpu_me_plan *const[2][XVC_CS_MAX_REFS], int) {
  std::printf("entry bi_refs_aqp\n");
  return XVCGPU_OK;
}
xvcgpu_status xvcgpu_frame_pass_bi_back(xvcgpu_ctx *, const xvcgpu_frame_pass_bi_refs_args *b,
                                        uint32_t *cost, const xvcgpu_aqp_args *q,
                                        const xvcgpu_me_plan *const plans[2][XVC_CS_MAX_REFS],
                                        int phases) {
  std::printf("entry bi_back\nflag %d\nq %d\nphases %d\n", b->force_l1_mvd_zero, q != nullptr,
              phases);
  std::printf("num_ref %d %d\nn_refs %d\n", b->num_ref[0], b->num_ref[1], b->n_refs);
  std::printf("side %u %u %u\n", b->side_bits_uni[0], b->side_bits_uni[1], b->side_bits_bi);
  std::printf("p %d %d %d %d %d %d %d %d %d %d\n", b->p.n_cus, b->p.n_cus_total,
              b->p.max_block_size, b->p.qp_y, b->p.qp_c, b->p.form, b->p.map_stride,
              b->p.db_y_begin, b->p.db_y_end, b->p.shift_bitdepth);
  for (int r = 0; r < XVC_CS_MAX_REFS; r++) std::printf("same %d\n", b->same_poc_in_l0[r]);
  for (int l = 0; l < 2; l++)
    for (int r = 0; r < b->num_ref[l]; r++)
      std::printf("entry %d %d slot %d poc %d me %zu res %zu plan %d\n", l, r, b->slot[l][r],
                  b->ref_poc[l][r], size_of(b->d_me[l][r]), size_of(b->d_results[l][r]),
                  plans[l][r] != nullptr);
  std::printf("work %zu %zu %zu %zu %zu %zu\n", size_of(b->d_bi_jobs), size_of(b->d_bi_results),
              size_of(b->d_bi_slots), size_of(b->d_choice), size_of(b->d_inter), size_of(cost));
  return XVCGPU_OK;
}
}

int main(int argc, char **) {
  xvc_gpu::Context ctx(reinterpret_cast<xvcgpu_ctx *>(0x10));
  xvcgpu_picture *h[5];
  for (int k = 0; k < 5; k++) xvcgpu_picture_create(nullptr, 0, 0, 0, &h[k]);
  xvc_gpu::Picture o(ctx, h[0]), rec(ctx, h[1]), p16(ctx, h[2]), p12(ctx, h[3]), p4(ctx, h[4]);
  xvc_gpu::Picture p0(ctx, h[0]);
  {
    xvc_gpu::FramePassBiRefs::RefLists lists(20, {16, 12}, {12, 4, 0}, true);
    xvc_gpu::FramePassBiRefs pass(ctx, 104, 72, 10, 32, lists);
    if (argc > 1) pass.SetAdaptiveQp(13);
    std::vector<const xvc_gpu::Picture *> pics[2] = {{&p16, &p12}, {&p12, &p4, &p0}};
    pass.Run(o, pics, &rec);
    const std::vector<size_t> work = pass.WorkArrayBytes();
    std::printf("class");
    for (size_t k = 0; k < work.size(); k++) std::printf(" %zu", work[k]);
    std::printf("\nlow_delay %d\n", pass.low_delay());
  }
  // the refusals: a forward reference with low_delay, back-only lists without
  int refused = 0;
  try {
    xvc_gpu::FramePassBiRefs::RefLists lists(8, {4, 0}, {12}, true);
    xvc_gpu::FramePassBiRefs pass(ctx, 104, 72, 10, 32, lists);
  } catch (const xvc_gpu::Error &e) {
    refused += e.status == XVCGPU_INVALID_ARGUMENT;
  }
  try {
    xvc_gpu::FramePassBiRefs::RefLists lists;
    lists.cur_poc = 20;
    lists.poc[0] = {16, 12};
    lists.poc[1] = {16, 12};
    xvc_gpu::FramePassBiRefs pass(ctx, 104, 72, 10, 32, lists);
  } catch (const xvc_gpu::Error &e) {
    refused += e.status == XVCGPU_INVALID_ARGUMENT;
  }
  {   // and a two-directional picture goes where it went
    xvc_gpu::FramePassBiRefs::RefLists lists = {8, {4, 0}, {12}};
    xvc_gpu::FramePassBiRefs pass(ctx, 104, 72, 10, 32, lists);
    std::vector<const xvc_gpu::Picture *> pics[2] = {{&p4, &p0}, {&p12}};
    pass.Run(o, pics, &rec);
  }
  std::printf("refused %d\n", refused);
  return 0;
}
'''


class _Buf:
    def __init__(self, ctx, nbytes):
        self.nbytes = nbytes
        self._keep = C.create_string_buffer(max(1, nbytes))
        self.ptr = C.addressof(self._keep)
        ctx.sizes[self.ptr] = nbytes

    def free(self):
        pass


class _Pic:
    def __init__(self, k):
        self.h_pic = 0x1000 + 16 * k

    def destroy(self):
        pass


class _Lib:
    """The entry points the pass object calls without a device: they record."""

    def __init__(self, ctx):
        self.ctx = ctx

    def xvcgpu_memset(self, *a):
        return 0

    def xvcgpu_frame_pass_bi_back(self, h, a, cost, q, plans, phases):
        self.ctx.calls.append(("bi_back", a._obj, cost, q is not None, plans, phases))
        return 0


class _Ctx:
    """What pipeline.BiRefsFramePass needs of api.Context to be built and to issue run()."""

    def __init__(self):
        self.h, self.sizes, self.calls, self.n_pics = 0x10, {}, [], 0
        self.lib = _Lib(self)

    def alloc(self, nbytes):
        return _Buf(self, nbytes)

    def buffer(self, arr):
        return _Buf(self, np.ascontiguousarray(arr).nbytes)

    def h2d(self, ptr, arr):
        pass

    def picture(self, *a):
        self.n_pics += 1
        return _Pic(self.n_pics)

    def _check(self, st):
        assert st == 0


def _python_side(aqp):
    from xvc_amd import api, pipeline
    ctx = _Ctx()
    kw = {"aqp_strength": 13} if aqp else {}
    fp = pipeline.BiRefsFramePass(ctx, W, H, BD, QP, cur_poc=CUR_POC, ref_pocs=LISTS,
                                  low_delay=True, **kw)
    by_poc = {poc: ctx.picture() for poc in (16, 12, 4, 0)}
    refs = [[by_poc[p] for p in LISTS[l]] for l in range(2)]
    fp.run(ctx.picture(), refs, ctx.picture())
    (entry, a, cost, has_q, plans, phases), = ctx.calls
    size = lambda p: ctx.sizes[p] if p else 0       # noqa: E731
    out = ["entry " + entry, "flag %d" % a.force_l1_mvd_zero, "q %d" % has_q,
           "phases %d" % phases, "num_ref %d %d" % tuple(a.num_ref), "n_refs %d" % a.n_refs,
           "side %d %d %d" % (a.side_bits_uni[0], a.side_bits_uni[1], a.side_bits_bi),
           "p %d %d %d %d %d %d %d %d %d %d" % (
               a.p.n_cus, a.p.n_cus_total, a.p.max_block_size, a.p.qp_y, a.p.qp_c, a.p.form,
               a.p.map_stride, a.p.db_y_begin, a.p.db_y_end, a.p.shift_bitdepth)]
    out += ["same %d" % a.same_poc_in_l0[r] for r in range(api.CS_MAX_REFS)]
    for l in range(2):
        for r in range(a.num_ref[l]):
            out.append("entry %d %d slot %d poc %d me %d res %d plan %d" % (
                l, r, a.slot[l][r], a.ref_poc[l][r], size(a.d_me[l][r]), size(a.d_results[l][r]),
                bool(plans[l][r])))
    work = (size(a.d_bi_jobs), size(a.d_bi_results), size(a.d_bi_slots), size(a.d_choice),
            size(a.d_inter), size(cost))
    out.append("work %d %d %d %d %d %d" % work)
    assert work[5] == 4 * api.CS_MAX_REFS * fp.desc.n_cus
    fp.destroy()
    return out, work


def test_python_and_cpp_hand_the_same_block_to_the_entry(tmp_path):
    src = tmp_path / "back.cc"
    src.write_text(_PROGRAM)
    exe = str(tmp_path / "back")
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Wextra", "-Werror", "-I", INC, "-I",
                           HOST, str(src), "-o", exe])
    for aqp in (False, True):
        lines = subprocess.check_output([exe] + (["aqp"] if aqp else [])).decode().splitlines()
        cut = lines.index("entry bi_back")
        end = next(k for k, v in enumerate(lines) if v.startswith("class"))
        py, work = _python_side(aqp)
        assert lines[cut:end] == py, (lines[cut:end], py)
        # the class says the sizes it allocated, and they are what it handed over
        assert lines[end] == "class " + " ".join(str(v) for v in work)
        assert lines[end + 1:] == ["low_delay 1", "entry bi_refs", "refused 2"]
        assert "flag 1" in py and ("q 1" if aqp else "q 0") in py and "same 1" in py
