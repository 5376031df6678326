"""CPU-side checks of the B pass's boundary: the entry points exported by the built library,
the two structs as the C compiler lays them out against their ctypes / numpy mirrors in
xvc_amd/api.py, and xvc_gpu::FramePassBiRefs against the public headers with plain g++."""
import ctypes as C
import os
import subprocess

import bi_refs_pass_model as rm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")

_NEW_SYMBOLS = ("xvcgpu_fp_bi_refs_uni_fold", "xvcgpu_fp_bi_refs_choice",
                "xvcgpu_cu_info_from_choice_refs", "xvcgpu_bipred_search_refs_planned",
                "xvcgpu_frame_pass_bi_refs")
_ARGS_FIELDS = ("p", "num_ref", "same_poc_in_l0", "force_l1_mvd_zero", "n_refs", "refs", "slot",
                "ref_poc", "d_me", "d_results", "side_bits_uni", "side_bits_bi", "d_bi_jobs",
                "d_bi_results", "d_bi_slots", "d_choice", "d_inter")
_RESULT_FIELDS = ("inter_dir", "search_list", "ref_idx", "mv", "cost_list", "cost_l1_unique",
                  "cost_bi", "cost", "best_ref", "best_ref_l1_unique", "cost_uni", "bi_cost",
                  "bi_mv")


def test_entry_points_are_exported():
    from xvc_amd import api
    lib = C.CDLL(os.path.join(ROOT, "xvc_amd", "libxvcgpu.so"))
    for name in _NEW_SYMBOLS:
        assert name in api.SYMBOLS and hasattr(lib, name), name


def test_struct_layouts_match_header(tmp_path):
    from xvc_amd import api
    what = ["sizeof(xvcgpu_frame_pass_bi_refs_args)", "sizeof(xvcgpu_fp_bi_refs_result)",
            "sizeof(xvcgpu_frame_pass_args)",
            "(size_t)XVC_CS_MAX_REFS", "(size_t)XVC_FP_BI_MAX_REF_PICS",
            "(size_t)XVC_FP_BI_NO_JOB"] + \
        ["offsetof(xvcgpu_frame_pass_bi_refs_args, %s)" % f for f in _ARGS_FIELDS] + \
        ["offsetof(xvcgpu_fp_bi_refs_result, %s)" % f for f in _RESULT_FIELDS]
    src = tmp_path / "t.c"
    src.write_text("#include <stdio.h>\n#include <stddef.h>\n#include \"xvcgpu.h\"\nint main(){"
                   + "".join('printf("%%zu\\n", %s);' % w for w in what) + "return 0;}")
    exe = str(tmp_path / "t")
    subprocess.check_call(["gcc", "-std=c99", "-I", INC, str(src), "-o", exe])
    out = [int(v) for v in subprocess.check_output([exe]).decode().split()]
    A, R = api.FramePassBiRefsArgs, api.FP_BI_REFS_RESULT_DTYPE
    assert out == [C.sizeof(A), R.itemsize,
                   C.sizeof(api.FramePassArgs), api.CS_MAX_REFS, api.FP_BI_MAX_REF_PICS,
                   api.FP_BI_NO_JOB] + [getattr(A, f).offset for f in _ARGS_FIELDS] + \
        [R.fields[f][1] for f in _RESULT_FIELDS]
    # the block embeds the P pass's, unchanged, at its start
    assert A.p.offset == 0 and A.p.size == C.sizeof(api.FramePassArgs) == 240
    assert R.itemsize == 124 and R == rm.CHOICE_DTYPE
    assert (api.CS_MAX_REFS, api.FP_BI_NO_JOB) == (rm.MAX_REFS, rm.NO_JOB)


def test_ref_list_tables_of_the_sets():
    """pipeline.ref_list_tables derives what the model's tables() and the reference report
    (test_bi_refs_pass_model.py compares the latter two), and a back-only picture is named."""
    import pytest
    from xvc_amd import pipeline
    for lists in rm.SETS.values():
        _, same, distinct, slot = rm.tables(lists)
        assert pipeline.ref_list_tables(rm.CUR_POC, lists) == (same, distinct, slot, False)
    assert pipeline.ref_list_tables(8, ((4, 0), (0, 4))) == ([1, 0], [4, 0], [[0, 1], [1, 0]], True)
    with pytest.raises(ValueError, match="only back references"):
        pipeline.BiRefsFramePass(None, 64, 64, ref_pocs=((4, 0), (0, 4)))


def test_frame_pass_bi_refs_host_class_compiles(tmp_path):
    """xvc_gpu::FramePassBiRefs (xvc_amd/host/xvc_frame_pass.h): both constructors, Run and
    the accessors instantiated, syntax only - no GPU, no library."""
    src = tmp_path / "bi.cc"
    src.write_text(r'''
#include "xvc_frame_pass.h"
int run(const xvc_gpu::Context &ctx, const xvc_gpu::Picture &o, const xvc_gpu::Picture &r0,
        const xvc_gpu::Picture &r1, xvc_gpu::Picture *rec) {
  xvc_gpu::FramePassBiRefs::RefLists lists;
  lists.cur_poc = 8;
  lists.poc[0] = {4, 0};
  lists.poc[1] = {0, 12};
  xvc_gpu::FramePassBiRefs grid(ctx, 104, 72, 10, 32, lists);
  std::vector<const xvc_gpu::Picture *> pics[2] = {{&r0, &r1}, {&r1, &r0}};
  grid.Run(o, pics, rec);
  std::vector<xvc_gpu::CuRect> parts(1);
  xvc_gpu::FramePassBiRefs part(ctx, 64, 64, 10, 32, lists, parts);
  part.Run(o, pics, rec);
  uint64_t ssd, samples;
  part.Ssd(&ssd, &samples);
  const std::vector<xvcgpu_fp_bi_refs_result> c = part.Choices();
  return static_cast<int>(c.size()) + grid.num_cus() + part.same_poc_in_l0(0);
}
''')
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Wextra", "-Werror", "-fsyntax-only",
                           "-I", INC, "-I", os.path.join(ROOT, "xvc_amd", "host"), str(src)])
