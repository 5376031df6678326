"""CPU-side checks of the B pass's boundary: the two new structs as the C compiler lays
them out against their ctypes / numpy mirrors in xvc_amd/api.py, and xvc_gpu::FramePassBi
against the public headers with plain g++."""
import ctypes as C
import os
import subprocess

import bi_pass_model as bm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")

_BI_FIELDS = ("p", "ref1", "d_me_l1", "d_results_l1", "ref_poc_l1", "side_bits_uni",
              "side_bits_bi", "d_bi_jobs", "d_bi_results", "d_choice", "d_inter")
_RESULT_FIELDS = ("inter_dir", "search_list", "cost_uni", "cost_bi", "cost", "mv", "bi_mv")


def test_bi_struct_layouts_match_header(tmp_path):
    from xvc_amd import api
    what = ["sizeof(xvcgpu_frame_pass_bi_args)", "sizeof(xvcgpu_fp_bi_result)"] + \
        ["offsetof(xvcgpu_frame_pass_bi_args, %s)" % f for f in _BI_FIELDS] + \
        ["offsetof(xvcgpu_fp_bi_result, %s)" % f for f in _RESULT_FIELDS]
    src = tmp_path / "t.c"
    src.write_text("#include <stdio.h>\n#include <stddef.h>\n#include \"xvcgpu.h\"\nint main(){"
                   + "".join('printf("%%zu\\n", %s);' % w for w in what) + "return 0;}")
    exe = str(tmp_path / "t")
    subprocess.check_call(["gcc", "-std=c99", "-I", INC, str(src), "-o", exe])
    out = [int(v) for v in subprocess.check_output([exe]).decode().split()]
    A, R = api.FramePassBiArgs, api.FP_BI_RESULT_DTYPE
    assert out == [C.sizeof(A), R.itemsize] + [getattr(A, f).offset for f in _BI_FIELDS] + \
        [R.fields[f][1] for f in _RESULT_FIELDS]
    # the block embeds the P pass's, unchanged, at its start
    assert A.p.offset == 0 and A.p.size == C.sizeof(api.FramePassArgs) == 240
    assert R.itemsize == 48 and R == bm.CHOICE_DTYPE


def test_frame_pass_bi_host_class_compiles(tmp_path):
    """xvc_gpu::FramePassBi (xvc_amd/host/xvc_frame_pass.h): both constructors, Run and the
    accessors instantiated, syntax only - no GPU, no library."""
    src = tmp_path / "bi.cc"
    src.write_text(r'''
#include "xvc_frame_pass.h"
int run(const xvc_gpu::Context &ctx, const xvc_gpu::Picture &o, const xvc_gpu::Picture &r0,
        const xvc_gpu::Picture &r1, xvc_gpu::Picture *rec) {
  xvc_gpu::FramePassBi grid(ctx, 104, 72, 10, 32);
  grid.Run(o, r0, r1, rec);
  std::vector<xvc_gpu::CuRect> parts(1);
  xvc_gpu::FramePassBi part(ctx, 64, 64, 10, 32, parts);
  part.Run(o, r0, r1, rec, 0, 4);
  uint64_t ssd, samples;
  part.Ssd(&ssd, &samples);
  const std::vector<xvcgpu_fp_bi_result> c = part.Choices();
  return static_cast<int>(c.size() + part.MotionVectors(1).size()) + grid.num_cus();
}
''')
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Wextra", "-Werror", "-fsyntax-only",
                           "-I", INC, "-I", os.path.join(ROOT, "xvc_amd", "host"), str(src)])
