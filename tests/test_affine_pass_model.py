"""The P frame pass with affine motion without a GPU: the search the model rests on against
the reference (where it is built), the bootstrap, the vector bits, the tie rule, the
conditions the scenes were built for, the Python and the C++ job lists byte for byte, the
struct layouts against the header, the new entry points' symbols and the refusals of
pipeline.FramePass (tests/affine_pass_model.py is the model)."""
import ctypes as C
import os
import subprocess
import types

import numpy as np
import pytest

import affine_pass_model as fm
import bi_refs_pass_model as rm
import oracle_affine_me as oa
import oracle_frame
import oracle_lib as ol

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("grid10", "grid8", "part10")
ENTRY_POINTS = ("xvcgpu_fp_affine_boot", "xvcgpu_affine_me_listed", "xvcgpu_fp_affine_choice",
                "xvcgpu_cu_info_from_affine_choice", "xvcgpu_frame_pass_affine")


@pytest.fixture(scope="module")
def xo():
    return ol.Lib("xo")


@pytest.fixture(scope="module")
def pipeline():
    from xvc_amd import build
    build.build()
    from xvc_amd import pipeline as p
    return p


@pytest.mark.skipif(not ol.have_ref(), reason="oracle/_ref not built")
@pytest.mark.parametrize("name", NAMES)
def test_affine_search_of_the_scenes_equals_reference(xo, pipeline, name):
    """Every affine job of the scene - bootstrapped from the plain search - through the
    reference's MotionEstAffine and the oracle's: the same record."""
    xr = ol.Lib("xr")
    pw, ph, bd, _, orig, ref = fm.scene(name)
    _, jobs, ares, _, _, order, _ = fm.search(xo, name)
    assert len(order) >= 23
    for i in order:
        got = oa.affine_me(xr, bd, jobs[i], pw, ph, orig[0], ref[0], fm.BL)
        # (the reference's function does not say how many iterations it ran)
        assert np.array_equal(got["mv"], ares[i]["mv"]) and got["dist"] == ares[i]["dist"], \
            (name, i, got, ares[i])


def _clip(x, y, pw, ph, mx, my):
    """ClipMv (inter_prediction.cc) restated"""
    lo_x, lo_y = -((64 + 8 + x - 1) << 4), -((64 + 8 + y - 1) << 4)
    hi_x, hi_y = (pw + 8 - x - 1) << 4, (ph + 8 - y - 1) << 4
    return min(max(mx, lo_x), hi_x), min(max(my, lo_y), hi_y)


def test_bootstrap_is_the_clipped_plain_vector_three_times(xo, pipeline):
    """DeriveMvAffine(mv, mv): ClipMv at the first two corners, the third derived from two
    equal ones is the first, clipped again.  Planted vectors of +-3000 make ClipMv act."""
    pw, ph = fm.INPUTS["part10"][:2]
    d = fm.descriptors("part10")
    jobs0, order, n_class = d.affine_jobs()
    assert n_class == [18, 4, 1]
    rng = np.random.default_rng(3)
    res = np.zeros(d.n_cus, ol.MERES_DTYPE)
    res["mv_x"], res["mv_y"] = rng.integers(-60, 61, d.n_cus), rng.integers(-60, 61, d.n_cus)
    res["mv_x"][order[::3]] = rng.choice([-3000, 3000], len(order[::3]))
    res["mv_y"][order[1::3]] = rng.choice([-3000, 3000], len(order[1::3]))
    res["subpel_dist"][order[5]] = fm.NONE
    jobs = fm.boot(xo, res, order, pw, ph, jobs0)
    clipped = 0
    for i in range(d.n_cus):
        j = jobs[i]
        if i not in order:
            assert j.tobytes() == jobs0[i].tobytes()
            continue
        if i == order[5]:
            assert int(j["flags"]) == fm.NO_JOB and not j["bootstrap"].any()
            continue
        mv = _clip(int(j["x"]), int(j["y"]), pw, ph, int(res["mv_x"][i]), int(res["mv_y"][i]))
        clipped += mv != (int(res["mv_x"][i]), int(res["mv_y"][i]))
        assert int(j["flags"]) == fm.HAS_BOOTSTRAP
        assert j["bootstrap"].tolist() == [list(mv)] * 3
        # the third corner of two equal ones (:624-627) is the first
        w, h = int(j["w"]), int(j["h"])
        assert (mv[0] - (mv[1] - mv[1]) * h // w, mv[1] + (mv[0] - mv[0]) * h // w) == mv
        # nothing but flags and bootstrap moved
        back = j.copy()
        back["flags"], back["bootstrap"] = 0, 0
        assert back.tobytes() == jobs0[i].tobytes()
    assert clipped >= 8


def test_vector_bits_are_the_oracles(xo):
    rng = np.random.default_rng(4)
    b = np.zeros(1, ol.ME_DTYPE)[0]
    for _ in range(400):
        mvp = rng.integers(-900, 900, (3, 2))
        mv = mvp + rng.integers(-700, 700, (3, 2)) * int(rng.integers(0, 2))
        exp = sum(int(xo._mvd_bits(int(mvp[k][0]), int(mvp[k][1]), int(mv[k][0]), int(mv[k][1]), 0))
                  for k in (0, 1))
        assert fm.corner_bits(mvp, mv) == exp
        for fullpel in (0, 1):
            b["mvp_x"], b["mvp_y"], b["fullpel_mv"] = mvp[0][0], mvp[0][1], fullpel
            assert rm.mvd_bits(b, (int(mv[2][0]), int(mv[2][1]))) == int(xo._mvd_bits(
                int(mvp[0][0]), int(mvp[0][1]), int(mv[2][0]), int(mv[2][1]), 2 * fullpel))


def _one_cu(dist_plain, dist_affine, lambda16=fm.LAMBDA16, w=16, h=16, flags=fm.HAS_BOOTSTRAP,
            fullpel=0):
    from xvc_amd import api
    me = np.zeros(1, api.ME_DTYPE)
    me["w"], me["h"], me["lambda16"], me["fullpel_mv"] = w, h, lambda16, fullpel
    res = np.zeros(1, api.MERES_DTYPE)
    res["mv_x"], res["mv_y"], res["subpel_dist"] = 16, -8, dist_plain
    jobs = np.zeros(1, api.AFFINE_ME_DTYPE)
    jobs["w"], jobs["h"], jobs["lambda16"], jobs["flags"] = w, h, lambda16, flags
    ares = np.zeros(1, api.AFFINE_ME_RESULT_DTYPE)
    ares["mv"], ares["dist"], ares["iterations"] = [[16, -8], [20, -8], [16, -4]], dist_affine, 2
    return me, res, jobs, ares


def test_tie_keeps_the_plain_state(pipeline):
    """best_cost <= cost keeps the first run's state (inter_search.cc:90): affine wins only
    when strictly cheaper; prices use the whole 64-bit product."""
    # plain: bits 1 + 1 + eg(4) + eg(-2) = 2 + 7 + 5; affine: 2 + eg(4) + eg(-2) + eg(5) + eg(-2)
    bits_p = 2 + rm.eg_bits(4) + rm.eg_bits(-2)
    bits_a = bits_p + rm.eg_bits(5) + rm.eg_bits(-2)
    lam = fm.LAMBDA16
    gap = ((bits_a * lam) >> 16) - ((bits_p * lam) >> 16)
    for delta, affine in ((0, 0), (1, 0), (-1, 1)):
        choice, inter = fm.choice_fold(*_one_cu(1000 + gap, 1000 + delta))
        c = choice[0]
        assert int(c["cost_plain"]) == 1000 + gap + ((bits_p * lam) >> 16)
        assert int(c["cost_affine"]) == int(c["cost_plain"]) + delta
        assert int(c["use_affine"]) == affine and int(inter[0]["flags"]) == affine
        assert int(c["cost"]) == min(int(c["cost_plain"]), int(c["cost_affine"]))
        assert c["mv"].tolist() == ([[16, -8], [20, -8], [16, -4]] if affine else [[16, -8]] * 3)
        assert inter["ref"].tolist() == [[0, -1]] * 3 and inter["comp"].tolist() == [0, 1, 2]
    # a lambda whose product passes 2^32: not cut to 32 bits
    c = fm.choice_fold(*_one_cu(5, 5, lambda16=0xfff00000))[0][0]
    assert int(c["cost_plain"]) == (5 + ((bits_p * 0xfff00000) >> 16)) & fm.NONE
    assert (bits_p * 0xfff00000) >> 32
    # not capable (a side of 8, a fullpel job, a job without bootstrap): the plain state
    for kw in (dict(w=8), dict(h=8), dict(fullpel=1), dict(flags=0), dict(flags=fm.NO_JOB)):
        c = fm.choice_fold(*_one_cu(10 ** 6, 1, **kw))[0][0]
        assert (int(c["use_affine"]), int(c["cost_affine"])) == (0, fm.NONE), kw
        assert c["mv"].tolist() == [[16, -8]] * 3 and not int(c["dist_affine"])
    # an unsupported plain search: all ones, jobs that name no list
    choice, inter = fm.choice_fold(*_one_cu(fm.NONE, 1))
    assert (choice.view(np.uint8) == 0xff).all() and inter["ref"].tolist() == [[-1, -1]] * 3


@pytest.mark.parametrize("name", NAMES)
def test_scenes_exercise_the_choice(xo, pipeline, name):
    """At least 4 CUs choose affine and 4 capable ones plain; on the partition affine wins
    in all three height classes and plain in at least two."""
    d = fm.descriptors(name)
    _, jobs, ares, choice, inter, order, n_class = fm.search(xo, name)
    use = choice["use_affine"]
    assert set(use.tolist()) <= {0, 1}
    assert int(use.sum()) >= 4 and int((use[order] == 0).sum()) >= 4
    assert not use[[i for i in range(d.n_cus) if i not in order]].any()
    assert len(order) == 24 - (name == "part10")
    if name == "part10":
        by_h = {h: [int(use[i]) for i in order if int(d.me[i]["h"]) == h] for h in fm.SIDES}
        assert all(sum(v) >= 1 for v in by_h.values()), by_h
        assert sum(1 for v in by_h.values() if v.count(0)) >= 2, by_h
        assert n_class == [18, 4, 1]
        assert any(int(d.me[i]["w"]) != int(d.me[i]["h"]) for i in order)
    # the affine winners' corners differ, their jobs say so; iterations happened
    win = np.flatnonzero(use == 1)
    assert all((choice["mv"][i][0] != choice["mv"][i][1]).any() for i in win)
    assert (inter["flags"][0::3] == use).all() and ares["iterations"][order].max() >= 2


def test_model_without_capable_cus_is_the_flat_oracle_pass(xo, pipeline):
    """On the 8-sample grid no CU is capable: the model's pass is xo_frame_pass."""
    pw, ph, bd, _, orig, ref = fm.scene("grid10")
    d = fm.descriptors("grid10", cu=8)
    assert d.affine_jobs()[2] == [0, 0, 0]
    got = fm.frame_pass(xo, d, bd, orig, ref, fm.search(xo, "grid10", d, key="grid10/8"))
    exp = oracle_frame.frame_pass(d, bd, orig, ref, fm.BL, lib=xo)
    assert got[1].tobytes() == exp[1].tobytes() and np.array_equal(got[2], exp[2])
    assert got[3].tobytes() == exp[3].tobytes() and got[4] == exp[4]
    assert all(np.array_equal(a, b) for a, b in zip(got[0], exp[0])) and exp[2].any()


def test_python_and_cpp_job_lists_are_the_same_bytes(pipeline, tmp_path):
    """FrameDescriptors.affine_jobs / affine_order against xvc_gpu::FramePass::AffineJobs,
    compiled with plain g++: jobs, order list and the args block (pointers null)."""
    from xvc_amd import api
    cases = []
    for name in NAMES:
        pw, ph, bd, part = fm.INPUTS[name]
        d = pipeline.FrameDescriptors(pw, ph, 27, search_range=64, bitdepth=bd,
                                      partition=part() if part else None)
        cases.append(d)
    body = ""
    for d in cases:
        rects = ", ".join("{%d, %d, %d, %d}" % tuple(int(b[k]) for k in ("x", "y", "w", "h"))
                          for b in d.me)
        body += ("  { const xvc_gpu::CuRect r[] = {%s};\n    dump(std::vector<xvc_gpu::CuRect>(r, r + %d),"
                 " %du); }\n" % (rects, d.n_cus, int(d.me["lambda16"][0])))
    src = tmp_path / "affine_jobs.cc"
    src.write_text(
        "#include <cstdio>\n#include \"xvc_frame_pass.h\"\n"
        "static void hex(const void *v, size_t n) {\n"
        "  const unsigned char *p = static_cast<const unsigned char *>(v);\n"
        "  for (size_t i = 0; i < n; i++) std::printf(\"%02x\", p[i]);\n  std::printf(\"\\n\");\n}\n"
        "static void dump(const std::vector<xvc_gpu::CuRect> &rects, uint32_t lambda16) {\n"
        "  std::vector<xvcgpu_affine_me_block> jobs;\n  std::vector<int32_t> order;\n"
        "  const xvcgpu_frame_pass_affine_args f =\n"
        "      xvc_gpu::FramePass::AffineJobs(rects, lambda16, 0, 0, 1, &jobs, &order);\n"
        "  hex(jobs.data(), jobs.size() * sizeof(jobs[0]));\n"
        "  hex(order.data(), order.size() * sizeof(order[0]));\n  hex(&f, sizeof(f));\n}\n"
        "int main() {\n" + body + "  return 0;\n}\n")
    exe = str(tmp_path / "affine_jobs")
    lib_dir = os.path.join(ROOT, "xvc_amd")
    subprocess.check_call([
        "g++", "-std=c++11", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
        "-I", os.path.join(lib_dir, "host"), str(src), "-o", exe, "-L", lib_dir, "-lxvcgpu",
        "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.check_output([exe]).decode().split("\n")
    for k, d in enumerate(cases):
        jobs, order, n_class = d.affine_jobs()
        f = api.FramePassAffineArgs()
        f.n_class[:] = n_class
        f.side_bits = 1
        assert bytes.fromhex(out[3 * k]) == jobs.tobytes(), k
        assert bytes.fromhex(out[3 * k + 1]) == order.tobytes(), k
        assert bytes.fromhex(out[3 * k + 2]) == bytes(f), k
        o2, c2 = fm.order_list(d.me)
        assert (order == o2).all() and n_class == c2 and order.dtype == np.int32


def test_order_list_leaves_out_fullpel_and_lic_jobs(pipeline):
    d = fm.descriptors("grid10")
    me = d.me.copy()
    me["fullpel_mv"][0], me["fullpel_mv"][1], me["fullpel_mv"][2] = 1, 2, 3
    order, n_class = pipeline.affine_order(me)
    assert n_class == [21, 0, 0] and order.tolist() == fm.order_list(me)[0].tolist()
    assert not {0, 1, 2} & set(order.tolist())
    mvp = np.arange(d.n_cus * 6).reshape(d.n_cus, 3, 2)
    assert (d.affine_jobs(mvp)[0]["mvp"] == mvp).all()


def test_struct_layouts_match_header(pipeline, tmp_path):
    from xvc_amd import api
    res_fields = ["use_affine", "mv", "cost_plain", "cost_affine", "cost", "dist_affine",
                  "iterations"]
    arg_fields = ["d_affine", "d_affine_results", "d_order", "n_class", "side_bits", "d_choice",
                  "d_inter"]
    src = tmp_path / "layout.c"
    src.write_text(
        "#include <stdio.h>\n#include <stddef.h>\n#include \"xvcgpu.h\"\nint main(){\n" +
        "".join("printf(\"%%zu \", offsetof(xvcgpu_fp_affine_result, %s));\n" % f
                for f in res_fields) +
        "".join("printf(\"%%zu \", offsetof(xvcgpu_frame_pass_affine_args, %s));\n" % f
                for f in arg_fields) +
        "printf(\"%zu %zu %zu %zu %d\\n\", sizeof(xvcgpu_fp_affine_result),"
        "sizeof(xvcgpu_frame_pass_affine_args), sizeof(xvcgpu_frame_pass_args),"
        "sizeof(xvcgpu_affine_me_block), XVC_AFFINE_ME_NO_JOB);return 0;}\n")
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src),
                           "-o", exe])
    out = [int(v) for v in subprocess.check_output([exe]).decode().split()]
    dt = api.FP_AFFINE_RESULT_DTYPE
    assert out == [dt.fields[f][1] for f in res_fields] + \
        [getattr(api.FramePassAffineArgs, f).offset for f in arg_fields] + \
        [dt.itemsize, C.sizeof(api.FramePassAffineArgs), C.sizeof(api.FramePassArgs),
         api.AFFINE_ME_DTYPE.itemsize, api.AFFINE_ME_NO_JOB]
    assert C.sizeof(api.FramePassArgs) == 240      # the flat pass's block stays what it was
    assert (fm.HAS_BOOTSTRAP, fm.NO_JOB, fm.INTER_AFFINE) == \
        (api.AFFINE_ME_HAS_BOOTSTRAP, api.AFFINE_ME_NO_JOB, api.INTER_AFFINE)


def test_entry_points_are_exported_and_refuse_without_a_context(pipeline):
    from xvc_amd import api
    lib = api.load_library()
    hdr = open(os.path.join(ROOT, "include", "xvcgpu.h")).read()
    for name in ENTRY_POINTS:
        assert name in api.SYMBOLS and hasattr(lib, name) and (name + "(") in hdr, name
    a, f = api.FramePassArgs(), api.FramePassAffineArgs()
    n_class = (C.c_int32 * 3)(0, 0, 0)
    assert lib.xvcgpu_fp_affine_boot(None, None, None, 0, 16, 16, None) == 10
    assert lib.xvcgpu_affine_me_listed(None, None, None, None, 0, None, n_class, None) == 10
    assert lib.xvcgpu_fp_affine_choice(None, None, None, 0, C.byref(f)) == 10
    assert lib.xvcgpu_cu_info_from_affine_choice(None, None, None, None, None, 0, 0, 0, 0,
                                                 None) == 10
    assert lib.xvcgpu_frame_pass_affine(None, C.byref(a), C.byref(f), None, 31) == 10


def test_python_refusals(pipeline):
    """affine=True with a form that predicts inside its kernels, with adaptive QP, with a row
    shard or through run_multi raises ValueError before anything is allocated (no context
    is touched); a partition the pass cannot run is check_partition's refusal as before."""
    P = pipeline
    with pytest.raises(ValueError, match="recon_from_me"):
        P.FramePass(None, 104, 72, 10, affine=True)
    with pytest.raises(ValueError, match="fwd_from_me"):
        P.FramePass(None, 104, 72, 10, rdoq=True, affine=True)
    with pytest.raises(ValueError, match="aqp_strength"):
        P.FramePass(None, 104, 72, 10, fused=False, aqp_strength=13, affine=True)
    with pytest.raises(ValueError, match="whole pictures"):
        P.FramePass(None, 104, 72, 10, fused=False, row_range=(0, 32), affine=True)
    with pytest.raises(ValueError, match="overlaps"):
        P.FramePass(None, 32, 32, 10, partition=[(0, 0, 32, 32), (16, 16, 16, 16)], affine=True)
    with pytest.raises(ValueError, match="a gap"):
        P.check_partition(32, 32, [(0, 0, 32, 16)])
    flat = types.SimpleNamespace(affine=None, plan=None)
    with pytest.raises(ValueError, match="run_multi"):
        P.run_multi([flat, types.SimpleNamespace(affine=object(), plan=None)], [], [], [])
