"""The P frame pass with merge mode without a GPU: the model's ranking against the
reference's SearchMergeCandidates (where it is built), the restated rules of the choice, the
conditions the candidates were drawn for, the model without a listed CU against the oracle's
flat pass, the Python and the C++ argument blocks byte for byte, the struct layouts against
the header, the new entry points' symbols and the refusals of pipeline.FramePass
(tests/merge_pass_model.py is the model)."""
import ctypes as C
import os
import subprocess
import types

import numpy as np
import pytest

import bi_refs_pass_model as rm
import merge_pass_model as mm
import oracle_frame
import oracle_lib as ol

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("grid10", "grid8", "part10")
ENTRY_POINTS = ("xvcgpu_fp_merge_rank", "xvcgpu_fp_merge_choice", "xvcgpu_fp_merge_skip",
                "xvcgpu_frame_pass_merge")


@pytest.fixture(scope="module")
def xo():
    return ol.Lib("xo")


@pytest.fixture(scope="module")
def pipeline():
    from xvc_amd import build
    build.build()
    from xvc_amd import pipeline as p
    return p


_passes = {}


def model_pass(xo, name, rdoq=False):
    if (name, rdoq) not in _passes:
        pw, ph, bd, _, orig, ref = mm.scene(name)
        _passes[name, rdoq] = mm.frame_pass(xo, mm.descriptors(name, rdoq), bd, orig, ref,
                                            mm.search(xo, name))
    return _passes[name, rdoq]


@pytest.mark.skipif(not ol.have_ref(), reason="oracle/_ref not built")
@pytest.mark.parametrize("name", NAMES)
def test_ranking_equals_reference(xo, pipeline, name):
    """dist, order and num of every CU against InterSearch::SearchMergeCandidates through
    xr_search_merge_candidates (with out_dist).  A candidate that is not valid is replaced by
    a valid far one for this comparison (the reference's list holds no such thing)."""
    xr = ol.Lib("xr")
    f = xr.dll.xr_search_merge_candidates
    f.restype = C.c_int
    f.argtypes = [C.c_int] * 7 + [C.c_void_p, C.c_ssize_t, C.c_void_p, C.c_ssize_t, C.c_void_p,
                                  C.c_ssize_t, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p]
    pw, ph, bd, _, orig, ref = mm.scene(name)
    desc = mm.descriptors(name)
    cands = mm.search(xo, name)[1].copy()
    bad = cands["ref_idx"][:, :, 0] != 0
    assert bad.any()
    cands["ref_idx"][bad] = (0, -1)
    cands["mv"][bad] = ((mm.FAR, -mm.FAR), (0, 0))
    ranks = mm.rank(xo, name, desc, cands)
    o, r = orig[0][mm.BL:, mm.BL:], ref[0][mm.BL:, mm.BL:]
    for i, b in enumerate(desc.me):
        c5 = np.zeros((mm.CANDS, 5), np.int32)
        c5[:, 1:3] = cands[i]["mv"][:, 0, :]
        order, dist = np.zeros(mm.CANDS, np.int32), np.zeros(mm.CANDS, np.uint64)
        num = f(bd, int(b["x"]), int(b["y"]), int(b["w"]), int(b["h"]), pw, ph, o.ctypes.data,
                orig[0].strides[0] // 2, r.ctypes.data, ref[0].strides[0] // 2, r.ctypes.data,
                ref[0].strides[0] // 2, c5.ctypes.data, mm.LAMBDA_SQRT, order.ctypes.data,
                dist.ctypes.data)
        got = ranks[i]
        assert got["dist"].tolist() == dist.tolist(), (name, i, got, dist)
        assert got["order"].tolist() == order.tolist() and int(got["num"]) == num, \
            (name, i, got, order, num)


def _one_cu(dist_plain, dists, mv=(16, -8), lambda16=mm.LAMBDA16, fullpel=0):
    from xvc_amd import api
    me = np.zeros(1, api.ME_DTYPE)
    me["w"], me["h"], me["lambda16"], me["fullpel_mv"] = 16, 16, lambda16, fullpel
    res = np.zeros(1, api.MERES_DTYPE)
    res["mv_x"], res["mv_y"], res["subpel_dist"] = mv[0], mv[1], dist_plain
    res["fullpel_x"], res["fullpel_y"], res["fullpel_cost"] = 1, -1, 77
    cands = mm.cand_array(1)
    cands["mv"][0, :, 0, :] = [(100 + m, -100 - m) for m in range(mm.CANDS)]
    ranks = np.zeros(1, api.FP_MERGE_RANK_DTYPE)
    cost, order, num = mm.rank_fold(dists)
    ranks[0] = (dists, order, num, 0, cost)
    return me, res, cands, ranks


def test_restated_rules(pipeline):
    """The tie (cost_merge == cost_plain -> merge), the 64-bit product, bits(4) == 4, the
    stable sort and the 1.25 x cut."""
    assert [mm.idx_bits(m) for m in range(5)] == [1, 2, 3, 4, 4]
    lam = mm.LAMBDA16
    bits_p = mm.SIDE_BITS + 1 + rm.eg_bits(4) + rm.eg_bits(-2)
    for m0 in (0, 4):
        bits_m = mm.MERGE_SIDE_BITS + mm.idx_bits(m0)
        gap = ((bits_p * lam) >> 16) - ((bits_m * lam) >> 16)
        for delta, merge in ((0, 1), (-1, 1), (1, 0)):
            dists = [10 ** 6] * 5
            dists[m0] = 1000 + gap + delta
            choice, chosen = mm.choice_fold(*_one_cu(1000, dists))
            c, q = choice[0], chosen[0]
            assert int(c["cost_plain"]) == 1000 + ((bits_p * lam) >> 16)
            assert int(c["cost_merge"]) == int(c["cost_plain"]) + delta
            assert (int(c["use_merge"]), int(c["merge_idx"])) == (merge, m0 if merge else -1)
            assert int(c["cost"]) == min(int(c["cost_plain"]), int(c["cost_merge"]))
            assert c["mv"].tolist() == ([100 + m0, -100 - m0] if merge else [16, -8])
            assert (int(q["mv_x"]), int(q["mv_y"])) == tuple(c["mv"].tolist())
            assert int(q["subpel_dist"]) == (dists[m0] if merge else 1000)
            assert (int(q["fullpel_x"]), int(q["fullpel_y"]), int(q["fullpel_cost"])) == (1, -1, 77)
            assert int(c["skip"]) == 0
    # a lambda16 whose product passes 2^32: not cut to 32 bits before the shift
    big = 0xfff00000
    c = mm.choice_fold(*_one_cu(5, [7, 9, 9, 9, 9], lambda16=big))[0][0]
    assert (bits_p * big) >> 32 and ((mm.MERGE_SIDE_BITS + 1) * big) >> 32
    assert int(c["cost_plain"]) == (5 + ((bits_p * big) >> 16)) & mm.NONE
    assert int(c["cost_merge"]) == (7 + (((mm.MERGE_SIDE_BITS + 1) * big) >> 16)) & mm.NONE
    # no merge: the best distortion is none, a LIC job, a CU the list does not name
    for kw, listed in ((dict(dists=[mm.NONE] * 5), None), (dict(dists=[1] * 5, fullpel=2), None),
                       (dict(dists=[1] * 5), [])):
        args = _one_cu(10 ** 6, kw.pop("dists"), **kw)
        choice, chosen = mm.choice_fold(*args, listed=listed)
        c = choice[0]
        assert (int(c["use_merge"]), int(c["merge_idx"]), int(c["cost_merge"])) == (0, -1, mm.NONE)
        assert chosen.tobytes() == args[1].tobytes() and int(c["cost"]) == int(c["cost_plain"])
    # an unsupported plain search: all ones, the result unchanged
    args = _one_cu(mm.NONE, [1] * 5)
    choice, chosen = mm.choice_fold(*args)
    assert (choice.view(np.uint8) == 0xff).all() and chosen.tobytes() == args[1].tobytes()
    # equal costs keep their index order (bits(3) == bits(4)); a strictly smaller one moves
    assert mm.rank_fold([500, 500, 500, 40, 40])[1] == [3, 4, 0, 1, 2]
    assert mm.rank_fold([mm.NONE, 500, mm.NONE, 40, 40])[1] == [3, 4, 1, 0, 2]
    # the cut: cost[k] > cost[0] * 1.25 for the last k downwards
    ls = mm.LAMBDA_SQRT
    assert mm.rank_fold([1000, 1000, 1000, 1000, 1000])[2] == 4
    assert mm.rank_fold([1000, 1000, 1000, 2000, 2000])[2] == 3
    assert mm.rank_fold([1000, 2000, 2000, 2000, 2000])[2] == 1
    d1 = int((1000 + ls) * 1.25 - 2 * ls)       # cost[1] just not above the bound
    assert mm.rank_fold([1000, d1, 9000, 9000, 9000])[2] == 2
    assert mm.rank_fold([1000, d1 + 2, 9000, 9000, 9000])[2] == 1


@pytest.mark.parametrize("name", NAMES)
def test_candidates_exercise_the_pass(xo, pipeline, name):
    """Conditions on the inputs, met by the model alone."""
    pw, ph = mm.INPUTS[name][:2]
    d = mm.descriptors(name)
    res, cands, ranks, _, chosen = mm.search(xo, name)
    choice = model_pass(xo, name)[5]
    nnz = model_pass(xo, name)[2]
    use = choice["use_merge"]
    assert set(use.tolist()) <= {0, 1}
    assert int(use.sum()) >= 4 and int((use == 0).sum()) >= 4
    assert len(set(ranks["num"].tolist())) >= 3
    # equal candidates that only the stable sort separates
    ties = [i for i in range(d.n_cus) for k in range(4)
            if ranks[i]["cost"][k] == ranks[i]["cost"][k + 1] and
            ranks[i]["dist"][ranks[i]["order"][k]] != mm.NONE and
            ranks[i]["order"][k] < ranks[i]["order"][k + 1]]
    assert ties
    # an invalid candidate somewhere, ranked behind every real one
    bad = np.argwhere(cands["ref_idx"][:, :, 0] != 0)
    assert len(bad) >= 4
    for i, m in bad:
        assert ranks[i]["dist"][m] == mm.NONE and ranks[i]["order"][4] == m
    # a merge winner whose vector ClipMv changes: the record keeps it unclipped
    moved = [i for i in np.flatnonzero(use == 1)
             if xo.clip_mv(int(d.me[i]["x"]), int(d.me[i]["y"]), pw, ph, int(chosen[i]["mv_x"]),
                           int(chosen[i]["mv_y"])) != (int(chosen[i]["mv_x"]), int(chosen[i]["mv_y"]))]
    assert moved
    cus = model_pass(xo, name)[3]
    assert all(cus[i]["mv"][0][0].tolist() == [int(chosen[i]["mv_x"]), int(chosen[i]["mv_y"])]
               for i in moved)
    assert any(mm.FAR in (abs(int(chosen[i]["mv_x"])), abs(int(chosen[i]["mv_y"]))) for i in moved)
    # skip, merge with levels, plain without levels (which is not skip)
    coded = np.array([nnz[3 * i:3 * i + 3].any() for i in range(d.n_cus)])
    assert int(choice["skip"].sum()) >= 1 and ((use == 1) & coded).any()
    assert ((use == 0) & ~coded).any() and not choice["skip"][use == 0].any()
    assert (choice["skip"] == ((use == 1) & ~coded)).all()
    if name == "part10":
        sides = np.minimum(d.me["w"], d.me["h"])
        assert use[sides == 4].any() and use[(d.me["w"] == 64) & (d.me["h"] == 64)].any()
        assert (use[sides == 4] == 0).any()


def test_first_ranks_cover_the_merge_indices(xo, pipeline):
    """order[0] over the inputs: at least three merge indices, index 4 among them - also among
    the winners."""
    first, won = set(), set()
    for name in NAMES:
        _, _, ranks, choice, _ = mm.search(xo, name)
        first |= set(ranks["order"][:, 0].tolist())
        won |= set(choice["merge_idx"][choice["use_merge"] == 1].tolist())
    assert len(first) >= 3 and 4 in first and len(won) >= 3 and 4 in won


@pytest.mark.parametrize("rdoq", [False, True])
def test_model_without_listed_cus_is_the_flat_oracle_pass(xo, pipeline, rdoq):
    pw, ph, bd, _, orig, ref = mm.scene("grid10")
    d = mm.descriptors("grid10", rdoq)
    got = mm.frame_pass(xo, d, bd, orig, ref, mm.search(xo, "grid10", listed=[], key="none"))
    exp = oracle_frame.frame_pass(d, bd, orig, ref, mm.BL, lib=xo)
    assert got[1].tobytes() == exp[1].tobytes() and np.array_equal(got[2], exp[2])
    assert got[3].tobytes() == exp[3].tobytes() and got[4] == exp[4]
    assert all(np.array_equal(a, b) for a, b in zip(got[0], exp[0])) and exp[2].any()
    assert not got[5]["use_merge"].any() and got[6].tobytes() == got[1].tobytes()


def test_python_and_cpp_args_are_the_same_bytes(pipeline, tmp_path):
    """pipeline.merge_cand_array / merge_args against xvc_gpu::FramePass::MergeCands /
    MergeArgs, compiled with plain g++: the candidate array and the args block (pointers
    null), with the default lambda_sqrt of three QPs."""
    rng = np.random.default_rng(5)
    cases = [(7, 22, None, 1, 1), (35, 32, None, 1, 2), (3, 37, [0, 2], 3, 1)]
    mvs = [rng.integers(-6000, 6000, (n, 5, 2)).astype(np.int32) for n, *_ in cases]
    body = ""
    for (n, qp, order, sb, msb), mv in zip(cases, mvs):
        body += ("  { const int32_t mv[] = {%s};\n    dump(mv, %d, %d, %d, %du, %du); }\n"
                 % (", ".join(str(int(v)) for v in mv.reshape(-1)), n, qp,
                    n if order is None else len(order), sb, msb))
    src = tmp_path / "merge_args.cc"
    src.write_text(
        "#include <cstdio>\n#include \"xvc_frame_pass.h\"\n"
        "static void hex(const void *v, size_t n) {\n"
        "  const unsigned char *p = static_cast<const unsigned char *>(v);\n"
        "  for (size_t i = 0; i < n; i++) std::printf(\"%02x\", p[i]);\n  std::printf(\"\\n\");\n}\n"
        "static void dump(const int32_t *mv, int n, int qp, int n_listed, uint32_t sb, uint32_t msb) {\n"
        "  const std::vector<xvcgpu_fp_merge_cand> c = xvc_gpu::FramePass::MergeCands(mv, n);\n"
        "  const xvcgpu_frame_pass_merge_args m = xvc_gpu::FramePass::MergeArgs(\n"
        "      n_listed, sb, msb, xvc_gpu::FramePass::LambdaSqrtForQp(qp));\n"
        "  hex(c.data(), c.size() * sizeof(c[0]));\n  hex(&m, sizeof(m));\n}\n"
        "int main() {\n" + body + "  return 0;\n}\n")
    exe = str(tmp_path / "merge_args")
    lib_dir = os.path.join(ROOT, "xvc_amd")
    subprocess.check_call([
        "g++", "-std=c++11", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
        "-I", os.path.join(lib_dir, "host"), str(src), "-o", exe, "-L", lib_dir, "-lxvcgpu",
        "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.check_output([exe]).decode().split("\n")
    for k, ((n, qp, order, sb, msb), mv) in enumerate(zip(cases, mvs)):
        cands = pipeline.merge_cand_array(mv, n)
        assert bytes.fromhex(out[2 * k]) == cands.tobytes(), k
        o, n_listed = pipeline.merge_order_array(order, n)
        m = pipeline.merge_args(n_listed, sb, msb, pipeline.lambda_sqrt_for_qp(qp))
        assert bytes.fromhex(out[2 * k + 1]) == bytes(m), k
        assert (cands["ref_idx"] == (0, -1)).all() and (cands["mv"][:, :, 0] == mv).all()
        assert not cands["mv"][:, :, 1].any() and not cands["reserved"].any()
    assert pipeline.lambda16_for_qp(32) == int(65536.0 * pipeline.lambda_sqrt_for_qp(32))


def test_struct_layouts_match_header(pipeline, tmp_path):
    from xvc_amd import api
    fields = {
        "xvcgpu_fp_merge_cand": (api.FP_MERGE_CAND_DTYPE, ["ref_idx", "reserved", "mv"]),
        "xvcgpu_fp_merge_ranking": (api.FP_MERGE_RANK_DTYPE,
                                    ["dist", "order", "num", "reserved", "cost"]),
        "xvcgpu_fp_merge_result": (api.FP_MERGE_RESULT_DTYPE,
                                   ["use_merge", "merge_idx", "skip", "num", "mv", "cost_plain",
                                    "cost_merge", "cost"])}
    arg_fields = ["d_cands", "d_order", "n_listed", "side_bits", "merge_side_bits", "reserved",
                  "lambda_sqrt", "d_rank", "d_choice", "d_chosen"]
    src = tmp_path / "layout.c"
    src.write_text(
        "#include <stdio.h>\n#include <stddef.h>\n#include \"xvcgpu.h\"\nint main(){\n" +
        "".join("printf(\"%%zu \", offsetof(%s, %s));\n" % (s, f)
                for s, (_, fs) in fields.items() for f in fs) +
        "".join("printf(\"%%zu \", offsetof(xvcgpu_frame_pass_merge_args, %s));\n" % f
                for f in arg_fields) +
        "".join("printf(\"%%zu \", sizeof(%s));\n" % s for s in fields) +
        "printf(\"%zu %zu %d\\n\", sizeof(xvcgpu_frame_pass_merge_args),"
        "sizeof(xvcgpu_frame_pass_args), XVC_FP_MERGE_CANDS);return 0;}\n")
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src),
                           "-o", exe])
    out = [int(v) for v in subprocess.check_output([exe]).decode().split()]
    assert out == [dt.fields[f][1] for dt, fs in fields.values() for f in fs] + \
        [getattr(api.FramePassMergeArgs, f).offset for f in arg_fields] + \
        [dt.itemsize for dt, _ in fields.values()] + \
        [C.sizeof(api.FramePassMergeArgs), C.sizeof(api.FramePassArgs), api.FP_MERGE_CANDS]
    assert C.sizeof(api.FramePassArgs) == 240      # the flat pass's block stays what it was
    assert (mm.CANDS, mm.ME_USE_LIC) == (api.FP_MERGE_CANDS, 2)


def test_entry_points_are_exported_and_refuse_without_a_context(pipeline):
    from xvc_amd import api
    lib = api.load_library()
    hdr = open(os.path.join(ROOT, "include", "xvcgpu.h")).read()
    for name in ENTRY_POINTS:
        assert name in api.SYMBOLS and hasattr(lib, name) and (name + "(") in hdr, name
    assert "merge" in open(os.path.join(ROOT, "xvc_amd", "pipeline.py")).read()
    a, m = api.FramePassArgs(), api.FramePassMergeArgs()
    assert lib.xvcgpu_fp_merge_rank(None, None, None, None, 0, C.byref(m)) == 10
    assert lib.xvcgpu_fp_merge_choice(None, None, None, 0, C.byref(m)) == 10
    assert lib.xvcgpu_fp_merge_skip(None, None, None, 0, None) == 10
    assert lib.xvcgpu_frame_pass_merge(None, C.byref(a), C.byref(m), None, 31) == 10
    assert lib.xvcgpu_frame_pass_merge(None, C.byref(a), None, None, 31) == 10


def test_python_refusals(pipeline):
    """merge_cands together with affine, aqp_strength, a row_range or run_multi, a lambda
    that is no number, and arrays of the wrong shape raise ValueError that names the pair,
    before anything is allocated (no context is touched)."""
    P = pipeline
    mv = np.zeros((35, 5, 2), np.int32)
    with pytest.raises(ValueError, match="merge_cands and affine"):
        P.FramePass(None, 104, 72, 10, fused=False, affine=True, merge_cands=mv)
    with pytest.raises(ValueError, match="merge_cands and aqp_strength"):
        P.FramePass(None, 104, 72, 10, fused=False, aqp_strength=13, merge_cands=mv)
    with pytest.raises(ValueError, match="merge_cands and row_range"):
        P.FramePass(None, 104, 72, 10, row_range=(0, 32), merge_cands=mv[:14])
    for bad in (float("nan"), float("inf"), -1.0):
        with pytest.raises(ValueError, match="merge_lambda_sqrt"):
            P.FramePass(None, 104, 72, 10, merge_cands=mv, merge_lambda_sqrt=bad)
    with pytest.raises(ValueError, match="merge_cands: expected"):
        P.FramePass(None, 104, 72, 10, merge_cands=mv[:34])
    with pytest.raises(ValueError, match="merge_cands: expected"):
        P.FramePass(None, 104, 72, 10, merge_cands=mv.astype(np.float32))
    with pytest.raises(ValueError, match="merge_order"):
        P.FramePass(None, 104, 72, 10, merge_cands=mv, merge_order=[3, 2])
    with pytest.raises(ValueError, match="merge_order"):
        P.FramePass(None, 104, 72, 10, merge_cands=mv, merge_order=[35])
    flat = types.SimpleNamespace(affine=None, merge=None, plan=None)
    with pytest.raises(ValueError, match="merge_cands and run_multi"):
        P.run_multi([flat, types.SimpleNamespace(affine=None, merge=object(), plan=None)],
                    [], [], [])
