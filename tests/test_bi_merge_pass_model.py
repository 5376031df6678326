"""The B frame pass with merge mode without a GPU: the model's distortions (and on one
picture per list its whole ranking) against the reference's SearchMergeCandidates, the
restated rules of the choice, the model without a listed CU against the plain B model, the
conditions the candidates were drawn for, the Python and the C++ argument blocks byte for
byte, the struct layouts against the header, the new entry points' symbols and the refusals
of pipeline.BiRefsFramePass (tests/bi_merge_pass_model.py is the model)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import bi_merge_pass_model as bm
import bi_refs_pass_model as rm
import merge_pass_model as mm
import oracle_lib as ol

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("grid10", "grid8", "part10")
WHICH = ("A", "C", "D")
ENTRY_POINTS = ("xvcgpu_fp_bi_merge_rank", "xvcgpu_fp_bi_merge_choice", "xvcgpu_fp_bi_merge_skip",
                "xvcgpu_frame_pass_bi_refs_merge")


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


def model_pass(xo, name, which, rdoq=False):
    if (name, which, rdoq) not in _passes:
        _passes[name, which, rdoq] = bm.frame_pass(xo, name, which, bm.descriptors(name, rdoq),
                                                   bm.search(xo, name, which))
    return _passes[name, which, rdoq]


def _xr_call():
    xr = ol.Lib("xr")
    f = xr.dll.xr_search_merge_candidates
    f.restype = C.c_int
    f.argtypes = [C.c_int] * 7 + [C.c_void_p, C.c_ssize_t, C.c_void_p, C.c_ssize_t, C.c_void_p,
                                  C.c_ssize_t, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p]
    return f


def _reference(f, name, b, pic0, pic1, c5):
    """(num, order, dist) of the reference for one CU with ref0 / ref1 the given planes"""
    pw, ph, bd, _, orig, _ = bm.scene(name)
    o = orig[0][bm.BL:, bm.BL:]
    r0, r1 = pic0[bm.BL:, bm.BL:], pic1[bm.BL:, bm.BL:]
    order, dist = np.zeros(bm.CANDS, np.int32), np.zeros(bm.CANDS, np.uint64)
    c5 = np.ascontiguousarray(c5, np.int32)
    num = f(bd, int(b["x"]), int(b["y"]), int(b["w"]), int(b["h"]), pw, ph, o.ctypes.data,
            orig[0].strides[0] // 2, r0.ctypes.data, pic0.strides[0] // 2, r1.ctypes.data,
            pic1.strides[0] // 2, c5.ctypes.data, bm.LAMBDA_SQRT, order.ctypes.data,
            dist.ctypes.data)
    return num, order.tolist(), dist.tolist()


FAR5 = (0, bm.FAR, -bm.FAR, 0, 0)       # a valid far candidate of list 0


def _c5(c):
    """The harness's row {direction, mv0, mv1} of a candidate"""
    r = [int(v) for v in c["ref_idx"]]
    d = 2 if min(r) >= 0 else (0 if r[0] >= 0 else 1)
    return (d,) + tuple(int(v) for v in c["mv"].reshape(-1))


@pytest.mark.skipif(not ol.have_ref(), reason="oracle/_ref not built")
@pytest.mark.parametrize("which", WHICH)
@pytest.mark.parametrize("name", NAMES)
def test_dist_equals_reference(xo, pipeline, name, which):
    """dist of every valid candidate of every CU against InterSearch::SearchMergeCandidates'
    own loop (xr_search_merge_candidates with out_dist).  The harness fixes ref_idx = 0, so it
    is called once per pair of pictures a CU's candidates name, that pair as ref0 / ref1 and
    the other candidates replaced by a valid far one.  On set D - one picture per list - the
    whole list goes in one call and order and num are compared too."""
    f = _xr_call()
    refs = bm.scene(name)[5]
    lists = bm.SETS[which]
    num_ref = [len(lists[0]), len(lists[1])]
    desc = bm.descriptors(name)
    _, cands, ranks = bm.search(xo, name, which)[:3]
    pairs, bi = set(), 0
    for i, b in enumerate(desc.me):
        ok = [bm.valid(c, num_ref) for c in cands[i]]
        keys = {}
        for m in range(bm.CANDS):
            if ok[m]:
                r = [int(v) for v in cands[i][m]["ref_idx"]]
                keys.setdefault((r[0], r[1]), []).append(m)
        for (r0, r1), ms in keys.items():
            poc0 = lists[0][r0] if r0 >= 0 else lists[1][r1]
            poc1 = lists[1][r1] if r1 >= 0 else poc0
            c5 = [_c5(cands[i][m]) if m in ms else FAR5 for m in range(bm.CANDS)]
            _, _, dist = _reference(f, name, b, refs[poc0][0], refs[poc1][0], c5)
            for m in ms:
                assert int(ranks[i]["dist"][m]) == dist[m], (name, which, i, m, ranks[i], dist)
            pairs.add((poc0, poc1))
            bi += r0 >= 0 and r1 >= 0
        if which == "D":
            c5 = [_c5(cands[i][m]) if ok[m] else FAR5 for m in range(bm.CANDS)]
            num, order, dist = _reference(f, name, b, refs[lists[0][0]][0], refs[lists[1][0]][0], c5)
            fixed = cands[i:i + 1].copy()
            for m in range(bm.CANDS):
                if not ok[m]:
                    fixed[0][m]["ref_idx"], fixed[0][m]["mv"] = (0, -1), ((bm.FAR, -bm.FAR), (0, 0))
            one = bm.rank(xo, name, which, desc, np.repeat(fixed, desc.n_cus, 0), listed=[i])[i]
            assert one["dist"].tolist() == dist and one["order"].tolist() == order and \
                int(one["num"]) == num, (name, i, one, dist, order, num)
    assert bi >= 8 and len(pairs) >= (1 if which == "D" else 4)


def _one_cu(cost_plain, dists, ref_idx=(0, 0), lambda16=bm.LAMBDA16, fullpel=0, lists=((4, 0), (12, 16))):
    from xvc_amd import api
    me = np.zeros(1, api.ME_DTYPE)
    me["x"], me["y"], me["w"], me["h"], me["lambda16"], me["fullpel_mv"] = 16, 32, 16, 8, lambda16, fullpel
    plain = np.zeros(1, api.FP_BI_REFS_RESULT_DTYPE)
    plain["inter_dir"], plain["search_list"], plain["ref_idx"] = 1, 1, (-1, 1)
    plain["mv"], plain["cost"], plain["cost_bi"] = ((0, 0), (24, -8)), cost_plain, 777
    inter = [(16, 32, 16, 8, (-1, 3), ((0, 0), (24, -8)))]
    cands = np.zeros((1, bm.CANDS), api.FP_MERGE_CAND_DTYPE)
    cands["ref_idx"] = ref_idx
    cands["mv"][0] = [((100 + m, -100 - m), (200 + m, -200 - m)) for m in range(bm.CANDS)]
    ranks = np.zeros(1, api.FP_MERGE_RANK_DTYPE)
    cost, order, num = mm.rank_fold(dists)
    ranks[0] = (dists, order, num, 0, cost)
    return lists, me, plain, inter, cands, ranks


def test_restated_rules(pipeline):
    """The tie (cost_merge == the plain cost -> merge), the 64-bit product, the chosen record
    and the jobs per direction, the three ways not to merge, the all-ones record; the stable
    sort and the cut are merge_pass_model.rank_fold's, restated there."""
    lam = bm.LAMBDA16
    for m0, ref_idx, d in ((0, (1, 0), 2), (4, (0, -1), 0), (2, (-1, 1), 1)):
        bits = bm.MERGE_SIDE_BITS + mm.idx_bits(m0)
        for delta, merge in ((0, 1), (-1, 1), (1, 0)):
            dists = [10 ** 6] * 5
            dists[m0] = 1000 + delta
            plain_cost = 1000 + ((bits * lam) >> 16)
            args = _one_cu(plain_cost, dists, ref_idx)
            choice, chosen, inter = bm.choice_fold(*args)
            c, q = choice[0], chosen[0]
            assert int(c["cost_plain"]) == plain_cost and int(c["cost_merge"]) == plain_cost + delta
            assert (int(c["use_merge"]), int(c["merge_idx"])) == (merge, m0 if merge else -1)
            assert int(c["cost"]) == min(int(c["cost_plain"]), int(c["cost_merge"])) == int(q["cost"])
            assert int(c["skip"]) == 0 and int(q["cost_bi"]) == 777 and int(q["search_list"]) == 1
            if merge:
                mv = [[100 + m0, -100 - m0] if ref_idx[0] >= 0 else [0, 0],
                      [200 + m0, -200 - m0] if ref_idx[1] >= 0 else [0, 0]]
                assert (int(q["inter_dir"]), q["ref_idx"].tolist(), q["mv"].tolist()) == \
                    (d, list(ref_idx), mv)
                slots = ((0, 1)[ref_idx[0]] if ref_idx[0] >= 0 else -1,       # set A's table
                         (2, 3)[ref_idx[1]] if ref_idx[1] >= 0 else -1)
                assert inter[0] == (16, 32, 16, 8, slots, tuple(tuple(v) for v in mv))
            else:
                assert q.tobytes() == args[2][0].tobytes() and inter == args[3]
            assert (int(c["inter_dir"]), c["ref_idx"].tolist(), c["mv"].tolist()) == \
                (int(q["inter_dir"]), q["ref_idx"].tolist(), q["mv"].tolist())
    big = 0xfff00000                # the product passes 2^32: not cut before the shift
    c = bm.choice_fold(*_one_cu(9, [7, 9, 9, 9, 9], lambda16=big))[0][0]
    assert ((bm.MERGE_SIDE_BITS + 1) * big) >> 32
    assert int(c["cost_merge"]) == (7 + (((bm.MERGE_SIDE_BITS + 1) * big) >> 16)) & bm.NONE
    for kw, listed in ((dict(dists=[bm.NONE] * 5), None), (dict(dists=[1] * 5, fullpel=2), None),
                       (dict(dists=[1] * 5), []), (dict(dists=[1] * 5, ref_idx=(2, -1)), None),
                       (dict(dists=[1] * 5, ref_idx=(-1, -1)), None)):
        args = _one_cu(10 ** 6, kw.pop("dists"), **kw)
        choice, chosen, inter = bm.choice_fold(*args, listed=listed)
        c = choice[0]
        assert (int(c["use_merge"]), int(c["merge_idx"]), int(c["cost_merge"])) == (0, -1, bm.NONE)
        assert chosen.tobytes() == args[2].tobytes() and inter == args[3]
        assert (int(c["inter_dir"]), c["ref_idx"].tolist()) == (1, [-1, 1])
    args = _one_cu(5, [1] * 5)
    args[2].view(np.uint8)[:] = 0xff
    choice, chosen, inter = bm.choice_fold(*args)
    assert (choice.view(np.uint8) == 0xff).all() and (chosen.view(np.uint8) == 0xff).all()
    assert inter == args[3]


@pytest.mark.parametrize("rdoq", [False, True])
def test_model_without_listed_cus_is_the_plain_b_model(xo, pipeline, rdoq):
    name, which = "grid10", "C"
    pw, ph, bd, _, orig, refs = bm.scene(name)
    d = bm.descriptors(name, rdoq)
    got = bm.frame_pass(xo, name, which, d, bm.search(xo, name, which, listed=[], key="none"))
    exp = rm.frame_pass(xo, d, bd, orig, refs, bm.SETS[which], bm.plain_search(xo, name, which))
    assert got[5].tobytes() == exp[5].tobytes() and np.array_equal(got[2], exp[2])
    assert got[3].tobytes() == exp[3].tobytes() and got[4] == exp[4] and exp[2].any()
    assert all(np.array_equal(a, b) for a, b in zip(got[0], exp[0]))
    assert all(np.array_equal(a, b) for a, b in zip(got[8], exp[8]))
    assert not got[10]["use_merge"].any() and got[11].tobytes() == exp[5].tobytes()


@pytest.mark.parametrize("which", WHICH)
@pytest.mark.parametrize("name", NAMES)
def test_winners_of_every_direction(xo, pipeline, name, which):
    """Per (set, input): at least 4 merge winners of each direction and 4 plain winners; the
    candidates that are not valid rank last."""
    lists = bm.SETS[which]
    num_ref = [len(lists[0]), len(lists[1])]
    _, cands, ranks, choice = bm.search(xo, name, which)[:4]
    use = choice["use_merge"]
    assert set(use.tolist()) <= {0, 1}
    for d in range(3):
        assert int(((use == 1) & (choice["inter_dir"] == d)).sum()) >= 4, (name, which, d)
    assert int((use == 0).sum()) >= 4
    bad = [(i, m) for i in range(len(cands)) for m in range(bm.CANDS)
           if not bm.valid(cands[i][m], num_ref)]
    assert len(bad) >= 4
    for i, m in bad:
        assert ranks[i]["dist"][m] == bm.NONE and ranks[i]["order"][4] == m


def test_candidates_exercise_the_pass(xo, pipeline):
    """Over the inputs: merge winners with ref_idx > 0 in each list, a bi-directional winner
    one of whose vectors ClipMv changes (the records keep it unclipped), a winner at index 4,
    equal candidates only the stable sort separates, a skip CU, a merge CU with levels; on the
    partition winners with a side of 4 and at 64x64."""
    hi, clipped, idx4, ties, skip, coded_merge = [0, 0], 0, 0, 0, 0, 0
    side4 = big = 0
    no_list = beyond = False        # candidates that are not valid: {-1, -1}, an index >= num_ref
    for name in NAMES:
        d = bm.descriptors(name)
        for which in WHICH:
            _, cands, ranks, choice, chosen, inter = bm.search(xo, name, which)
            use = choice["use_merge"] == 1
            for l in range(2):
                hi[l] += int((use & (chosen["ref_idx"][:, l] > 0)).sum())
            idx4 += int((use & (choice["merge_idx"] == 4)).sum())
            no_list |= bool((cands["ref_idx"] == -1).all(-1).any())
            beyond |= bool((cands["ref_idx"][:, :, 0] >= len(bm.SETS[which][0])).any())
            for i in np.flatnonzero(use & (chosen["inter_dir"] == 2)):
                b = d.me[i]
                for l in range(2):
                    mv = tuple(int(v) for v in chosen[i]["mv"][l])
                    if xo.clip_mv(int(b["x"]), int(b["y"]), d.w, d.h, *mv) != mv:
                        clipped += bm.FAR in (abs(mv[0]), abs(mv[1]))
                        assert inter[i][5][l] == mv
            ties += sum(1 for i in range(d.n_cus) for k in range(4)
                        if ranks[i]["cost"][k] == ranks[i]["cost"][k + 1] and
                        ranks[i]["dist"][ranks[i]["order"][k]] != bm.NONE and
                        ranks[i]["order"][k] < ranks[i]["order"][k + 1])
            if name == "part10":
                side4 += int((use & (np.minimum(d.me["w"], d.me["h"]) == 4)).sum())
                big += int((use & (d.me["w"] == 64) & (d.me["h"] == 64)).sum())
        e = model_pass(xo, name, "A")
        won, nnz = e[10], e[2]
        coded = np.array([nnz[t:t + 3].any() for t in d.luma_idx[:d.n_cus]])
        assert (won["skip"] == ((won["use_merge"] == 1) & ~coded)).all()
        skip += int(won["skip"].sum())
        coded_merge += int(((won["use_merge"] == 1) & coded).sum())
        # the CU records carry the chosen state
        cus, chosen = e[3], e[5]
        lists = bm.SETS["A"]
        for i in np.flatnonzero(won["use_merge"] == 1)[:8]:
            r = [int(v) for v in chosen[i]["ref_idx"]]
            assert cus[i]["ref_poc"].tolist() == [lists[l][r[l]] if r[l] >= 0 else -1 for l in range(2)]
            assert int(cus[i]["ref_idx0"]) == r[0]
            assert cus[i]["mv"][:, 0, :].tolist() == chosen[i]["mv"].tolist()
    assert min(hi) >= 1 and clipped >= 1 and idx4 >= 1 and ties >= 1, (hi, clipped, idx4, ties)
    assert skip >= 1 and coded_merge >= 1 and side4 >= 1 and big >= 1, (skip, coded_merge, side4, big)
    assert no_list and beyond


def test_python_and_cpp_args_are_the_same_bytes(pipeline, tmp_path):
    """pipeline.bi_merge_cand_array / bi_merge_args against
    xvc_gpu::FramePassBiRefs::MergeCands / MergeArgs, compiled with plain g++."""
    rng = np.random.default_rng(6)
    cases = [(7, 22, None, 1), (35, 32, None, 2), (3, 37, [0, 2], 1)]
    data = [(rng.integers(-2, 3, (n, 5, 2)).astype(np.int32),
             rng.integers(-6000, 6000, (n, 5, 2, 2)).astype(np.int32)) for n, *_ in cases]
    body = ""
    for (n, qp, order, msb), (ri, mv) in zip(cases, data):
        body += ("  { const int32_t ri[] = {%s};\n    const int32_t mv[] = {%s};\n"
                 "    dump(ri, mv, %d, %d, %d, %du); }\n"
                 % (", ".join(str(int(v)) for v in ri.reshape(-1)),
                    ", ".join(str(int(v)) for v in mv.reshape(-1)), n, qp,
                    n if order is None else len(order), msb))
    src = tmp_path / "bi_merge_args.cc"
    src.write_text(
        "#include <cstdio>\n#include \"xvc_frame_pass.h\"\n"
        "static void hex(const void *v, size_t n) {\n"
        "  const unsigned char *p = static_cast<const unsigned char *>(v);\n"
        "  for (size_t i = 0; i < n; i++) std::printf(\"%02x\", p[i]);\n  std::printf(\"\\n\");\n}\n"
        "static void dump(const int32_t *ri, const int32_t *mv, int n, int qp, int n_listed,\n"
        "                 uint32_t msb) {\n"
        "  const std::vector<xvcgpu_fp_merge_cand> c = xvc_gpu::FramePassBiRefs::MergeCands(ri, mv, n);\n"
        "  const xvcgpu_frame_pass_bi_merge_args m = xvc_gpu::FramePassBiRefs::MergeArgs(\n"
        "      n_listed, msb, xvc_gpu::FramePass::LambdaSqrtForQp(qp));\n"
        "  hex(c.data(), c.size() * sizeof(c[0]));\n  hex(&m, sizeof(m));\n}\n"
        "int main() {\n" + body + "  return 0;\n}\n")
    exe = str(tmp_path / "bi_merge_args")
    lib_dir = os.path.join(ROOT, "xvc_amd")
    subprocess.check_call([
        "g++", "-std=c++11", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
        "-I", os.path.join(lib_dir, "host"), str(src), "-o", exe, "-L", lib_dir, "-lxvcgpu",
        "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.check_output([exe]).decode().split("\n")
    for k, ((n, qp, order, msb), (ri, mv)) in enumerate(zip(cases, data)):
        cands = pipeline.bi_merge_cand_array((ri, mv), n)
        assert bytes.fromhex(out[2 * k]) == cands.tobytes(), k
        assert pipeline.bi_merge_cand_array(cands, n).tobytes() == cands.tobytes()
        _, n_listed = pipeline.merge_order_array(order, n)
        m = pipeline.bi_merge_args(n_listed, msb, pipeline.lambda_sqrt_for_qp(qp))
        assert bytes.fromhex(out[2 * k + 1]) == bytes(m), k
        assert (cands["ref_idx"] == ri).all() and (cands["mv"] == mv).all()
        assert not cands["reserved"].any()


def test_struct_layouts_match_header(pipeline, tmp_path):
    from xvc_amd import api
    fields = ["use_merge", "merge_idx", "skip", "num", "inter_dir", "ref_idx", "mv", "cost_plain",
              "cost_merge", "cost"]
    arg_fields = ["d_cands", "d_order", "n_listed", "merge_side_bits", "lambda_sqrt", "d_rank",
                  "d_choice", "d_chosen"]
    src = tmp_path / "layout.c"
    src.write_text(
        "#include <stdio.h>\n#include <stddef.h>\n#include \"xvcgpu.h\"\nint main(){\n" +
        "".join("printf(\"%%zu \", offsetof(xvcgpu_fp_bi_merge_result, %s));\n" % f for f in fields) +
        "".join("printf(\"%%zu \", offsetof(xvcgpu_frame_pass_bi_merge_args, %s));\n" % f
                for f in arg_fields) +
        "printf(\"%zu %zu %zu %zu\\n\", sizeof(xvcgpu_fp_bi_merge_result),"
        "sizeof(xvcgpu_frame_pass_bi_merge_args), sizeof(xvcgpu_frame_pass_bi_refs_args),"
        "sizeof(xvcgpu_fp_bi_refs_result));return 0;}\n")
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src),
                           "-o", exe])
    out = [int(v) for v in subprocess.check_output([exe]).decode().split()]
    dt = api.FP_BI_MERGE_RESULT_DTYPE
    assert out == [dt.fields[f][1] for f in fields] + \
        [getattr(api.FramePassBiMergeArgs, f).offset for f in arg_fields] + \
        [dt.itemsize, C.sizeof(api.FramePassBiMergeArgs), C.sizeof(api.FramePassBiRefsArgs),
         api.FP_BI_REFS_RESULT_DTYPE.itemsize]
    assert C.sizeof(api.FramePassBiRefsArgs) == 488     # the B pass's block stays what it was


def test_entry_points_are_exported_and_refuse_without_a_context(pipeline):
    from xvc_amd import api
    lib = api.load_library()
    hdr = open(os.path.join(ROOT, "include", "xvcgpu.h")).read()
    for name in ENTRY_POINTS:
        assert name in api.SYMBOLS and hasattr(lib, name) and (name + "(") in hdr, name
    a, m = api.FramePassBiRefsArgs(), api.FramePassBiMergeArgs()
    assert lib.xvcgpu_fp_bi_merge_rank(None, C.byref(a), C.byref(m)) == 10
    assert lib.xvcgpu_fp_bi_merge_choice(None, C.byref(a), C.byref(m)) == 10
    assert lib.xvcgpu_fp_bi_merge_skip(None, None, None, 0, None) == 10
    assert lib.xvcgpu_frame_pass_bi_refs_merge(None, C.byref(a), C.byref(m), None, 31) == 10
    assert lib.xvcgpu_frame_pass_bi_refs_merge(None, C.byref(a), None, None, 31) == 10


def test_python_refusals(pipeline):
    """merge_cands together with affine, aqp_strength or low_delay, a lambda that is no
    number, and arrays of the wrong shape raise ValueError before anything is allocated (no
    context is touched)."""
    P = pipeline
    good = (np.zeros((35, 5, 2), np.int32), np.zeros((35, 5, 2, 2), np.int32))
    with pytest.raises(ValueError, match="merge_cands: not together with affine"):
        P.BiRefsFramePass(None, 104, 72, 10, affine=True, merge_cands=good)
    with pytest.raises(ValueError, match="merge_cands: not together with aqp_strength"):
        P.BiRefsFramePass(None, 104, 72, 10, aqp_strength=13, merge_cands=good)
    with pytest.raises(ValueError, match="merge_cands: not together with low_delay"):
        P.BiRefsFramePass(None, 104, 72, 10, low_delay=True, ref_pocs=((4,), (0,)),
                          merge_cands=good)
    for bad in (float("nan"), float("inf"), -1.0):
        with pytest.raises(ValueError, match="merge_lambda_sqrt"):
            P.BiRefsFramePass(None, 104, 72, 10, merge_cands=good, merge_lambda_sqrt=bad)
    for bad in ((good[0][:34], good[1]), (good[0], good[1][:, :, :1]), good[1],
                (good[0].astype(np.float32), good[1]), (good[0] + 300, good[1])):
        with pytest.raises(ValueError, match="merge_cands"):
            P.BiRefsFramePass(None, 104, 72, 10, merge_cands=bad)
    with pytest.raises(ValueError, match="merge_side_bits"):
        P.BiRefsFramePass(None, 104, 72, 10, merge_cands=good, merge_side_bits=-1)
    with pytest.raises(ValueError, match="merge_order"):
        P.BiRefsFramePass(None, 104, 72, 10, merge_cands=good, merge_order=[3, 2])
    with pytest.raises(ValueError, match="merge_order"):
        P.BiRefsFramePass(None, 104, 72, 10, merge_cands=good, merge_order=[35])
    part = rm.partition_128()
    with pytest.raises(ValueError, match="merge_cands"):
        P.BiRefsFramePass(None, 128, 128, 10, partition=part, merge_cands=good)
