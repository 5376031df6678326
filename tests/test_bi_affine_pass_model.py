"""The B frame pass with affine motion without a GPU: the searches the model rests on against
the reference (where it is built), the bootstrap, the corner bits, the tie rule and the 64-bit
product, the conditions the scenes were built for, the model without capable CUs against the
plain B model, the pin of the bi-directional affine prediction, Python's job arrays, the
struct layouts against the header, the new entry points' symbols and the refusals of
pipeline.BiRefsFramePass (tests/bi_affine_pass_model.py is the model)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import bi_affine_pass_model as am
import bi_refs_pass_model as rm
import oracle_affine_me as oa
import oracle_lib as ol
import stream_fixture as sf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (input, reference set): the grids with A and C, the partition with A, set D once
CASES = [("grid10", "A"), ("grid8", "A"), ("grid10", "C"), ("grid8", "C"), ("part10", "A"),
         ("grid10", "D")]
ENTRY_POINTS = ("xvcgpu_fp_bi_affine_boot", "xvcgpu_affine_me_listed_refs",
                "xvcgpu_fp_bi_affine_uni_fold", "xvcgpu_fp_bi_affine_choice",
                "xvcgpu_cu_info_from_bi_affine_choice", "xvcgpu_frame_pass_bi_refs_affine")


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
@pytest.mark.parametrize("name,which", CASES)
def test_affine_searches_of_the_scenes_equal_reference(xo, pipeline, name, which):
    """Every affine job of the scene, uni-directional (bootstrapped from the plain search) and
    BIPRED (the fold's refinement jobs), through the reference's MotionEstAffine and the
    oracle's: the same record."""
    xr = ol.Lib("xr")
    pw, ph, bd, _, orig, refs = am.scene(name)
    found = am.search(xo, name, which)
    _, _, distinct, _ = am.tables(am.SETS[which])
    ran = [0, 0]
    for k, (jobs, slots, res) in enumerate(((found["jobs"], found["slots"], found["ures"]),
                                            (found["bjobs"], found["bslots"], found["bres"]))):
        for i in found["order"]:
            for e in range(jobs.shape[1]):
                s0, s1 = (int(v) for v in slots[i][e])
                if s0 == am.NO_SLOT:
                    continue
                assert bool(int(jobs[i][e]["flags"]) & am.BIPRED) == bool(k)
                got = oa.affine_me(xr, bd, jobs[i][e], pw, ph, orig[0], refs[distinct[s0]][0],
                                   am.BL, refs[distinct[s1]][0] if k else None)
                # (the reference's function does not say how many iterations it ran)
                assert np.array_equal(got["mv"], res[i][e]["mv"]) and \
                    got["dist"] == res[i][e]["dist"], (name, which, k, i, e, got, res[i][e])
                ran[k] += 1
    assert ran[0] >= 2 * len(found["order"]) and ran[1] >= len(found["order"]), ran


def _clip(x, y, pw, ph, mx, my):
    """ClipMv (inter_prediction.cc) restated"""
    lo_x, lo_y = -((64 + 8 + x - 1) << 4), -((64 + 8 + y - 1) << 4)
    hi_x, hi_y = (pw + 8 - x - 1) << 4, (ph + 8 - y - 1) << 4
    return min(max(mx, lo_x), hi_x), min(max(my, lo_y), hi_y)


def test_bootstrap_is_the_clipped_plain_vector_of_its_picture(xo, pipeline):
    """Per (list, picture): ClipMv of that picture's plain vector at all three corners;
    planted vectors of +-3000 make ClipMv act.  A re-used entry, a slot beyond the list and
    an unlisted CU keep their bytes; an unsupported plain result gives NO_JOB."""
    lists = am.SETS["C"]
    pw, ph = am.INPUTS["part10"][:2]
    d = am.descriptors("part10")
    me = rm.jobs(d, lists)
    order, n_class = am.order_list(me[0][0])
    assert n_class == [18, 4, 1]
    jobs0, slots = am.uni_jobs(lists, me)
    num_ref, same, _, slot = am.tables(lists)
    rmax = max(num_ref)
    assert (num_ref, same, rmax) == ([3, 2], [2, -1], 3)
    rng = np.random.default_rng(5)
    res = [[None] * num_ref[l] for l in range(2)]
    for l in range(2):
        for r in range(num_ref[l]):
            if l == 1 and same[r] >= 0:
                continue
            q = res[l][r] = np.zeros(d.n_cus, ol.MERES_DTYPE)
            q["mv_x"], q["mv_y"] = rng.integers(-60, 61, d.n_cus), rng.integers(-60, 61, d.n_cus)
            q["mv_x"][order[(l + r)::3]] = rng.choice([-3000, 3000], len(order[(l + r)::3]))
    res[0][2]["subpel_dist"][order[5]] = am.NONE
    jobs = am.boot(xo, lists, res, jobs0, slots, order, pw, ph)
    clipped = 0
    for i in range(d.n_cus):
        for e in range(2 * rmax):
            l, r = divmod(e, rmax)
            j = jobs[i][e]
            job = r < num_ref[l] and (l == 0 or same[r] < 0)
            assert int(slots[i][e][0]) == (slot[l][r] if job else am.NO_SLOT)
            assert int(slots[i][e][1]) == am.NO_SLOT
            if i not in order or not job:
                assert j.tobytes() == jobs0[i][e].tobytes()
                continue
            if (i, l, r) == (order[5], 0, 2):
                assert int(j["flags"]) == am.NO_JOB and not j["bootstrap"].any()
                continue
            q = res[l][r][i]
            mv = _clip(int(j["x"]), int(j["y"]), pw, ph, int(q["mv_x"]), int(q["mv_y"]))
            clipped += mv != (int(q["mv_x"]), int(q["mv_y"]))
            assert int(j["flags"]) == am.HAS_BOOTSTRAP and j["bootstrap"].tolist() == [list(mv)] * 3
            back = j.copy()
            back["flags"], back["bootstrap"] = 0, 0
            assert back.tobytes() == jobs0[i][e].tobytes()
    assert clipped >= 16
    assert not am.searched(me[0][0], jobs, slots, int(order[5]))
    assert am.searched(me[0][0], jobs, slots, int(order[4]))


def test_corner_bits_are_the_oracles(xo):
    rng = np.random.default_rng(6)
    for _ in range(400):
        mvp = rng.integers(-900, 900, (3, 2))
        mv = mvp + rng.integers(-700, 700, (3, 2)) * int(rng.integers(0, 2))
        exp = sum(int(xo._mvd_bits(int(mvp[k][0]), int(mvp[k][1]), int(mv[k][0]), int(mv[k][1]), 0))
                  for k in (0, 1))
        assert am.corner_bits(mvp, mv) == exp


LISTS = ((4, 0), (12, 4))     # Rmax 2; list 1's second picture is list 0's first


def _one_cu(dist, bi_dist, plain_cost, lambda16=am.LAMBDA16, flags=am.HAS_BOOTSTRAP):
    """One 16x16 CU with given uni-directional distortions dist[e] (e = l * 2 + r; the re-used
    entry's is ignored) and refinement distortions bi_dist[k]: the model's folds' answer."""
    from xvc_amd import api
    me = [[np.zeros(1, api.ME_DTYPE) for _ in LISTS[l]] for l in range(2)]
    for row in me:
        for m in row:
            m["w"], m["h"], m["lambda16"] = 16, 16, lambda16
    jobs, slots = am.uni_jobs(LISTS, me)
    jobs["flags"][slots[:, :, 0] != am.NO_SLOT] = flags
    ures = np.zeros((1, 4), oa.RESULT_DTYPE)
    ures["dist"][0] = dist
    ures["mv"][0] = [[[16 * (e + 1), -8], [16 * (e + 1) + 4, -8], [16 * (e + 1), -4]]
                     for e in range(4)]
    fold, bjobs, bslots = am.uni_fold(LISTS, me[0][0], jobs, slots, ures)
    bres = np.zeros((1, 2), oa.RESULT_DTYPE)
    bres["dist"][0] = bi_dist
    bres["mv"][0] = [[[8, 8], [12, 8], [8, 12]], [[-8, 8], [-4, 8], [-8, 12]]]
    plain = np.zeros(1, rm.CHOICE_DTYPE)
    plain["inter_dir"], plain["ref_idx"], plain["mv"] = 0, (1, -1), ((40, 4), (0, 0))
    plain["cost"] = plain_cost
    inter = am.plain_inter([(0, 0, 16, 16, (1, -1), ((40, 4), (0, 0)))])
    choice, out = am.choice_fold(LISTS, me[0][0], jobs, slots, ures, bres, fold, plain, inter)
    return choice[0], out, fold[0], bjobs[0], bslots[0], inter


def test_folds_in_integers(pipeline):
    """The re-used entry takes list 0's distortion and vectors, search_list and the slot
    bytes, the refinement jobs, ChooseUniOrBi, the tie with the plain state (:90) and the
    64-bit product, on one hand-made CU."""
    lam = am.LAMBDA16
    eg = rm.eg_bits

    def bits(side, num_ref, r, mv0):    # zero predictors: corner 0 (x, -8), corner 1 (x + 4, -8)
        return side + rm.ref_idx_bits(num_ref, r) + 1 + eg(mv0 >> 2) + eg((mv0 + 4) >> 2) + \
            2 * eg(-8 >> 2)
    # list 0: picture 1 cheaper; list 1: its unique picture 0 dearer than the re-used entry
    c, inter, fold, bjobs, bslots, inter0 = _one_cu([900, 700, 800, 12345], [5000, 5000], 10 ** 6)
    cost = [[900 + ((bits(3, 2, 0, 16) * lam) >> 16), 700 + ((bits(3, 2, 1, 32) * lam) >> 16)],
            [800 + ((bits(3, 2, 0, 48) * lam) >> 16), 900 + ((bits(3, 2, 1, 16) * lam) >> 16)]]
    # (the re-used entry (1, 1): list 0's distortion and vectors of picture 0, list 1's index)
    assert c["cost_uni"][:, :2].tolist() == cost and c["cost_uni"][:, 2].tolist() == [am.NONE] * 2
    assert c["best_ref"].tolist() == [1, 0] and int(c["best_ref_l1_unique"]) == 0
    assert int(c["cost_l1_unique"]) == cost[1][0] == int(c["cost_list"][1])
    assert int(c["search_list"]) == 1 and cost[0][1] <= cost[1][0]
    # the refinement jobs of list 1: bootstrap = (1, k)'s vectors, the twin's for k = 1
    assert bjobs["flags"].tolist() == [3, 3]
    assert bjobs["bootstrap"][:, 0, 0].tolist() == [48, 16]
    assert bjobs["other_mv"][:, 0, 0].tolist() == [32, 32]
    _, _, _, slot = am.tables(LISTS)
    assert bslots.tolist() == [[slot[1][0], slot[0][1]], [slot[1][1], slot[0][1]]]
    assert slot[1][1] == slot[0][0]
    # list 0 wins the affine run and beats the plain state
    assert (int(c["use_affine"]), int(c["inter_dir"])) == (1, 0)
    assert c["ref_idx"].tolist() == [1, -1] and int(c["cost"]) == cost[0][1] == int(c["cost_affine"])
    assert c["mv"][0].tolist() == [[32, -8], [36, -8], [32, -4]] and not c["mv"][1].any()
    assert inter["flags"].tolist() == [1] * 3 and inter["ref"].tolist() == [[slot[0][1], -1]] * 3
    assert inter["mv"][0][0].tolist() == c["mv"][0].tolist() and not inter["mv"][:, 1].any()
    # the tie: cost_affine == cost_plain keeps plain, one below takes affine, one above not
    for delta, affine in ((0, 0), (1, 1), (-1, 0)):
        c, inter, _, _, _, inter0 = _one_cu([900, 700, 800, 0], [5000, 5000], cost[0][1] + delta)
        assert int(c["use_affine"]) == affine and int(c["cost_affine"]) == cost[0][1]
        assert int(c["cost"]) == min(cost[0][1], cost[0][1] + delta)
        if not affine:
            assert inter.tobytes() == inter0.tobytes()
            assert c["mv"][0].tolist() == [[40, 4]] * 3 and not c["mv"][1].any()
            assert (int(c["inter_dir"]), c["ref_idx"].tolist()) == (0, [1, -1])
    # bi wins: the refined pair of list 1's picture 1 (the re-used entry's slot) with list 0's best
    c, inter, _, _, _, _ = _one_cu([900, 700, 800, 0], [650, 300], 10 ** 6)
    bits_o = bits(5, 2, 1, 32)
    bi = [650 + (((bits_o + rm.ref_idx_bits(2, 0) + 1 + 3 * eg(2) + eg(3)) * lam) >> 16),
          300 + (((bits_o + rm.ref_idx_bits(2, 1) + 1 + eg(-2) + eg(-1) + 2 * eg(2)) * lam) >> 16)]
    assert c["bi_cost"][:2].tolist() == bi and int(c["cost_bi"]) == bi[1] == int(c["cost"])
    assert (int(c["use_affine"]), int(c["inter_dir"]), c["ref_idx"].tolist()) == (1, 2, [1, 1])
    assert c["mv"][1].tolist() == [[-8, 8], [-4, 8], [-8, 12]] and c["mv"][0][0].tolist() == [32, -8]
    assert inter["ref"].tolist() == [[slot[0][1], slot[1][1]]] * 3
    # cost_bi == cost_l0 gives bi; list 1's unique picture wins where it is cheapest
    c = _one_cu([900, 700, 800, 0], [5000, 300 + cost[0][1] - bi[1]], 10 ** 6)[0]
    assert int(c["cost_bi"]) == cost[0][1] and int(c["inter_dir"]) == 2
    c = _one_cu([900, 700, 100, 0], [5000, 5000], 10 ** 6)[0]
    assert (int(c["inter_dir"]), c["ref_idx"].tolist(), int(c["search_list"])) == (1, [-1, 0], 0)
    assert c["mv"][1][0].tolist() == [48, -8] and not c["mv"][0].any()
    # a lambda whose product passes 2^32: not cut to 32 bits
    big = 0xfff00000
    c = _one_cu([5, 5, 5, 5], [5, 5], 10 ** 6, lambda16=big)[0]
    assert int(c["cost_uni"][0][0]) == (5 + ((bits(3, 2, 0, 16) * big) >> 16)) & am.NONE
    assert (bits(3, 2, 0, 16) * big) >> 32
    # not searched (a job without bootstrap): the plain state, the affine fields unused
    for flags in (0, am.NO_JOB):
        c, inter, _, _, bslots, inter0 = _one_cu([1, 1, 1, 1], [1, 1], 10 ** 6, flags=flags)
        assert (int(c["use_affine"]), int(c["cost_affine"]), int(c["search_list"])) == (0, am.NONE, -1)
        assert (bslots == am.NO_SLOT).all() and inter.tobytes() == inter0.tobytes()
        assert c["cost_uni"].tolist() == [[am.NONE] * 3] * 2 and c["best_ref"].tolist() == [-1, -1]


@pytest.mark.parametrize("name,which", CASES)
def test_scenes_exercise_the_choice(xo, pipeline, name, which):
    """The conditions the scenes were tuned for, on the model alone."""
    lists = am.SETS[which]
    found = am.search(xo, name, which)
    c = am.census(found, lists)
    print(name, which, c)
    ch, order = found["choice"], found["order"]
    assert set(ch["use_affine"].tolist()) <= {0, 1}
    assert not ch["use_affine"][[i for i in range(len(ch)) if i not in order]].any()
    assert c["capable"] == 24 - (name == "part10")
    if name != "part10":
        assert c["affine"] >= 4 and c["plain"] >= 4
        assert min(c["affine_dir"]) >= 1, c["affine_dir"]
        assert c["search_list"] == [0, 1]
        if which == "C":
            assert c["l1_best_reused"] >= 1 and c["unique_differs"] >= 1
    else:
        assert all(a >= 1 for a, _ in c["by_height"].values()), c["by_height"]
        assert sum(1 for _, p in c["by_height"].values() if p >= 1) >= 2, c["by_height"]
        assert found["n_class"] == [18, 4, 1]
    win = np.flatnonzero(ch["use_affine"] == 1)
    for i in win:       # a winner's corners differ in a list it uses; its jobs say so
        used = [l for l in range(2) if int(ch["ref_idx"][i][l]) >= 0]
        assert any((ch["mv"][i][l][0] != ch["mv"][i][l][1]).any() for l in used)
    assert (found["inter"]["flags"][0::3] == ch["use_affine"]).all()
    assert found["ures"]["iterations"][order].max() >= 2


def test_model_without_capable_cus_is_the_plain_b_model(xo, pipeline):
    """On the 8-sample grid no CU is capable: the model's pass is bi_refs_pass_model's."""
    pw, ph, bd, _, orig, refs = am.scene("grid10")
    lists = am.SETS["A"]
    d = am.descriptors("grid10", cu=8)
    assert am.order_list(d.me)[1] == [0, 0, 0]
    found = am.search(xo, "grid10", "A", d, key="grid10/8")
    got = am.frame_pass(xo, d, bd, orig, refs, lists, found)
    exp = rm.frame_pass(xo, d, bd, orig, refs, lists, found["plain"])
    assert all(np.array_equal(a, b) for a, b in zip(got[0], exp[0]))
    assert np.array_equal(got[1], exp[2]) and exp[2].any()
    assert got[2].tobytes() == exp[3].tobytes() and got[3] == exp[4]
    assert all(np.array_equal(a, b) for a, b in zip(got[4], exp[8]))
    assert not found["choice"]["use_affine"].any()


def test_bi_directional_affine_prediction_is_pinned_by_a_stream():
    """xo_inter_pred_block predicts the model's bi-directional affine CUs; what ties it to the
    reference for such CUs is the oracle's decode of a reference stream that holds them."""
    fx = sf.StreamFixture("warpld")
    count = 0
    for i in range(fx.n):
        cus = fx.cus(i)
        count += int(((cus["affine"] == 1) & (cus["inter_dir"] == 2) & (cus["pred_mode"] == 1)).sum())
    print("bi-directional affine CUs in stream_warpld:", count)
    assert count >= 1
    pics = [(fx.info[i], fx.cus(i), fx.levels(i)) for i in range(fx.n)]
    seen = []

    def check(i, pic, pre, nb):
        md5 = sf.picture_md5(pic.planes, int(fx.info[i]["bitdepth"]))
        assert np.array_equal(md5, fx.info[i]["md5"]), i
        seen.append(i)
    sf.oracle_decode_stream(pics, check)
    assert len(seen) == fx.n


def test_python_job_arrays_are_the_models(pipeline):
    """pipeline.bi_affine_jobs against the model's uni_jobs and order_list, byte for byte,
    with the default and with given corner predictors."""
    for name, which in (("grid10", "C"), ("part10", "A"), ("grid10", "D")):
        lists = am.SETS[which]
        d = am.descriptors(name)
        me = rm.jobs(d, lists)
        _, same, _, slot = am.tables(lists)
        jobs, slots, order, n_class = pipeline.bi_affine_jobs(me, same, slot)
        e_jobs, e_slots = am.uni_jobs(lists, me)
        e_order, e_class = am.order_list(me[0][0])
        assert jobs.tobytes() == e_jobs.tobytes() and slots.tobytes() == e_slots.tobytes()
        assert order.dtype == np.int32 and order.tolist() == e_order.tolist() and n_class == e_class
        rng = np.random.default_rng(8)
        mvp = [[rng.integers(-50, 50, (d.n_cus, 3, 2)) for _ in lists[l]] for l in range(2)]
        jobs = pipeline.bi_affine_jobs(me, same, slot, mvp)[0]
        assert jobs.tobytes() == am.uni_jobs(lists, me, mvp)[0].tobytes()


def test_python_and_cpp_job_arrays_are_the_same_bytes(pipeline, tmp_path):
    """pipeline.bi_affine_jobs against xvc_gpu::FramePassBiRefs::AffineJobs, compiled with
    plain g++: jobs, slot bytes, order list and the args block (pointers null)."""
    from xvc_amd import api
    cases = []
    for name, which in (("grid10", "C"), ("part10", "A"), ("grid8", "D")):
        pw, ph, bd, part = am.INPUTS[name]
        d = pipeline.FrameDescriptors(pw, ph, 27, search_range=64, bitdepth=bd,
                                      partition=part() if part else None)
        cases.append((d, am.SETS[which]))
    body = ""
    for d, lists in cases:
        num_ref, same, _, slot = am.tables(lists)
        rects = ", ".join("{%d, %d, %d, %d}" % tuple(int(b[k]) for k in ("x", "y", "w", "h"))
                          for b in d.me)
        pad = lambda v: list(v) + [0] * (3 - len(v))    # noqa: E731
        body += ("  { const xvc_gpu::CuRect r[] = {%s};\n    const int num_ref[2] = {%d, %d};\n"
                 "    const int same[3] = {%s};\n    const int slot[2][3] = {{%s}, {%s}};\n"
                 "    dump(std::vector<xvc_gpu::CuRect>(r, r + %d), %du, num_ref, same, slot); }\n"
                 % (rects, num_ref[0], num_ref[1], ", ".join(map(str, pad(same))),
                    ", ".join(map(str, pad(slot[0]))), ", ".join(map(str, pad(slot[1]))),
                    d.n_cus, int(d.me["lambda16"][0])))
    src = tmp_path / "bi_affine_jobs.cc"
    src.write_text(
        "#include <cstdio>\n#include \"xvc_frame_pass.h\"\n"
        "static void hex(const void *v, size_t n) {\n"
        "  const unsigned char *p = static_cast<const unsigned char *>(v);\n"
        "  for (size_t i = 0; i < n; i++) std::printf(\"%02x\", p[i]);\n  std::printf(\"\\n\");\n}\n"
        "static void dump(const std::vector<xvc_gpu::CuRect> &rects, uint32_t lambda16,\n"
        "                 const int num_ref[2], const int *same, const int slot[2][3]) {\n"
        "  std::vector<xvcgpu_affine_me_block> jobs;\n  std::vector<uint8_t> slots;\n"
        "  std::vector<int32_t> order;\n"
        "  const xvcgpu_frame_pass_bi_affine_args f = xvc_gpu::FramePassBiRefs::AffineJobs(\n"
        "      rects, lambda16, 0, 0, num_ref, same, slot, &jobs, &slots, &order);\n"
        "  hex(jobs.data(), jobs.size() * sizeof(jobs[0]));\n  hex(slots.data(), slots.size());\n"
        "  hex(order.data(), order.size() * sizeof(order[0]));\n  hex(&f, sizeof(f));\n}\n"
        "int main() {\n" + body + "  return 0;\n}\n")
    exe = str(tmp_path / "bi_affine_jobs")
    lib_dir = os.path.join(ROOT, "xvc_amd")
    subprocess.check_call([
        "g++", "-std=c++11", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
        "-I", os.path.join(lib_dir, "host"), str(src), "-o", exe, "-L", lib_dir, "-lxvcgpu",
        "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.check_output([exe]).decode().split("\n")
    for k, (d, lists) in enumerate(cases):
        _, same, _, slot = am.tables(lists)
        me = [[d.me for _ in lists[l]] for l in range(2)]
        jobs, slots, order, n_class = pipeline.bi_affine_jobs(me, same, slot)
        f = api.FramePassBiAffineArgs()
        f.n_class[:] = n_class
        assert bytes.fromhex(out[4 * k]) == jobs.tobytes(), k
        assert bytes.fromhex(out[4 * k + 1]) == slots.tobytes(), k
        assert bytes.fromhex(out[4 * k + 2]) == order.tobytes(), k
        assert bytes.fromhex(out[4 * k + 3]) == bytes(f), k


def test_struct_layouts_match_header(pipeline, tmp_path):
    from xvc_amd import api
    res_fields = list(api.FP_BI_AFFINE_RESULT_DTYPE.names)
    arg_fields = [f[0] for f in api.FramePassBiAffineArgs._fields_]
    src = tmp_path / "layout.c"
    src.write_text(
        "#include <stdio.h>\n#include <stddef.h>\n#include \"xvcgpu.h\"\nint main(){\n" +
        "".join("printf(\"%%zu \", offsetof(xvcgpu_fp_bi_affine_result, %s));\n" % f
                for f in res_fields) +
        "".join("printf(\"%%zu \", offsetof(xvcgpu_frame_pass_bi_affine_args, %s));\n" % f
                for f in arg_fields) +
        "printf(\"%zu %zu %zu %zu %zu %d\\n\", sizeof(xvcgpu_fp_bi_affine_result),"
        "sizeof(xvcgpu_frame_pass_bi_affine_args), sizeof(xvcgpu_frame_pass_bi_refs_args),"
        "sizeof(xvcgpu_frame_pass_args), sizeof(xvcgpu_fp_bi_refs_result), XVC_FP_BI_NO_JOB);"
        "return 0;}\n")
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src),
                           "-o", exe])
    out = [int(v) for v in subprocess.check_output([exe]).decode().split()]
    dt = api.FP_BI_AFFINE_RESULT_DTYPE
    assert out == [dt.fields[f][1] for f in res_fields] + \
        [getattr(api.FramePassBiAffineArgs, f).offset for f in arg_fields] + \
        [dt.itemsize, C.sizeof(api.FramePassBiAffineArgs), C.sizeof(api.FramePassBiRefsArgs),
         C.sizeof(api.FramePassArgs), api.FP_BI_REFS_RESULT_DTYPE.itemsize, api.FP_BI_NO_JOB]
    # the flat pass's block, embedded in the plain B pass's, stays what it was
    assert C.sizeof(api.FramePassArgs) == 240 and api.FP_BI_REFS_RESULT_DTYPE.itemsize == 124
    assert am.RESULT_DTYPE == dt and am.INTER_DTYPE == api.INTER_DTYPE
    assert oa.BLOCK_DTYPE == api.AFFINE_ME_DTYPE and oa.RESULT_DTYPE == api.AFFINE_ME_RESULT_DTYPE
    assert (am.HAS_BOOTSTRAP, am.BIPRED, am.NO_JOB, am.INTER_AFFINE, am.NO_SLOT) == \
        (api.AFFINE_ME_HAS_BOOTSTRAP, api.AFFINE_ME_BIPRED, api.AFFINE_ME_NO_JOB,
         api.INTER_AFFINE, api.FP_BI_NO_JOB)


def test_entry_points_are_exported_and_refuse_without_a_context(pipeline):
    from xvc_amd import api
    lib = api.load_library()
    hdr = open(os.path.join(ROOT, "include", "xvcgpu.h")).read()
    for name in ENTRY_POINTS:
        assert name in api.SYMBOLS and hasattr(lib, name) and (name + "(") in hdr, name
    a, f = api.FramePassBiRefsArgs(), api.FramePassBiAffineArgs()
    n_class = (C.c_int32 * 3)(0, 0, 0)
    for name in ENTRY_POINTS[:1] + ENTRY_POINTS[2:5]:
        assert getattr(lib, name)(None, C.byref(a), C.byref(f)) == 10, name
    assert lib.xvcgpu_affine_me_listed_refs(None, None, None, 0, None, None, 0, 1, None, n_class,
                                            None) == 10
    assert lib.xvcgpu_frame_pass_bi_refs_affine(None, C.byref(a), C.byref(f), None, 31) == 10


def test_python_refusals(pipeline):
    """affine=True with low_delay or with adaptive QP raises ValueError before anything is
    allocated (no context is touched); back-only lists stay refused as before."""
    P = pipeline
    with pytest.raises(ValueError, match="affine: .*low_delay"):
        P.BiRefsFramePass(None, 104, 72, 10, cur_poc=20, ref_pocs=((16,), (12,)), low_delay=True,
                          affine=True)
    with pytest.raises(ValueError, match="affine: .*aqp_strength"):
        P.BiRefsFramePass(None, 104, 72, 10, aqp_strength=13, affine=True)
    with pytest.raises(ValueError, match="force_l1_mvd_zero"):
        P.BiRefsFramePass(None, 104, 72, 10, cur_poc=20, ref_pocs=((16,), (12,)), affine=True)
