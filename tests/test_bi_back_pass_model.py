"""The model of the low-delay B pass (tests/bi_back_pass_model.py) against the reference: its
SearchMotion half under force_l1_mvd_zero - the predictor as list 1's candidate, the unique
pictures' searches, list 0 refined against the predictor, the folds and the choice - must
equal InterSearch::SearchMotion (xr_search_motion_multi of oracle/_ref) CU for CU on the
inputs and picture sets the GPU tests run, and its predictor cost must equal EvalStartMvp
(xr_eval_start_mvp), so that the device pass is pinned to the reference through the model.
No neighbours: every AMVP list is zero, as the jobs' predictors are.

Also here, without a GPU: the tie rules in integers, the coverage the GPU tests rely on
(printed: DESIGN section 12 states the counts), the new symbols against the header and the
library, and the refusals of pipeline.BiRefsFramePass."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import bi_back_pass_model as bm
import bi_refs_pass_model as rm
import helpers
import oracle_lib as ol

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
needs_ref = pytest.mark.skipif(not ol.have_ref(), reason="oracle/_ref not built")

_inputs, _models = {}, {}


def model_input(name):
    if name not in _inputs:
        _inputs[name] = bm.make_refs(name)
    return _inputs[name]


def reference(name, which):
    """xr_search_motion_multi per CU of the input: out[n, 80]."""
    xr = ol.Lib("xr").dll
    xr.xr_search_motion_multi.restype = None
    xr.xr_search_motion_multi.argtypes = [C.c_int] * 6 + [C.c_uint32] + [C.c_int] * 3 + \
        [C.c_void_p, C.c_ssize_t, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
         C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    pw, ph, bd, _, orig, refs = model_input(name)
    lists = bm.SETS[which]
    num_ref, _, distinct, slot = bm.tables(lists)
    desc = bm.descriptors(name)
    planes = [refs[p][0] for p in distinct]
    ptrs = (C.c_void_p * len(planes))(*[p[bm.BL:, bm.BL:].ctypes.data for p in planes])
    strides = np.array([p.strides[0] // 2 for p in planes], np.int64)
    pocs = np.array(distinct, np.int32)
    ref_pic = np.full((2, 3), -1, np.int32)
    for l in range(2):
        ref_pic[l, :num_ref[l]] = slot[l]
    nr = np.array(num_ref, np.int32)
    nb = np.full((2, 2, 3), -1, np.int32)       # no neighbours: zero AMVP lists
    o = orig[0][bm.BL:, bm.BL:]
    exp = np.zeros((desc.n_cus, 80), np.int64)
    for i, b in enumerate(desc.me):
        xr.xr_search_motion_multi(bd, int(b["x"]), int(b["y"]), int(b["w"]), int(b["h"]), 0,
                                  bm.LAMBDA16, 1, pw, ph, o.ctypes.data,
                                  orig[0].strides[0] // 2, len(planes), ptrs,
                                  strides.ctypes.data, pocs.ctypes.data, bm.CUR_POC,
                                  nr.ctypes.data, ref_pic.ctypes.data, nb.ctypes.data,
                                  exp[i].ctypes.data)
    return exp


def model(name, which):
    if (name, which) not in _models:
        xo = ol.Lib("xo")
        pw, ph, bd, _, orig, refs = model_input(name)
        lists = bm.SETS[which]
        desc = bm.descriptors(name)
        _models[name, which] = desc, bm.search_motion(xo, bd, pw, ph, orig[0], refs, lists,
                                                      bm.jobs(desc, lists), key=name)
    return _models[name, which]


@needs_ref
@pytest.mark.parametrize("which", ["E", "F", "G", "H"])
@pytest.mark.parametrize("name", ["grid10", "grid8", "part10"])
def test_search_motion_half_equals_reference(name, which):
    lists = bm.SETS[which]
    num_ref, same, _, _ = bm.tables(lists)
    exp = reference(name, which)
    desc, (res, bi, slots, choice, inter, l1_cost, jobs) = model(name, which)
    assert (exp[:, 10] == 1).all()                   # the picture derives the flag itself
    for l in range(2):
        for r in range(num_ref[l]):
            q = exp[:, 16 + 8 * (3 * l + r):]
            assert (q[:, 0] == bm.search_range(lists[l][r])).all()   # what the jobs carry
            assert not q[:, 1:5].any()                          # zero AMVP lists
            assert (q[:, 5] == (same[r] if l == 1 else -1)).all()
    assert (choice["search_list"] == 0).all()
    for i in range(desc.n_cus):
        e, c = exp[i], choice[i]
        d = int(e[1])
        want = [d, int(e[0])]
        got = [int(c["inter_dir"]), int(c["cost"])]
        for l in range(2):
            # ref_idx, vector, predictor index of the chosen state
            want += [int(e[2 + 4 * l]), int(e[3 + 4 * l]), int(e[4 + 4 * l]), int(e[5 + 4 * l])]
            got += [int(c["ref_idx"][l]), int(c["mv"][l][0]), int(c["mv"][l][1]), 0]
        assert got == want, (i, tuple(desc.me[i]), got, want)
        # the lists alone: cost, ref_idx, vector, predictor index.  List 1's is the predictor
        # of its best picture at the predictor's price
        r0, r1 = int(c["best_ref"][0]), int(c["best_ref"][1])
        uni = [int(c["cost_list"][0]), r0, int(res[0][r0][i]["mv_x"]), int(res[0][r0][i]["mv_y"]), 0]
        assert uni == [int(v) for v in e[64:69]], (i, 0, uni, e[64:76])
        p1 = bm.jobs(desc, lists)[1][r1][i]
        uni = [int(c["cost_list"][1]), r1, int(p1["mvp_x"]), int(p1["mvp_y"]), 0]
        assert uni == [int(v) for v in e[70:75]], (i, 1, uni, e[64:76])
        assert int(c["cost_list"][1]) == int(l1_cost[i][r1]) == int(l1_cost[i][:num_ref[1]].min())
        # (the reference leaves the unique cost at Distortion's max where there is none)
        assert int(c["cost_l1_unique"]) == int(e[75]) & 0xffffffff, (i, c["cost_l1_unique"], e[75])
        if d == 2:      # a bi-directional CU carries list 1's (zero) predictor
            assert not c["mv"][1].any()


def _planted_jobs(rng, bd, pw, ph, rects, spread):
    me = np.zeros(len(rects), ol.ME_DTYPE)
    me["x"], me["y"], me["w"], me["h"] = rects[:, 0], rects[:, 1], rects[:, 2], rects[:, 3]
    me["depth_nonzero"] = 1
    me["lambda16"] = rng.choice([120000, 498000, 1500000], len(rects))
    me["search_range"] = 96
    me["mvp_x"], me["mvp_y"] = rng.integers(-spread, spread + 1, (2, len(rects)))
    return me


@needs_ref
@pytest.mark.parametrize("bd", [8, 10, 12])
def test_predictor_cost_equals_eval_start_mvp(bd):
    """bm.mvp_cost against InterSearch::EvalStartMvp with both AMVP entries the same vector,
    on every shape of partition_128: predictors of up to +-40 quarter samples, and +-3000
    ones, which ClipMv changes (the picture is 128 x 128: 3000 / 16 samples leave it)."""
    xr, xo = ol.Lib("xr"), ol.Lib("xo")
    xr.dll.xr_eval_start_mvp.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                                         C.c_ssize_t, C.c_void_p, C.c_ssize_t, C.c_void_p,
                                         C.c_void_p]
    rng = np.random.default_rng(5300 + bd)
    pw = ph = 128
    orig, ref = helpers.make_pics(rng, bd, pw, ph, bm.BL, (3, -2))
    rects = rm.partition_128()
    assert {(int(w), int(h)) for _, _, w, h in rects} >= {
        (64, 64), (32, 32), (32, 16), (16, 32), (16, 16), (8, 8), (8, 4), (4, 8)}
    o, r = orig[bm.BL:, bm.BL:], ref[bm.BL:, bm.BL:]
    costs = set()
    for spread, planted in ((40, None), (0, 3000)):
        me = _planted_jobs(rng, bd, pw, ph, rects, spread)
        if planted:
            me["mvp_x"] = rng.choice([-planted, planted], len(me))
            me["mvp_y"] = rng.choice([-planted, planted, 0], len(me))
        for b in me:
            mvp = np.array([b["mvp_x"], b["mvp_y"]] * 2, np.int32)
            c = C.c_uint32(0)
            s = helpers.me_struct(b)
            idx = xr.dll.xr_eval_start_mvp(bd, C.byref(s), pw, ph, o.ctypes.data,
                                           orig.strides[0] // 2, r.ctypes.data,
                                           ref.strides[0] // 2, mvp.ctypes.data, C.byref(c))
            got = bm.mvp_cost(xo, bd, pw, ph, orig, ref, b)
            assert (0, got) == (idx, c.value), (tuple(b), got, c.value)
            costs.add(got)
    assert len(costs) > len(rects)
    # a shape outside the kernel's set has no price
    odd = _planted_jobs(rng, bd, pw, ph, np.array([(0, 0, 12, 8), (0, 0, 8, 2)]), 8)
    assert [bm.mvp_cost(xo, bd, pw, ph, orig, ref, b) for b in odd] == [bm.NONE, bm.NONE]


def _hand_made(lists, n, seed):
    """Random jobs and search results per (list, picture), refinement results and predictor
    costs: what the folds read."""
    num_ref, same, _, _ = bm.tables(lists)
    rng = np.random.default_rng(seed)
    base = np.zeros(n, ol.ME_DTYPE)
    base["x"], base["y"] = 8 * (np.arange(n) % 8), 8 * (np.arange(n) // 8)
    base["w"] = base["h"] = 8
    base["depth_nonzero"], base["lambda16"] = 1, 498000
    me = [[base.copy() for _ in range(num_ref[l])] for l in range(2)]
    res = [[None] * num_ref[l] for l in range(2)]
    for l in range(2):
        for r in range(num_ref[l]):
            me[l][r]["mvp_x"], me[l][r]["mvp_y"] = rng.integers(-160, 161, (2, n))
            if l == 0 or same[r] < 0:
                q = res[l][r] = np.zeros(n, ol.MERES_DTYPE)
                q["mv_x"], q["mv_y"] = rng.integers(-300, 301, (2, n))
                q["subpel_dist"] = rng.integers(400, 3000, n)
    bi = np.zeros((n, max(num_ref)), ol.MERES_DTYPE)
    bi["mv_x"], bi["mv_y"] = rng.integers(-300, 301, (2,) + bi.shape)
    bi["subpel_dist"] = rng.integers(300, 2500, bi.shape)
    l1 = np.full((n, bm.MAX_REFS), bm.NONE, np.uint32)
    l1[:, :num_ref[1]] = rng.integers(500, 4000, (n, num_ref[1]))
    return me, res, bi, l1


def test_tie_rules_in_integers():
    """Equal predictor costs take the lower index; cost_bi == cost_l0 gives bi; cost_l0 ==
    cost_l1_unique gives list 0 (ChooseUniOrBi, inter_search.cc:247-257)."""
    lists = bm.SETS["F"]                    # list 1: (12 re-used, 4 unique, 0 unique)
    me, res, bi, l1 = _hand_made(lists, 8, 3)
    l1[:, 0], l1[:, 1], l1[:, 2] = 900, 700, 700
    choice, jobs, slots = bm.uni_fold(lists, me, res, l1)
    assert (choice["best_ref"][:, 1] == 1).all() and (choice["cost_list"][:, 1] == 700).all()
    assert (choice["cost_uni"][:, 1] == (900, 700, 700)).all()
    assert (choice["search_list"] == 0).all() and (slots[:, 2, 0] == bm.NO_JOB).all()
    assert (jobs["other_mv_x"][:, 0] == me[1][1]["mvp_x"]).all()
    assert (jobs["boot_mv_y"][:, 1] == res[0][1]["mv_y"]).all()
    assert (slots[:, 0] == (0, 2)).all() and (slots[:, 1] == (1, 2)).all()
    # the re-used picture's search result (list 0's) never prices list 1
    assert (choice["best_ref_l1_unique"] >= 1).all()
    # cost_bi == cost_l0: the refined picture 0 gets the distortion that makes it so
    trial, _ = bm.choice_fold(lists, me, res, bi, choice)
    bi2 = bi.copy()
    for i in range(8):
        c = trial[i]
        bits_cost = int(c["bi_cost"][0]) - int(bi[i][0]["subpel_dist"])
        res[1][1]["subpel_dist"][i] = res[1][2]["subpel_dist"][i] = 60000    # no list-1 win
        bi2["subpel_dist"][i] = 100000
        bi2[i][0]["subpel_dist"] = int(c["cost_list"][0]) - bits_cost
    choice, _, _ = bm.uni_fold(lists, me, res, l1)
    tied, inter = bm.choice_fold(lists, me, res, bi2, choice)
    assert (tied["cost_bi"] == tied["cost_list"][:, 0]).all() and (tied["inter_dir"] == 2).all()
    # ... and a bi-directional CU carries the predictor of list 1's best picture, unclipped
    assert (tied["mv"][:, 1, 0] == me[1][1]["mvp_x"]).all()
    assert (tied["mv"][:, 1, 1] == me[1][1]["mvp_y"]).all()
    assert all(q[4] == (0, 2) and q[5][1] == (int(me[1][1]["mvp_x"][i]), int(me[1][1]["mvp_y"][i]))
               for i, q in enumerate(inter))
    # cost_l0 == cost_l1_unique below cost_bi: list 0
    for i in range(8):
        for a in (me, res):
            a[1][1][i] = a[0][0][i]
        res[0][0]["subpel_dist"][i] = res[1][1]["subpel_dist"][i] = 500
    bi2["subpel_dist"] = 100000
    choice, _, _ = bm.uni_fold(lists, me, res, l1)
    # (list 1's index 1 of three costs one bit more than list 0's index 0 of two: the
    # distortion takes the difference back)
    res[1][1]["subpel_dist"] -= choice["cost_l1_unique"] - choice["cost_list"][:, 0]
    choice, _, _ = bm.uni_fold(lists, me, res, l1)
    tied, _ = bm.choice_fold(lists, me, res, bi2, choice)
    assert (tied["cost_list"][:, 0] == tied["cost_l1_unique"]).all()
    assert (tied["inter_dir"] == 0).all() and (tied["ref_idx"] == (0, -1)).all()
    # one more on list 0's side: the unique list-1 picture with its searched vector
    res[0][0]["subpel_dist"] += 1
    choice, _, _ = bm.uni_fold(lists, me, res, l1)
    lost, _ = bm.choice_fold(lists, me, res, bi2, choice)
    assert (lost["inter_dir"] == 1).all() and (lost["ref_idx"] == (-1, 1)).all()
    assert (lost["mv"][:, 1, 0] == res[1][1]["mv_x"]).all()


def test_bits_of_a_bi_directional_state():
    """List 1 adds RefIdxBits + GetMvpBits and no vector-difference bits (GetForceMvdZero;
    the host twin: xvc_gpu_ops.h, SearchMotionMultiBatch)."""
    lists = bm.SETS["E"]
    me, res, bi, l1 = _hand_made(lists, 4, 9)
    choice, _, _ = bm.uni_fold(lists, me, res, l1)
    done, _ = bm.choice_fold(lists, me, res, bi, choice)
    for i in range(4):
        r1 = int(done[i]["best_ref"][1])
        for k in range(2):
            mv = (int(bi[i][k]["mv_x"]), int(bi[i][k]["mv_y"]))
            bits = 5 + bm.ref_idx_bits(2, k) + 1 + bm.mvd_bits(me[0][k][i], mv) + \
                bm.ref_idx_bits(2, r1) + 1
            assert int(done[i]["bi_cost"][k]) == int(bi[i][k]["subpel_dist"]) + \
                ((bits * 498000) >> 16)


def test_coverage_of_the_picture_sets():
    """What the tables were chosen for; the GPU tests compare against this model on these
    inputs, so what is not chosen here is not tested there."""
    for which in ("E", "F", "G", "H"):
        total, l1_in_bi, l0_idx = np.zeros(3, int), set(), set()
        for name in ("grid10", "grid8", "part10"):
            _, (res, bi, slots, choice, inter, l1_cost, jobs) = model(name, which)
            num_ref, same, _, _ = bm.tables(bm.SETS[which])
            dirs = np.bincount(choice["inter_dir"], minlength=3)
            total += dirs
            is_bi = choice["inter_dir"] == 2
            l1_in_bi |= set(choice["ref_idx"][is_bi, 1].tolist())
            l0_idx |= set(choice["ref_idx"][choice["inter_dir"] != 1, 0].tolist())
            print(which, name, "L0 / L1 / bi =", dirs.tolist(), "list-1 index of bi CUs:",
                  np.bincount(choice["ref_idx"][is_bi, 1], minlength=num_ref[1]).tolist(),
                  "list-0 index chosen:",
                  np.bincount(choice["ref_idx"][choice["inter_dir"] != 1, 0],
                              minlength=num_ref[0]).tolist())
            assert (choice["search_list"] == 0).all()
            assert (slots[:, :num_ref[0], 0] != bm.NO_JOB).all()
            assert (slots[:, num_ref[0]:, 0] == bm.NO_JOB).all()
            assert not choice["mv"][is_bi, 1].any()         # the zero predictor
            if which in ("E", "H"):
                assert dirs[1] == 0 and (choice["cost_l1_unique"] == bm.NONE).all()
        if which == "E":
            assert total[2] >= 5 and total[0] >= 5 and l1_in_bi == {0, 1}, (total, l1_in_bi)
        if which == "F":
            assert (total >= 3).all(), total
        if which == "G":
            assert l0_idx == {0, 1, 2} and total[1] >= 1, (l0_idx, total)
        if which == "H":
            assert total[0] >= 1 and total[2] >= 1, total


# ---- the boundary, without a GPU ---------------------------------------------------------
_NEW_SYMBOLS = ("xvcgpu_fp_bi_back_mvp_cost", "xvcgpu_fp_bi_back_uni_fold",
                "xvcgpu_fp_bi_back_choice", "xvcgpu_frame_pass_bi_back")


def test_entry_points_are_declared_and_exported():
    from xvc_amd import api
    lib = C.CDLL(os.path.join(ROOT, "xvc_amd", "libxvcgpu.so"))
    hdr = open(os.path.join(ROOT, "include", "xvcgpu.h")).read()
    for name in _NEW_SYMBOLS:
        assert name in api.SYMBOLS and hasattr(lib, name) and \
            re.search(r"xvcgpu_status %s\(" % name, hdr), name
    # the args block and the record are the B pass's, unchanged
    assert api.FP_BI_REFS_RESULT_DTYPE.itemsize == 124
    assert api.FP_BI_REFS_RESULT_DTYPE == bm.CHOICE_DTYPE


def test_low_delay_accepts_only_back_references():
    from xvc_amd import pipeline
    with pytest.raises(ValueError, match="low_delay"):
        pipeline.BiRefsFramePass(None, 64, 64, cur_poc=8, ref_pocs=((4, 0), (12,)),
                                 low_delay=True)
    with pytest.raises(ValueError, match="low_delay"):
        pipeline.BiRefsFramePass(None, 64, 64, cur_poc=8, ref_pocs=((8,), (4,)), low_delay=True)
    with pytest.raises(ValueError, match="only back references"):
        pipeline.BiRefsFramePass(None, 64, 64, cur_poc=8, ref_pocs=((4, 0), (0, 4)))
    with pytest.raises(ValueError, match="only back references"):
        pipeline.BiRefsFramePass(None, 64, 64, cur_poc=20, ref_pocs=bm.SETS["E"],
                                 low_delay=False)
    for lists in bm.SETS.values():
        _, same, distinct, slot = bm.tables(lists)
        assert pipeline.ref_list_tables(bm.CUR_POC, lists) == (same, distinct, slot, True)
