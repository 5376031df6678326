"""The model of the B pass (tests/bi_refs_pass_model.py) against the reference: its SearchMotion half - the searches
per picture, the re-use of list 0's results, the SearchBiIterative step into every picture,
the folds and the choice against the best unique list-1 picture - must equal
InterSearch::SearchMotion (xr_search_motion_multi of oracle/_ref) CU for CU on the inputs
and picture sets the GPU tests run, so that the device pass is pinned to the reference
through the model.  No neighbours: every AMVP list is zero, as the jobs' predictors are.

The coverage the GPU tests rely on is checked here too (and printed: DESIGN section 9
states the counts)."""
import ctypes as C

import numpy as np
import pytest

import bi_refs_pass_model as rm
import oracle_lib as ol

pytestmark = pytest.mark.skipif(not ol.have_ref(), reason="oracle/_ref not built")


def reference(name, which):
    """xr_search_motion_multi per CU of the input: out[n, 80]."""
    xr = ol.Lib("xr").dll
    xr.xr_search_motion_multi.restype = None
    xr.xr_search_motion_multi.argtypes = [C.c_int] * 6 + [C.c_uint32] + [C.c_int] * 3 + \
        [C.c_void_p, C.c_ssize_t, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
         C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    pw, ph, bd, _, orig, refs = rm.make_refs(name)
    lists = rm.SETS[which]
    num_ref, _, distinct, slot = rm.tables(lists)
    desc = rm.descriptors(name)
    planes = [refs[p][0] for p in distinct]
    ptrs = (C.c_void_p * len(planes))(*[p[rm.BL:, rm.BL:].ctypes.data for p in planes])
    strides = np.array([p.strides[0] // 2 for p in planes], np.int64)
    pocs = np.array(distinct, np.int32)
    ref_pic = np.full((2, 3), -1, np.int32)
    for l in range(2):
        ref_pic[l, :num_ref[l]] = slot[l]
    nr = np.array(num_ref, np.int32)
    nb = np.full((2, 2, 3), -1, np.int32)       # no neighbours: zero AMVP lists
    o = orig[0][rm.BL:, rm.BL:]
    exp = np.zeros((desc.n_cus, 80), np.int64)
    for i, b in enumerate(desc.me):
        xr.xr_search_motion_multi(bd, int(b["x"]), int(b["y"]), int(b["w"]), int(b["h"]), 0,
                                  rm.LAMBDA16, 1, pw, ph, o.ctypes.data,
                                  orig[0].strides[0] // 2, len(planes), ptrs,
                                  strides.ctypes.data, pocs.ctypes.data, rm.CUR_POC,
                                  nr.ctypes.data, ref_pic.ctypes.data, nb.ctypes.data,
                                  exp[i].ctypes.data)
    return exp


def model(name, which):
    xo = ol.Lib("xo")
    pw, ph, bd, _, orig, refs = rm.make_refs(name)
    lists = rm.SETS[which]
    desc = rm.descriptors(name)
    return desc, rm.search_motion(xo, bd, pw, ph, orig[0], refs, lists, rm.jobs(desc, lists),
                                  key=name)


@pytest.mark.parametrize("which", ["A", "B", "C", "D"])
@pytest.mark.parametrize("name", ["grid10", "grid8", "part10"])
def test_search_motion_half_equals_reference(name, which):
    lists = rm.SETS[which]
    num_ref, same, _, _ = rm.tables(lists)
    exp = reference(name, which)
    desc, (res, bi, slots, choice, inter) = model(name, which)
    assert not exp[:, 10].any()                      # no picture with only back references
    for l in range(2):
        for r in range(num_ref[l]):
            q = exp[:, 16 + 8 * (3 * l + r):]
            assert (q[:, 0] == rm.search_range(lists[l][r])).all()   # what the jobs carry
            assert not q[:, 1:5].any()                          # zero AMVP lists
            assert (q[:, 5] == (same[r] if l == 1 else -1)).all()
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
        # the lists alone: cost, ref_idx, vector, predictor index; list 1's unique cost
        for l in range(2):
            r = int(c["best_ref"][l])
            q = res[l][r] if res[l][r] is not None else res[0][same[r]]
            uni = [int(c["cost_list"][l]), r, int(q[i]["mv_x"]), int(q[i]["mv_y"]), 0]
            assert uni == [int(v) for v in e[64 + 6 * l:69 + 6 * l]], (i, l, uni, e[64:76])
        # (the reference leaves the unique cost at Distortion's max where there is none)
        assert int(c["cost_l1_unique"]) == int(e[75]) & 0xffffffff, (i, c["cost_l1_unique"], e[75])


def test_coverage_of_the_picture_sets():
    """What the seeds were chosen for; the GPU tests compare against this model on these
    inputs, so what is not chosen here is not tested there."""
    for which in ("A", "B", "C", "D"):
        total = np.zeros(3, int)
        idx_gt0 = [0, 0]
        l1_best_reused_chosen_unique = 0
        for name in ("grid10", "grid8", "part10"):
            _, (res, bi, slots, choice, inter) = model(name, which)
            _, same, _, _ = rm.tables(rm.SETS[which])
            dirs = np.bincount(choice["inter_dir"], minlength=3)
            total += dirs
            for l in range(2):
                idx_gt0[l] += int((choice["ref_idx"][:, l] > 0).sum())
            for c in choice:
                if int(c["inter_dir"]) == 1 and same[int(c["best_ref"][1])] >= 0:
                    l1_best_reused_chosen_unique += 1
            print(which, name, "L0 / L1 / bi =", dirs.tolist(),
                  "ref_idx > 0 chosen per list (so far):", idx_gt0,
                  "cost_l1 != cost_l1_unique:",
                  int((choice["cost_list"][:, 1] != choice["cost_l1_unique"]).sum()))
            if which in ("A", "C"):
                assert (dirs >= 3).all(), (which, name, dirs)
            if which == "B":
                assert dirs[1] == 0 and (choice["cost_l1_unique"] == rm.NONE).all()
                assert (slots[:, :, 0] != rm.NO_JOB).all()
            if which == "D":        # one picture per list: every direction, every slot a job
                assert (dirs >= 4).all(), (which, name, dirs)
                assert (slots != rm.NO_JOB).all()
            if which == "C":        # list 1's third slot is never a job
                s1 = choice["search_list"] == 1
                assert s1.any() and (slots[s1, 2, 0] == rm.NO_JOB).all()
                assert (slots[~s1, 2, 0] != rm.NO_JOB).all()
        if which in ("A", "C"):
            assert min(idx_gt0) >= 3, (which, idx_gt0)
        if which == "C":
            print("C: list 1's best is the re-used picture, the unique one is chosen:",
                  l1_best_reused_chosen_unique)
            assert l1_best_reused_chosen_unique >= 1
