"""The B pass's model (tests/bi_pass_model.py) against the reference: its SearchMotion half
- both lists' searches, the SearchBiIterative step, the folds and the choice - must equal
InterSearch::SearchMotion (inter_search.cc:198-259, xr_search_motion of oracle/_ref) CU for
CU on the inputs the GPU tests run, so that the device pass is pinned to the reference
through the model."""
import ctypes as C

import numpy as np
import pytest

import bi_pass_model as bm
import oracle_lib as ol

pytestmark = pytest.mark.skipif(not ol.have_ref(), reason="oracle/_ref not built")


@pytest.mark.parametrize("name", sorted(bm.INPUTS))
def test_search_motion_half_equals_reference(name):
    xo, xr = ol.Lib("xo"), ol.Lib("xr").dll
    xr.xr_search_motion.restype = None
    xr.xr_search_motion.argtypes = [C.c_int] * 6 + [C.c_uint32] + [C.c_int] * 3 + \
        [C.c_void_p, C.c_ssize_t] * 3 + [C.c_void_p, C.c_void_p]
    pw, ph, bd, _, orig, ref0, ref1 = bm.make_input(name)
    desc = bm.descriptors(name)
    n = desc.n_cus
    planes = [p[0][bm.BL:, bm.BL:] for p in (orig, ref0, ref1)]
    args = []
    for p, full in zip(planes, (orig, ref0, ref1)):
        args += [p.ctypes.data, full[0].strides[0] // 2]
    nb = np.zeros(8, np.int32)
    exp = np.zeros((n, 26), np.int64)
    me = (desc.me, desc.me)
    for i, b in enumerate(desc.me):
        xr.xr_search_motion(bd, int(b["x"]), int(b["y"]), int(b["w"]), int(b["h"]), 0,
                            bm.LAMBDA16, 1, pw, ph, *args, nb.ctypes.data, exp[i].ctypes.data)
    # the inputs' conditions: zero AMVP lists (the jobs' zero mvp stands for both entries)
    # and every direction chosen for at least 4 CUs
    assert not exp[:, 10:18].any()
    assert (exp[:, 8:10] == bm.SEARCH_RANGE).all()      # what the jobs carry
    counts = np.bincount(exp[:, 1].astype(int), minlength=3)
    print(name, "L0 / L1 / bi =", counts.tolist())
    assert (counts >= 4).all(), counts
    res, _, choice = bm.search_motion(xo, bd, pw, ph, orig[0], (ref0[0], ref1[0]), me)
    for i in range(n):
        e, c = exp[i], choice[i]
        d = int(e[1])
        want_mv = [[int(e[2 + 2 * l]), int(e[3 + 2 * l])] if d in (2, l) else [0, 0]
                   for l in range(2)]
        got = (int(c["inter_dir"]), c["mv"].tolist(), int(c["cost"]))
        assert got == (d, want_mv, int(e[0])), (i, tuple(desc.me[i]), got, e.tolist())
        # the uni-directional halves: cost, vector, predictor index per list
        uni = [v for l in range(2) for v in (int(c["cost_uni"][l]), int(res[l][i]["mv_x"]),
                                             int(res[l][i]["mv_y"]), 0)]
        assert uni == [int(v) for v in e[18:26]], (i, tuple(desc.me[i]), uni, e[18:26].tolist())
