"""What each whole-stream fixture holds (tests/golden/stream_*.npz, made by
tools/gen_stream_golden.py): the depths, filter settings and coding tools a
fixture was made for must still be in it after a regeneration, or the decoder
tests that read it (test_stream_oracle.py, test_gpu_stream.py,
test_gpu_output_format.py) silently stop covering them.  Reads only the .npz;
CPU only."""
import functools

import numpy as np
import pytest

import stream_fixture as sf

# name: (internal bit depth, deblock, beta_offset, tc_offset) of every picture
SETTINGS = {
    "t8": (8, 1, 0, 0), "t12": (12, 1, 0, 0), "t9": (9, 1, 0, 0), "t11": (11, 1, 0, 0),
    "tq8": (10, 1, 0, 0), "t12q2": (12, 1, 0, 0), "tq50": (10, 1, 0, 0), "tdb": (10, 1, 4, -3),
    "t8db": (8, 1, -6, 6), "t12nodb": (12, 0, 0, 0), "tld": (10, 1, 0, 0),
    "warp": (10, 1, 0, 0), "warpld": (10, 1, 0, 0),
}
assert sorted(SETTINGS) == sorted(sf.OTHER_STREAMS)
FIRST_SIX = ["tiny", "c0", "c0q22", "c0q37", "c1", "c1x"]
PIC_BI, PIC_UNI, PIC_INTRA = 0, 1, 2        # include/xvc_syntax.h XVC_PIC_*


@functools.lru_cache(maxsize=None)
def load(name):
    """(info[], all CUs with their picture's index, all levels) of a fixture."""
    fx = sf.StreamFixture(name)
    cus = [fx.cus(i) for i in range(fx.n)]
    pic = np.concatenate([np.full(len(c), i) for i, c in enumerate(cus)])
    return fx.info, np.concatenate(cus), pic, np.concatenate([fx.levels(i) for i in range(fx.n)])


def has_comp(info, cus, pic, c):
    """The CUs that carry component c: in a picture of two trees luma lies in the
    primary tree, chroma in the secondary."""
    two = info["two_trees"][pic] != 0
    return np.where(two, cus["tree"] == (1 if c else 0), True)


@pytest.mark.parametrize("name", sorted(SETTINGS))
def test_settings_of_every_picture(name):
    info = load(name)[0]
    bd, deblock, beta, tc = SETTINGS[name]
    assert len(info) >= 5
    assert (info["bitdepth"] == bd).all(), info["bitdepth"]
    assert (info["deblock"] == deblock).all(), info["deblock"]
    assert (info["beta_offset"] == beta).all(), info["beta_offset"]
    assert (info["tc_offset"] == tc).all(), info["tc_offset"]
    assert (info["conforming"] == 1).all()
    assert not any(k.startswith(("post_", "pre_")) for k in sf.StreamFixture(name).z.files)


@pytest.mark.parametrize("name", ["tq8", "t12q2"])
def test_fine_quantiser_streams(name):
    """Transform skip in luma AND both chroma components, many intra modes, levels
    beyond anything the first six fixtures hold (+-188)."""
    info, cus, pic, lv = load(name)
    for c in range(3):
        n = int(((cus["cbf"][:, c] != 0) & (cus["tx_skip"][:, c] != 0) &
                 has_comp(info, cus, pic, c)).sum())
        assert n >= 1, (name, c)
    luma_intra = (cus["pred_mode"] == 0) & has_comp(info, cus, pic, 0)
    modes = set(cus["intra_mode"][luma_intra, 0].tolist())
    assert min(modes) >= 0 and max(modes) <= 66
    assert len(modes) >= 30, sorted(modes)
    assert int(np.abs(lv.astype(np.int32)).max()) >= 300


def test_coarse_quantiser_stream():
    """The in-loop filter's tc index, qp + 2 * (bs - 1) + tc_offset, clamps at 53: a
    luma QP of 56 is beyond it whatever the strength."""
    info, cus, pic, _ = load("tq50")
    assert int(cus["qp"][has_comp(info, cus, pic, 0), 0].max()) >= 56


def test_chroma_qp_offset_stream():
    info, cus, pic, _ = load("t8db")
    chroma = has_comp(info, cus, pic, 1)
    assert int((cus["qp"][chroma, 1] != cus["qp"][chroma, 2]).sum()) >= 1
    assert (cus["ref_idx"][cus["pred_mode"] == 1] == 1).any()


def test_low_delay_stream():
    """Low delay: decoding order is output order and no list holds a later picture.
    (The reference encoder gives every inter picture the bi-predictive type, low
    delay included: both lists, each of earlier pictures; its uni-predictive type
    exists in restricted mode only.)"""
    info, cus, _, _ = load("tld")
    assert (cus["ref_idx"][cus["pred_mode"] == 1] == 3).any()
    assert np.array_equal(info["poc"], info["doc"])
    assert (info["tid"] == 0).all()
    for p in info:
        for l in range(2):
            refs = p["ref_poc"][l][:int(p["num_ref"][l])]
            assert (refs < p["poc"]).all() and (refs >= 0).all(), (p["poc"], refs)
    assert set(info["pic_type"][1:].tolist()) == {PIC_BI} and info["pic_type"][0] == PIC_INTRA
    assert int(info["num_ref"].max()) == 4


def test_affine_streams():
    _, cus, _, _ = load("warp")
    aff = cus["affine"] == 1
    assert int((aff & (cus["inter_dir"] != 2)).sum()) >= 10
    info, cus, _, _ = load("warpld")
    aff = cus["affine"] == 1
    assert int((aff & (cus["inter_dir"] != 2)).sum()) >= 1
    assert int((aff & (cus["inter_dir"] == 2)).sum()) >= 1
    assert (cus["ref_idx"][cus["pred_mode"] == 1] == 2).any()
    assert np.array_equal(info["poc"], info["doc"])


@pytest.mark.parametrize("name", ["t8", "t12", "t9", "t11", "tdb", "t12nodb"])
def test_depth_and_filter_streams(name):
    """Local illumination compensation and an intra picture of two CU trees at
    every depth and filter setting."""
    _, cus, _, _ = load(name)
    assert int(cus["lic"].sum()) >= 1
    assert (cus["tree"] == 0).any() and (cus["tree"] == 1).any()


# The luma transform-type pairs (vertical, horizontal) over the adaptive types 2 to 5
# that some fixture holds in a coded luma block without transform skip.  A record, no
# floor: the reference encoder never chose the four others - (2, 4), (3, 4), (4, 2),
# (4, 3) - in any of the 19 streams, so no stream test takes the inverse transform
# through them.
LUMA_TX_PAIRS = {(2, 2), (2, 3), (2, 5), (3, 2), (3, 3), (3, 5), (4, 4), (4, 5), (5, 2), (5, 3),
                 (5, 4), (5, 5)}


def test_luma_transform_pairs_are_listed():
    seen = set()
    for name in FIRST_SIX + sorted(SETTINGS):
        info, cus, pic, _ = load(name)
        coded = (cus["cbf"][:, 0] != 0) & (cus["tx_skip"][:, 0] == 0) & has_comp(info, cus, pic, 0)
        seen |= set(map(tuple, np.unique(cus["tx_type"][coded, 0], axis=0).tolist()))
    adaptive = {p for p in seen if 2 <= p[0] <= 5 and 2 <= p[1] <= 5}
    assert adaptive == LUMA_TX_PAIRS, (sorted(adaptive - LUMA_TX_PAIRS),
                                      sorted(LUMA_TX_PAIRS - adaptive))
