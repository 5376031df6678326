"""The frame pass's descriptors over a caller's CU partition (no GPU needed):
pipeline.check_partition, FrameDescriptors(partition=...) against the cu x cu grid, and
the checker of the GPU partition pass pinned on the new ground - the oracle's frame pass
(xo_frame_pass) against the same composition run by the reference's own classes
(xr_frame_pass) on real partitions out of the committed stream fixtures."""
import numpy as np
import pytest

import oracle_lib as ol
from partition_fixture import luma_partition, picture_size

# (fixture, picture): the luma trees the GPU tests run (tests/test_gpu_partition_pass.py)
SMALL = [("tiny", 1), ("tiny", 3), ("c0", 1), ("c0q22", 1)]
LARGE = [("c1", 1), ("c1x", 3)]


@pytest.mark.parametrize("name,pic", SMALL + LARGE)
def test_check_partition_accepts_fixture_partitions(name, pic):
    from xvc_amd import pipeline
    parts = luma_partition(name, pic)
    w, h = picture_size(name, pic)
    out = pipeline.check_partition(w, h, parts)
    assert out == [tuple(int(v) for v in p) for p in parts]
    assert sum(p[2] * p[3] for p in out) == w * h
    # a list of tuples is taken as well as the array
    assert pipeline.check_partition(w, h, out) == out


def test_check_partition_refuses():
    from xvc_amd import pipeline
    good = [(0, 0, 32, 64), (32, 0, 32, 32), (32, 32, 32, 32)]
    assert pipeline.check_partition(64, 64, good) == good
    cases = {
        "overlap": ([(0, 0, 32, 64), (32, 0, 32, 32), (16, 32, 32, 32), (48, 32, 16, 32)], "CU 2"),
        "gap": ([(0, 0, 32, 64), (32, 0, 32, 32)], "x=32, y=32"),
        "12 wide": ([(0, 0, 12, 64), (12, 0, 4, 64), (16, 0, 16, 64), (32, 0, 32, 64)], "CU 0"),
        "off grid": ([(0, 0, 32, 64), (32, 0, 32, 32), (34, 32, 30, 32)], "CU 2"),
        "outside": ([(0, 0, 32, 64), (32, 0, 64, 64)], "CU 1"),
        "40 wide inside": ([(0, 0, 40, 64), (40, 0, 8, 64), (48, 0, 16, 64), (64, 0, 64, 64)], "CU 0"),
    }
    for what, (parts, names) in cases.items():
        w = 128 if what == "40 wide inside" else 64
        with pytest.raises(ValueError) as e:
            pipeline.check_partition(w, 64, parts)
        assert names in str(e.value), (what, str(e.value))
    # a side cut by the right / bottom picture edge to a multiple of 4 is a CU
    assert pipeline.check_partition(88, 40, [(0, 0, 64, 40), (64, 0, 24, 40)])
    with pytest.raises(ValueError):
        pipeline.FrameDescriptors(64, 64, 32, partition=good, row_range=(0, 32))
    with pytest.raises(ValueError):
        pipeline.FrameDescriptors(64, 64, 32, partition=good, xcd_tiles=True)


@pytest.mark.parametrize("w,h", [(352, 288), (136, 72)])
@pytest.mark.parametrize("cu", [8, 16, 32, 64])
@pytest.mark.parametrize("rdoq", [False, True])
def test_grid_partition_equals_grid(w, h, cu, rdoq):
    from xvc_amd import pipeline
    a = pipeline.FrameDescriptors(w, h, 27, cu, rdoq=rdoq, bitdepth=8)
    b = pipeline.FrameDescriptors(w, h, 27, partition=pipeline.cu_partition(w, h, cu),
                                  rdoq=rdoq, bitdepth=8)
    for f in ("me", "tx", "luma_idx", "cu_map"):
        x, y = getattr(a, f), getattr(b, f)
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), f
    if rdoq:
        assert a.rdoq_params.tobytes() == b.rdoq_params.tobytes()
        assert a.rdoq_contexts.tobytes() == b.rdoq_contexts.tobytes()
    assert (a.n_cus, a.n_cus_total, a.cu_base, a.qp_c) == (b.n_cus, b.n_cus_total, b.cu_base, b.qp_c)
    assert b.cu_size == max(16, cu) and b.cu_rows is None and b.cus_per_row is None


def compare_oracle_and_reference(name, pic, bd, qp, rdoq):
    """The comparison of test_frame_pass_composition (test_oracle_vs_ref.py) on a
    partition; returns the number of transform blocks that kept levels.  One thread on
    both sides (the default).  Observed while writing this test: with threads=4 the two
    checkers differed in one 8x2 chroma block of `tiny` picture 1 (10 bit, QP 32,
    QuantFast: nnz 1 against 0) and agreed with threads=1.  Which side is wrong with
    four threads, and why, is not established (it deserves an issue of its own against
    the checkers); the GPU tests compare with the single-threaded oracle, which this
    test pins against the single-threaded reference."""
    import oracle_frame
    from xvc_amd import pipeline, synth
    xo, xr = ol.Lib("xo"), ol.Lib("xr")
    xr._set_simd(1)
    BL = 128
    w, h = picture_size(name, pic)
    clip = synth.SyntheticClip(w, h, bd)
    desc = pipeline.FrameDescriptors(w, h, qp, partition=luma_partition(name, pic), rdoq=rdoq,
                                     bitdepth=bd)

    def padded(planes):
        return [np.ascontiguousarray(np.pad(p, BL >> (c > 0), mode="edge"))
                for c, p in enumerate(planes)]

    ref, orig = padded(clip.frame(0)), padded(clip.frame(1))
    o_rec, o_res, o_nnz, o_cus, o_ssd = oracle_frame.frame_pass(desc, bd, orig, ref, BL, 0, lib=xo)
    r_rec, r_res, r_nnz, r_cus, r_ssd = oracle_frame.frame_pass(desc, bd, orig, ref, BL, 0, lib=xr,
                                                                reference=True)
    for f in ("fullpel_x", "fullpel_y", "mv_x", "mv_y", "subpel_dist"):
        assert np.array_equal(o_res[f], r_res[f]), f
    assert not (o_res["subpel_dist"] == 0xffffffff).any()      # every search was taken
    assert np.array_equal(o_nnz, r_nnz)
    assert o_cus.tobytes() == r_cus.tobytes()
    for c in range(3):
        assert np.array_equal(o_rec[c], r_rec[c]), c
    assert o_ssd == r_ssd
    return int(np.count_nonzero(o_nnz))


needs_ref = pytest.mark.skipif(not ol.have_ref(), reason="reference harness not built")


def partition_cases():
    """Every fixture of SMALL at (10, 32) and (8, 27), and - the row-major sub-pel path of
    bd > 10 - (12, 32) on two of them; RDOQ off and on.  The ids are those of the stacked
    parameter lists this replaces."""
    cases = [(n, p, bd, qp, rdoq) for rdoq in (False, True) for bd, qp in [(10, 32), (8, 27)]
             for n, p in SMALL]
    cases += [(n, p, 12, 32, rdoq) for rdoq in (False, True) for n, p in [("tiny", 1), ("c0", 1)]]
    return [pytest.param(*c, id="%s-%d-%d-%d-%s" % c) for c in cases]


@needs_ref
@pytest.mark.parametrize("name,pic,bd,qp,rdoq", partition_cases())
def test_oracle_equals_reference_on_partitions(name, pic, bd, qp, rdoq):
    assert compare_oracle_and_reference(name, pic, bd, qp, rdoq) > 0


@needs_ref
@pytest.mark.parametrize("name,pic", LARGE)
def test_oracle_equals_reference_on_1080p_partitions(name, pic):
    assert compare_oracle_and_reference(name, pic, 10, 32, True) > 0
