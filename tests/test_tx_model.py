"""The transform stages on their directed case set, decisions counted (CPU).

tests/tx_model.py (the four stages, the 4x4 DST, transform skip, InvDct2Dc, the dequantiser,
AddClip and the residual-domain SSD in numpy, a counter on every decision) on the cases of
tests/tx_cases.py:
  - model == oracle (xo), bit exact, on every case: coefficients, residual, reconstruction, levels
    and count (xo_residual_pipeline for the cases that enter at the residual; xo_dequant +
    xo_inv_transform / xo_inv_transform_skip for the crafted levels);
  - oracle == the reference's own transforms (where the harness is built) on the same inputs, the
    restricted forms standing in for XVC_TX_DCT2_LOW where the reference can express the pair;
  - the census: every decision class occurs on every device path (tx_model.device_path) that can
    reach it; a class a path cannot reach is a named entry of tx_model.EXCLUDED and never occurs.
`python tests/test_tx_model.py` prints the census table of DESIGN.md.
"""
import collections
import functools

import numpy as np
import pytest

import oracle_lib as ol
import tx_cases as tc
import tx_model as tm

ALL_DEPTHS = tc.ALL_DEPTHS
modelled, describe = tc.modelled, tc.describe
GRID_N = 50     # any n <= 16384 names the same paths (tx_model.device_path); the grids hold 50


@pytest.fixture(scope="module")
def xo():
    return ol.Lib("xo")


def tx_struct(b, x=0, y=0):
    s = ol.TxBlock()
    s.x, s.y = x, y
    for k, v in b.items():
        setattr(s, k, int(v))
    return s


@pytest.mark.parametrize("bd", ALL_DEPTHS)
def test_model_equals_oracle(xo, bd):
    for cs, m in zip(tc.cases(bd), modelled(bd)):
        b = cs["blk"]
        skip = b["tx_hor"] == tm.TX_SKIP
        assert set(m["fwd"]) | set(m["inv"]) | set(m["dist_n"]) <= set(tm.KEYS)
        if cs["levels"] is None:
            resi = np.ascontiguousarray((cs["orig"].astype(np.int32) - cs["pred"]).astype(np.int16))
            want = xo.fwd_transform_skip(bd, resi) if skip else \
                xo.fwd_transform(bd, resi, b["tx_hor"], b["tx_ver"], b["dst4x4"])
            assert np.array_equal(m["coeff"], want), describe(cs, m)
            rec, lv, nnz = xo.residual_pipeline(bd, tx_struct(b), np.ascontiguousarray(cs["orig"]),
                                                np.ascontiguousarray(cs["pred"]))
            assert nnz == m["nnz"] and (not nnz or np.array_equal(lv, m["levels"])), describe(cs, m)
            assert np.array_equal(rec, m["rec"]), describe(cs, m)
        elif m["nnz"]:
            lv = np.ascontiguousarray(cs["levels"])
            deq = xo.dequant(bd, b["qp"], lv)
            dc_only = int(m["nnz"] == 1 and lv[0, 0] != 0)
            want = xo.inv_transform_skip(bd, deq) if skip else \
                xo.inv_transform(bd, deq, b["tx_hor"], b["tx_ver"], b["dst4x4"], dc_only)
            assert np.array_equal(m["resi"], want), describe(cs, m)
            rec = np.clip(cs["pred"].astype(np.int64) + want, 0, (1 << bd) - 1)
            assert np.array_equal(rec, m["rec"]), describe(cs, m)
        else:
            assert np.array_equal(m["rec"], cs["pred"])


def reference_types(b):
    """(tx_hor, tx_ver, restricted) as the reference takes the block, or None where it cannot:
    under Restrictions::disable_ext2_transform_high_precision EVERY DCT-2 of a side 4 .. 32 is the
    6-bit one, so a pair that mixes XVC_TX_DCT2_LOW with a high-precision DCT-2 of such a side
    is the binding's alone."""
    th, tv = b["tx_hor"], b["tx_ver"]
    if tm.TX_LOW not in (th, tv):
        return th, tv, False
    low = lambda t, size: tm.TX_LOW if t in (0, 1) and 4 <= size <= 32 else t
    rh, rv = (1 if th == tm.TX_LOW else th), (1 if tv == tm.TX_LOW else tv)
    if (low(rh, b["w"]), low(rv, b["h"])) != (th, tv):
        return None
    return rh, rv, True


@pytest.mark.skipif(not ol.have_ref(), reason="reference harness not built")
@pytest.mark.parametrize("bd", ALL_DEPTHS)
def test_oracle_equals_reference(xo, bd):
    """The reference on the inputs of every case it can express; what it is compared with is the
    oracle's answer, which test_model_equals_oracle ties to the model's."""
    xr = ol.Lib("xr")
    done = skipped = 0
    for cs, m in zip(tc.cases(bd), modelled(bd)):
        b = cs["blk"]
        skip = b["tx_hor"] == tm.TX_SKIP
        rt = (0, 0, False) if skip else reference_types(b)
        if rt is None:
            skipped += 1
            continue
        th, tv, restricted = rt
        fwd = xr.fwd_transform_restricted if restricted else xr.fwd_transform
        inv = xr.inv_transform_restricted if restricted else xr.inv_transform
        if cs["levels"] is None:
            resi = np.ascontiguousarray((cs["orig"].astype(np.int32) - cs["pred"]).astype(np.int16))
            got = xr.fwd_transform_skip(bd, resi) if skip else fwd(bd, resi, th, tv, b["dst4x4"])
            want = xo.fwd_transform_skip(bd, resi) if skip else \
                xo.fwd_transform(bd, resi, b["tx_hor"], b["tx_ver"], b["dst4x4"])
            assert np.array_equal(got, want), describe(cs)
        if m["nnz"]:
            lv = np.ascontiguousarray(np.asarray(m["levels"], np.int16).reshape(b["h"], b["w"]))
            deq = xr.dequant(bd, b["qp"], lv)
            assert np.array_equal(deq, xo.dequant(bd, b["qp"], lv)), describe(cs)
            dc_only = int(m["nnz"] == 1 and lv[0, 0] != 0)
            got = xr.inv_transform_skip(bd, deq) if skip else \
                inv(bd, deq, th, tv, b["dst4x4"], dc_only)
            assert np.array_equal(got, m["resi"]), describe(cs, m)
        done += 1
    assert done > 5 * skipped, (done, skipped)     # (the mixed pairs are an eighth of the cases)
    outside = [cs for cs in tc.cases(bd) if cs["kind"] == "outside"]
    assert len(outside) >= 3 and all(reference_types(cs["blk"]) for cs in outside)


# ---- the census ---------------------------------------------------------------------------------

def grid_runs(cs):
    """(entry, one_launch, in place) of every run tests/test_gpu_tx_cases.py gives a grid case."""
    runs = [("inv", True, False), ("inv", False, False), ("inv_dist", True, False)]
    if cs["levels"] is None:
        runs += [("residual", True, False), ("fwd", True, False)]
    if cs["family"] == 5:
        runs += [("inv", True, True), ("inv", False, True), ("inv_dist", True, True)]
    return runs


def add_run(total, path, m, entry, in_place, times=1):
    parts = {"residual": ("fwd", "inv"), "fwd": ("fwd",), "inv": ("inv",),
             "inv_dist": ("inv", "dist_n")}[entry]
    for part in parts:
        for k, v in m[part].items():
            if in_place and k == "nnz0_copied":
                k = "nnz0_in_place"
            total[path][k] += v * times


@functools.lru_cache(maxsize=None)
def census():
    """device path -> Counter over every run of every case, all depths, the launch batches of
    family 6 included (their tiles are cases of the launch depth, counted once per descriptor)."""
    total = collections.defaultdict(collections.Counter)
    for bd in ALL_DEPTHS:
        for cs, m in zip(tc.cases(bd), modelled(bd)):
            for entry, one_launch, in_place in grid_runs(cs):
                add_run(total, tm.device_path(cs["blk"], entry, GRID_N, one_launch), m, entry,
                        in_place)
    models = modelled(tc.LAUNCH_BD)
    for run in tc.LAUNCHES:
        if run["entry"] == "rdoq":      # the dispatch alone is under test there
            continue
        batch = tc.launch_batch(run["mode"], run["n"], run["per_row"])
        count = np.bincount(batch["tile"], minlength=len(batch["tiles"]))
        for t, cs in enumerate(batch["tiles"]):
            m = models[cs["i"]] if cs["kind"] != "flat" else flat_model(cs)
            add_run(total, tm.device_path(cs["blk"], run["entry"], run["n"]), m, run["entry"],
                    run["in_place"], int(count[t]))
    return total


def flat_model(cs):
    """A tile whose original is its prediction: zero residual, nothing coded."""
    n_fwd, n_inv, n_dist = (collections.Counter() for _ in range(3))
    coeff = tm.forward(cs["bd"], cs["blk"], np.zeros(cs["pred"].shape, np.int64), n_fwd)
    assert not coeff.any()
    tm.reconstruct(cs["bd"], cs["blk"], cs["pred"], None, 0, n_inv)
    tm.ssd(cs["bd"], cs["blk"], cs["orig"], cs["pred"], np.zeros(cs["pred"].shape, np.int64), n_dist)
    return dict(fwd=n_fwd, inv=n_inv, dist_n=n_dist)


@pytest.mark.parametrize("path", tm.PATHS)
def test_census(path):
    total = census()
    ex = dict(tm.EXCLUDED["*"], **tm.EXCLUDED[path])
    assert all(reason for reason in ex.values()), "an exclusion states its reason"
    short = [k for k in tm.KEYS if k not in ex and not total[path][k]]
    assert not short, (path, "classes the cases do not reach", short)
    stale = [k for k in ex if total[path][k]]
    assert not stale, (path, "excluded classes that do occur", stale)


def test_paths_are_the_ones_named():
    assert set(census()) == set(tm.PATHS)
    assert set(tm.EXCLUDED) == set(tm.PATHS) | {"*"}


def test_device_path_thresholds():
    small, big = tc.blk(16, 16, 0), tc.blk(32, 32, 0)
    dst, two = tc.blk(4, 4, 0, dst4x4=1), tc.blk(2, 8, 1)
    assert not any(tm.tx_small_job(b) for b in (big, dst, two, tc.blk(4, 4, 0, tm.TX_SKIP)))
    assert all(tm.tx_small_job(tc.blk(w, h, 0)) for w in (4, 8, 16) for h in (4, 8, 16))
    p = tm.device_path
    assert p(small, "inv", 16384) == "tx2_job/residual_cu_kernel"
    assert p(small, "inv", 16385) == p(small, "inv", 5, False) == "tx2_job/residual_wave_kernel"
    assert p(big, "inv", 16384) == "residual_job/residual_cu_kernel"
    assert p(big, "inv", 16385) == p(big, "inv_dist", 1) == "residual_job/residual_per_job_kernel"
    assert p(big, "inv", 65536) == "residual_job/residual_per_job_kernel"
    for entry in ("inv", "inv_dist", "fwd", "residual"):
        assert p(big, entry, 65537) == "residual_job/residual_kernel"
        assert p(small, entry, 65537) == "tx2_job/residual_wave_kernel"
    assert p(big, "rdoq", 64) == "residual_job/residual_cu_kernel"
    assert p(big, "rdoq", 65) == p(big, "rdoq", 262144) == "residual_job/residual_per_job_kernel"
    assert p(big, "rdoq", 262145) == "residual_job/residual_kernel"


def test_every_valid_descriptor_is_there():
    """Family 1 holds every valid pair at every shape, and nothing the binding never passes."""
    for bd in tc.DEPTHS:
        seen = {(c["blk"]["w"], c["blk"]["h"], c["blk"]["comp"], c["blk"]["tx_hor"], c["blk"]["tx_ver"])
                for c in tc.cases(bd) if c["family"] == 1 and c["kind"] == "types"}
        for comp, pairs in ((0, tc.LUMA_PAIRS), (1, tc.CHROMA_PAIRS)):
            for w, h, _ in tc.shapes(comp):
                want = {(w, h, comp) + p for p in pairs if tc.pair_for(p, w, h, comp)}
                assert want <= seen, want - seen
                assert len(want) == len([p for p in pairs if tm.valid_type(p[0], w) and
                                         tm.valid_type(p[1], h)])
    for bd in ALL_DEPTHS:
        assert all(tm.valid_block(c["blk"]) for c in tc.cases(bd))
        assert {c["family"] for c in tc.cases(bd)} == {1, 2, 3, 4, 5}
    assert not tm.valid_type(tm.TX_LOW, 64) and not tm.valid_type(tm.TX_LOW, 2)
    assert not tm.valid_type(5, 2) and tm.valid_type(1, 2)
    assert set(tc.EXCLUSIONS) == {"low_precision_side_2_or_64", "side_2_beyond_dct2",
                                  "dst4x4_elsewhere", "skip_above_4x4"}


def test_families_do_what_they_say():
    """Family 2 drives each forward stage to its bound; family 3 holds blocks in which both inverse
    stages clip both ways, blocks in which only stage 2 clips and blocks in which nothing clips,
    on both stage codes; its dequantised coefficients are 32767 / -32768; AddClip saturates both
    ways and not at all; at 12 bits the distortion needs more than 32 bits even on a 4x4 block;
    family 4's single levels sit where they should."""
    for bd in tc.DEPTHS:
        top = ((1 << bd) - 1) << (15 - bd)
        seen = collections.Counter()
        for cs, m in zip(tc.cases(bd), modelled(bd)):
            small = tm.tx_small_job(cs["blk"])
            n = m["inv"]
            clip1 = n["inv1_clip_high"] + n["inv1_clip_low"]
            clip2 = n["inv2_clip_high"] + n["inv2_clip_low"]
            if cs["family"] == 2 and cs["kind"] == "dc" and cs["blk"]["tx_hor"] in (0, 1, 7) and \
                    cs["blk"]["tx_ver"] in (0, 1, 7) and not cs["blk"]["dst4x4"]:
                assert int(m["coeff"][0, 0]) == top, describe(cs, m)
                seen["fwd_bound"] += 1
            if cs["family"] == 3 and cs["kind"].startswith("both") and n["form_matrix"]:
                deq = tm.dequant(bd, cs["blk"]["qp"], cs["blk"]["w"], cs["blk"]["h"], cs["levels"],
                                 collections.Counter())
                assert set(np.unique(deq)) <= {-32768, 0, 32767}
                assert n["inv1_clip_high"] and n["inv1_clip_low"], describe(cs, m)
                seen[("both2", small)] += bool(n["inv2_clip_high"] and n["inv2_clip_low"])
                seen[("sat", small)] += bool(n["add_at_0"] and n["add_at_max"])
            if cs["family"] == 3 and cs["kind"].startswith("stage2"):
                assert not clip1 and not n["deq_clip_high"] + n["deq_clip_low"], describe(cs, m)
                seen[("only2", small)] += bool(clip2)
            if cs["family"] == 3 and cs["kind"].startswith("none"):
                assert not clip1 and not clip2 and not n["dst1_clip_high"] + n["dst1_clip_low"]
                seen[("none", small)] += 1
            if cs["family"] == 3 and cs["kind"] == "small_pmid":
                seen[("unsat", small)] += bool(n["add_inside"] and not n["add_at_0"] + n["add_at_max"])
            if cs["family"] == 3 and (cs["blk"]["w"], cs["blk"]["h"]) == (4, 4):
                seen["dist_4x4"] += m["dist_n"]["dist_ge_2p32"]
            if cs["family"] == 4 and cs["kind"] == "outside":
                assert m["nnz"] == 1 and not m["resi"].any() and np.array_equal(m["rec"], cs["pred"])
                seen["outside"] += 1
        assert seen["fwd_bound"] and seen["outside"] >= 3, seen
        for small in (True, False):
            assert seen[("sat", small)] and seen[("none", small)] and seen[("unsat", small)], (bd, seen)
            if bd == 12:    # (stage 2 shifts by 22 - depth: at 8 bits no column sum gets there)
                assert seen[("both2", small)] and seen[("only2", small)] and seen["dist_4x4"], seen


def test_forward_stays_inside_int16(xo):
    """The bound behind the fwd*_wrap exclusion, evaluated on the oracle's matrices."""
    for t in tc.LUMA_TYPES:
        for size in (2, 4, 8, 16, 32, 64):
            if tm.valid_type(t, size):
                m = np.abs(tm.matrix(t, size))
                assert m[:min(size, 32)].sum(axis=1).max() <= (64 if t == tm.TX_LOW else 256) * size
    assert np.abs(tm.DST4).sum(axis=1).max() == 242
    for bd in ALL_DEPTHS:
        assert ((1 << bd) - 1) << (15 - bd) < 32768


@pytest.mark.parametrize("bd", [8, 10, 12])
@pytest.mark.parametrize("kind", ["16", "8", "mixed"])
def test_frame_pass_inputs_are_what_they_say(xo, kind, bd):
    """CPU only: the oracle alone on the pictures tests/test_gpu_tx_cases.py gives the frame pass,
    at the two ends of the QP range the pass clamps its tables to."""
    import test_gpu_fwd_inv_paths as fip
    from xvc_amd import pipeline
    parts, partition = tc.partitions(kind)
    for qp in tc.FRAME_QPS:
        orig, ref = tc.swing_pictures(bd, parts, weak_v=True)
        desc = pipeline.FrameDescriptors(tc.FW, tc.FH, qp, rdoq=True, bitdepth=bd,
                                         partition=partition)
        nnz = fip.oracle_encode(xo, desc, bd, fip.pad_planes(orig), fip.pad_planes(ref),
                                [(0, 0)] * desc.n_cus)[1]
        tc.check_frame_pass_counts(qp, nnz)


def census_table():
    total = census()
    lines = ["| class | " + " | ".join("`%s`" % p for p in tm.PATHS) + " |",
             "|---|" + "---:|" * len(tm.PATHS)]
    for k in tm.KEYS:
        cells = ["-" if k in dict(tm.EXCLUDED["*"], **tm.EXCLUDED[p]) else str(total[p][k])
                 for p in tm.PATHS]
        lines.append("| %s | " % k + " | ".join(cells) + " |")
    return "\n".join(lines)


if __name__ == "__main__":
    print(census_table())
    for path, d in tm.EXCLUDED.items():
        for k, why in d.items():
            print("- `%s`: `%s` - %s" % (path, k, why))
    for bd in ALL_DEPTHS:
        print(bd, "cases", len(tc.cases(bd)),
              dict(collections.Counter(c["family"] for c in tc.cases(bd))))
