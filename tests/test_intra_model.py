"""Intra prediction on its directed case set, decisions counted (CPU).

tests/intra_model.py (the prediction and the LM model in plain integers, a counter on every
decision) on the cases of tests/intra_cases.py:
  - model == oracle (xo), bit exact: every job's block, the 67 SATDs of every luma target;
  - oracle == the reference's own IntraPrediction (where the harness is built) on the same;
  - the oracle's prediction writes nothing outside the jobs' blocks;
  - the census floor: over the cases each device path of tests/test_gpu_intra_cases.py is
    given, every decision class occurs at least FLOOR times - a condition on the inputs, so
    that an edit of the generator cannot quietly drop a class.
"""
import collections
import functools

import numpy as np
import pytest

import intra_cases as ic
import intra_model as im
import oracle_intra as oi
import oracle_lib as ol

PASSES = ic.all_depths()
SENTINEL = 0xa5a5


@pytest.fixture(scope="module")
def xo():
    return ol.Lib("xo")


@pytest.fixture(scope="module")
def libs():
    return ol.Lib("xo"), ol.Lib("xr")


@functools.lru_cache(maxsize=None)
def modelled(bd, reduced):
    """Per sheet, per target: (the reference samples' census, [(block, census) per mode of the
    target], the 67 SATDs of a luma target or None) - computed once."""
    out = []
    for sheet in ic.sheets(bd, reduced):
        res = []
        for t in sheet["targets"]:
            n_refs = collections.Counter()
            refs = im.ref_samples(bd, t["w"], t["h"], t["nb"], t["ar"], t["bl"],
                                  sheet["planes"][t["comp"]], t["x"], t["y"], n_refs)
            per = []
            for m in t["modes"]:
                n = collections.Counter()
                blk = im.predict(bd, t["comp"] == 0, m, t["w"], t["h"], refs, n)
                assert blk.min() >= 0 and blk.max() < 1 << bd
                per.append((blk.astype(np.uint16), n))
            dist = None
            if t["comp"] == 0:
                o = sheet["orig"][t["y"]:t["y"] + t["h"], t["x"]:t["x"] + t["w"]]
                dist = np.array([im.satd(bd, o, b) for b, _ in per], np.uint32)
            res.append((n_refs, per, dist))
        out.append(res)
    return out


@functools.lru_cache(maxsize=None)
def modelled_lm(bd, reduced):
    """Per sheet, per target, per chroma component: (block, census)."""
    return [[[im_lm(sheet, t, comp) for comp in (1, 2)] for t in sheet["targets"]]
            for sheet in ic.lm_sheets(bd, reduced)]


def im_lm(sheet, t, comp):
    n = collections.Counter()
    blk = im.lm_chroma(sheet["bd"], t["x"], t["y"], t["w"], t["h"], sheet["planes"][0],
                       sheet["planes"][comp], n)
    return blk, n


def oracle_rounds(lib, prefix, sheet):
    """Per round of a sheet: (jobs, the three prediction planes over a sentinel)."""
    for r in range(ic.rounds(sheet)):
        jobs = ic.round_jobs(sheet, r)
        pred = [np.full_like(p, SENTINEL) for p in sheet["planes"]]
        for c in range(3):
            oi.pred_jobs(lib, prefix, sheet["bd"], jobs[jobs["comp"] == c], sheet["planes"][c],
                         pred[c], ic.SHEET, ic.SHEET)
        yield jobs, pred


@pytest.mark.parametrize("bd,reduced", PASSES)
def test_model_equals_oracle(xo, bd, reduced):
    """Every job's block, nothing written outside the blocks, the SATD table."""
    jobs_seen = 0
    for sheet, res in zip(ic.sheets(bd, reduced), modelled(bd, reduced)):
        for r, (jobs, got) in enumerate(oracle_rounds(xo, "xo", sheet)):
            exp = [np.full_like(p, SENTINEL) for p in sheet["planes"]]
            for t, (_, per, _) in zip(sheet["targets"], res):
                if r < len(per):
                    exp[t["comp"]][t["y"]:t["y"] + t["h"], t["x"]:t["x"] + t["w"]] = per[r][0]
            for c in range(3):
                if not np.array_equal(got[c], exp[c]):
                    bad = [dict(t, modes=None, mode=t["modes"][r]) for t in sheet["targets"]
                           if t["comp"] == c and r < len(t["modes"]) and not np.array_equal(
                               got[c][t["y"]:t["y"] + t["h"], t["x"]:t["x"] + t["w"]],
                               exp[c][t["y"]:t["y"] + t["h"], t["x"]:t["x"] + t["w"]])]
                    assert not bad, bad[:3]
                    assert False, "the oracle wrote outside the blocks"
            jobs_seen += len(jobs)
        for j, t, (_, _, dist) in zip(ic.luma_jobs(sheet),
                                      [t for t in sheet["targets"] if t["comp"] == 0],
                                      [x for t, x in zip(sheet["targets"], res) if t["comp"] == 0]):
            got = oi.satd_modes(xo, "xo", bd, j, sheet["orig"], sheet["planes"][0])
            assert np.array_equal(got, dist), (t, np.flatnonzero(got != dist))
    assert jobs_seen > 1000


@pytest.mark.parametrize("bd,reduced", PASSES)
def test_model_equals_oracle_lm(xo, bd, reduced):
    for sheet, res in zip(ic.lm_sheets(bd, reduced), modelled_lm(bd, reduced)):
        for t, both in zip(sheet["targets"], res):
            for comp, (blk, _) in zip((1, 2), both):
                got = oi.lm_chroma(xo, "xo", bd, comp, t["x"], t["y"], t["w"], t["h"],
                                   sheet["planes"])
                assert np.array_equal(got, blk), (t, comp)


@pytest.mark.skipif(not ol.have_ref(), reason="reference harness not built")
@pytest.mark.parametrize("bd,reduced", PASSES)
def test_oracle_equals_reference(libs, bd, reduced):
    xo_, xr = libs
    for sheet in ic.sheets(bd, reduced):
        for (jobs, got), (_, exp) in zip(oracle_rounds(xo_, "xo", sheet),
                                         oracle_rounds(xr, "xr", sheet)):
            for c in range(3):
                assert np.array_equal(got[c], exp[c]), (bd, c, jobs[:1])
        for j in ic.luma_jobs(sheet):
            a = (bd, j, sheet["orig"], sheet["planes"][0])
            assert np.array_equal(oi.satd_modes(xo_, "xo", *a), oi.satd_modes(xr, "xr", *a)), j
    for sheet in ic.lm_sheets(bd, reduced):
        for t in sheet["targets"]:
            for comp in (1, 2):
                a = (bd, comp, t["x"], t["y"], t["w"], t["h"], sheet["planes"])
                assert np.array_equal(oi.lm_chroma(xo_, "xo", *a), oi.lm_chroma(xr, "xr", *a)), t


@functools.lru_cache(maxsize=None)
def census(path):
    """What the cases given to a device path reach, all depths together."""
    total = collections.Counter()
    for bd, reduced in PASSES:
        if path == "lm":
            for res in modelled_lm(bd, reduced):
                for both in res:
                    for _, n in both:
                        total.update(n)
            continue
        for sheet, res in zip(ic.sheets(bd, reduced), modelled(bd, reduced)):
            for t, (n_refs, per, _) in zip(sheet["targets"], res):
                if path == "pred" or (path == "wave" and ic.in_wave(t)):
                    for _, n in per:         # a job per mode: the references built each time
                        total.update(n_refs)
                        total.update(n)
                elif (path == "satd" and t["comp"] == 0) or (path == "rows" and ic.in_rows(t)):
                    total.update(n_refs)     # a job per target, 67 modes
                    for _, n in per:
                        total.update(n)
    return total


@pytest.mark.parametrize("path", ic.PATHS)
def test_census_floor(path):
    total = census(path)
    short = [(k, total[k]) for k in ic.path_keys(path) if total[k] < ic.FLOOR]
    assert not short, short
    if path != "lm":     # an exempted key is one the path cannot reach
        reached = [k for k in ic.EXEMPT[path] if total[k]]
        assert not reached, reached
        assert set(total) <= set(ic.PRED_KEYS), set(total) - set(ic.PRED_KEYS)
    else:
        assert set(total) <= set(im.LM_KEYS), set(total) - set(im.LM_KEYS)


def test_every_mode_and_size_is_there():
    """All 67 modes on every luma size, the chroma decision modes on every chroma size, all
    eight neighbour values with every extent, at every full depth."""
    for bd in ic.DEPTHS:
        seen = collections.defaultdict(set)
        for sheet in ic.sheets(bd):
            for t in sheet["targets"]:
                seen[(t["comp"] > 0, t["w"], t["h"])] |= set(t["modes"])
                seen["nb"].add((t["nb"], bool(t["ar"]), t["ar"] == t["h"], bool(t["bl"]),
                                t["bl"] == t["w"]))
                edge_filtered = t["comp"] == 0 and max(t["w"], t["h"]) <= 16
                seen[("content", edge_filtered)].add(t["content"])
        for w in ic.LUMA_SIZES:
            for h in ic.LUMA_SIZES:
                assert seen[(False, w, h)] == set(range(67))
        for w in ic.CHROMA_SIZES:
            for h in ic.CHROMA_SIZES:
                assert seen[(True, w, h)] == set(ic.CHROMA_MODES)
        assert {k[0] for k in seen["nb"]} == set(range(8)) and len(seen["nb"]) == 2 + 6 + 6 + 18
        assert seen[("content", True)] == {"steps", "sat_high", "sat_low", "full"}


def test_lm_targets_are_there():
    """Every chroma size, every kind in both components, the four picture-edge positions,
    neighbour counts from 2 to 64 and both 16:1 shapes inside the picture, at every depth."""
    for bd in ic.DEPTHS:
        sizes, kinds, edges, counts = set(), [set(), set()], set(), set()
        for sheet in ic.lm_sheets(bd):
            for t in sheet["targets"]:
                w, h, above, left = t["w"], t["h"], t["y"] > 0, t["x"] > 0
                sizes.add((w, h))
                edges.add((above, left))
                for c in range(2):
                    kinds[c].add(t["kinds"][c])
                both = above and left
                counts.add((w // max(w // h, 1) if both else w) * above +
                           (h // max(h // w, 1) if both else h) * left)
                if both and max(w, h) == 16 * min(w, h):
                    sizes.add(("inside", w, h))
        assert sizes >= {(w, h) for w in ic.CHROMA_SIZES for h in ic.CHROMA_SIZES} | \
            {("inside", 32, 2), ("inside", 2, 32)}
        assert kinds[0] == kinds[1] == set(ic.LM_KINDS) and len(edges) == 4
        assert counts >= {2, 4, 8, 16, 32, 64}


def census_table():
    """The table of intra_model's docstring."""
    lines = ["  %-24s" % "key" + "".join("%14s" % ic.PATH_TITLES[p] for p in ic.PATHS)]
    for k in ic.PRED_KEYS + im.LM_KEYS:
        cells = ""
        for p in ic.PATHS:
            mine = (k in im.LM_KEYS) == (p == "lm")
            cells += "%14s" % ("" if not mine else "-" if k in ic.EXEMPT.get(p, ()) else
                               str(census(p)[k]))
        lines.append(("  %-24s" % k + cells).rstrip())
    return "\n".join(lines)


def test_census_table_is_documented():
    """intra_model's docstring shows what the case set pins."""
    assert census_table() in im.__doc__


if __name__ == "__main__":
    print(census_table())
