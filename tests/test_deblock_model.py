"""The deblocking filter over its whole QP / offset range, decisions counted (CPU).

tests/deblock_model.py (DeblockPicture in Python integers, a counter on every decision) on
the cases of tests/deblock_cases.py:
  - model == oracle (xo_deblock_picture), bit exact, sub-block sizes 4 and 8;
  - oracle == the reference's own DeblockingFilter (where the harness is built) on every
    case that stays inside the reference's tables, sub-block sizes 4 and 8;
  - the census floor: every decision class occurs at least FLOOR times per pass, per family
    of partitions, over all cases and over the cases compared with the reference - a
    condition on the inputs, so that an edit of the generator cannot quietly drop a class.
"""
import collections
import functools

import numpy as np
import pytest

import deblock_cases as dc
import deblock_model as dm
import oracle_lib as ol

FLOOR = 8
NO_BORDER = [0, 0, 0]


@pytest.fixture(scope="module")
def xo():
    return ol.Lib("xo")


@functools.lru_cache(maxsize=None)
def modelled(family, sub):
    """[(filtered planes, census)] of the family's cases, computed once."""
    return [dm.deblock_picture(c["bd"], c["pw"], c["ph"], c["bipred"], c["beta"], c["tc"], sub,
                               c["cus"], c["cu_map"], c["planes"]) for c in dc.cases(family)]


def in_reference_tables(census):
    """The reference reads past kBetaTable at index 64 and past kTcTable at index 54: it
    defines nothing for a picture that gets there."""
    return not any(census[p + k] for p in ("v.", "h.") for k in dm.UNDEFINED_IN_REFERENCE)


def oracle_planes(lib, c, sub):
    planes = [p.copy() for p in c["planes"]]
    lib.deblock(c["bd"], c["pw"], c["ph"], c["bipred"], c["beta"], c["tc"], sub, c["cus"],
                c["cu_map"], planes, NO_BORDER, c["l0"], c["l1"])
    return planes


@pytest.mark.parametrize("family,sub", [("g4", 4), ("g8", 4), ("g8", 8)])
def test_model_equals_oracle(xo, family, sub):
    changed = 0
    for c, (exp, _) in zip(dc.cases(family), modelled(family, sub)):
        got = oracle_planes(xo, c, sub)
        for k in range(3):
            assert np.array_equal(got[k], exp[k]), (c["name"], sub, k)
            changed += int((got[k] != c["planes"][k]).sum())
    assert changed > 0


@pytest.mark.skipif(not ol.have_ref(), reason="reference harness not built")
@pytest.mark.parametrize("family,sub", [("g4", 4), ("g8", 4), ("g8", 8)])
def test_oracle_equals_reference(xo, family, sub):
    xr = ol.Lib("xr")
    cases = dc.cases(family)
    compared = 0
    for c, (_, census) in zip(cases, modelled(family, sub)):
        if not in_reference_tables(census):
            assert c["recipe"] not in ("last", "band", "zero"), c["name"]
            continue
        compared += 1
        got, exp = oracle_planes(xo, c, sub), oracle_planes(xr, c, sub)
        for k in range(3):
            assert np.array_equal(got[k], exp[k]), (c["name"], sub, k)
    assert 2 * compared >= len(cases)      # at most half of the cases may be left out


def totals(family, compared_only):
    total = collections.Counter()
    for _, census in modelled(family, 4):
        if not compared_only or in_reference_tables(census):
            total.update(census)
    return total


@pytest.mark.parametrize("family", dc.FAMILIES)
def test_census_floor(family):
    """Sub-block size 4: the two-pass kernels' on "g4", the fused tail's on "g8"."""
    everything, compared = totals(family, False), totals(family, True)
    short = [(k, everything[k]) for k in dm.census_keys() if everything[k] < FLOOR]
    assert not short, short
    short = [(k, compared[k]) for k in dm.census_keys()
             if compared[k] < FLOOR and k[2:] not in dm.UNDEFINED_IN_REFERENCE]
    assert not short, short
    assert not any(compared[p + k] for p in ("v.", "h.") for k in dm.UNDEFINED_IN_REFERENCE)
    assert set(everything) <= set(dm.census_keys())


@pytest.mark.parametrize("family", dc.FAMILIES)
def test_last_table_entries_are_compared(family):
    """The clip at tc index 53 and the last indices inside the reference's tables (qp +
    beta_off == 63, cqp + tc_off + 2 == 53) are defined there: those cases are compared."""
    n = 0
    for c, (_, census) in zip(dc.cases(family), modelled(family, 4)):
        if c["recipe"] != "last":
            continue
        n += 1
        assert in_reference_tables(census)
        cus = c["cus"]
        assert (cus["qp_y"] + c["beta"] == 63).all() and (cus["qp_c"] + c["tc"] + 2 == 53).all()
        for p in ("v.", "h."):
            assert census[p + "clip.tc_over"] >= FLOOR and census[p + "chroma.filtered"] >= FLOOR
            assert census[p + "luma.bs1.off"] + census[p + "luma.bs2.off"] < \
                sum(census[p + k] for k in dm.LUMA_KEYS)      # beta 88 lets groups through
    assert n >= 6


def census_table():
    """The table of deblock_model's docstring."""
    fams = [(f, totals(f, False), totals(f, True)) for f in dc.FAMILIES]
    lines = ["  %-24s" % "key" + "".join("%16s%16s" % (f + " all v/h", f + " cmp v/h")
                                         for f, _, _ in fams)]
    keys = dm.BS_KEYS + sorted(set(dm.CORNER_KEYS["v"] + dm.CORNER_KEYS["h"])) + dm.LUMA_KEYS + \
        dm.LINE_KEYS + dm.CHROMA_KEYS + dm.CLIP_KEYS
    for k in keys:
        def cell(t):
            return "%16s" % "/".join(str(t["%s.%s" % (p, k)]) if "%s.%s" % (p, k) in
                                     dm.census_keys() else "-" for p in "vh")
        lines.append("  %-24s" % k + "".join(cell(a) + cell(b) for _, a, b in fams))
    return "\n".join(lines)


def test_census_table_is_documented():
    """deblock_model's docstring shows what the case set pins."""
    assert census_table() in dm.__doc__


if __name__ == "__main__":
    print(census_table())
