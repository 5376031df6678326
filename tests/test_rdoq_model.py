"""The RDO quantiser on its directed case set, decisions counted (CPU).

tests/rdoq_model.py (RdoQuant::QuantRdo with CoeffSignHideRdo in plain integers, a counter on
every decision) on the cases of tests/rdoq_cases.py:
  - model == oracle (xo), bit exact: levels and count of every case, and of every block of
    the residual entry's pictures (there on the oracle's own forward coefficients, against
    xo_residual_pipeline_rdoq);
  - oracle == the reference's own QuantRdo (where the harness is built) on every case the
    reference can express, and the host-side constants the cases carry are the reference's;
  - the census: on both entry points every decision class occurs on every walk instance
    (rdoq_model.device_walk) that can reach it; a class a walk cannot reach is a named entry of
    rdoq_model.EXCLUDED / RESIDUAL_EXCLUDED and never occurs there.
`python tests/test_rdoq_model.py` prints the census tables of DESIGN.md.
"""
import collections
import ctypes as C
import functools

import numpy as np
import pytest

import oracle_lib as ol
import oracle_rdoq as oq
import rdoq_cases as rc
import rdoq_model as rm

PACKED_WALKS = ["packed4/wave_rdoq4<16,1>", "packed4/wave_rdoq4<64,1>", "packed4/wave_rdoq<16>",
                "packed/wave_rdoq4<64,4>", "packed/wave_rdoq<64>/scan", "packed/wave_rdoq<64>/2x2"]
RESIDUAL_WALKS = ["wave/wave_rdoq4<64,1>", "wave/wave_rdoq<64>/scan", "workgroup/wave_rdoq4<64,1>",
                  "workgroup/wave_rdoq4<64,4>", "workgroup/wave_rdoq<64>/2x2"]


@pytest.fixture(scope="module")
def xo():
    return ol.Lib("xo")


@functools.lru_cache(maxsize=None)
def entropy():
    f = ol.Lib("xo").dll.xo_entropy_bits_table
    f.restype = C.POINTER(C.c_uint32)
    return [int(f()[i]) for i in range(128)]


def ctx_dict(rec):
    return {k: rec[k].tolist() for k in oq.RDOQ_CTX_DTYPE.names}


def case_params(cs):
    prm = np.zeros(1, oq.RDOQ_PARAMS_DTYPE)
    prm["lambda"], prm["rd_factor"], prm["flags"] = cs["lam_fix"], cs["rd_factor"], cs["flags"]
    return prm


@functools.lru_cache(maxsize=None)
def modelled(bd):
    """Per case: (nnz, levels as an array - zeros where nnz == 0 -, census), or None for the
    2-wide blocks of NO_2X2 (QuantFast)."""
    snaps = rc.snapshots(bd)
    out = []
    for cs in rc.cases(bd):
        n = collections.Counter()
        r = rm.quant_rdo(entropy(), bd, cs["qp"], cs["luma"], cs["scan"], cs["sign_hide"],
                         cs["flags"], cs["w"], cs["h"], cs["src"].tolist(),
                         ctx_dict(snaps[cs["ctx"]]), cs["lam_fix"], cs["rd_factor"], n)
        out.append(None if r is None else (r[0], np.array(r[1], np.int16), n))
    return out


@functools.lru_cache(maxsize=None)
def oracle_results(bd):
    """Per case: (nnz, levels; zeros where nnz == 0: the reference leaves them unspecified)."""
    xo_, snaps = ol.Lib("xo"), rc.snapshots(bd)
    out = []
    for cs in rc.cases(bd):
        nnz, lv = oq.quant_rdo_oracle(xo_, bd, cs["qp"], cs["comp"], cs["scan"], cs["sign_hide"],
                                      snaps[cs["ctx"]:cs["ctx"] + 1], case_params(cs), cs["src"])
        out.append((nnz, lv if nnz else np.zeros_like(lv)))
    return out


def describe(cs, n):
    """A failing case by its construction and the decision classes it went through."""
    return dict(depth=cs["bd"], case=cs["i"], kind=cs["kind"], v=cs["v"], shape=(cs["w"], cs["h"]),
                scan=cs["scan"], qp=cs["qp"], classes=sorted(k for k in n if n[k]))


@pytest.mark.parametrize("bd", rc.DEPTHS)
def test_model_equals_oracle(bd):
    done = 0
    for cs, m, (e_nnz, e_lv) in zip(rc.cases(bd), modelled(bd), oracle_results(bd)):
        if m is None:
            assert min(cs["w"], cs["h"]) == 2 and cs["flags"] & rm.NO_2X2
            continue
        nnz, lv, n = m
        assert nnz == e_nnz and np.array_equal(lv, e_lv), describe(cs, n)
        assert set(n) <= set(rm.KEYS), set(n) - set(rm.KEYS)
        done += 1
    assert done > 4000


def reference_expresses(cs):
    """DetermineScanOrder gives a non-diagonal scan to an intra CU below 16x16 only."""
    s = 1 if cs["comp"] else 0
    return cs["scan"] == 0 or (cs["flags"] & rm.INTRA_CU and (cs["w"] << s) < 16 and
                               (cs["h"] << s) < 16)


@pytest.mark.skipif(not ol.have_ref(), reason="reference harness not built")
@pytest.mark.parametrize("bd", rc.DEPTHS)
def test_oracle_equals_reference(bd):
    """Every case the reference can express: its levels and count, and the component QP, lambda
    and rd_factor it derives from the case's (luma QP, lambda) are the case's own."""
    xr, snaps = ol.Lib("xr"), rc.snapshots(bd)
    done = 0
    for cs, (e_nnz, e_lv) in zip(rc.cases(bd), oracle_results(bd)):
        if not reference_expresses(cs):
            continue
        r_nnz, r_lv, prm, cqp = oq.quant_rdo_reference(
            xr, bd, cs["qp_luma"], cs["lam"], cs["comp"], cs["scan"], cs["sign_hide"],
            snaps[cs["ctx"]:cs["ctx"] + 1], cs["flags"], cs["src"])
        assert (cqp, int(prm["lambda"][0]), int(prm["rd_factor"][0])) == \
            (cs["qp"], cs["lam_fix"], cs["rd_factor"]), describe(cs, {})
        assert r_nnz == e_nnz and (not e_nnz or np.array_equal(r_lv, e_lv)), describe(cs, {})
        done += 1
    assert done > 3000      # (of about 4900: the rest are scans the reference never gives)


@functools.lru_cache(maxsize=None)
def packed_census():
    """walk instance -> Counter over the cases xvcgpu_quant_rdo_batch gives it, all depths.
    The long class-1 list (tests/test_gpu_rdoq_cases.py) repeats the class-1 cases."""
    total = collections.defaultdict(collections.Counter)
    for bd in rc.DEPTHS:
        for cs, m in zip(rc.cases(bd), modelled(bd)):
            walk = rm.device_walk("packed", cs["w"], cs["h"], cs["scan"], cs["flags"])
            assert (walk is None) == (m is None)
            if m is not None:
                total[walk].update(m[2])
                if walk == "packed4/wave_rdoq4<64,1>":
                    total[rm.device_walk("packed", cs["w"], cs["h"], cs["scan"], cs["flags"],
                                         long_list=True)].update(m[2])
    return total


@functools.lru_cache(maxsize=None)
def residual_modelled(bd):
    """Per block of the depth's picture: (walk, nnz, levels, census) from the model on the
    oracle's forward coefficients; a QuantFast block: (walk, None, None, None)."""
    xo_ = ol.Lib("xo")
    orig, pred, blocks, params, snaps = rc.residual_picture(bd)
    out = []
    for b, prm in zip(blocks, params):
        w, h, comp = int(b["w"]), int(b["h"]), int(b["comp"])
        x, y = int(b["x"]), int(b["y"])
        scan = (int(b["intra_pic"]) >> 2) & 3
        walk = rm.device_walk("residual", w, h, scan, int(prm["flags"]))
        if walk == "QuantFast":
            out.append((walk, None, None, None))
            continue
        resi = (orig[comp][y:y + h, x:x + w].astype(np.int32) -
                pred[comp][y:y + h, x:x + w]).astype(np.int16)
        coeff = xo_.fwd_transform(bd, np.ascontiguousarray(resi))
        n = collections.Counter()
        nnz, lv = rm.quant_rdo(entropy(), bd, int(b["qp"]), comp == 0, scan,
                               0 if int(b["intra_pic"]) & 2 else 1, int(prm["flags"]), w, h,
                               coeff.tolist(), ctx_dict(snaps[int(prm["ctx_index"])]),
                               int(prm["lambda"]), int(prm["rd_factor"]), n)
        out.append((walk, nnz, np.array(lv, np.int16), n))
    return out


@functools.lru_cache(maxsize=None)
def residual_oracle(bd):
    """The oracle's TransformAndReconstruct of the depth's picture: ([Y, U, V] reconstruction,
    [(nnz, levels w * h)] per block)."""
    xo_ = ol.Lib("xo")
    orig, pred, blocks, params, snaps = rc.residual_picture(bd)
    f = xo_.dll.xo_residual_pipeline_rdoq
    f.restype = C.c_int
    vp = C.c_void_p
    rec = [np.zeros_like(p) for p in orig]
    coeff = np.zeros(64 * 64, np.int16)
    out = []
    for i, b in enumerate(blocks):
        c = int(b["comp"])
        st = orig[c].shape[1]
        nnz = f(bd, vp(blocks[i:i + 1].ctypes.data), vp(snaps.ctypes.data),
                vp(params[i:i + 1].ctypes.data), vp(orig[c].ctypes.data), C.c_ssize_t(st),
                vp(pred[c].ctypes.data), C.c_ssize_t(st), vp(rec[c].ctypes.data), C.c_ssize_t(st),
                vp(coeff.ctypes.data))
        n_el = int(b["w"]) * int(b["h"])
        out.append((nnz, coeff[:n_el].copy() if nnz else np.zeros(n_el, np.int16)))
    return rec, out


@pytest.mark.parametrize("bd", rc.DEPTHS)
def test_model_equals_oracle_residual(bd):
    """The model on the oracle's forward coefficients == the oracle's whole pipeline, block by
    block: the census of the residual entry is counted on what that entry quantises."""
    _, recs = residual_oracle(bd)
    blocks = rc.residual_picture(bd)[2]
    coded = 0
    for b, (walk, nnz, lv, n), (e_nnz, e_lv) in zip(blocks, residual_modelled(bd), recs):
        if walk == "QuantFast":
            continue
        assert nnz == e_nnz and np.array_equal((lv if nnz else 0 * lv).reshape(-1), e_lv), \
            (tuple(b), walk, sorted(k for k in n if n[k]))
        coded += nnz > 0
    assert coded > len(blocks) // 2


@functools.lru_cache(maxsize=None)
def residual_census():
    total = collections.defaultdict(collections.Counter)
    for bd in rc.DEPTHS:
        for walk, _, _, n in residual_modelled(bd):
            if n is not None:
                total[walk].update(n)
            else:
                total[walk]["blocks"] += 1
    return total


def check_census(total, walk, excluded):
    ex = dict(rm.EXCLUDED["*"], **excluded[walk])
    assert all(reason for reason in ex.values()), "an exclusion states its reason"
    short = [k for k in rm.KEYS if k not in ex and not total[walk][k]]
    assert not short, (walk, "classes the cases do not reach", short)
    stale = [k for k in ex if total[walk][k]]
    assert not stale, (walk, "excluded classes that do occur", stale)


@pytest.mark.parametrize("walk", PACKED_WALKS)
def test_census_packed(walk):
    check_census(packed_census(), walk, rm.EXCLUDED)


@pytest.mark.parametrize("walk", RESIDUAL_WALKS)
def test_census_residual(walk):
    check_census(residual_census(), walk, rm.RESIDUAL_EXCLUDED)


def test_each_construction_serves_its_classes():
    """Every construction of rdoq_cases reaches the classes it is there for, and every class
    has a construction: taking one out of the case set fails here, by the class's name."""
    per = collections.defaultdict(collections.Counter)
    for bd in rc.DEPTHS:
        for cs, m in zip(rc.cases(bd), modelled(bd)):
            if m is not None:
                per[cs["kind"]].update(m[2])
    assert set(per) == set(rc.SERVES) == set(rc.KINDS) | set(rc.TIES)
    for kind, keys in rc.SERVES.items():
        short = [k for k in keys if not per[kind][k]]
        assert not short, (kind, "does not reach", short)
    served = set(sum(rc.SERVES.values(), []))
    assert served | set(rc.UNSERVED) == set(rm.KEYS) and not served & set(rc.UNSERVED)


def test_walks_are_the_ones_named():
    """No case falls to a walk the census does not list, QuantFast gets its 2-wide blocks, and
    the packed entry's long class-1 list can be built from each depth's cases."""
    assert set(packed_census()) == set(PACKED_WALKS)
    assert set(residual_census()) == set(RESIDUAL_WALKS) | {"QuantFast"}
    assert residual_census()["QuantFast"]["blocks"] >= 3
    for bd in rc.DEPTHS:
        assert sum(rm.rq_class_of(cs["w"], cs["h"], cs["scan"]) == 1 and e_nnz > 0
                   for cs, (e_nnz, _) in zip(rc.cases(bd), oracle_results(bd))) >= 64


def test_every_shape_is_there():
    """The shapes of each walk instance, both orientations; the 2-wide ones with NO_2X2 set and
    clear; every shape up to 16x16 under the three scans; at every depth every QP remainder at
    a low and a high quotient, the three components, sign hiding on and off, every snapshot;
    every shape in the residual entry's picture as well; the 2x2 block at 8 bits."""
    for bd in rc.DEPTHS:
        seen = collections.defaultdict(set)
        for cs in rc.cases(bd):
            seen[(cs["w"], cs["h"])].add((cs["scan"], bool(cs["flags"] & rm.NO_2X2)))
            seen["qp"].add((cs["qp_luma"] % 6, cs["qp_luma"] // 6 >= 7))
            seen["comp"].add(cs["comp"])
            seen["sign_hide"].add(cs["sign_hide"])
            seen["ctx"].add(cs["ctx"])
        for w, h in rc.both(rc.SHAPES_4 + rc.SHAPES_16 + rc.SHAPES_64):
            want = {(s, False) for s in rc.scans_of(w, h)}
            assert seen[(w, h)] == want, (w, h)
        for w, h in rc.both(rc.SHAPES_2):
            assert seen[(w, h)] == {(s, f) for s in rc.scans_of(w, h) for f in (False, True)}
        assert seen["qp"] >= {(r, hi) for r in range(6) for hi in (False, True)}
        assert seen["comp"] == {0, 1, 2} and seen["sign_hide"] == {0, 1}
        assert seen["ctx"] == set(range(len(rc.snapshots(bd))))
        shapes = {(int(b["w"]), int(b["h"])) for b in rc.residual_picture(bd)[2]}
        want = set(rc.both(rc.SHAPES_4 + rc.SHAPES_16 + rc.SHAPES_64 + rc.SHAPES_2))
        assert shapes >= want, want - shapes
    assert (8, 2, 2) in {(cs["bd"], cs["w"], cs["h"]) for cs in rc.cases(8)}
    assert packed_census()["packed/wave_rdoq<64>/2x2"]["iq_shift_left"]


def test_saturation_is_out_of_reach():
    """The largest level the forward quantiser can give at a raw QP >= 0: below 32767 - 1 for
    every shape and depth (the derivation of rdoq_model's docstring, evaluated)."""
    for bd in rc.DEPTHS:
        for w in (2, 4, 8, 16, 32, 64):
            for h in (2, 4, 8, 16, 32, 64):
                for qp in range(0, 6):
                    k = rm.quant_constants(bd, qp, w, h)
                    top = (32768 * k["scale"] + (1 << (k["fq_shift"] - 1))) >> k["fq_shift"]
                    assert top <= 26215, (bd, w, h, qp, top)


def test_forward_coefficients_stay_inside_int16(xo):
    """The bound behind the residual entry's int16 exclusions, evaluated on the oracle's
    matrices: no row or column sums to more than 256 N in absolute value, so a residual of
    at most 2^depth - 1 leaves either stage at no more than (2^depth - 1) * 2^(15 - depth); and
    the pictures' own coefficients stay there."""
    gain = {}
    for n in (2, 4, 8, 16, 32, 64):
        m = np.abs(xo.transform_matrix(0, n).astype(np.int64))
        gain[n] = int(max(m.sum(axis=0).max(), m.sum(axis=1).max()))
        assert gain[n] == 256 * n
    for bd in rc.DEPTHS:
        top = ((1 << bd) - 1) << (15 - bd)
        assert top < 32767
        for w in gain:
            for h in gain:
                s1, s2 = rm.log2(w) + bd - 9 + 2, rm.log2(h) + 6 + 2
                t = (((1 << bd) - 1) * gain[w] + (1 << (s1 - 1))) >> s1
                assert (t * gain[h] + (1 << (s2 - 1))) >> s2 == t == top, (bd, w, h)
        orig, pred, blocks, _, _ = rc.residual_picture(bd)
        for b in blocks:
            x, y, w, h, c = (int(b[k]) for k in ("x", "y", "w", "h", "comp"))
            resi = (orig[c][y:y + h, x:x + w].astype(np.int32) - pred[c][y:y + h, x:x + w])
            coeff = xo.fwd_transform(bd, np.ascontiguousarray(resi.astype(np.int16)))
            assert np.abs(coeff.astype(np.int32)).max() <= top, tuple(b)


def census_table(total, walks, excluded):
    lines = ["| class | " + " | ".join("`%s`" % w for w in walks) + " |",
             "|---|" + "---:|" * len(walks)]
    for k in rm.KEYS:
        cells = ["-" if k in dict(rm.EXCLUDED["*"], **excluded[w]) else str(total[w][k])
                 for w in walks]
        lines.append("| %s | " % k + " | ".join(cells) + " |")
    return "\n".join(lines)


if __name__ == "__main__":
    print(census_table(packed_census(), PACKED_WALKS, rm.EXCLUDED))
    print()
    print(census_table(residual_census(), RESIDUAL_WALKS, rm.RESIDUAL_EXCLUDED))
    for name, ex in (("packed", rm.EXCLUDED), ("residual", rm.RESIDUAL_EXCLUDED)):
        for walk, d in ex.items():
            for k, why in d.items():
                print("- %s `%s`: `%s` - %s" % (name, walk, k, why))
