"""Adaptive QP without a GPU: the thresholds of the xvcgpu_aqp_table against the oracle's
(and, where it is built, the reference's) CalcDeltaQpFromVariance, the table's entries
against the per-QP constants the flat pass uses, the Python and the C++ filler byte for byte,
the struct layouts against the header, and the model of the passes (tests/aqp_pass_model.py)
on the conditions its scene was built for."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import aqp_pass_model as am
import oracle_lib as ol
import oracle_stats as st

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEPTHS, STRENGTHS = (8, 10, 12), (0, 5, 13, 20)
NEVER = 0xffffffffffffffff


@pytest.fixture(scope="module")
def xo():
    return ol.Lib("xo")


@pytest.fixture(scope="module")
def pipeline():
    from xvc_amd import build
    build.build()
    from xvc_amd import pipeline as p
    return p


@pytest.mark.parametrize("bd", DEPTHS)
@pytest.mark.parametrize("strength", STRENGTHS)
def test_thresholds_are_the_oracles_steps(xo, pipeline, bd, strength):
    """var_min[k] is the smallest statistic whose delta reaches -2 + k."""
    t = pipeline.aqp_table(32, bd, strength, am.W)
    reached = 0
    for k in range(am.DELTAS - 1):
        v, want = int(t.var_min[k]), am.DELTA_MIN + 1 + k
        if v == NEVER:      # not even the largest statistic gets there
            assert st.xo_aqp_delta_qp(xo, 1 << 63, bd, strength) < want
            continue
        reached += 1
        assert v >= 1 and st.xo_aqp_delta_qp(xo, v, bd, strength) >= want, (k, v)
        if v > 1:
            assert st.xo_aqp_delta_qp(xo, v - 1, bd, strength) < want, (k, v)
        else:               # v = 1, the smallest statistic there is, has it already
            assert st.xo_aqp_delta_qp(xo, 1, bd, strength) >= want
    assert list(t.var_min) == sorted(t.var_min)
    if strength == 0:       # delta 0 everywhere
        assert reached == 3 and all(am.table_delta(t, v) == 0 for v in (1, 77, 1 << 40, 1 << 63))
    else:
        assert reached == am.DELTAS - 1
    # ... and between the steps the count is the oracle's delta
    rng = np.random.default_rng(31 + bd + strength)
    for v in [1, 2, 1 << 63] + [int(x) for x in 2 ** rng.uniform(0, 40, 400)]:
        assert am.table_delta(t, v) == st.xo_aqp_delta_qp(xo, v, bd, strength), v


def test_negative_strength_is_refused(pipeline):
    with pytest.raises(ValueError, match="strength"):
        pipeline.aqp_table(32, 10, -1, am.W)
    with pytest.raises(ValueError, match="ctu_size"):
        pipeline.aqp_table(32, 10, 13, am.W, ctu_size=48)


@pytest.mark.parametrize("bd", (8, 10))
def test_scene_holds_the_deltas_it_was_built_for(xo, pipeline, bd):
    """The condition on the input: the reference's own deltas (the oracle's where the
    reference is not built) for the 200x136 scene at its strength are the ones it was built
    for - both ends, at least five values, a cut CTU away from 0 - and the table gives the
    reference's delta for every CTU and every strength.

    The reference computes its own statistic, and in the CTUs the picture edge cuts it reads
    the 16x16 blocks that hang over the edge on into the next row and behind the plane, where
    xvcgpu_variance_map (and xo_variance_map) read the border.  So for every strength the
    thresholds are checked on the statistic as the reference reads it
    (ctu_variances_as_the_reference_reads: equal to the border's reading in the eight whole
    CTUs, asserted), and at the scene's own strength the border's reading must give the
    reference's delta in the cut CTUs too - the scene is built so that it does."""
    orig, _ = am.scene(bd)
    luma = np.ascontiguousarray(orig[0][am.BL:am.BL + am.H, am.BL:am.BL + am.W])
    ctu_var = am.ctu_variances(xo, am.W, am.H, orig[0])
    ref_var = am.ctu_variances_as_the_reference_reads(luma)
    assert ctu_var.shape == ref_var.shape == (3, 4)
    assert np.array_equal(ctu_var[:2, :3], ref_var[:2, :3])
    xr = ol.Lib("xr") if ol.have_ref() else None
    for strength in STRENGTHS:
        t = pipeline.aqp_table(am.QP, bd, strength, am.W)
        for r in range(3):
            for q in range(4):
                got = am.table_delta(t, int(ref_var[r, q]))
                assert got == st.xo_aqp_delta_qp(xo, int(ref_var[r, q]), bd, strength)
                assert am.table_delta(t, int(ctu_var[r, q])) == \
                    st.xo_aqp_delta_qp(xo, int(ctu_var[r, q]), bd, strength)
                if xr is not None:
                    assert got == st.xr_aqp_delta_qp(xr, bd, luma, 64 * q, 64 * r, 64,
                                                     strength), (strength, r, q)
    t = pipeline.aqp_table(am.QP, bd, am.STRENGTH, am.W)
    deltas = [[am.table_delta(t, int(v)) for v in row] for row in ctu_var]
    assert deltas == [list(row) for row in am.SCENE_DELTAS], deltas
    assert deltas == [[am.table_delta(t, int(v)) for v in row] for row in ref_var]
    if xr is not None:
        assert deltas == [[st.xr_aqp_delta_qp(xr, bd, luma, 64 * q, 64 * r, 64, am.STRENGTH)
                           for q in range(4)] for r in range(3)]
    flat = sum(deltas, [])
    assert min(flat) == -3 and max(flat) == 7 and len(set(flat)) >= 5
    assert deltas[1][3] != 0 and deltas[2][0] != 0       # cut CTUs


@pytest.mark.parametrize("pic_qp", (2, 32, 60))
@pytest.mark.parametrize("bd", DEPTHS)
def test_table_entries_are_the_flat_pass_constants(pipeline, pic_qp, bd):
    t = pipeline.aqp_table(pic_qp, bd, 13, 1920)
    assert (t.pic_qp, t.ctu_size, t.ctus_per_row) == (pic_qp, 64, 30)
    qps = []
    for k in range(am.DELTAS):
        qp = max(0, min(63, pic_qp + am.DELTA_MIN + k))
        qps.append(qp)
        assert (t.qp_y[k], t.qp_c[k]) == (qp, pipeline.chroma_qp(qp))
        assert t.lambda16[k] == pipeline.lambda16_for_qp(qp)
        for c, (lam, rdf) in enumerate(pipeline.rdoq_host_params(qp, bd)):
            assert (t.rdoq_lambda[k][c], t.rdoq_rd_factor[k][c]) == (lam, rdf)
    if pic_qp == 2:
        assert qps[:3] == [0, 0, 1]       # the clip at 0
    if pic_qp == 60:
        assert qps[-5:] == [63] * 5       # ... and at 63
    # the entry of delta 0 is what FrameDescriptors gives a flat picture of pic_qp
    d = pipeline.FrameDescriptors(64, 64, pic_qp, rdoq=True, bitdepth=bd)
    k0 = -am.DELTA_MIN
    assert d.me["lambda16"][0] == t.lambda16[k0]
    assert (d.tx["qp"][0], d.tx["qp"][1]) == (t.qp_y[k0], t.qp_c[k0])
    assert [int(d.rdoq_params["lambda"][c]) for c in range(3)] == list(t.rdoq_lambda[k0])
    assert [int(d.rdoq_params["rd_factor"][c]) for c in range(3)] == list(t.rdoq_rd_factor[k0])


_CASES = [(32, 10, 13, 200, 64), (2, 8, 5, 1920, 64), (60, 12, 20, 136, 32), (27, 10, 0, 64, 128),
          (45, 8, 13, 3840, 16)]


def test_python_and_cpp_tables_are_the_same_bytes(pipeline, tmp_path):
    """pipeline.aqp_table against xvc_gpu::AdaptiveQp::Table, compiled with plain g++."""
    from xvc_amd import api
    calls = "".join("  dump(xvc_gpu::AdaptiveQp::Table(%d, %d, %d, %d, %d));\n" % c for c in _CASES)
    src = tmp_path / "aqp_table.cc"
    src.write_text(
        "#include <cstdio>\n#include \"xvc_gpu_ops.h\"\n"
        "static void dump(const xvcgpu_aqp_table &t) {\n"
        "  const unsigned char *p = reinterpret_cast<const unsigned char *>(&t);\n"
        "  for (size_t i = 0; i < sizeof(t); i++) std::printf(\"%02x\", p[i]);\n"
        "  std::printf(\"\\n\");\n}\n"
        "int main() {\n" + calls +
        "  try { xvc_gpu::AdaptiveQp::Table(32, 10, -1, 64); } catch (const xvc_gpu::Error &e) {\n"
        "    std::printf(\"refused %d\\n\", (int)e.status); }\n"
        "  std::printf(\"%zu %zu\\n\", sizeof(xvcgpu_aqp_table), sizeof(xvcgpu_aqp_args));\n"
        "  return 0;\n}\n")
    exe = str(tmp_path / "aqp_table")
    lib_dir = os.path.join(ROOT, "xvc_amd")
    subprocess.check_call([
        "g++", "-std=c++11", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
        "-I", os.path.join(lib_dir, "host"), str(src), "-o", exe, "-L", lib_dir, "-lxvcgpu",
        "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.check_output([exe]).decode().split("\n")
    for case, line in zip(_CASES, out):
        assert bytes.fromhex(line) == bytes(pipeline.aqp_table(*case)), case
    assert out[len(_CASES)] == "refused 10"       # XVCGPU_INVALID_ARGUMENT
    assert out[len(_CASES) + 1].split() == [str(C.sizeof(api.AqpTable)), str(C.sizeof(api.AqpArgs))]


def test_struct_layouts_match_header(pipeline, tmp_path):
    from xvc_amd import api
    fields = ["pic_qp", "ctu_size", "ctus_per_row", "var_min", "qp_y", "qp_c", "lambda16",
              "rdoq_lambda", "rdoq_rd_factor"]
    arg_fields = ["table", "d_var16", "d_ctu_var", "d_ctu_dqp", "d_cu_qp"]
    src = tmp_path / "layout.c"
    src.write_text(
        "#include <stdio.h>\n#include <stddef.h>\n#include \"xvcgpu.h\"\nint main(){\n" +
        "".join("printf(\"%%zu \", offsetof(xvcgpu_aqp_table, %s));\n" % f for f in fields) +
        "".join("printf(\"%%zu \", offsetof(xvcgpu_aqp_args, %s));\n" % f for f in arg_fields) +
        "printf(\"%zu %zu %zu %d %d\\n\", sizeof(xvcgpu_aqp_table), sizeof(xvcgpu_aqp_args),"
        "sizeof(xvcgpu_frame_pass_args), XVC_AQP_DELTA_MIN, XVC_AQP_DELTAS);return 0;}\n")
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src),
                           "-o", exe])
    out = [int(v) for v in subprocess.check_output([exe]).decode().split()]
    assert out == [getattr(api.AqpTable, f).offset for f in fields] + \
        [getattr(api.AqpArgs, f).offset for f in arg_fields] + \
        [C.sizeof(api.AqpTable), C.sizeof(api.AqpArgs), C.sizeof(api.FramePassArgs),
         api.AQP_DELTA_MIN, api.AQP_DELTAS]
    assert C.sizeof(api.FramePassArgs) == 240      # the flat pass's block stays what it was
    assert (am.DELTA_MIN, am.DELTAS) == (api.AQP_DELTA_MIN, api.AQP_DELTAS)


def test_model_apply_touches_the_named_fields_only(xo, pipeline):
    """The model's apply on the partition: per CU the table's entry of its CTU's delta in
    the named fields, every other byte of the records as it was."""
    from xvc_amd import api
    bd = 10
    desc = am.descriptors(bd, rdoq=True, part=True)
    assert desc.n_cus == len(am.partition_200()) and desc.min_side == 4 and desc.max_side == 64
    t = pipeline.aqp_table(am.QP, bd, am.STRENGTH, am.W)
    ctu_var = am.ctu_variances(xo, am.W, am.H, am.scene(bd)[0][0])
    second = desc.me.copy()
    second["mvp_x"] = 5
    (me, me2), tx, prm, cu_qp, ctu_dqp, written = am.apply(
        t, ctu_var, [desc.me, second], desc.tx, desc.rdoq_params, desc.luma_idx)
    assert written.all() and ctu_dqp.reshape(3, 4).tolist() == [list(r) for r in am.SCENE_DELTAS]
    for i, (x, y, w, h) in enumerate(am.partition_200()):
        k = am.SCENE_DELTAS[y // 64][x // 64] - am.DELTA_MIN
        assert me["lambda16"][i] == me2["lambda16"][i] == t.lambda16[k]
        assert tx["qp"][3 * i:3 * i + 3].tolist() == [t.qp_y[k], t.qp_c[k], t.qp_c[k]]
        assert prm["lambda"][3 * i:3 * i + 3].tolist() == list(t.rdoq_lambda[k])
        assert cu_qp[i].tolist() == [t.qp_y[k], t.qp_c[k]]
    for new, old, field in ((me, desc.me, "lambda16"), (me2, second, "lambda16"),
                            (tx, desc.tx, "qp")):
        a, b = new.copy(), old.copy()
        a[field] = b[field] = 0
        assert a.tobytes() == b.tobytes()
    a, b = prm.copy(), desc.rdoq_params.copy()
    for f in ("lambda", "rd_factor"):
        a[f] = b[f] = 0
    assert a.tobytes() == b.tobytes()
    assert len(set(cu_qp[:, 0].tolist())) >= 5 and api.ME_DTYPE == desc.me.dtype


def test_model_pass_with_strength_zero_is_the_flat_oracle_pass(xo, pipeline):
    """The model's P pass with a table of strength 0 is xo_frame_pass as it stands."""
    import oracle_frame
    bd = 8
    orig, ref = am.scene(bd)
    desc = am.descriptors(bd, rdoq=True)
    t0 = pipeline.aqp_table(am.QP, bd, 0, am.W)
    rec, res, nnz, cus, ssd, cu_qp, dqp, _ = am.p_pass(xo, desc, bd, orig, ref, t0, levels=False)
    e_rec, e_res, e_nnz, e_cus, e_ssd = oracle_frame.frame_pass(desc, bd, orig, ref, am.BL, lib=xo)
    assert not dqp.any() and (cu_qp == (am.QP, pipeline.chroma_qp(am.QP))).all()
    assert res.tobytes() == e_res.tobytes() and np.array_equal(nnz, e_nnz)
    assert all((nnz[desc.tx["comp"] == c] != 0).sum() >= 10 for c in range(3))
    assert cus.tobytes() == e_cus.tobytes() and ssd == e_ssd
    assert all(np.array_equal(a, b) for a, b in zip(rec, e_rec))
    # ... and with the default strength it is another picture
    t = pipeline.aqp_table(am.QP, bd, am.STRENGTH, am.W)
    rec2, _, _, cus2, _, _, dqp2, _ = am.p_pass(xo, desc, bd, orig, ref, t, levels=False)
    assert dqp2.tolist() == [list(r) for r in am.SCENE_DELTAS]
    assert len(set(cus2["qp_y"].tolist())) >= 5
    assert any(not np.array_equal(a, b) for a, b in zip(rec2, e_rec))


def test_b_scenes_hold_three_deltas(xo, pipeline):
    """The condition on the B inputs: at least three distinct deltas among their CTUs."""
    import bi_refs_pass_model as rm
    for name in ("grid10", "part10"):
        pw, ph, bd, _, orig, _ = am.b_scene(name)
        t = pipeline.aqp_table(rm.QP, bd, am.STRENGTH, pw)
        deltas = [am.table_delta(t, int(v)) for v in am.ctu_variances(xo, pw, ph, orig[0]).ravel()]
        assert len(set(deltas)) >= 3, (name, deltas)
        for v in am.ctu_variances(xo, pw, ph, orig[0]).ravel():
            assert am.table_delta(t, int(v)) == st.xo_aqp_delta_qp(xo, int(v), bd, am.STRENGTH)
