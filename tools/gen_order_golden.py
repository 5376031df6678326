#!/usr/bin/env python3
"""The ORDER of a real encoder run's RD search, and the motion searches' prices
(authoring container only: needs oracle/_ref/libxvcref.so).

    python tools/gen_order_golden.py [tiny] [c0] [c1]

tools/gen_me_golden.py and tools/gen_rd_golden.py record WHAT the reference
encoder's RD search computes on the hot path - each table in its own capture
order.  This run records both in one encode and adds

  seq/<table>  a sequence number over ALL tables (me calls, steps, merges, evals,
          calls, cands, finals): the order in which CuEncoder::CompressCu
          (cu_encoder.cc:123-273) really issued the work - one CU state after
          the other, each a chain whose results feed the next;
  cands   every candidate InterSearch::SearchRefIdx prices
          (inter_search.cc:556-571): list, picture, vector, final predictor,
          distortion and the bits GetInterPredBits returned for it with the
          encoder's DEFAULT setting (fast_inter_pred_bits == 0: a throw-away
          RdoSyntaxWriter on the live CABAC state, :1131-1135);
  ictx    the states of the contexts CuWriter::WriteInterPrediction reads for
          that CU (include/xvcgpu_types.h: xvcgpu_inter_contexts);
  finals  the motion state SearchMotion ends with (:247-257).

The stream must equal the committed fixture and the me / rd tables of this run
must equal the committed me_calls / rd_calls fixtures record for record: the
sequence numbers index THOSE.  Written to tests/golden/rd_order_<clip>.npz."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import gen_me_golden as gmg  # noqa: E402
import gen_rd_golden as grg  # noqa: E402
import gen_stream_golden as gsg  # noqa: E402
import oracle_lib as ol  # noqa: E402
import order_fixture as of  # noqa: E402
import rd_fixture as rf  # noqa: E402
import stream_fixture as sf  # noqa: E402
from xvc_amd import synth  # noqa: E402

KEEP = {"tiny": None, "c0": None, "c1": 2}
# round 5: the INTRA states of the picture tests/rd_serial.py walks (CompressIntra,
# cu_encoder.cc:518-541): every DetermineSlowIntraModes call and every
# TransformAndReconstruct of its intra CUs, stamped with the same sequence counter ->
# tests/golden/intra_order_<clip>.npz.  clip -> (picture, at most this many inter records
# of the order in front of a kept intra record: the 1080p picture's capture is cut to the
# stretch the tests walk)
INTRA_WALK = {"tiny": (2, None), "c0": (4, None), "c1": (2, None)}
SEQ_TABLES = ["me", "steps", "merges", "evals", "calls", "cands", "finals"]


def fetch(lib, which, dt):
    n = lib.xr_rd_count(which)
    assert lib.xr_rd_size(which) == dt.itemsize, (which, lib.xr_rd_size(which), dt.itemsize)
    if n == 0:
        return np.zeros(0, dt)
    buf = (C.c_char * (n * dt.itemsize)).from_address(lib.xr_rd_data(which))
    return np.frombuffer(buf, dt).copy()


def write_intra(lib, name, poc, cut, pos, stamp):
    """tests/golden/intra_order_<clip>.npz: calls / evals / samples (intra_fixture.CALL_DTYPE,
    EVAL_DTYPE), itx / itx_samples / contexts / qps (ITX_DTYPE; LM chroma = mode 67, its luma
    rectangle behind its reference samples), pos/<table>: inter records of the order in front
    of each record, stamp/<table>: the records' own order among the intra records."""
    import ctypes as C
    import intra_fixture as ifx
    lib.xr_intra_count.restype = C.c_long
    lib.xr_intra_data.restype = C.c_void_p

    def ifetch(which, dt):
        n = lib.xr_intra_count(which)
        assert lib.xr_intra_size(which) == dt.itemsize
        if n == 0:
            return np.zeros(0, dt)
        return np.frombuffer((C.c_char * (n * dt.itemsize)).from_address(lib.xr_intra_data(which)), dt).copy()

    calls, evals, samples = ifetch(0, ifx.CALL_DTYPE), ifetch(1, ifx.EVAL_DTYPE), ifetch(2, np.dtype("<u2"))
    itx, itx_samples = fetch(lib, 9, ifx.ITX_DTYPE), fetch(lib, 10, np.dtype("<u2"))
    ctx = fetch(lib, 14, np.dtype(("u1", rf.CTX_BYTES)))
    qps = fetch(lib, 15, rf.QP_DTYPE)
    assert len(calls) == len(pos[0]) and len(itx) == len(pos[1]), (len(calls), len(pos[0]), len(itx), len(pos[1]))
    assert (calls["poc"] == poc).all() and (itx["poc"] == poc).all()
    rank = np.argsort(np.argsort(np.concatenate(stamp)))      # own order among the intra records
    st = [rank[:len(calls)], rank[len(calls):]]
    if cut is not None:          # keep the leading stretch only (sample arrays re-packed)
        kc, kt = pos[0] < cut, pos[1] < cut
        new_off, chunks = [], []
        total = 0
        ends = np.r_[calls["sample_off"][1:], len(samples)]
        for i in np.flatnonzero(kc):
            a, b = int(calls["sample_off"][i]), int(ends[i])
            new_off.append(total)
            chunks.append(samples[a:b])
            total += b - a
        ev_keep = kc[evals["call"]]
        remap = np.cumsum(kc) - 1
        evals = evals[ev_keep].copy()
        evals["call"] = remap[evals["call"]]
        calls = calls[kc].copy()
        calls["sample_off"] = new_off
        calls["first_eval"] = np.r_[0, np.cumsum(calls["n_eval"])[:-1]]
        samples = np.concatenate(chunks) if chunks else samples[:0]
        ends = np.r_[itx["sample_off"][1:], len(itx_samples)]
        new_off, chunks, total = [], [], 0
        for i in np.flatnonzero(kt):
            a, b = int(itx["sample_off"][i]), int(ends[i])
            new_off.append(total)
            chunks.append(itx_samples[a:b])
            total += b - a
        itx = itx[kt].copy()
        itx["sample_off"] = new_off
        itx_samples = np.concatenate(chunks) if chunks else itx_samples[:0]
        pos = [pos[0][kc], pos[1][kt]]
        st = [st[0][kc], st[1][kt]]
        uc, inv = np.unique(itx["ctx_index"], return_inverse=True)      # the snapshots still used
        ctx, itx["ctx_index"] = ctx[uc], inv
    cols = {}
    for t, a in (("calls", calls), ("evals", evals), ("itx", itx)):
        for f in a.dtype.names:
            if not f.startswith("pad"):
                cols["%s/%s" % (t, f)] = np.ascontiguousarray(a[f])
    cols.update({"samples": samples, "itx_samples": itx_samples, "contexts": ctx, "qps": qps.view("u1"),
                 "pos/calls": pos[0].astype(np.int64), "pos/itx": pos[1].astype(np.int64),
                 "stamp/calls": st[0].astype(np.int64), "stamp/itx": st[1].astype(np.int64)})
    path = os.path.join(sf.GOLDEN, "intra_order_%s.npz" % name)
    np.savez_compressed(path, **cols)
    print("  %s: %d DetermineSlowIntraModes calls (%d mode evaluations), %d TransformAndReconstruct "
          "calls of intra CUs (%d LM chroma), %d context snapshots -> %s (%.1f KB)" % (
              name, len(calls), len(evals), len(itx), int((itx["mode"] == 67).sum()), len(ctx), path,
              os.path.getsize(path) / 1024))
    gsg.update_manifest("intra_order_%s.npz" % name)


def main():
    lib = C.CDLL(ol.REF_SO)
    lib.xr_rd_count.restype = C.c_long
    lib.xr_rd_data.restype = C.c_void_p
    lib.xr_me_capture_end.restype = C.c_long
    lib.xr_me_calls.restype = C.c_void_p
    for name, only in KEEP.items():
        if len(sys.argv) > 1 and name not in sys.argv[1:]:
            continue
        c = gsg.CLIPS[name]
        clip = synth.SyntheticClip(c["w"], c["h"], 8)
        lib.xr_me_capture_begin(-1 if only is None else only)
        lib.xr_rd_capture_begin(-1 if only is None else only)
        ipoc, icut = INTRA_WALK[name]
        lib.xr_intra_capture_begin(1 << 30, 1)
        lib.xr_intra_capture_poc(ipoc)
        lib.xr_rd_capture_intra_walk(1 << 30, ipoc)
        stream = gsg.encode(lib, clip, dict(c, threads=0))
        n_me = lib.xr_me_capture_end()
        lib.xr_rd_capture_end()
        lib.xr_intra_capture_end()
        committed = np.load(os.path.join(sf.GOLDEN, "stream_%s.npz" % name))["stream"]
        assert np.array_equal(stream, committed), "stream differs from the committed fixture"
        # the tables of this run = the committed fixtures
        buf = (C.c_char * (n_me * gmg.CALL_DTYPE.itemsize)).from_address(lib.xr_me_calls())
        me = np.frombuffer(buf, gmg.CALL_DTYPE)
        assert np.array_equal(me, np.load(os.path.join(sf.GOLDEN, "me_calls_%s.npz" % name))["calls"])
        rd = rf.load(name)
        for k, t in enumerate(grg.NAMES[:5]):
            got = grg.fetch(lib, k)
            want = rd[t]
            if t == "calls":       # the fixture keeps 16 bits of the reconstruction's CRC
                got = got.copy()
                got["rec_crc"] &= 0xffff
            assert len(got) == len(want) and all(
                np.array_equal(got[f], want[f]) for f in want.dtype.names if not f.startswith("pad")), t
        out = {"cands": fetch(lib, 11, of.CAND_DTYPE), "finals": fetch(lib, 12, of.FINAL_DTYPE),
               "ictx": fetch(lib, 13, of.ICTX_DTYPE)}
        seqs = [fetch(lib, 20 + t, np.dtype("<u4")) for t in range(7)]
        sizes = [n_me, len(rd["steps"]), len(rd["merges"]), len(rd["evals"]), len(rd["calls"]),
                 len(out["cands"]), len(out["finals"])]
        assert [len(s) for s in seqs] == sizes, ([len(s) for s in seqs], sizes)
        allseq = np.sort(np.concatenate(seqs))
        # the intra records share the counter: the seven tables' numbers are made dense
        # again (rd_order_<clip>.npz as before), an intra record is placed by the number of
        # inter records in front of it
        iseq = [fetch(lib, 27, np.dtype("<u4")), fetch(lib, 28, np.dtype("<u4"))]
        both = np.sort(np.concatenate(seqs + iseq))
        assert np.array_equal(both, np.arange(len(both), dtype=np.uint32) + both[0])
        seqs = [np.searchsorted(allseq, q).astype(np.uint32) for q in seqs]
        write_intra(lib, name, ipoc, icut, [np.searchsorted(allseq, q) for q in iseq], iseq)
        allseq = np.arange(len(allseq), dtype=np.uint32)
        cols = of.to_columns(out)
        for t, s in zip(SEQ_TABLES, seqs):
            cols["seq/" + t] = np.diff(s.astype(np.int64) - int(allseq[0]), prepend=0).astype(np.int32)
        path = os.path.join(sf.GOLDEN, "rd_order_%s.npz" % name)
        np.savez_compressed(path, **cols)
        cd = out["cands"]
        print("  %s: %d records in order; %d priced candidates (uni %d, re-used %d, bi %d, affine "
              "uni %d, affine bi %d), %d context snapshots, %d SearchMotion results -> %s (%.1f KB)"
              % (name, len(allseq), len(cd), int(((cd["kind"] == 0) & (cd["reused"] == 0)).sum()),
                 int(cd["reused"].sum()), int((cd["kind"] == 1).sum()), int((cd["kind"] == 2).sum()),
                 int((cd["kind"] == 3).sum()), len(out["ictx"]), len(out["finals"]), path,
                 os.path.getsize(path) / 1024))
        gsg.update_manifest("rd_order_%s.npz" % name)


if __name__ == "__main__":
    main()
