#!/usr/bin/env python3
"""Whole-stream golden fixtures (authoring container only: needs
oracle/_ref/libxvcref.so, i.e. /root/reference).

    python tools/gen_stream_golden.py [c0] [c1] ...

For each clip: generate the integer synthetic clip (xvc_amd/synth.py, SURVEY
8d), encode it with the REFERENCE encoder through its public C API (xvcenc's
defaults, the clip's QP and whatever else its CLIPS entry sets), decode the
stream with the REFERENCE decoder and capture, per picture in decoding order,
the parsed syntax the decoder's reconstruction stage starts from (CU tree
leaves, modes, vectors, transform types, levels) and what it produces (planes
before / after the in-loop filter, the picture MD5).  Written to
tests/golden/stream_<clip>.npz.

The fixture is data (bitstream bytes, syntax records, planes); no reference
source goes into it.
"""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import oracle_lib as ol  # noqa: E402
import stream_fixture as sf  # noqa: E402
from xvc_amd import synth  # noqa: E402

# name: width, height, frames, qp, sub_gop (0 = default), planes / pre = keep the
# final / unfiltered planes of the first k pictures.  Optional, xvcenc's default
# where absent: bd = internal bit depth, speed = speed mode, settings = explicit
# encoder settings (a string), content = "synth" (xvc_amd/synth.py) or "warp"
# (warped_clip below), threads, and the public encoder parameters of TOOLS.
TOOLS = ("deblock", "beta_offset", "tc_offset", "low_delay", "num_ref_pics",
         "chroma_qp_offset_u", "chroma_qp_offset_v")
KEEP = -2 ** 31          # XR_STREAM_KEEP of oracle/ref_stream.cc
SMALL = dict(w=136, h=72, n=5, sub_gop=4, planes=0, pre=0, threads=1)
WARP = dict(w=256, h=192, planes=0, pre=0, threads=1, content="warp")
CLIPS = {
    # BASELINE config 0: CIF, 10 frames, QP 32, xvcenc defaults
    "c0": dict(w=352, h=288, n=10, qp=32, sub_gop=0, planes=3, pre=0),
    # BASELINE config 1 (1080p QP 32), the first pictures: one intra picture +
    # one sub-GOP of 4 (hierarchical B); planes are pinned by MD5 only
    "c1": dict(w=1920, h=1080, n=5, qp=32, sub_gop=4, planes=0, pre=0),
    # BASELINE config 1 as SURVEY 8d specifies it: 33 pictures (two default
    # sub-GOPs of 16 + 1), xvcenc's defaults; MD5 only.  The decoder figure of
    # bench.py and tests/test_gpu_stream.py use it; the motion-search / RD-search
    # captures stay on the short clip above.
    "c1x": dict(w=1920, h=1080, n=33, qp=32, sub_gop=0, planes=0, pre=0),
    # CIF at the ends of the QP range (dense levels with escape codes / nearly empty
    # blocks): the RD-search captures of tools/gen_rd_golden.py at other operating
    # points than QP 32; MD5 only
    "c0q22": dict(w=352, h=288, n=5, qp=22, sub_gop=4, planes=0, pre=0),
    "c0q37": dict(w=352, h=288, n=5, qp=37, sub_gop=4, planes=0, pre=0),
    # small, for CPU-side checks of the host driver (oracle engine)
    "tiny": dict(w=136, h=72, n=5, qp=27, sub_gop=4, planes=5, pre=5),
    # ---- the small clip at other depths, settings and tool mixes; one thread (a
    # regeneration is deterministic), MD5 only.  tests/test_stream_fixture_content.py
    # says what each must hold.
    # internal bit depth 8 / 12 / 9 / 11
    "t8": dict(SMALL, qp=27, bd=8),
    "t12": dict(SMALL, qp=27, bd=12),
    "t9": dict(SMALL, qp=27, bd=9),
    "t11": dict(SMALL, qp=32, bd=11),
    # fine quantisers: transform skip in all three components, large levels, many
    # intra modes
    "tq8": dict(SMALL, qp=8, bd=10),
    "t12q2": dict(SMALL, qp=2, bd=12),
    # coarse: CU QPs beyond the in-loop filter's tc table (index clamps at 53)
    "tq50": dict(SMALL, qp=50, bd=10),
    # the in-loop filter's offsets, chroma QP offsets, no filter at all
    "tdb": dict(SMALL, qp=27, beta_offset=4, tc_offset=-3),
    "t8db": dict(SMALL, qp=30, bd=8, beta_offset=-6, tc_offset=6, chroma_qp_offset_u=3,
                 chroma_qp_offset_v=-4),
    "t12nodb": dict(SMALL, qp=27, bd=12, deblock=0),
    # low delay: P-like chains over up to four reference pictures
    "tld": dict(SMALL, n=7, qp=32, sub_gop=1, low_delay=1, num_ref_pics=4),
    # a zooming, turning, sliding texture: affine CUs, uni-directional too
    "warp": dict(WARP, n=5, qp=27, sub_gop=4),
    "warpld": dict(WARP, n=6, qp=30, sub_gop=1, low_delay=1, num_ref_pics=3),
}


class WarpedClip:
    """Frame i: the texture of tests/oracle_affine_me.warped_pics seen through a
    similarity transform that grows with i; flat mid-grey chroma, 8 bit."""

    def __init__(self, w, h):
        self.w, self.h = w, h

    def frame(self, i):
        import oracle_affine_me as am
        y = am.warped_pics(np.random.default_rng(77), 8, self.w, self.h, 0, zoom=1 + 0.012 * i,
                           rot=0.01 * i, shift=(0.7 * i, -0.4 * i), noise=1)[0]
        c = np.full((self.h // 2, self.w // 2), 128, np.uint16)
        return y, c, c


def encode(lib, clip, c):
    w, h, n = c["w"], c["h"], c["n"]
    frames = np.concatenate([np.concatenate([p.reshape(-1) for p in clip.frame(i)])
                             for i in range(n)]).astype(np.uint8)
    cap = 64 << 20
    out = np.zeros(cap, np.uint8)
    lib.xr_stream_encode_tools.restype = C.c_long
    lib.xr_stream_encode_tools.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_double,
                                           C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                           C.c_char_p, C.c_void_p, C.c_int, C.c_void_p,
                                           C.c_void_p, C.c_long]
    keep = {k: KEEP if "offset" in k else -1 for k in TOOLS}
    tools = np.array([c.get(k, keep[k]) for k in TOOLS], np.int32)
    settings = c["settings"].encode() if c.get("settings") else None
    t = time.time()
    used = lib.xr_stream_encode_tools(w, h, 8, c.get("bd", 0), 30.0, c["qp"], c["sub_gop"],
                                      c.get("speed", -1), -1, c.get("threads", -1), settings,
                                      tools.ctypes.data, n, frames.ctypes.data, out.ctypes.data,
                                      cap)
    assert used > 0, used
    print("  encoded %d frames -> %d bytes in %.1f s" % (n, used, time.time() - t))
    return out[:used].copy()


def features(pics):
    """The per-fixture line: what the stream holds that a decoder can get wrong."""
    info = np.stack([p[0] for p in pics])
    cus = np.concatenate([p[1] for p in pics])
    lv = np.concatenate([p[2] for p in pics])
    aff = cus["affine"] == 1
    intra0 = (cus["pred_mode"] == 0) & (cus["tree"] == 0)
    inter = cus["pred_mode"] == 1
    coded = (cus["cbf"] != 0) & (cus["tx_skip"] != 0)
    return ("bd %s; pic types %s; pic QP %d..%d, CU QP up to %d; deblock %s beta %s tc %s; "
            "%d CUs; tx_skip Y/U/V %d/%d/%d; %d luma modes; levels %d..%d; affine %d (uni %d, "
            "bi %d); LIC %d; ref_idx up to %d; num_ref up to (%d, %d)" % (
                sorted(set(info["bitdepth"].tolist())), sorted(set(info["pic_type"].tolist())),
                info["pic_qp"].min(), info["pic_qp"].max(), cus["qp"].max(),
                sorted(set(info["deblock"].tolist())), sorted(set(info["beta_offset"].tolist())),
                sorted(set(info["tc_offset"].tolist())), len(cus),
                *(int(coded[:, k].sum()) for k in range(3)),
                len(set(cus["intra_mode"][intra0, 0].tolist())),
                lv.min() if len(lv) else 0, lv.max() if len(lv) else 0, int(aff.sum()),
                int((aff & (cus["inter_dir"] != 2)).sum()),
                int((aff & (cus["inter_dir"] == 2)).sum()),
                int(cus["lic"].sum()), cus["ref_idx"][inter].max() if inter.any() else -1,
                info["num_ref"][:, 0].max(), info["num_ref"][:, 1].max()))


def main(names):
    lib = C.CDLL(ol.REF_SO)
    reuse = "--reuse" in names      # keep the committed stream, only re-run the decoder side
    for name in [n for n in names if not n.startswith("--")]:
        c = CLIPS[name]
        print("clip %s: %dx%d, %d frames, QP %d" % (name, c["w"], c["h"], c["n"], c["qp"]))
        path = os.path.join(sf.GOLDEN, "stream_%s.npz" % name)
        if reuse and os.path.exists(path):
            stream = np.load(path)["stream"]
        else:
            clip = (WarpedClip(c["w"], c["h"]) if c.get("content") == "warp" else
                    synth.SyntheticClip(c["w"], c["h"], 8))
            stream = encode(lib, clip, c)
        pics = sf.decode_with_reference(stream, keep_planes=True)
        arrays = {"stream": stream,
                  "info": np.stack([p[0] for p in pics]).view(np.uint8)}
        for i, (info, cus, lv, pre, post) in enumerate(pics):
            md5 = sf.picture_md5(post, int(info["bitdepth"]))
            assert np.array_equal(md5, info["md5"]), "host MD5 restatement differs"
            arrays["cus_%d" % i] = cus.view(np.uint8)
            arrays["levels_%d" % i] = lv
            for k in range(3):
                if i < c["planes"]:
                    arrays["post_%d_%d" % (i, k)] = post[k]
                if i < c["pre"]:
                    arrays["pre_%d_%d" % (i, k)] = pre[k]
            # invariants the reconstruction stage relies on
            inter = cus["pred_mode"] == 1
            aff = cus["affine"] == 1
            mv = cus["mv"].astype(np.int64)
            assert np.array_equal(mv[aff][:, :, 3], mv[aff][:, :, 1] + mv[aff][:, :, 2]
                                  - mv[aff][:, :, 0])
            na = inter & ~aff
            assert all(np.array_equal(mv[na][:, :, k], mv[na][:, :, 0]) for k in (1, 2, 3))
            assert not np.any(cus["lic"][aff])
            for cu in cus:
                for k in range(3):
                    if cu["cbf"][k] and not cu["tx_skip"][k]:
                        n = (int(cu["w"]) * int(cu["h"])) >> (2 if k else 0)
                        a = lv[int(cu["level_off"][k]):int(cu["level_off"][k]) + n]
                        assert bool(cu["dc_only"][k]) == (np.count_nonzero(a) == 1 and a[0] != 0)
            kinds = (int((cus["pred_mode"] == 0).sum()), int(cus["affine"].sum()),
                     int(cus["lic"].sum()), int((cus["inter_dir"] == 2).sum()))
            print("  pic %d: poc %d tid %d type %d qp %d, %d CUs (intra %d, affine %d, lic %d, "
                  "bi %d), %d levels, md5 %s" %
                  (i, info["poc"], info["tid"], info["pic_type"], info["pic_qp"], len(cus),
                   *kinds, len(lv), bytes(info["md5"]).hex()))
        print("  " + features(pics))
        np.savez_compressed(path, **arrays)
        print("  -> %s (%.1f KB)" % (path, os.path.getsize(path) / 1024))
        update_manifest("stream_%s.npz" % name)


def update_manifest(fname):
    """tests/golden/MANIFEST.md5: one line per fixture (test_golden_manifest)."""
    import hashlib
    mpath = os.path.join(sf.GOLDEN, "MANIFEST.md5")
    lines = [l for l in open(mpath).read().split("\n") if l.strip() and l.split()[1] != fname]
    digest = hashlib.md5(open(os.path.join(sf.GOLDEN, fname), "rb").read()).hexdigest()
    lines.append("%s  %s" % (digest, fname))
    open(mpath, "w").write("\n".join(sorted(lines, key=lambda l: l.split()[1])) + "\n")


if __name__ == "__main__":
    main(sys.argv[1:] or ["tiny", "c0"])
