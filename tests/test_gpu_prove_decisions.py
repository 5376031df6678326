"""Which blocks the all-zero proof of the RDO quantiser takes off the class lists - the
decisions, not only the levels.

Stand-alone kernel (rdoq_prove_zero_kernel behind xvcgpu_quant_rdo_batch): the blocks on
no list are exactly those in which nothing quantises to a level plus those for which the
numpy bound of tests/test_rdoq_zero_proof.py (proves_zero) holds - block by block, over
sizes 4x4 ... 32x32, the three scans, the three components, bit depths 8 / 10 / 12 and
QP 24 ... 45, with planted blocks for every edge of the candidate collection and of a
candidate's neighbourhood.  Levels and counts are the oracle's.

Fused path (recon_from_me_kernel<false, true>, the proof inside the forward kernel): a
frame pass in form fwd_from_me builds the same class lists as the same pass in form
fwd_transform with the stand-alone proof forced on, and the same reconstruction, counts,
CU records and SSD; the lists are also held against the numpy bound.  Over a short chain
of passes the pictures meet every kind of block: no candidate, 1 ... 16, more than 16,
proved.  A fused pass leaves zeros in the levels of every block it takes off the lists
and touches nothing around the level array, with 16-byte aligned offsets and without."""
import numpy as np
import pytest

import oracle_lib as ol
import oracle_rdoq as oq
import test_rdoq_zero_proof as zp

FWD = zp.FWD
SHAPES = [(4, 4), (8, 8), (16, 16), (32, 32), (4, 16), (16, 4), (8, 16), (16, 8), (8, 4), (32, 16)]
BATCH = 64
N_BATCHES = 6


def thresholds(bd, qp, w, h):
    """The smallest magnitudes that quantise to a level of 1 and of 2."""
    lw, lh = w.bit_length() - 1, h.bit_length() - 1
    qpb = max(qp + 6 * (bd - 8), 0)
    bias = (lw + lh) & 1
    scale = FWD[qpb % 6] * (181 if bias else 1)
    fq_shift = 14 + qpb // 6 + 15 - bd - ((lw + lh) >> 1) + (7 if bias else 0)
    off = 1 << (fq_shift - 1)
    return -((-off) // scale), -((-3 * off) // scale), scale, fq_shift


def n_candidates(bd, qp, src):
    h, w = src.shape
    _, _, scale, fq_shift = thresholds(bd, qp, w, h)
    a = np.abs(src.astype(np.int64))
    return int((((a * scale + (1 << (fq_shift - 1))) >> fq_shift) > 0).sum())


def host_params(rng, bd, qp, lam_scale=None, lam_fixed=None):
    lam = 0.57 * 2.0 ** ((qp - 12) / 3.0) * (lam_scale or float(rng.choice([0.5, 1.0, 2.0])))
    prm = np.zeros(1, oq.RDOQ_PARAMS_DTYPE)
    prm["lambda"] = int(lam * 65536 + 0.5) if lam_fixed is None else lam_fixed
    qpb = qp + 6 * (bd - 8)
    inv_scale = zp.INV[qpb % 6] << (qpb // 6)
    prm["rd_factor"] = int(inv_scale * inv_scale / lam / 16 / (1 << (2 * (bd - 8))) + 0.5)
    prm["flags"] = oq.RDOQ_INTRA_CU if rng.integers(0, 2) else 0
    return prm


def random_block(rng, bd):
    """A block of _cases' kind (magnitudes around the quantiser's threshold) of any shape."""
    comp = int(rng.integers(0, 3))
    w, h = SHAPES[int(rng.integers(0, len(SHAPES)))]
    scan = int(rng.integers(0, 3)) if max(w, h) < 16 else 0
    qp = int(rng.integers(24, 46))
    t1 = thresholds(bd, qp, w, h)[0]
    yy, xx = np.mgrid[0:h, 0:w]
    decay = np.exp(-(xx + yy) / float(rng.choice([0.5, 1.0, 2.0])))
    src = np.rint(rng.laplace(0, 1, (h, w)) * decay * t1 * float(rng.choice([1.0, 2.0, 4.0])))
    src = np.clip(src, -32767, 32767).astype(np.int16)
    return dict(comp=comp, scan=scan, qp=qp, prm=host_params(rng, bd, qp), src=src)


def planted_blocks(rng, bd):
    """Every edge of the candidate collection and of a candidate's neighbourhood, on a luma
    16x16, a chroma 8x8 and a luma 8x16 (w x h)."""
    out = []
    for (w, h), comp in (((16, 16), 0), ((8, 8), 1), ((8, 16), 0)):
        qp = int(rng.integers(28, 40))
        t1, t2 = thresholds(bd, qp, w, h)[:2]
        small = max(t1 - 1, 0)

        def block(cells, fill=0, lam_fixed=None, scan=0):
            src = np.full((h, w), fill, np.int16)
            src[::2, 1::2] *= -1
            for (x, y), v in cells:
                src[y, x] = v
            out.append(dict(comp=comp, scan=scan, qp=qp, src=src,
                            prm=host_params(rng, bd, qp, 1.0, lam_fixed)))

        cells = [(x, y) for y in range(h) for x in range(w)]
        spread = [cells[(7 * k * len(cells)) // 128 % len(cells)] for k in range(17)]
        assert len(set(spread)) == 17
        block([], fill=small)                                   # no candidate, nothing is zero
        block([((0, 0), t1)])                                   # one, at (0, 0)
        block([((0, 0), -t1)], fill=small)
        block([(p, t1) for p in spread[:16]])                   # sixteen: the last that is tried
        block([(p, -t1) for p in spread])                       # seventeen: left to the walk
        block([((4, 0), t1)])                                   # a sub-block's DC behind the first
        block([((0, 4), t1), ((1, 0), t1)])
        block([((w - 1, 1), t1), ((2, h - 1), -t1)])            # last column, last row
        block([((w - 1, h - 1), t1)])
        block([((1, 1), t1), ((2, 1), t1), ((1, 2), -t1)])      # neighbours with q = 1 ...
        block([((1, 1), t1), ((2, 1), t2), ((1, 2), -(t2 + 3)), ((3, 1), 2 * t2)])   # ... q >= 2
        block([((0, 0), t2), ((1, 0), t2), ((0, 1), t2), ((1, 1), t2), ((2, 0), t2), ((0, 2), t2)])
        block([((1, 0), -32768)])                               # the magnitude that wraps
        block([((0, 0), t1), ((3, 3), -32768)])
        block([((0, 0), t1)], lam_fixed=(1 << 32) + 12345)      # lambda above 2^32
        block([((2, 1), t2), ((1, 1), t1)], lam_fixed=(5 << 32) + 1)
        if max(w, h) < 16:
            block([((1, 1), t1), ((5, 2), t1)], scan=1)
            block([((1, 1), t1), ((5, 2), t1)], scan=2)
    return out


def make_batches():
    """[(bd, contexts, blocks)]: N_BATCHES random batches and one of planted blocks per bit
    depth, one random context snapshot each."""
    rng = np.random.default_rng(20261020)
    batches = []
    for k in range(N_BATCHES):
        bd = (8, 10, 12)[k % 3]
        batches.append((bd, oq.random_contexts(rng), [random_block(rng, bd) for _ in range(BATCH)]))
    for bd in (8, 10, 12):
        batches.append((bd, oq.random_contexts(rng), planted_blocks(rng, bd)))
    return batches


def expect(xo, ent, bd, ctxs, blocks):
    """Per block: (candidates, proved by the bound, the oracle's count and levels)."""
    out = []
    for b in blocks:
        nc = n_candidates(bd, b["qp"], b["src"])
        proved = zp.proves_zero(ent, bd, b["qp"], b["comp"], b["scan"], ctxs[0], b["prm"][0],
                                b["src"])
        nnz, lv = oq.quant_rdo_oracle(xo, bd, b["qp"], b["comp"], b["scan"], 1, ctxs, b["prm"],
                                      b["src"])
        if proved:
            assert nnz == 0
        out.append((nc, proved, nnz, lv if nnz else np.zeros_like(b["src"])))
    return out


@pytest.fixture(scope="module")
def world():
    """The batches and what is expected of them, computed once on the CPU."""
    xo = ol.Lib("xo")
    ent = zp.entropy_table(xo)
    batches = make_batches()
    return xo, ent, [(bd, c, bl, expect(xo, ent, bd, c, bl)) for bd, c, bl in batches]


def is_tried(b, nc):
    return 1 <= nc <= 16 and not (np.abs(b["src"].astype(np.int64)) == 32768).any()


def test_generator_meets_its_condition(world):
    """(no GPU) at least 50 blocks proved, at least 50 tried and not proved, and the planted
    counts are what they are meant to be."""
    _, _, batches = world
    proved = sum(e[1] for _, _, _, ex in batches for e in ex)
    tried = sum(is_tried(b, e[0]) and not e[1] for _, _, bl, ex in batches for b, e in zip(bl, ex))
    n = sum(len(bl) for _, _, bl, _ in batches)
    print("blocks %d, proved %d, tried and not proved %d" % (n, proved, tried))
    assert n >= 300 and proved >= 50 and tried >= 50
    for bd, _, bl, ex in batches[N_BATCHES:]:
        counts = [e[0] for e in ex]
        assert counts[0:5] == [0, 1, 1, 16, 17], (bd, counts[:5])
        # the magnitude of 32768 is never proved, the lambda above 2^32 is priced
        for b, e in zip(bl, ex):
            if (np.abs(b["src"].astype(np.int64)) == 32768).any():
                assert not e[1]
        assert any(int(b["prm"][0]["lambda"]) > 1 << 32 and e[1] for b, e in zip(bl, ex))


@pytest.mark.gpu
def test_standalone_proof_block_by_block(world):
    """xvcgpu_quant_rdo_batch with the proof on: the blocks on no list are those without a
    candidate and those the numpy bound proves, and no other; levels and counts are the
    oracle's."""
    from xvc_amd import api
    _, _, batches = world
    ctx = api.Context(0)
    ctx.set_rdoq_prove_zero(1)
    proved_n = tried_n = 0
    try:
        for k, (bd, ctxs, bl, ex) in enumerate(batches):
            n = len(bl)
            blocks = np.zeros(n, api.TX_DTYPE)
            prm = np.zeros(n, api.RDOQ_PARAMS_DTYPE)
            off = np.zeros(n, np.uint32)
            coeffs, pos = [], 0
            for i, b in enumerate(bl):
                h, w = b["src"].shape
                blocks[i]["w"], blocks[i]["h"], blocks[i]["qp"] = w, h, b["qp"]
                blocks[i]["comp"] = b["comp"]
                blocks[i]["intra_pic"] = api.TXF_RDOQ | (b["scan"] << api.TXF_SCAN_SHIFT)
                for f in ("lambda", "rd_factor", "flags"):
                    prm[i][f] = b["prm"][0][f]
                off[i] = pos
                coeffs.append(b["src"].reshape(-1))
                pos += w * h
            levels, nnz = ctx.quant_rdo_batch(bd, blocks, np.concatenate(coeffs), off, ctxs, prm)
            lists = ctx.debug_rdoq_lists(n)
            listed = np.concatenate(lists)
            assert len(np.unique(listed)) == len(listed)
            off_list = set(range(n)) - set(int(v) for v in listed)
            want = {i for i, e in enumerate(ex) if e[0] == 0 or e[1]}
            assert off_list == want, (k, bd, sorted(off_list ^ want),
                                      [(ex[i][0], ex[i][1], bl[i]["src"].shape)
                                       for i in sorted(off_list ^ want)])
            for i, (b, e) in enumerate(zip(bl, ex)):
                assert int(nnz[i]) == e[2], (k, i)
                got = levels[off[i]:off[i] + b["src"].size].reshape(b["src"].shape)
                assert np.array_equal(got, e[3]), (k, i)
                proved_n += bool(e[1])
                tried_n += is_tried(b, e[0]) and not e[1]
    finally:
        ctx.set_rdoq_prove_zero(-1)
        ctx.close()
    print("proved %d, tried and not proved %d" % (proved_n, tried_n))
    assert proved_n >= 50 and tried_n >= 50


# ---- the fused path ----------------------------------------------------------------------
BORDER = 128
CHAIN = 3
FUSED_CASES = [(64, 48, 10), (64, 40, 10), (32, 32, 8), (32, 32, 12)]
FUSED_QPS = [27, 32, 37]
SENTINEL = 0x5a5b
GUARD = 64      # int16 of sentinel in front of block 0 and behind the last block


def _pad(planes):
    return [np.ascontiguousarray(np.pad(p, BORDER if c == 0 else BORDER // 2, mode="edge"))
            for c, p in enumerate(planes)]


class _Pass:
    """A frame pass whose level array sits between two guards of sentinels; shift: the
    offsets start that many int16 into the array (4: on 8 bytes, not on 16)."""

    def __init__(self, ctx, pw, ph, bd, qp, form, shift=0):
        from xvc_amd import pipeline
        self.ctx = ctx
        self.fp = fp = pipeline.FramePass(ctx, pw, ph, bd, qp=qp, rdoq=True, form=form)
        self.off, self.total = ctx.level_offsets(fp.desc.tx)
        self.first = GUARD + shift
        self.size = self.total + 2 * GUARD + 8
        for b in (fp.d_levels, fp.d_level_off, fp.d_coeffs):
            b.free()
        fp.d_level_off = ctx.buffer((self.off + self.first).astype(np.uint32))
        fp.d_levels = ctx.buffer(np.full(self.size, SENTINEL, np.int16))
        fp.d_coeffs = ctx.buffer(np.full(self.size, SENTINEL, np.int16))
        fp.n_levels = self.size
        ctx._check(ctx.lib.xvcgpu_quant_rdo_reserve(ctx.h, len(fp.desc.tx), self.size))

    def run(self, orig, ref, rec):
        self.fp.run(orig, ref, rec)
        self.ctx.sync()
        n = len(self.fp.desc.tx)
        res, nnz, cus, ssd = self.fp.results()
        return dict(lists=self.ctx.debug_rdoq_lists(n), res=res, nnz=nnz, cus=cus, ssd=ssd,
                    levels=self.fp.d_levels.to_array(np.int16, self.size),
                    coeffs=self.fp.d_coeffs.to_array(np.int16, self.size),
                    rec=rec.download(BORDER))

    def destroy(self):
        self.fp.destroy()


def _histogram(ent, p, out_fused, out_alone, bd):
    """Per block of a pass: candidates from the stand-alone form's coefficients (it stores
    every block's), on a list or not; the fused lists against the numpy bound."""
    d = p.fp.desc
    listed = set(int(v) for v in np.concatenate(out_fused["lists"]))
    ctxs, bins = d.rdoq_contexts, dict(zero=0, few=0, many=0, proved=0)
    for i, t in enumerate(d.tx):
        w, h = int(t["w"]), int(t["h"])
        a = p.first + int(p.off[i])
        src = out_alone["coeffs"][a:a + w * h].reshape(h, w)
        nc = n_candidates(bd, int(t["qp"]), src)
        proved = zp.proves_zero(ent, bd, int(t["qp"]), int(t["comp"]), 0, ctxs[0],
                                d.rdoq_params[i], src)
        assert (i not in listed) == (nc == 0 or proved), (i, nc, proved, w, h, int(t["comp"]))
        bins["zero" if nc == 0 else ("few" if nc <= 16 else "many")] += 1
        bins["proved"] += bool(proved)
        if i not in listed:     # taken off the lists: zeros, and a count of zero
            assert not out_fused["levels"][a:a + w * h].any(), i
            assert out_fused["nnz"][i] == 0, i
    return bins


@pytest.fixture(scope="module")
def fused_bins():
    return {}


@pytest.mark.gpu
@pytest.mark.parametrize("qp", FUSED_QPS)
@pytest.mark.parametrize("pw,ph,bd", FUSED_CASES)
def test_fused_proof_equals_standalone(world, fused_bins, pw, ph, bd, qp):
    """A chain of CHAIN passes (each reconstruction is the next reference) in form
    fwd_from_me and in form fwd_transform with the stand-alone proof forced on: identical
    class lists, equal reconstruction, counts, CU records and SSD; the lists follow the numpy
    bound; blocks off the lists hold zeros; the guards around the level array are untouched
    (the fused pass's offsets are 16-byte aligned here)."""
    from xvc_amd import api, synth
    _, ent, _ = world
    ctx = api.Context(0)
    clip = synth.SyntheticClip(pw, ph, bd)
    pics = [ctx.picture(pw, ph, bd) for _ in range(5)]
    O, Ra, Rb, Ea, Eb = pics
    fused = _Pass(ctx, pw, ph, bd, qp, None)
    alone = _Pass(ctx, pw, ph, bd, qp, "fwd_transform")
    assert fused.fp.form == "fwd_from_me" and len(fused.fp.desc.tx) == 3 * fused.fp.desc.n_cus
    bins = dict(zero=0, few=0, many=0, proved=0)
    try:
        ref = _pad(clip.frame(0))
        Ra.upload(ref, BORDER)
        Rb.upload(ref, BORDER)
        for k in range(1, CHAIN + 1):
            O.upload(_pad(clip.frame(k)), BORDER)
            ctx.set_rdoq_prove_zero(-1)
            f = fused.run(O, Ra, Ea)
            ctx.set_rdoq_prove_zero(1)
            s = alone.run(O, Rb, Eb)
            for c in range(3):
                assert np.array_equal(f["lists"][c], s["lists"][c]), (k, c)
                assert np.array_equal(f["rec"][c], s["rec"][c]), (k, c)
            assert np.array_equal(f["res"], s["res"]) and np.array_equal(f["nnz"], s["nnz"]), k
            assert f["cus"].tobytes() == s["cus"].tobytes(), k
            assert np.array_equal(f["ssd"], s["ssd"]), k
            for out, p in ((f, fused), (s, alone)):
                assert (out["levels"][:p.first] == SENTINEL).all(), k
                assert (out["levels"][p.first + p.total:] == SENTINEL).all(), k
            got = _histogram(ent, fused, f, s, bd)
            for key in bins:
                bins[key] += got[key]
            Ra, Ea = Ea, Ra
            Rb, Eb = Eb, Rb
    finally:
        ctx.set_rdoq_prove_zero(-1)
        fused.destroy()
        alone.destroy()
        for p in pics:
            p.destroy()
        ctx.close()
    print("%dx%d bd %d qp %d: %s" % (pw, ph, bd, qp, bins))
    fused_bins[(pw, ph, bd, qp)] = bins


@pytest.mark.gpu
def test_fused_cases_meet_every_kind_of_block(fused_bins):
    """Over the cases above: blocks without a candidate, with 1 ... 16, with more than 16,
    and proved ones."""
    assert len(fused_bins) == len(FUSED_CASES) * len(FUSED_QPS)
    total = {k: sum(b[k] for b in fused_bins.values()) for k in ("zero", "few", "many", "proved")}
    print(total)
    assert all(v > 0 for v in total.values()), total


@pytest.mark.gpu
@pytest.mark.parametrize("shift", [0, 4])
def test_fused_zero_fill_keeps_to_its_blocks(shift):
    """A fused pass of a 64x40 picture (16x16 and 16x8 CUs): every block it takes off the
    lists holds zeros afterwards, listed blocks and the sentinels in front of block 0 and
    behind the last block are as they were.  shift 4: every offset on 8 bytes and not on 16
    - the 2-byte stores."""
    from xvc_amd import api, synth
    pw, ph, bd, qp = 64, 40, 10, 32
    ctx = api.Context(0)
    clip = synth.SyntheticClip(pw, ph, bd)
    O, R, E = (ctx.picture(pw, ph, bd) for _ in range(3))
    p = _Pass(ctx, pw, ph, bd, qp, None, shift)
    try:
        O.upload(_pad(clip.frame(1)), BORDER)
        R.upload(_pad(clip.frame(0)), BORDER)
        ctx.set_rdoq_prove_zero(-1)
        # the forward kernel alone: what the quantiser's walk writes afterwards is not its
        fp, d = p.fp, p.fp.desc
        steps = dict(fp.kernel_steps(O, R, E))
        steps["me_search"]()
        steps["fwd_from_me"]()
        ctx.sync()
        levels = fp.d_levels.to_array(np.int16, p.size)
        cls_off = 0
        assert (levels[:p.first] == SENTINEL).all()
        assert (levels[p.first + p.total:] == SENTINEL).all()
        steps["quant_rdo"]()
        ctx.sync()
        listed = set(int(v) for v in np.concatenate(ctx.debug_rdoq_lists(len(d.tx))))
        for i, t in enumerate(d.tx):
            a = p.first + int(p.off[i])
            blk = levels[a:a + int(t["w"]) * int(t["h"])]
            if i in listed:
                assert (blk == SENTINEL).all(), i       # left to the walk, untouched so far
            else:
                assert not blk.any(), i
                cls_off += 1
        assert 0 < cls_off < len(d.tx)
    finally:
        p.destroy()
        for q in (O, R, E):
            q.destroy()
        ctx.close()
