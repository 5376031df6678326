"""DeblockingFilter::DeblockPicture (deblocking_filter.cc:56-450) restated in plain Python
integers, with a counter on every decision the filter takes.

The vertical pass, then the horizontal pass, each over the sub-block positions in raster
order: along a band of four lines that is the order of the reference's CTU walk, so the
chains of edges four samples apart (4-wide / 4-tall CUs) come out as they do there.  Luma
and 4:2:0 chroma, sub-block size 4 (kSubblockSizeExt) and 8 (kSubblockSize), one CU tree.
Two table indices lie outside the reference's tables, which it reads past; the project
defines them as oracle/xvc_oracle_pic.c does: beta index 64 -> beta 0, chroma tc index
54 -> tc 0.  tests/test_deblock_model.py pins this file to the oracle on every case of
tests/deblock_cases.py, and the oracle to the reference's own code on the cases that stay
inside its tables.

deblock_picture() returns the filtered planes and a collections.Counter; its keys, each
prefixed with the pass ("v." vertical edges, "h." horizontal edges):

  bs.*      why GetBoundaryStrength returned what it did: intra, cbf; in P pictures
            uni_ref (list-0 indices differ), uni_far / uni_near (a vector component
            differs by >= 16 / none does); in B pictures bi_refs (the POC pairs differ),
            bi_straight_far / _near (rp0 == rq0, cond1), bi_swapped_far / _near (cond2),
            bi_same_<c1><c2> (both of P's POCs equal: cond1 && cond2)
  corner.*  the corner vectors compared, <P's corner><Q's corner>, wherever vectors are
  luma.bs<1|2>.*  a group of four lines: off (d >= beta), strong, normal_<p1><q1>
            (the weak filter with filter_p1 / filter_q1)
  line.*    a line of the weak filter skipped (|delta| >= 10 tc), its delta clipped at
            +-tc, a ClipBD of it saturating at 0 (sat_zero) or at the maximum (sat_max);
            a difference of the strong filter clipped at +-2 tc (strong_clipped)
  chroma.*  a chroma line filtered, its delta clipped at +-tc, a ClipBD saturating
  clip.*    a table index clipped: beta_neg, beta_64, tc_neg, tc_over (> 53), ctc_neg,
            ctc_54 (chroma); tc_over_binds: a line of such a group at which a clip at
            +-tc or +-2 tc binds, so that the value of the table's last entry shows in the
            result (reaching the index alone does not pin it)

What the case set of tests/deblock_cases.py reaches (sub-block size 4; per family of
partitions, vertical / horizontal pass; test_census_floor asserts at least FLOOR = 8 of
every key, on all cases and on those compared with the reference):

  key                           g4 all v/h      g4 cmp v/h      g8 all v/h      g8 cmp v/h
  bs.intra                       4698/4262       3838/3608       2590/2468       2064/2016
  bs.cbf                         5406/5506       4258/4447       3352/3358       2706/2716
  bs.uni_ref                       963/932         717/760         498/586         360/434
  bs.uni_far                       844/774         631/600         457/424         349/340
  bs.uni_near                      406/388         344/325         201/230         139/182
  bs.bi_refs                     2446/2396       2086/2045       1356/1302       1116/1054
  bs.bi_straight_far               305/330         241/279         225/246         181/192
  bs.bi_straight_near                55/74           49/61           29/34           25/32
  bs.bi_swapped_far                312/229         267/197         124/171         114/146
  bs.bi_swapped_near                 61/38           58/36           18/33           18/32
  bs.bi_same_00                      59/28           57/27           22/30           22/30
  bs.bi_same_01                      18/29           18/29           14/24           14/24
  bs.bi_same_10                      25/29           25/28           26/14           26/14
  bs.bi_same_11                    197/193         187/190          96/106          90/106
  corner.dlul                       -/1322          -/1100           -/504           -/416
  corner.dlur                        -/194           -/162           -/147           -/128
  corner.drdl                        454/-           379/-           452/-           362/-
  corner.drul                      225/215         175/181         157/146         123/120
  corner.drur                        -/381           -/329           -/515           -/434
  corner.urdl                        212/-           180/-           162/-           135/-
  corner.urul                       1391/-          1143/-           441/-           358/-
  luma.bs1.off                   2103/2042         737/838       1261/1298         485/497
  luma.bs1.strong                4163/4128       4124/4098       2576/2541       2551/2504
  luma.bs1.normal_00               345/264         333/248         108/101           98/97
  luma.bs1.normal_01               583/500         541/472         344/338         318/309
  luma.bs1.normal_10               462/494         428/464         313/263         293/240
  luma.bs1.normal_11             2817/2932       2224/2398       1506/1652       1171/1341
  luma.bs2.off                     947/797         375/396         644/522         241/190
  luma.bs2.strong                2104/1816       2091/1810       1271/1139       1261/1131
  luma.bs2.normal_00               135/101          124/94           25/44           20/39
  luma.bs2.normal_01               215/186         199/173          84/102           77/91
  luma.bs2.normal_10               193/157         179/149           73/83           70/77
  luma.bs2.normal_11             1104/1205         870/986         493/578         395/488
  line.skipped                 10099/10484       6595/7308       5504/5399       3640/3723
  line.delta_clipped             5946/5761       5930/5761       3592/4009       3592/4009
  line.strong_clipped            1773/1713       1773/1713       2037/2304       2037/2304
  line.sat_zero                     158/76          145/76           50/54           40/49
  line.sat_max                      111/79          111/78           37/47           34/43
  chroma.filtered                8720/7928       7016/6712       7056/7056       5584/5728
  chroma.delta_clipped           3378/3385       2323/2558       3286/3120       2344/2248
  chroma.saturated                   49/37           43/33           16/52           15/50
  clip.beta_neg                    788/717         186/207         604/574         159/164
  clip.beta_64                     801/653             0/0         363/385             0/0
  clip.tc_neg                    1408/1489         602/766         797/811         386/424
  clip.tc_over                   3412/3004       3280/2907       1634/1658       1561/1553
  clip.tc_over_binds                112/78           96/78           49/32           49/32
  clip.ctc_neg                     203/208         108/118         254/256         178/184
  clip.ctc_54                      165/110             0/0         190/158             0/0

TEST INFRASTRUCTURE."""
import collections

import numpy as np

TC_TABLE = [0] * 18 + [1] * 9 + [2] * 4 + [3] * 4 + [4] * 3 + [5, 5, 6, 6, 7, 8, 9, 10, 11, 13,
                                                              14, 16, 18, 20, 22, 24]
BETA_TABLE = [0] * 16 + list(range(6, 19)) + list(range(20, 90, 2))
assert len(TC_TABLE) == 54 and len(BETA_TABLE) == 64 and BETA_TABLE[63] == 88
UL, UR, DL, DR = 0, 1, 2, 3     # XVC_CORNER_*
CORNER = ["ul", "ur", "dl", "dr"]

BS_KEYS = ["bs.intra", "bs.cbf", "bs.uni_ref", "bs.uni_far", "bs.uni_near", "bs.bi_refs",
           "bs.bi_straight_far", "bs.bi_straight_near", "bs.bi_swapped_far",
           "bs.bi_swapped_near", "bs.bi_same_00", "bs.bi_same_01", "bs.bi_same_10",
           "bs.bi_same_11"]
CORNER_KEYS = {"v": ["corner.urul", "corner.urdl", "corner.drul", "corner.drdl"],
               "h": ["corner.dlul", "corner.dlur", "corner.drul", "corner.drur"]}
LUMA_KEYS = ["luma.bs%d.%s" % (bs, o) for bs in (1, 2)
             for o in ("off", "strong", "normal_00", "normal_01", "normal_10", "normal_11")]
LINE_KEYS = ["line.skipped", "line.delta_clipped", "line.strong_clipped", "line.sat_zero",
             "line.sat_max"]
CHROMA_KEYS = ["chroma.filtered", "chroma.delta_clipped", "chroma.saturated"]
CLIP_KEYS = ["clip.beta_neg", "clip.beta_64", "clip.tc_neg", "clip.tc_over",
             "clip.tc_over_binds", "clip.ctc_neg", "clip.ctc_54"]
# the two indices outside the reference's tables
UNDEFINED_IN_REFERENCE = ("clip.beta_64", "clip.ctc_54")


def census_keys():
    """Every key of the census, both passes."""
    return [p + "." + k for p in ("v", "h")
            for k in BS_KEYS + CORNER_KEYS[p] + LUMA_KEYS + LINE_KEYS + CHROMA_KEYS + CLIP_KEYS]


def clip3(v, lo, hi):
    return lo if v < lo else (hi if v > hi else v)


class _Filter:
    def __init__(self, bd, pw, ph, bipred, beta_off, tc_off, sub, cus, cu_map, planes,
                 comp_mask):
        self.bd, self.pw, self.ph, self.bipred = bd, pw, ph, bipred
        self.beta_off, self.tc_off, self.sub, self.comp_mask = beta_off, tc_off, sub, comp_mask
        self.cus = [dict(zip(cus.dtype.names, c)) for c in cus.tolist()]
        self.map = np.asarray(cu_map).tolist()
        self.planes = [np.asarray(p).astype(np.int64).tolist() for p in planes]
        self.smax = (1 << bd) - 1
        self.n = collections.Counter()
        self.tc_over = False
        self.pre = ""

    def count(self, key, k=1):
        if k:
            self.n[self.pre + key] += k

    def cu_at(self, x, y):
        """PictureData::GetCuAt (picture_data.h:102-107); x - 1 / y - 1 == -1 lands in cell
        0, the same CU, by C's truncating division."""
        x, y = max(x, 0), max(y, 0)
        if y >> 2 >= len(self.map) or x >> 2 >= len(self.map[0]):
            return None
        i = self.map[y >> 2][x >> 2]
        return None if i < 0 else self.cus[i]

    def clip_bd(self, v):
        if v < 0:
            self.count("line.sat_zero")
            return 0
        if v > self.smax:
            self.count("line.sat_max")
            return self.smax
        return v

    def boundary_strength(self, p, q, x, y, vertical):
        """GetBoundaryStrength, deblocking_filter.cc:154-241 (default restrictions)."""
        if vertical:
            cp = UR if y - p["y"] < p["h"] >> 1 else DR
            cq = UL if y - q["y"] < q["h"] >> 1 else DL
        else:
            cp = DL if x - p["x"] < p["w"] >> 1 else DR
            cq = UL if x - q["x"] < q["w"] >> 1 else UR
        if p["intra"] or q["intra"]:
            self.count("bs.intra")
            return 2
        if p["cbf_luma"] or q["cbf_luma"]:
            self.count("bs.cbf")
            return 1

        def far(a, b):
            return abs(a[0] - b[0]) >= 16 or abs(a[1] - b[1]) >= 16

        if self.bipred:
            (rp0, rp1), (rq0, rq1) = p["ref_poc"], q["ref_poc"]
            if not ((rp0 == rq0 and rp1 == rq1) or (rp0 == rq1 and rp1 == rq0)):
                self.count("bs.bi_refs")
                return 1
            self.count("corner." + CORNER[cp] + CORNER[cq])
            p0, p1 = p["mv"][0][cp], p["mv"][1][cp]
            q0, q1 = q["mv"][0][cq], q["mv"][1][cq]
            cond1 = far(p0, q0) or far(p1, q1)
            cond2 = far(p0, q1) or far(p1, q0)
            if rp0 != rp1:
                if rp0 == rq0:
                    self.count("bs.bi_straight_" + ("far" if cond1 else "near"))
                    return int(cond1)
                self.count("bs.bi_swapped_" + ("far" if cond2 else "near"))
                return int(cond2)
            self.count("bs.bi_same_%d%d" % (cond1, cond2))
            return int(cond1 and cond2)
        if p["ref_idx0"] != q["ref_idx0"]:
            self.count("bs.uni_ref")
            return 1
        self.count("corner." + CORNER[cp] + CORNER[cq])
        if far(p["mv"][0][cp], q["mv"][0][cq]):
            self.count("bs.uni_far")
            return 1
        self.count("bs.uni_near")
        return 0

    # a sample across / along the edge: k = -4 .. 3 is p3 .. q3, i the line
    def _get(self, pl, x, y, vertical, i, k):
        return pl[y + i][x + k] if vertical else pl[y + k][x + i]

    def _put(self, pl, x, y, vertical, i, k, v):
        if vertical:
            pl[y + i][x + k] = v
        else:
            pl[y + k][x + i] = v

    def filter_edge_luma(self, x, y, vertical, bs, qp):
        """FilterEdgeLuma with the weak and the strong filter, :243-401."""
        pl, bsh = self.planes[0], self.bd - 8
        for g in range(self.sub // 4):
            gx, gy = (x, y + 4 * g) if vertical else (x + 4 * g, y)
            s = [[self._get(pl, gx, gy, vertical, i, k) for k in range(-4, 4)] for i in range(4)]
            index_beta = qp + self.beta_off
            if index_beta < 0:
                self.count("clip.beta_neg")
            if index_beta >= 64:
                self.count("clip.beta_64")
            index_beta = clip3(index_beta, 0, 64)
            beta = (BETA_TABLE[index_beta] if index_beta < 64 else 0) << bsh
            dp0, dq0 = (abs(s[0][1] - 2 * s[0][2] + s[0][3]), abs(s[0][4] - 2 * s[0][5] + s[0][6]))
            dp3, dq3 = (abs(s[3][1] - 2 * s[3][2] + s[3][3]), abs(s[3][4] - 2 * s[3][5] + s[3][6]))
            d0, d3 = dp0 + dq0, dp3 + dq3
            key = "luma.bs%d." % bs
            if d0 + d3 >= beta:
                self.count(key + "off")
                continue
            index_tc = qp + self.tc_off + 2 * (bs - 1)
            if index_tc < 0:
                self.count("clip.tc_neg")
            if index_tc > 53:
                self.count("clip.tc_over")
            tc = TC_TABLE[clip3(index_tc, 0, 53)] << bsh
            self.tc_over = index_tc > 53
            strong = (d0 << 1) < (beta >> 2) and (d3 << 1) < (beta >> 2)
            for e in (0, 3):     # CheckStrongFilter :314-323
                p3, p0, q0, q3 = s[e][0], s[e][3], s[e][4], s[e][7]
                strong = strong and abs(p3 - p0) + abs(q0 - q3) < (beta >> 3) and \
                    abs(p0 - q0) < ((tc * 5 + 1) >> 1)
            if strong:
                self.count(key + "strong")
                for i in range(4):
                    self._strong_line(s[i], 2 * tc)
            else:
                side = (beta + (beta >> 1)) >> 3
                filter_p1, filter_q1 = dp0 + dp3 < side, dq0 + dq3 < side
                self.count(key + "normal_%d%d" % (filter_p1, filter_q1))
                for i in range(4):
                    self._weak_line(s[i], tc, filter_p1, filter_q1)
            for i in range(4):
                for k in range(-3, 3):
                    self._put(pl, gx, gy, vertical, i, k, s[i][k + 4])

    def _strong_line(self, t, tc2):
        """FilterLumaStrong :368-401; Sample + Sample(Clip3(..)) wraps modulo 2^16 there,
        which no valid sample reaches (asserted)."""
        p3, p2, p1, p0, q0, q1, q2, q3 = t
        new = [(2 * p3 + 3 * p2 + p1 + p0 + q0 + 4) >> 3,
               (p2 + p1 + p0 + q0 + 2) >> 2,
               (p2 + 2 * p1 + 2 * p0 + 2 * q0 + q1 + 4) >> 3,
               (p1 + 2 * p0 + 2 * q0 + 2 * q1 + q2 + 4) >> 3,
               (p0 + q0 + q1 + q2 + 2) >> 2,
               (p0 + q0 + q1 + 3 * q2 + 2 * q3 + 4) >> 3]
        for k, nv in enumerate(new):
            old = t[1 + k]
            if abs(nv - old) > tc2:
                self.count("line.strong_clipped")
                self.count("clip.tc_over_binds", int(self.tc_over))
            v = old + clip3(nv - old, -tc2, tc2)
            assert 0 <= v <= self.smax
            t[1 + k] = v & 0xffff

    def _weak_line(self, t, tc, filter_p1, filter_q1):
        """FilterLumaWeak :325-366."""
        p2, p1, p0, q0, q1, q2 = t[1:7]
        delta = (9 * (q0 - p0) - 3 * (q1 - p1) + 8) >> 4
        if abs(delta) >= tc * 10:
            self.count("line.skipped")
            return
        if abs(delta) > tc:
            self.count("line.delta_clipped")
            self.count("clip.tc_over_binds", int(self.tc_over))
        delta = clip3(delta, -tc, tc)
        t[3] = self.clip_bd(p0 + delta)
        t[4] = self.clip_bd(q0 - delta)
        half_tc = tc >> 1
        if filter_p1:
            t[2] = self.clip_bd(p1 + clip3((((p2 + p0 + 1) >> 1) - p1 + delta) >> 1,
                                           -half_tc, half_tc))
        if filter_q1:
            t[5] = self.clip_bd(q1 + clip3((((q2 + q0 + 1) >> 1) - q1 - delta) >> 1,
                                           -half_tc, half_tc))

    def filter_edge_chroma(self, cx, cy, vertical, qp):
        """FilterEdgeChroma / FilterChroma<N>, :403-450 (4:2:0)."""
        index_tc = qp + self.tc_off + 2
        if index_tc < 0:
            self.count("clip.ctc_neg")
        if index_tc >= 54:
            self.count("clip.ctc_54")
        index_tc = clip3(index_tc, 0, 54)
        tc = (TC_TABLE[index_tc] if index_tc < 54 else 0) << (self.bd - 8)
        for c in (1, 2):
            pl = self.planes[c]
            for i in range(self.sub >> 1):
                p1, p0, q0, q1 = (self._get(pl, cx, cy, vertical, i, k) for k in range(-2, 2))
                delta = (((q0 - p0) * 4) + p1 - q1 + 4) >> 3
                self.count("chroma.filtered")
                if abs(delta) > tc:
                    self.count("chroma.delta_clipped")
                delta = clip3(delta, -tc, tc)
                for k, v in ((-1, p0 + delta), (0, q0 - delta)):
                    if v < 0 or v > self.smax:
                        self.count("chroma.saturated")
                    self._put(pl, cx, cy, vertical, i, k, clip3(v, 0, self.smax))

    def run_pass(self, vertical, y_begin=0, y_end=None):
        """DeblockCtu :79-152 at every sub-block position of rows [y_begin, y_end)."""
        self.pre = "v." if vertical else "h."
        y_end = self.ph if y_end is None else min(y_end, self.ph)
        for y in range(y_begin, y_end, self.sub):
            for x in range(0, self.pw, self.sub):
                q = self.cu_at(x, y)
                if q is None:
                    continue
                p = self.cu_at(x - 1, y) if vertical else self.cu_at(x, y - 1)
                if p is None or (p["x"] == q["x"] and p["y"] == q["y"]):
                    continue
                bs = self.boundary_strength(p, q, x, y, vertical)
                if not bs:
                    continue
                if self.comp_mask & 1:
                    self.filter_edge_luma(x, y, vertical, bs, (p["qp_y"] + q["qp_y"] + 1) >> 1)
                if bs == 2 and self.comp_mask & 2:
                    cx, cy = x >> 1, y >> 1
                    if (cx & 7) == 0 if vertical else (cy & 7) == 0:
                        self.filter_edge_chroma(cx, cy, vertical,
                                                (p["qp_c"] + q["qp_c"] + 1) >> 1)


def deblock_picture(bd, pw, ph, bipred, beta_off, tc_off, sub, cus, cu_map, planes,
                    comp_mask=3):
    """planes: the picture's three planes (2-D arrays, no border; left untouched).  Returns
    (the filtered planes as uint16 arrays, the Counter of decisions)."""
    f = _Filter(bd, pw, ph, bipred, beta_off, tc_off, sub, cus, cu_map, planes, comp_mask)
    f.run_pass(True)
    f.run_pass(False)
    return [np.array(p, np.uint16) for p in f.planes], f.n
