"""Directed gate tests of the HIP stereo matcher (k_stereo_rows / k_stereo_match, stereo_kernels.hip) against the oracle.

The scene tests of test_stereo_gpu.py reach a gate only where a scene happens to put a keypoint.  Here the keypoint and
descriptor lists are hand-made (stereo_gate_cases.py): every gate of Frame::ComputeStereoMatches gets one left keypoint on
its last accepted value and one on its first rejected value.  Each call also carries the pair's extracted keypoints, a
few hundred ordinary matches, so that the median of the SADs is positive and the closing median cut keeps the case under
test; that, and the intended outcome of every hand-made keypoint (depth > 0 on the accepted side, -1 on the other), is
asserted from the oracle's output alone before uRight, depth and SAD of the product are compared with it bit for bit.

The pairs.  "small" is 320 x 241: 241 and not 240 rows because the band of a right keypoint of octave 7 that is clipped at the
last row reaches a left keypoint whose 11-row window still fits level 6 only if that level keeps 81 rows.  "tall" is
1104 x 2050: more than kStereoMaxRows = 2048 rows, so launch_stereo_match takes k_stereo_match<false>, the form without row
lists (rows as int16_t in RightRec, all right keypoints staged in LDS); every gate case runs on both pairs.  It cannot be much
narrower: DistributeOctTree starts from round(width / height) nodes of the keypoint area (ORBextractor.cc), which is 0 for an
area more than twice as tall as wide, and the reference then indexes an empty vector; level 7 of 2050 rows needs 1088 columns.

Safety.  Every hand-made keypoint keeps all windows that either side reads inside the level image (Geometry.safe):
round(x * inv_scale) +- 5 and round(y * inv_scale) +- 5 on the left, round(uR0 * inv_scale) +- 10 on the right.  The reference
itself reads outside the image when scaleduR0 < 10 (its check is iniu < 0 with iniu = scaleduR0, while the window starts at
scaleduR0 - 10); that region is out of scope here, as are more than 4096 right keypoints (rejected, see test_too_many_right_keypoints).

The order inside a row list of k_stereo_rows is set by LDS atomics and cannot be dictated from outside, so "the smaller index
comes later in the list" is approached from both forms: in k_stereo_match<false> list order is index order, and in the row-list
form the tied pair sits in different waves and trips of k_stereo_rows (test_descriptor_threshold_and_ties)."""
import numpy as np
import pytest

from stereo_gate_cases import SHIFT, SYM_COL, SYM_ROWS, Batch, Geometry, find_sites, keypoint, shifted_pair, sparse_pair

pytestmark = pytest.mark.gpu
f32 = np.float32
BF, B = 32.0, 0.5  # maxD = 64


class Pair:
    """One extracted pair: the oracle side is complete on its own (oracle=...), the product side is added by the fixture."""

    def __init__(self, oracle, left, right, nfeat=500):
        self.oracle, self.left, self.right = oracle, left, right
        self.h, self.w = left.shape
        self.ol, self.orr = oracle.OrbOracle(nfeatures=nfeat), oracle.OrbOracle(nfeatures=nfeat)
        _, self.kl, self.dl = self.ol.extract(left)
        _, self.kr, self.dr = self.orr.extract(right)
        self.levels_l = [self.ol.level(l) for l in range(8)]
        self.levels_r = [self.orr.level(l) for l in range(8)]
        scale = self.ol.tables()[0]
        self.geom = Geometry(scale, f32(1.0) / scale, [(lv.shape[1], lv.shape[0]) for lv in self.levels_l])
        self._sites = {}
        self.el = self.er = None
        sads = oracle.stereo_match(self.ol, self.orr, self.kl, self.dl, self.kr, self.dr, BF, B)[2]
        self.max_sad = 1.5 * float(np.median(sads[sads >= 0])) if (sads >= 0).any() else 0.0  # the cut is at 2.1 medians

    def attach(self, pkg, nfeat=500):
        self.pkg = pkg
        self.el = pkg.OrbExtractor(nfeatures=nfeat, max_width=self.w, max_height=self.h, max_images=1)
        self.er = pkg.OrbExtractor(nfeatures=nfeat, max_width=self.w, max_height=self.h, max_images=1)
        _, kl, dl = self.el.extract(self.left)
        _, kr, dr = self.er.extract(self.right)
        assert np.array_equal(dl, self.dl) and np.array_equal(dr, self.dr)
        for f in ("x", "y", "octave"):
            assert np.array_equal(kl[f], self.kl[f]) and np.array_equal(kr[f], self.kr[f]), f
        assert np.array_equal(self.el.GetScaleFactors(), self.geom.scale)
        assert np.array_equal(self.el.GetInverseScaleFactors(), self.geom.inv)
        assert [self.el.level_size(l) for l in range(8)] == self.geom.sizes
        return self

    def sites(self, level, want, tag="", **kw):
        """find_sites, once per (level, want, tag): `tag` names the restriction that **kw states."""
        key = (level, want, tag)
        if key not in self._sites:
            self._sites[key] = find_sites(self.geom, self.levels_l, self.levels_r, level, want, self.max_sad, **kw)
        return self._sites[key]

    def left_kp(self, site, level, fx=0.0):
        return keypoint(self.geom.coord(site[0], level, fx), self.geom.coord(site[1], level), level)

    def right_kp(self, site, level, shift=0, octave=None, y=None):
        """A right keypoint `shift` level pixels from the site's best column (level = the left keypoint's octave)."""
        return keypoint(self.geom.coord(site[2] + shift, level), self.geom.coord(site[1], level) if y is None else y,
                        level if octave is None else octave)

    def fillers(self, batch, n, y=None, octave=None, x_to=None):
        """Right keypoints with random descriptors: candidates that never win.  Their columns keep every window inside at any level."""
        rng = batch.rng
        for _ in range(n):
            x = f32(rng.uniform(40, min(self.w - 48, x_to if x_to is not None else self.w)))
            batch.right(keypoint(x, f32(rng.uniform(8, self.h - 9)) if y is None else y, int(rng.integers(0, 8)) if octave is None else octave),
                        batch.descriptor())

    def run(self, batch, bf=BF, b=B, real_first=False):
        """The oracle's verdict on the hand-made keypoints (asserted), then the product's output compared with it bit for bit."""
        hl, hdl, hr, hdr = batch.arrays()
        kl, dl = np.concatenate([hl, self.kl]), np.concatenate([hdl, self.dl])
        order = (self.kr, hr) if real_first else (hr, self.kr)
        kr, dr = np.concatenate(order), np.concatenate((self.dr, hdr) if real_first else (hdr, self.dr))
        want = self.oracle.stereo_match(self.ol, self.orr, kl, dl, kr, dr, bf, b)
        sads = np.sort(want[2][want[2] >= 0])
        assert len(sads) > 30 and sads[len(sads) // 2] > 0, "the median SAD must be positive"
        for i, (name, acc) in enumerate(zip(batch.names, batch.expect)):
            if acc:
                assert want[1][i] > 0 and want[0][i] >= 0, (name, want[0][i], want[1][i], want[2][i])
            else:
                assert want[1][i] == -1 and want[0][i] == -1, (name, want[0][i], want[1][i], want[2][i])
        if self.el is not None:
            got = self.pkg.compute_stereo_matches(self.el, self.er, kl, dl, kr, dr, bf, b)
            assert np.array_equal(got[2], want[2]), "SAD"
            assert np.array_equal(got[0], want[0]), "uRight"
            assert np.array_equal(got[1], want[1]), "depth"
        return want


SIZES = {"small": (320, 241), "tall": (1104, 2050)}


def make_pair(oracle, which):
    w, h = SIZES[which]
    return Pair(oracle, *shifted_pair(11 if which == "small" else 12, w, h))


@pytest.fixture(scope="module", params=["small", "tall"])
def pair(request, pkg, oracle):
    p = make_pair(oracle, request.param).attach(pkg)
    yield p
    p.el.close(); p.er.close()


# ---- 1. the row band ------------------------------------------------------------------------------------------------
def build_row_band(p):
    g, b = p.geom, Batch(p.geom, 1)
    for o, lo in ((0, 0), (3, 3), (7, 6)):  # right octave, left octave (level 6 holds the pair's shift as 3.01 pixels: small SADs)
        r = f32(2.0) * g.scale[o]
        for site, (name, dy, edge, delta, acc) in zip(p.sites(lo, 4), [("floor(y-r)", r + f32(0.25), 0, 0, True), ("floor(y-r)-1", r + f32(1.25), 0, 1, False),
                                                                        ("ceil(y+r)", -r - f32(0.25), 1, 0, True), ("ceil(y+r)+1", -r - f32(1.25), 1, -1, False)]):
            kl = p.left_kp(site, lo)
            row = int(kl["y"])
            yr = f32(f32(row) + dy)
            assert yr != np.floor(yr) and g.band(yr, o)[edge] == row + delta, (o, name)
            b.pair("octave %d row %s" % (o, name), kl, p.right_kp(site, lo, octave=o, y=yr), acc)
    # bands clipped to the image: a right keypoint of octave 7 within r of the first / last row, the left one of octave 6
    r = f32(2.0) * g.scale[7]
    for name, yr, edge, inside in (("clipped at row 0", f32(r - f32(0.05)), 1, -1), ("clipped at the last row", f32(f32(p.h - 1) - r + f32(0.05)), 0, 1)):
        lo, hi = g.band(yr, 7)
        assert (lo < 0) if edge == 1 else (hi > p.h - 1), name
        last = (lo, hi)[edge]  # the band's last row on the side that is not clipped
        for acc, row in ((True, last), (False, last - inside)):
            y = f32(row + 0.3)
            site = p.sites(6, 1, tag="row %d" % row, vls=[g.level_px(y, 6)], uls=range(16, g.sizes[6][0] - 12, 3))[0]
            kl = keypoint(g.coord(site[0], 6), y, 6)
            assert int(kl["y"]) == row
            b.pair("%s, row %d" % (name, row), kl, p.right_kp(site, 6, octave=7, y=yr), acc)
    return b


def test_row_band(pair):
    """Right octaves 0, 3 and 7 with non-integer y: the left row on floor(y - r) and on ceil(y + r) is a candidate, one row further
    out is none; and a band clipped at row 0 / at the last row (max(0, .) and min(rows - 1, .) in k_stereo_rows, negative and
    too large int16 rows in RightRec) still holds its last row and not the next."""
    pair.run(build_row_band(pair))


# ---- 2. the octave gate ---------------------------------------------------------------------------------------------
def build_octave_gate(p):
    b = Batch(p.geom, 2)
    for lo in (0, 4, 7):
        site = p.sites(lo, 1)[0]
        for d in (-2, -1, 0, 1, 2):
            if 0 <= lo + d <= 7:
                b.pair("left octave %d, right octave %+d" % (lo, d), p.left_kp(site, lo), p.right_kp(site, lo, octave=lo + d), abs(d) <= 1)
    return b


def test_octave_gate(pair):
    """Right octave = left - 2 ... left + 2 at left octaves 0, 4 and 7: only -1, 0, +1 are candidates."""
    pair.run(build_octave_gate(pair))


# ---- 3. the disparity window ----------------------------------------------------------------------------------------
def build_disparity_window(p, max_d):
    g, b = p.geom, Batch(p.geom, 3)
    # uR == minU: the right keypoint lies max_d left of the left one, two pixels left of the true correspondence (SHIFT = max_d - 2)
    site = p.sites(0, 1)[0]
    kl = p.left_kp(site, 0, 0.25)
    min_u = f32(kl["x"] - f32(max_d))
    assert g.level_px(min_u, 0) == site[2] - 2
    b.pair("uR == minU", kl, keypoint(min_u, kl["y"], 0), True)
    b.pair("uR just below minU", kl, keypoint(np.nextafter(min_u, f32(-np.inf)), kl["y"], 0), False)
    # uR == uL: on octave 6 the true correspondence is 3 level pixels left of the left keypoint, within the SAD search
    site = p.sites(6, 1)[0]
    kl = p.left_kp(site, 6)
    assert 1 <= site[0] - site[2] <= 4
    b.pair("uR == uL", kl, keypoint(kl["x"], kl["y"], 6), True)
    b.pair("uR just above uL", kl, keypoint(np.nextafter(kl["x"], f32(np.inf)), kl["y"], 6), False)
    return b


def test_disparity_window(pair):
    """uR on minU = uL - maxD and on uL is a candidate, the neighbouring float outside is none (maxD = SHIFT + 2)."""
    max_d = SHIFT + 2
    pair.run(build_disparity_window(pair, max_d), bf=float(max_d) * 0.5, b=0.5)


def build_max_disparity(p):
    b = Batch(p.geom, 4)
    site = p.sites(0, 1)[0]
    return b, b.pair("refined disparity against maxD", p.left_kp(site, 0), p.right_kp(site, 0, shift=2), True)  # uR stays right of minU


def test_max_disparity(pair):
    """`disparity < max_d`: with maxD the next float above the keypoint's refined disparity it is accepted, with maxD equal to
    it rejected.  The disparity is read from the oracle's result at a wide maxD (uL - uRight, the expression of both sides)."""
    b, i = build_max_disparity(pair)
    want = pair.run(b)
    disparity = f32(b.kl[i]["x"] - want[0][i])
    assert SHIFT - 1 < disparity < SHIFT + 1
    pair.run(b, bf=float(np.nextafter(disparity, f32(np.inf))), b=1.0)
    b.expect[i] = False
    pair.run(b, bf=float(disparity), b=1.0)


# ---- 4. the descriptor threshold and ties ---------------------------------------------------------------------------
def build_descriptor(p):
    b = Batch(p.geom, 5)
    s = p.sites(0, 4, tag="room for fillers", ok=lambda ul, vl, us: ul >= 56)
    b.pair("74 bits", p.left_kp(s[0], 0), p.right_kp(s[0], 0), True, flip=74)
    b.pair("75 bits", p.left_kp(s[1], 0), p.right_kp(s[1], 0), False, flip=75)
    # ties: A sits on the true correspondence (accepted if it wins), B five level pixels to its right (bestInc == -5: rejected if it
    # wins), both ten bits from the left descriptor; fillers on the same row put them 64 / 128 places apart
    for site, gap, a_first in ((s[2], 64, True), (s[3], 128, False)):
        kl, d = p.left_kp(site, 0), b.descriptor()
        ka, kb = p.right_kp(site, 0), p.right_kp(site, 0, shift=5)
        assert b.geom.safe(kl, ka) and b.geom.safe(kl, kb) and kb["x"] <= kl["x"]
        first = b.right(ka if a_first else kb, Batch.flipped(d, 10, b.rng))
        p.fillers(b, gap - 1, y=kl["y"], octave=0, x_to=float(kl["x"]))
        second = b.right(kb if a_first else ka, Batch.flipped(d, 10, b.rng))
        assert second - first == gap
        b.left("tie %d apart, the true correspondence %s" % (gap, "first" if a_first else "second"), kl, d, a_first)
    return b


def test_descriptor_threshold_and_ties(pair):
    """Best distance 74 is accepted and 75 rejected (exactly that many bits flipped); of two candidates at equal distance the smaller
    right index wins, 64 and 128 places apart on one row (different trips of the lane-strided loops, different waves of k_stereo_rows)."""
    pair.run(build_descriptor(pair))


# ---- 5. long lists --------------------------------------------------------------------------------------------------
def build_long_lists(p, n_right):
    """More than 64 and more than 128 candidates on one row with the best one behind them, then fillers on all rows up to n_right
    right keypoints (extracted ones included, placed first), and a match whose right keypoint is the very last index."""
    b = Batch(p.geom, 6)
    s = p.sites(0, 3, tag="room for fillers", ok=lambda ul, vl, us: ul >= 56)
    for site, n in ((s[0], 70), (s[1], 135)):
        kl, d = p.left_kp(site, 0), b.descriptor()
        p.fillers(b, n, y=kl["y"], octave=0, x_to=float(kl["x"]))
        b.right(p.right_kp(site, 0), Batch.flipped(d, 10, b.rng))
        b.left("best after %d candidates" % n, kl, d, True)
    p.fillers(b, n_right - len(p.kr) - len(b.kr) - 1)
    last = b.pair("right index %d" % (n_right - 1), p.left_kp(s[2], 0), p.right_kp(s[2], 0), True)
    assert len(b.kr) + len(p.kr) == n_right
    return b, last


def test_long_lists(pair):
    """Rows with more than 64 and 128 candidates (the best in the last trip), and the full 4096 right keypoints with index 4095 matched."""
    b, _ = build_long_lists(pair, 4096)
    pair.run(b, real_first=True)


def test_too_many_right_keypoints(pair, pkg):
    """4097 right keypoints: the invalid-argument error, and nothing written to the outputs."""
    b, _ = build_long_lists(pair, 4097)
    hl, hdl, hr, hdr = b.arrays()
    kr, dr = np.ascontiguousarray(np.concatenate([pair.kr, hr])), np.ascontiguousarray(np.concatenate([pair.dr, hdr]))
    assert len(kr) == 4097
    with pytest.raises(pkg.capi.Tc2liError) as e:
        pkg.compute_stereo_matches(pair.el, pair.er, hl, hdl, kr, dr, BF, B)
    assert "4096" in str(e.value)
    u, d, s = np.full(len(hl), 7, f32), np.full(len(hl), 7, f32), np.full(len(hl), 7, np.int32)
    rc = pkg.capi.lib().tc2li_stereo_match(pair.el._h, pair.er._h, hl.ctypes.data, hdl.ctypes.data, len(hl), kr.ctypes.data, dr.ctypes.data,
                                           len(kr), BF, B, u.ctypes.data, d.ctypes.data, s.ctypes.data)
    assert rc == e.value.code < 0
    assert np.all(u == 7) and np.all(d == 7) and np.all(s == 7)


# ---- 6. the SAD search ----------------------------------------------------------------------------------------------
def build_sad_search(p):
    g, b = p.geom, Batch(p.geom, 7)
    for lv in (0, 3):
        site = p.sites(lv, 1, ok=lambda ul, vl, us: ul - us >= 5, tag="room")[0]
        for shift in (-4, 4, -5, 5):  # bestInc = -shift
            kl, kr = p.left_kp(site, lv), p.right_kp(site, lv, shift=shift)
            assert kr["x"] <= kl["x"]
            b.pair("level %d, %+d pixels from the true correspondence" % (lv, shift), kl, kr, abs(shift) < 5)
        # the right window against the image's last columns: endu = scaleduR0 + 11 >= width rejects
        w = g.sizes[lv][0]
        site = p.sites(lv, 1, uls=range(w - 12, w - 5), vls=range(6, g.sizes[lv][1] - 6, 3), ok=lambda ul, vl, us, w=w: w - 15 <= us <= w - 8, tag="edge")[0]
        for col, acc in ((w - 12, True), (w - 11, False)):
            kr = keypoint(g.coord(col, lv), g.coord(site[1], lv), lv)
            assert abs(site[2] - col) <= 4  # the best column is inside the search either way: only the endu check rejects
            b.pair("level %d, scaleduR0 = width - %d" % (lv, w - col), p.left_kp(site, lv), kr, acc)
    return b


def test_sad_search(pair):
    """The right keypoint 4 level pixels either side of the best column is accepted, 5 pixels rejected (bestInc == -5 / +5), and
    scaleduR0 = width - 12 is accepted while width - 11 is rejected (endu >= width), on level 0 and on level 3."""
    pair.run(build_sad_search(pair))


# ---- 7. disparity <= 0 ----------------------------------------------------------------------------------------------
def build_zero_disparity(p):
    b = Batch(p.geom, 8)
    y = f32((SYM_ROWS[0] + SYM_ROWS[1]) // 2)
    k = keypoint(f32(SYM_COL), y, 0)
    return b, b.pair("zero disparity", k, k.copy(), True)


def test_zero_disparity(pair):
    """In the band of rows where the right image equals the left and the rows are mirror-symmetric about the keypoint's column,
    SAD(0) == 0 and SAD(-1) == SAD(+1): deltaR == 0, disparity == 0, so uRight = float(double(uL) - 0.01) and depth = bf / 0.01f.
    The rest of the pair gives a positive median, so the result survives the cut and is compared."""
    b, i = build_zero_disparity(pair)
    want = pair.run(b)
    assert want[2][i] == 0
    assert want[0][i] == f32(np.float64(f32(SYM_COL)) - 0.01)
    assert want[1][i] == f32(BF) / f32(0.01)


# ---- 8. the form without row lists on a rendered scene --------------------------------------------------------------
TALL_SCENE = (3, 1104, 2050)  # seed, width, height: the oracle accepts 994 left keypoints after the median cut


def test_tall_scene(pkg, oracle, synthetic):
    """A rendered pair of 1104 x 2050 (over kStereoMaxRows rows): extraction and k_stereo_match<false> against the oracle, which
    accepts 994 of the 2006 left keypoints after the median cut."""
    seed, w, h = TALL_SCENE
    left, right = synthetic.stereo_pair(seed, w, h)
    p = Pair(oracle, left, right, nfeat=2000).attach(pkg, nfeat=2000)
    bf = f32(synthetic.BF)
    b = f32(bf / f32(synthetic.FX))
    want = oracle.stereo_match(p.ol, p.orr, p.kl, p.dl, p.kr, p.dr, float(bf), float(b))
    assert (want[1] > 0).sum() >= 50
    got = pkg.compute_stereo_matches(p.el, p.er, p.kl, p.dl, p.kr, p.dr, float(bf), float(b))
    for g_, w_ in zip(got, want):
        assert np.array_equal(g_, w_)
    p.el.close(); p.er.close()


# ---- 9. the batch form ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_frames", [1, 3, 9])
def test_batch_form(pkg, oracle, n_frames):
    """extract_batch_dev + stereo_match_batch on 1, 3 and 9 frames of 320 x 240, one with a blank right image, one with a blank left
    image (n_left == 0: its workgroups leave at `first >= fr.n_left`), one with far fewer keypoints (the grid is sized by the
    largest frame, so its tail leaves there too); 15 workgroups a frame give counts that the XCD remap rounds up to a multiple
    of 8 (`logical >= total`).  Every frame equals the single-frame entry and the oracle."""
    import torch
    w, h, NF = 320, 240, 450  # about 455 keypoints a frame: 15 workgroups each, so 15, 45 and 135 in all -- no multiple of 8
    blank = np.full((h, w), 90, np.uint8)
    frames = []
    for f in range(n_frames):
        left, right = shifted_pair(20 + f, w, h, sym_rows=None)
        if n_frames > 1 and f == 1:
            right = blank
        if n_frames > 1 and f == 2:
            left, right = sparse_pair(20 + f, w, h)
        if f == 4:
            left = blank
        frames.append((left, right))
    n = 2 * n_frames
    dev = torch.from_numpy(np.ascontiguousarray(np.array(frames, np.uint8).reshape(n, h, w))).cuda()
    e = pkg.OrbExtractor(nfeatures=NF, max_width=w, max_height=h, max_images=n)
    kps, desc, counts, mono = e.extract_batch_dev(dev.data_ptr(), n, w, h, w, w * h)
    u, d, s = pkg.stereo_match_batch(e, n_frames, BF, B)
    el = pkg.OrbExtractor(nfeatures=NF, max_width=w, max_height=h, max_images=1)
    er = pkg.OrbExtractor(nfeatures=NF, max_width=w, max_height=h, max_images=1)
    for f, (left, right) in enumerate(frames):
        p = Pair(oracle, left, right, nfeat=NF)
        nl, nr = counts[2 * f], counts[2 * f + 1]
        assert nl == len(p.kl) and nr == len(p.kr)
        assert np.array_equal(desc[2 * f, :nl], p.dl) and np.array_equal(desc[2 * f + 1, :nr], p.dr)
        want = oracle.stereo_match(p.ol, p.orr, p.kl, p.dl, p.kr, p.dr, BF, B)
        if n_frames > 1 and f == 1:
            assert nr == 0 and nl > 100 and np.all(want[1] == -1)
        elif f == 4:
            assert nl == 0
        elif n_frames > 1 and f == 2:
            assert 0 < nl < 100 and (want[1] > 0).sum() > 5
        else:
            assert nl > 300 and (want[1] > 0).sum() > 100
        for got_f, w_ in zip((u, d, s), want):
            assert np.array_equal(got_f[f, :nl], w_)
        if nl:
            el.extract(left); er.extract(right)
            single = pkg.compute_stereo_matches(el, er, kps[2 * f, :nl], desc[2 * f, :nl], kps[2 * f + 1, :nr], desc[2 * f + 1, :nr], BF, B)
            for got_f, s_ in zip((u, d, s), single):
                assert np.array_equal(got_f[f, :nl], s_)
    for x in (e, el, er):
        x.close()
