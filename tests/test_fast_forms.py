"""The per-pixel forms of the FAST kernel (csrc/fast_forms.hpp: packed 16-bit arithmetic, the source k_fast_cells runs) through the host entry
tc2li_host_fast_forms, against numpy restatements of the plain definitions and against the oracle's FAST: CPU only."""
import numpy as np
import pytest

# cv::FAST's circle of 16 (dx, dy), pixel 0 three rows below the centre
CIRCLE = [(0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3), (0, -3), (-1, -3), (-2, -2), (-3, -1), (-3, 0), (-3, 1), (-2, 2), (-1, 3)]
THRESHOLDS = (0, 1, 7, 12, 20, 128, 255)


def flags(v, p, th):
    v = v.astype(np.int32)[:, None]
    p = p.astype(np.int32)
    return p > v + th, p < v - th


def pack_mask(f):
    return (f.astype(np.uint32) << np.arange(16, dtype=np.uint32)).sum(axis=1).astype(np.uint16)


def arc9(f):
    """[n, 16] flags -> does the circle hold nine contiguous set ones"""
    out = np.zeros(len(f), bool)
    for s in range(16):
        run = np.ones(len(f), bool)
        for i in range(9):
            run &= f[:, (s + i) % 16]
        out |= run
    return out


def arc_contrast(v, p, dark):
    d = v.astype(np.int32)[:, None] - p.astype(np.int32)
    if not dark:
        d = -d
    best = np.full(len(d), -256, np.int32)
    for s in range(16):
        best = np.maximum(best, np.min(d[:, [(s + i) % 16 for i in range(9)]], axis=1))
    return best


def pretest_plain(v, p, th):
    v = v.astype(np.int32)
    p = p.astype(np.int32)
    most = np.minimum(np.maximum(p[:, 0], p[:, 8]), np.maximum(p[:, 4], p[:, 12]))
    least = np.maximum(np.minimum(p[:, 0], p[:, 8]), np.minimum(p[:, 4], p[:, 12]))
    return (most > v + th) | (least < v - th)


@pytest.fixture(scope="module")
def byte_pairs():
    value, centre = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8))
    return value.reshape(-1), centre.reshape(-1)


@pytest.mark.parametrize("th", THRESHOLDS)
def test_predicates_exhaustive(pkg, byte_pairs, th):
    """Every (value, centre) pair of bytes.  The pre-test with `value` on each of the 16 subsets of the four compass pixels (the others equal
    the centre); both flag predicates with `value` on the whole circle and on one position that moves with the item."""
    value, centre = byte_pairs
    n = len(value)
    for subset in range(16):
        p = np.repeat(centre[:, None], 16, axis=1)
        for b, j in enumerate((0, 4, 8, 12)):
            if subset >> b & 1:
                p[:, j] = value
        got = pkg.capi.host_fast_forms(centre, p, th)
        assert np.array_equal(got["pretest"].astype(bool), pretest_plain(centre, p, th)), subset
    whole = np.repeat(value[:, None], 16, axis=1)
    one = np.repeat(centre[:, None], 16, axis=1)
    one[np.arange(n), np.arange(n) % 16] = value
    for p in (whole, one):
        got = pkg.capi.host_fast_forms(centre, p, th)
        fb, fd = flags(centre, p, th)
        assert np.array_equal(got["mask_bright"], pack_mask(fb))
        assert np.array_equal(got["mask_dark"], pack_mask(fd))


@pytest.mark.parametrize("th", (0, 7, 20, 128))
def test_masks_to_polarity(pkg, th):
    """All 2^16 bright patterns and all 2^16 dark patterns at amplitude th + 1: the masks are the patterns, the polarity is "nine contiguous"
    of the pattern's sign and never both."""
    pat = np.arange(1 << 16, dtype=np.uint32)
    bits = (pat[:, None] >> np.arange(16, dtype=np.uint32) & 1).astype(bool)
    want = arc9(bits)
    for dark in (False, True):
        v = np.full(len(pat), 200 if dark else 100, np.uint8)
        p = np.where(bits, v[:, None].astype(np.int32) + (-(th + 1) if dark else th + 1), v[:, None]).astype(np.uint8)
        got = pkg.capi.host_fast_forms(v, p, th)
        assert np.array_equal(got["mask_dark" if dark else "mask_bright"], pat.astype(np.uint16))
        assert not got["mask_bright" if dark else "mask_dark"].any()
        assert np.array_equal(got["polarity"], np.where(want, 1 if dark else 2, 0))
        assert np.array_equal(got["pretest"].astype(bool) | ~want, np.ones(len(pat), bool))  # the pre-test is necessary for an arc


def structured_circles(th):
    """Arcs of length 7 .. 12 at every start, amplitudes of -1, 0, +1, +2 around the threshold, on centres that pin values at 0 and 255."""
    vs, ps = [], []
    for length in range(7, 13):
        for start in range(16):
            on = np.zeros(16, bool)
            on[[(start + i) % 16 for i in range(length)]] = True
            for amp in (th - 1, th, th + 1, th + 2):
                for sign in (1, -1):
                    for v in (0, 1, amp, 128, 255 - amp, 254, 255):
                        if 0 <= v <= 255:
                            vs.append(v)
                            ps.append(np.clip(np.where(on, v + sign * amp, v + (start % 3 - 1)), 0, 255))
    return np.array(vs, np.uint8), np.array(ps, np.uint8)


@pytest.mark.parametrize("th", (7, 12, 20))
def test_scores(pkg, th):
    rng = np.random.default_rng(th)
    n = 120000
    v = rng.integers(0, 256, n).astype(np.uint8)
    p = rng.integers(0, 256, (n, 16)).astype(np.uint8)
    # a third of the random circles near their centre, so that arcs at the threshold occur
    near = rng.random(n) < 0.34
    p[near] = np.clip(v[near, None].astype(np.int32) + rng.integers(-th - 3, th + 4, (int(near.sum()), 16)), 0, 255).astype(np.uint8)
    sv, sp = structured_circles(th)
    v, p = np.concatenate([v, sv]), np.concatenate([p, sp])
    got = pkg.capi.host_fast_forms(v, p, th)
    sd, sb = arc_contrast(v, p, True), arc_contrast(v, p, False)
    assert np.array_equal(got["score_dark"], sd) and np.array_equal(got["score_bright"], sb)
    fb, fd = flags(v, p, th)
    pol = got["polarity"]
    assert np.array_equal(pol & 1, arc9(fd)) and np.array_equal(pol >> 1, arc9(fb))
    assert not (pol == 3).any()  # a survivor has exactly one polarity: the kernel scores that one only
    assert np.array_equal(pol & 1, sd > th) and np.array_equal(pol >> 1, sb > th)  # a corner <=> score > th
    assert (pol != 0).sum() > 1000 and (pol == 1).sum() > 100 and (pol == 2).sum() > 100


def corners_by_forms(pkg, img, th, nms):
    """cv::FAST on `img` (3-px border excluded) as the kernel's passes compute it: pre-test, segment test, score of the pixel's polarity, NMS."""
    h, w = img.shape
    ys, xs = np.mgrid[3:h - 3, 3:w - 3]
    ys, xs = ys.reshape(-1), xs.reshape(-1)
    p = np.stack([img[ys + dy, xs + dx] for dx, dy in CIRCLE], axis=1)
    got = pkg.capi.host_fast_forms(img[ys, xs], p, th)
    pol = got["polarity"]
    assert not (pol == 3).any()
    assert not ((pol != 0) & (got["pretest"] == 0)).any()
    corner = (got["pretest"] != 0) & (pol != 0)
    S = np.where(pol == 1, got["score_dark"], got["score_bright"]).astype(np.int32)
    score = np.zeros((h, w), np.int32)
    score[ys[corner], xs[corner]] = S[corner] - 1  # cv::FAST's response (>= th > 0; 0 where there is no corner)
    out = []
    for y, x in zip(ys[corner], xs[corner]):
        if nms:
            nb = score[y - 1:y + 2, x - 1:x + 2].copy()
            nb[1, 1] = -1
            if not (score[y, x] > nb.max()):
                continue
        out.append((x, y, score[y, x]))
    return np.array(out, np.float32).reshape(-1, 3)


@pytest.mark.parametrize("th", (20, 7))
@pytest.mark.parametrize("nms", (True, False))
def test_window_against_oracle(pkg, oracle, synthetic, th, nms):
    """A 48 x 48 window (the small instantiation's tile) of a rendered frame and one of noise with pinned values."""
    frame = synthetic.Scene(0).render(0.0, synthetic.WIDTH, synthetic.HEIGHT, noise_seed=1)[0]
    rng = np.random.default_rng(5)
    noise = rng.integers(0, 256, (48, 48)).astype(np.uint8)
    noise[rng.random((48, 48)) < 0.3] = 0
    noise[rng.random((48, 48)) < 0.2] = 255
    for img in (np.ascontiguousarray(frame[100:148, 300:348]), noise):
        want = oracle.fast9_16(img, th, nms=nms)
        got = corners_by_forms(pkg, img, th, nms)
        assert len(want) > 5
        if not nms:
            got[:, 2] = 0  # cv::FAST computes no response without the suppression
        assert np.array_equal(got, want)


def test_thresholds_outside_a_byte_are_refused(pkg):
    """The forms hold sums and differences of bytes and the threshold in 16-bit halves: the extractor accepts 0 .. 255 only."""
    for bad in ({"ini_th_fast": 256}, {"ini_th_fast": -1}, {"min_th_fast": 256}, {"min_th_fast": -1}):
        with pytest.raises(pkg.capi.Tc2liError):
            pkg.OrbExtractor(max_width=64, max_height=64, max_images=1, **bad)
    z = np.zeros(4, np.uint8)
    for bad in (-1, 256):
        with pytest.raises(pkg.capi.Tc2liError):
            pkg.capi.host_fast_forms(z, np.zeros((4, 16), np.uint8), bad)
