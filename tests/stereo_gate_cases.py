"""Hand-made inputs for the gate tests of the stereo matcher (test_stereo_gates_gpu.py).

The pair: the right image is the left image moved by SHIFT whole pixels (right[x] == left[x + SHIFT], so a left
keypoint at x has its true correspondence at x - SHIFT on level 0), plus a little noise of its own, so that no window
compares equal and the median of the SADs is positive.  One band of rows is different: there the left rows are
mirror-symmetric about the column SYM_COL and the right rows equal the left ones exactly (the `disparity <= 0` case).

Everything here is plain numpy on the oracle's pyramid levels: it chooses where hand-made keypoints go (a "site": a
left level pixel whose 11x11 window has one strict SAD minimum among the right windows around its true
correspondence), and turns level pixels into image coordinates that round back to them.  What the matcher makes of
the keypoints is never computed here -- that is the oracle's job."""
import numpy as np

# 9: at most 9, so that a left window 6 columns from the right edge still has its correspondence 15 columns from it (a right keypoint at
# width - 12 or width - 11 finds it within +-4); at least 9, so that on level 3 (5.2 level pixels) a right keypoint 5 level pixels right
# of the correspondence is still not right of the left keypoint.  On level 6 the shift is 3.01 level pixels: small SADs there.
SHIFT = 9
SYM_ROWS = (100, 131)  # the band of rows with zero disparity, [first, last)
SYM_COL = 64
KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4")])
f32 = np.float32


def texture(seed, w, h):
    """Blocks of random grey (corners for FAST) under a smooth random field (a SAD minimum for every window)."""
    rng = np.random.default_rng(seed)
    blocks = np.kron(rng.integers(70, 186, (h // 6 + 1, w // 6 + 1)), np.ones((6, 6)))[:h, :w]
    blocks = blocks + np.kron(rng.integers(-45, 46, (h // 21 + 1, w // 21 + 1)), np.ones((21, 21)))[:h, :w]  # contrast for the coarse levels
    fine = rng.integers(-24, 25, (h + 2, w + 2)).astype(np.float64)
    fine = (fine[:-2, :-2] + fine[1:-1, :-2] + fine[2:, :-2] + fine[:-2, 1:-1] + fine[1:-1, 1:-1] + fine[2:, 1:-1] +
            fine[:-2, 2:] + fine[1:-1, 2:] + fine[2:, 2:]) / 3.0
    return np.clip(np.rint(blocks + fine), 0, 255).astype(np.uint8)


def shifted_pair(seed, w, h, sym_rows=SYM_ROWS, sym_col=SYM_COL):
    t = texture(seed, w + SHIFT, h)
    left = t[:, :w].copy()
    noise = np.random.default_rng(seed + 1000).integers(-2, 3, (h, w))
    right = np.clip(t[:, SHIFT:SHIFT + w].astype(np.int64) + noise, 0, 255).astype(np.uint8)
    if sym_rows is not None:
        r0, r1 = sym_rows
        half = left[r0:r1, sym_col:sym_col + 40]
        left[r0:r1, sym_col - 39:sym_col + 1] = half[:, ::-1]  # left[y, c - k] == left[y, c + k] for k < 40
        right[r0:r1] = left[r0:r1]
    return left, right


def sparse_pair(seed, w, h):
    """A pair with texture in one corner only: far fewer keypoints than shifted_pair."""
    left, right = shifted_pair(seed, w, h, sym_rows=None)
    flat = np.full((h, w), 128, np.uint8)
    flat[30:110, 40:140] = left[30:110, 40:140]
    fr = flat.copy()
    fr[30:110, 40 - SHIFT:140 - SHIFT] = left[30:110, 40:140]
    return flat, fr


def sad(lv_l, lv_r, ul, vl, ur):
    a = lv_l[vl - 5:vl + 6, ul - 5:ul + 6].astype(np.int64)
    b = lv_r[vl - 5:vl + 6, ur - 5:ur + 6].astype(np.int64)
    return int(np.abs(a - b).sum())


class Geometry:
    """Scale tables and level sizes of one pair, and the float32 arithmetic both matchers apply to a keypoint."""

    def __init__(self, scale, inv_scale, sizes):
        self.scale, self.inv, self.sizes = np.asarray(scale, f32), np.asarray(inv_scale, f32), sizes

    def level_px(self, v, level):
        """round(v * inv_scale[level]) as the matchers compute it (float32 product, round half away from zero)."""
        p = f32(v) * self.inv[level]
        return int(np.floor(np.abs(p) + f32(0.5)) * np.sign(p))

    def coord(self, px, level, frac=0.0):
        """An image coordinate (float32) that level_px() maps back to `px`."""
        v = f32(f32(px + frac) * self.scale[level])
        for _ in range(4):
            got = self.level_px(v, level)
            if got == px:
                return v
            v = f32(v + f32(0.25) * self.scale[level] * f32(np.sign(px - got)))
        raise AssertionError("no image coordinate for level pixel %d of level %d" % (px, level))

    def band(self, y, octave):
        """The rows [floor(y - r), ceil(y + r)], r = 2 * scale[octave], before clipping to the image."""
        r = f32(2.0) * self.scale[octave]
        return int(np.floor(f32(f32(y) - r))), int(np.ceil(f32(f32(y) + r)))

    def safe(self, kl, kr):
        """The safety condition: every window either side can read for this (left, right) keypoint pair lies in the level image."""
        lv = int(kl["octave"])
        w, h = self.sizes[lv]
        ul, vl, ur = self.level_px(kl["x"], lv), self.level_px(kl["y"], lv), self.level_px(kr["x"], lv)
        return 5 <= ul <= w - 6 and 5 <= vl <= h - 6 and 10 <= ur <= w - 11


def keypoint(x, y, octave):
    k = np.zeros(1, KP_DTYPE)
    k["x"], k["y"], k["octave"] = x, y, octave
    return k[0]


def find_sites(geom, levels_l, levels_r, level, want, max_sad, uls=None, vls=None, ok=None):
    """`want` sites (ul, vl, ustar) of `level`, one per row: the left window at (ul, vl) has its one strict SAD minimum at right
    column ustar among the columns within 10 of it, at most max_sad (so that the median cut keeps it), ustar lies within 2 pixels of the true
    correspondence, every window stays in the level image and clear of the symmetric band, and ok(ul, vl, ustar) holds."""
    w, h = geom.sizes[level]
    lv_l, lv_r = levels_l[level], levels_r[level]
    s = float(geom.scale[level])
    band = (int(SYM_ROWS[0] / s) - 7, int(SYM_ROWS[1] / s) + 7)
    uls = range(int(24 + SHIFT / s), w - 22, 3) if uls is None else uls
    vls = range(6, h - 6, 7 if level < 4 else 2) if vls is None else vls
    out = []
    for vl in vls:
        if band[0] <= vl <= band[1] or not 5 <= vl <= h - 6:
            continue
        for ul in uls:
            guess = int(round(ul - SHIFT / s))
            if not (5 <= ul <= w - 6 and guess - 2 >= 10 and guess + 2 <= w - 11):
                continue
            cols = list(range(max(guess - 12, 5), min(guess + 12, w - 6) + 1))  # clipped to the columns a window fits around
            c = [sad(lv_l, lv_r, ul, vl, u) for u in cols]
            ustar = cols[int(np.argmin(c))]
            if abs(ustar - guess) > 2 or (ok is not None and not ok(ul, vl, ustar)):
                continue
            if sum(v == min(c) for v in c) != 1 or min(c) > max_sad:
                continue
            out.append((ul, vl, ustar))
            break
        if len(out) == want:
            return out
    raise AssertionError("only %d of %d sites on level %d" % (len(out), want, level))


class Batch:
    """Hand-made left/right keypoints with descriptors of their own, and what each left one must come to."""

    def __init__(self, geom, seed):
        self.geom, self.rng = geom, np.random.default_rng(seed)
        self.kl, self.dl, self.kr, self.dr, self.expect, self.names = [], [], [], [], [], []

    def descriptor(self):
        return self.rng.integers(0, 256, 32).astype(np.uint8)

    @staticmethod
    def flipped(desc, nbits, rng):
        bits = np.unpackbits(desc)
        bits[rng.choice(256, nbits, replace=False)] ^= 1
        return np.packbits(bits)

    def left(self, name, k, desc, accepted):
        self.kl.append(k); self.dl.append(desc); self.expect.append(accepted); self.names.append(name)
        return len(self.kl) - 1

    def right(self, k, desc):
        self.kr.append(k); self.dr.append(desc)
        return len(self.kr) - 1

    def pair(self, name, kl, kr, accepted, flip=10):
        """One left keypoint and one right candidate `flip` descriptor bits away from it."""
        assert self.geom.safe(kl, kr), name
        d = self.descriptor()
        self.right(kr, self.flipped(d, flip, self.rng))
        return self.left(name, kl, d, accepted)

    def arrays(self):
        return (np.array(self.kl, KP_DTYPE), np.array(self.dl, np.uint8).reshape(-1, 32),
                np.array(self.kr, KP_DTYPE), np.array(self.dr, np.uint8).reshape(-1, 32))
