"""Cases shared by tests/test_image_prep.py (host twin) and tests/test_image_prep_gpu.py (device): the smallest shapes at which the ingest
can go wrong -- every width around the 4- and 16-pixel units of the kernels, rows whose stride, base address and gray stride break the
alignment of the wide loads and stores, 1 / 3 / 4 channels with both channel orders, batches that mix the left and the right map -- with
the buffers they live in and the reference's bytes (tests/image_prep_ref.py), computed once per case."""
import functools

import numpy as np

import image_prep_ref as ref

WIDTHS = (1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 257)
HEIGHTS = (1, 2, 3, 19)
STRIDE_PADS = (0, 1, 3)
BASE_OFFSETS = (0, 1, 2, 3)
GRAY_PADS = (0, 5, 16)
N_IMAGES = (1, 2, 3, 5)
MAP_KINDS = ("identity", "shift", "half", "ties", "saturate", "warp", "borders")
WIDE = 1057   # more than 1 024 pixels of 16-pixel groups: a row of the gray kernel takes two wavefronts
RESIZES = ((67, 19, 40, 11), (40, 11, 67, 19))   # source w, h -> destination w, h
SENTINEL = 0xA5


def make_map(kind, sw, sh, dw, dh, seed):
    """A CV_32F map pair [dh, dw] into a source of sw x sh."""
    x, y = np.meshgrid(np.arange(dw, dtype=np.float32), np.arange(dh, dtype=np.float32))
    rng = np.random.default_rng(seed)
    if kind == "identity":
        return x, y
    if kind == "shift":                      # whole pixels: the shifted source, zeros where it ends
        return x + np.float32(2), y - np.float32(1)
    if kind == "half":                       # (a + b + 1) >> 1 along x
        return x + np.float32(0.5), y
    if kind == "ties":                       # products that fall between two fixed-point steps, on both sides of zero
        off = np.array([1 / 64, 3 / 64, -1 / 64, -3 / 64, 5 / 64, -5 / 64], np.float32)
        return x + off[(np.arange(dw) + seed) % 6][None, :], y + off[(np.arange(dh) + 1) % 6][:, None]
    if kind == "saturate":                   # coordinates beyond int16 after the shift, and the largest the maps may hold
        mx, my = x.copy(), y.copy()
        mx[::2, ::3] = 40000.0
        my[1::2, 1::3] = -40000.0
        mx[0, -1] = np.float32(16777215.0)
        my[-1, 0] = np.float32(-16777215.0)
        return mx, my
    if kind == "warp":                       # smooth, sub-pixel, a little beyond the source on every side
        ax, ay = rng.uniform(0.5, 2.5, 2)
        mx = x * np.float32(sw / dw) + np.float32(ax) * np.sin(y / np.float32(3.0) + np.float32(rng.uniform(0, 6))) + np.float32(rng.uniform(-0.5, 0.5))
        my = y * np.float32(sh / dh) + np.float32(ay) * np.cos(x / np.float32(5.0) + np.float32(rng.uniform(0, 6))) + np.float32(rng.uniform(-0.5, 0.5))
        return mx.astype(np.float32), my.astype(np.float32)
    if kind == "borders":                    # taps on all four borders: from one and a half pixels outside to the same beyond the far side
        mx = np.linspace(-1.5, sw + 0.5, dw, dtype=np.float32)[None, :] + np.zeros((dh, 1), np.float32) + rng.uniform(0, 1, (dh, dw)).astype(np.float32) * np.float32(0.25)
        my = np.linspace(-1.5, sh + 0.5, dh, dtype=np.float32)[:, None] + np.zeros((1, dw), np.float32) + rng.uniform(0, 1, (dh, dw)).astype(np.float32) * np.float32(0.25)
        return mx.astype(np.float32), my.astype(np.float32)
    raise ValueError(kind)


class Case:
    """One call: the source buffer (images at base + i * pitch, rows `stride` apart), the gray buffer's geometry, the maps."""

    def __init__(self, mode, channels, rgb, sw, sh, dw, dh, n, stride_pad, base, gray_pad, gray_base, kinds, seed):
        self.mode, self.channels, self.rgb = mode, channels, rgb
        self.sw, self.sh, self.dw, self.dh, self.n = sw, sh, dw, dh, n
        self.stride = sw * channels + stride_pad
        self.pitch = self.stride * sh + 7    # an odd distance: the images of a batch differ in alignment
        self.base = base
        self.gray_stride = dw + gray_pad
        self.gray_pitch = self.gray_stride * dh + 3
        self.gray_base = gray_base
        self.kinds, self.seed = kinds, seed
        self.id = "m%d-c%d-rgb%d-%dx%d-to-%dx%d-n%d-pad%d-base%d-gpad%d-gbase%d-%s" % (
            mode, channels, rgb, sw, sh, dw, dh, n, stride_pad, base, gray_pad, gray_base, "+".join(kinds))

    def params(self, capi):
        return capi.image_prep_params(self.sw, self.sh, self.channels, self.rgb, self.mode, self.dw, self.dh)

    @functools.cached_property
    def source(self):
        """The byte buffer that holds the images (read it from self.base on)."""
        return np.random.default_rng(self.seed).integers(0, 256, self.base + self.n * self.pitch, dtype=np.uint8)

    @functools.cached_property
    def images(self):
        out = np.empty((self.n, self.sh, self.sw, self.channels), np.uint8)
        for i in range(self.n):
            start = self.base + i * self.pitch
            out[i] = self.source[start:start + self.stride * self.sh].reshape(self.sh, self.stride)[:, :self.sw * self.channels].reshape(
                self.sh, self.sw, self.channels)
        return out[..., 0] if self.channels == 1 else out

    @functools.cached_property
    def maps(self):
        if self.mode != ref.RECTIFY:
            return None
        left = make_map(self.kinds[0], self.sw, self.sh, self.dw, self.dh, self.seed)
        right = make_map(self.kinds[1], self.sw, self.sh, self.dw, self.dh, self.seed + 1)
        return left + right

    def gray_buffer(self):
        return np.full(self.gray_base + self.n * self.gray_pitch, SENTINEL, np.uint8)

    @functools.cached_property
    def expected(self):
        """The whole gray buffer after the call: the reference's bytes in place, every other byte untouched."""
        want = ref.image_prep_batch(self.images, self.mode, self.rgb, self.maps, (self.dw, self.dh))
        buf = self.gray_buffer()
        for i in range(self.n):
            start = self.gray_base + i * self.gray_pitch
            buf[start:start + self.gray_stride * self.dh].reshape(self.dh, self.gray_stride)[:, :self.dw] = want[i]
        return buf


def run_host(pkg, case):
    """The host twin on the case's buffers -> the whole gray buffer."""
    gray = case.gray_buffer()
    n = pkg.capi.host_image_prep_batch_ptr(case.params(pkg.capi), case.maps, case.source.ctypes.data + case.base, case.n, case.stride, case.pitch,
                                           gray.ctypes.data + case.gray_base, case.gray_stride, case.gray_pitch)
    assert n == case.n
    return gray


def _cases():
    out = []
    j = 0
    for mode in (ref.COPY, ref.RECTIFY, ref.RESIZE):
        for channels in (1, 3, 4):
            for rgb in (0, 1):
                for i, w in enumerate(WIDTHS):
                    k = i + j
                    h = HEIGHTS[(k + j // 4) % 4]
                    n = N_IMAGES[(k // 2 + j) % 4]
                    pad, base = STRIDE_PADS[(k + j // 3) % 3], BASE_OFFSETS[(k // 3 + j) % 4]
                    gpad, gbase = GRAY_PADS[(k // 2 + j // 3) % 3], BASE_OFFSETS[(k + j // 2) % 4]
                    kinds = (MAP_KINDS[k % 7], MAP_KINDS[(k + 3) % 7])
                    if mode == ref.RECTIFY and n == 1:
                        n = 2 if i % 2 else 1            # mostly pairs: the right map differs from the left one
                    if mode == ref.RESIZE:
                        continue
                    dw, dh = (w, h) if mode == ref.COPY or i % 3 else (w + 3, h + 2)   # RECTIFY: maps larger than the source too
                    out.append(Case(mode, channels, rgb, w, h, dw, dh, n, pad, base, gpad, gbase, kinds if mode == ref.RECTIFY else (), 1000 + 37 * j + i))
                if mode == ref.COPY:
                    # nothing padded, nothing offset: in the first image every row's body starts on a 16-byte boundary of the source as
                    # well (the 16-byte loads); the second image, an odd distance on, takes the shifted dwords
                    out.append(Case(mode, channels, rgb, 257, 3, 257, 3, 2, 0, 0, 0, 0, (), 4000 + j))
                    # a row longer than one wavefront's 1 024 pixels, every channel count
                    out.append(Case(mode, channels, rgb, WIDE, 2, WIDE, 2, 2, STRIDE_PADS[j % 3], BASE_OFFSETS[(j + 1) % 4], GRAY_PADS[(j + 1) % 3],
                                    BASE_OFFSETS[(j + 2) % 4], (), 4500 + j))
                if mode == ref.RESIZE:
                    for i, (sw, sh, dw, dh) in enumerate(RESIZES):
                        k = i + j
                        out.append(Case(mode, channels, rgb, sw, sh, dw, dh, N_IMAGES[k % 4], STRIDE_PADS[k % 3], BASE_OFFSETS[(k + 1) % 4],
                                        GRAY_PADS[(k + 1) % 3], BASE_OFFSETS[(k + 2) % 4], (), 5000 + 37 * j + i))
                    # the kernels' four-column units and the last column at small sizes, enlarging and reducing
                    for i, (sw, sh, dw, dh) in enumerate(((5, 3, 17, 2), (17, 2, 5, 3), (1, 1, 4, 3), (16, 19, 15, 1))):
                        k = i + j
                        out.append(Case(mode, channels, rgb, sw, sh, dw, dh, N_IMAGES[(k + 1) % 4], STRIDE_PADS[(k + 1) % 3], BASE_OFFSETS[k % 4],
                                        GRAY_PADS[k % 3], BASE_OFFSETS[(k + 3) % 4], (), 6000 + 37 * j + i))
                j += 1
    return out


CASES = _cases()
GROUPS = sorted({(c.mode, c.channels, c.rgb) for c in CASES})


def group(mode, channels, rgb):
    return [c for c in CASES if (c.mode, c.channels, c.rgb) == (mode, channels, rgb)]


def coverage():
    """What the list covers, for the test that pins it."""
    cov = dict(widths=set(), heights=set(), pads=set(), bases=set(), gray_pads=set(), n=set(), kinds=set(), resizes=set(), wide=set())
    for c in CASES:
        if c.mode != ref.RESIZE and c.sw == WIDE:
            cov["wide"].add(c.channels)
        elif c.mode != ref.RESIZE:
            cov["widths"].add(c.sw); cov["heights"].add(c.sh)
        else:
            cov["resizes"].add((c.sw, c.sh, c.dw, c.dh))
        cov["pads"].add(c.stride - c.sw * c.channels); cov["bases"].add(c.base); cov["gray_pads"].add(c.gray_stride - c.dw); cov["n"].add(c.n)
        cov["kinds"].update(c.kinds)
    return cov
