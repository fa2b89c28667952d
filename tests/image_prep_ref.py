"""numpy restatement of the two steps a camera image passes before ORBextractor::operator() (include/tc2li_hip.h "image ingest"):
System::TrackStereoLidar's clone / cv::remap / cv::resize (SF/src/System.cc:240-257) and Tracking::GrabImageStereoLidar's cvtColor
(SF/src/Tracking.cc:1646-1671).  It DEFINES parity for tc2li_image_prep_batch and tc2li_host_image_prep_batch: OpenCV is not available
where this project is built, the arithmetic below is a recollection of OpenCV 4.2 ("parity unpinned").

Order: remap or resize first, on the image as delivered, every channel on its own and rounded to 8 bits; the colour conversion runs on
that result.  (Gray first and remap second gives other bytes.)"""
import numpy as np

COPY, RECTIFY, RESIZE = 0, 1, 2
R2Y, G2Y, B2Y = 9798, 19235, 3735   # 15-bit fixed point, the sum is 32768


def gray(img, rgb):
    """cvtColor RGB2GRAY / BGR2GRAY / RGBA2GRAY / BGRA2GRAY on 8U: [h, w, 3 or 4] -> [h, w]; [h, w] passes.  rgb: channel 0 is R."""
    img = np.asarray(img, np.uint8)
    if img.ndim == 2:
        return img.copy()
    c = img.astype(np.int64)
    r, b = (c[..., 0], c[..., 2]) if rgb else (c[..., 2], c[..., 0])   # a fourth channel is not read
    return ((r * R2Y + c[..., 1] * G2Y + b * B2Y + 16384) >> 15).astype(np.uint8)


def cv_round(v):
    """cvRound: to nearest, ties to even.  float32 in, int64 out."""
    return np.rint(np.asarray(v, np.float32)).astype(np.int64)


def remap_fixed(map_x, map_y):
    """The fixed-point form of a CV_32F map pair: (ix, iy, fx, fy).  The product map * 32 is taken in float32."""
    sx = cv_round(np.asarray(map_x, np.float32) * np.float32(32))
    sy = cv_round(np.asarray(map_y, np.float32) * np.float32(32))
    ix = np.clip(sx >> 5, -32768, 32767)   # arithmetic shift, then saturate_cast<short>
    iy = np.clip(sy >> 5, -32768, 32767)
    return ix, iy, sx & 31, sy & 31


def remap(img, map_x, map_y):
    """cv::remap(INTER_LINEAR, BORDER_CONSTANT 0) on 8U with float maps of the destination's size, every channel on its own.
    OpenCV's weight table holds (32767, 0, 0, 1) instead of (32768, 0, 0, 0) for fx = fy = 0: (32767 p00 + p11 + 16384) >> 15 is p00 for
    every pair of bytes (p11 - p00 + 16384 stays inside [0, 32768)), so the plain weights below give the same bytes."""
    img = np.asarray(img, np.uint8)
    h, w = img.shape[:2]
    ix, iy, fx, fy = remap_fixed(map_x, map_y)
    src = img.reshape(h, w, -1).astype(np.int64)

    def tap(y, x):
        ok = (y >= 0) & (y < h) & (x >= 0) & (x < w)
        return src[np.clip(y, 0, h - 1), np.clip(x, 0, w - 1)] * ok[..., None]   # a tap outside the source reads 0

    w00, w01, w10, w11 = (32 - fx) * (32 - fy) * 32, fx * (32 - fy) * 32, (32 - fx) * fy * 32, fx * fy * 32
    acc = tap(iy, ix) * w00[..., None] + tap(iy, ix + 1) * w01[..., None] + tap(iy + 1, ix) * w10[..., None] + tap(iy + 1, ix + 1) * w11[..., None]
    out = ((acc + 16384) >> 15).astype(np.uint8)
    return out.reshape(ix.shape + img.shape[2:])


def _resize_table(n_src, n_dst, clamp):
    scale = 1.0 / (float(n_dst) / float(n_src))
    f = ((np.arange(n_dst, dtype=np.float64) + 0.5) * scale - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int64)
    f = (f - s.astype(np.float32)).astype(np.float32)
    if clamp:   # the column table clamps here; the row table leaves it to the row fetch (same bytes)
        lo, hi = s < 0, s >= n_src - 1
        f = np.where(lo | hi, np.float32(0), f)
        s = np.where(lo, 0, np.where(hi, n_src - 1, s))
    sat = lambda v: np.clip(cv_round(v), -32768, 32767)
    return s, sat((np.float32(1) - f) * np.float32(2048)), sat(f * np.float32(2048))


def resize(img, dst_width, dst_height):
    """cv::resize(INTER_LINEAR) on 8U, any source and destination size, every channel on its own: 11-bit weights, the vertical combine of
    SURVEY.md Appendix B.  cv::resize takes its area form for exact 2 x reductions; the linear form gives the same byte there,
    (a + b + c + d + 2) >> 2 (tests/test_image_prep.py asserts it), so this is the one path."""
    img = np.asarray(img, np.uint8)
    h, w = img.shape[:2]
    src = img.reshape(h, w, -1).astype(np.int64)
    xo, a0, a1 = _resize_table(w, dst_width, True)
    yo, b0, b1 = _resize_table(h, dst_height, False)
    x1 = np.minimum(xo + 1, w - 1)   # its weight is 0 wherever the clamp acts

    def hrow(y):
        rows = src[np.clip(y, 0, h - 1)]
        return rows[:, xo] * a0[None, :, None] + rows[:, x1] * a1[None, :, None]

    r0, r1 = hrow(yo), hrow(yo + 1)
    out = ((((b0[:, None, None] * (r0 >> 4)) >> 16) + ((b1[:, None, None] * (r1 >> 4)) >> 16) + 2) >> 2).astype(np.uint8)
    return out.reshape((dst_height, dst_width) + img.shape[2:])


def image_prep(img, mode=COPY, rgb=1, maps=None, dst_size=None):
    """One image through both steps.  maps = (map_x, map_y) for RECTIFY, dst_size = (width, height) for RESIZE."""
    if mode == RECTIFY:
        img = remap(img, maps[0], maps[1])
    elif mode == RESIZE:
        img = resize(img, dst_size[0], dst_size[1])
    return gray(img, rgb)


def image_prep_batch(images, mode=COPY, rgb=1, maps=None, dst_size=None):
    """images [n, h, w] or [n, h, w, c]; image i belongs to camera i & 1; maps = (xl, yl, xr, yr)."""
    return np.stack([image_prep(im, mode, rgb, None if maps is None else maps[2 * (i & 1):2 * (i & 1) + 2], dst_size)
                     for i, im in enumerate(images)])
