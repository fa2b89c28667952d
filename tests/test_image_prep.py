"""CPU tests of the image ingest (include/tc2li_hip.h "image ingest"): the numpy restatement (tests/image_prep_ref.py) pinned by closed
forms, the host twin tc2li_host_image_prep_batch against it byte for byte, and every refusal of the ABI.  The semantics are a recollection
of OpenCV 4.2 (parity unpinned): the closed forms below are what that recollection says, not a run of OpenCV."""
import ctypes as C

import numpy as np
import pytest

import image_prep_cases as K
import image_prep_ref as ref


# ---- the reference, pinned by closed forms ---------------------------------------------------------------------------------------------
def test_gray_closed_forms():
    v = np.arange(256, dtype=np.uint8)
    same = np.stack([v, v, v], 1)[None]
    assert np.array_equal(ref.gray(same, 1)[0], v) and np.array_equal(ref.gray(same, 0)[0], v)      # the weights sum to 32768
    pure = np.array([[[255, 0, 0], [0, 255, 0], [0, 0, 255]]], np.uint8)
    assert ref.gray(pure, 1).tolist() == [[76, 150, 29]]
    assert ref.gray(pure, 0).tolist() == [[29, 150, 76]]
    rng = np.random.default_rng(1)
    rgb = rng.integers(0, 256, (7, 9, 3), dtype=np.uint8)
    assert np.array_equal(ref.gray(rgb[..., ::-1], 0), ref.gray(rgb, 1))                            # BGR with rgb = 0 is RGB with rgb = 1
    for alpha in (0, 255):
        rgba = np.concatenate([rgb, np.full((7, 9, 1), alpha, np.uint8)], 2)
        assert np.array_equal(ref.gray(rgba, 1), ref.gray(rgb, 1)) and np.array_equal(ref.gray(rgba, 0), ref.gray(rgb, 0))
    gray = rng.integers(0, 256, (7, 9), dtype=np.uint8)
    assert np.array_equal(ref.gray(gray, 1), gray)


def test_remap_closed_forms():
    rng = np.random.default_rng(2)
    for shape in ((6, 11), (6, 11, 3), (6, 11, 4)):
        src = rng.integers(0, 256, shape, dtype=np.uint8)
        h, w = shape[:2]
        x, y = np.meshgrid(np.arange(w, dtype=np.float32), np.arange(h, dtype=np.float32))
        assert np.array_equal(ref.remap(src, x, y), src)                                            # the identity map
        want = np.zeros_like(src)
        want[1:, :w - 2] = src[:h - 1, 2:]
        assert np.array_equal(ref.remap(src, x + 2, y - 1), want)                                   # whole pixels: shifted, zero fill
        half = ref.remap(src, x + np.float32(0.5), y).astype(np.int64)
        s = src.astype(np.int64)
        assert np.array_equal(half[:, :w - 1], (s[:, :w - 1] + s[:, 1:] + 1) >> 1)
        assert np.array_equal(half[:, w - 1], (s[:, w - 1] + 1) >> 1)                               # the last column blends with the border's 0
        far = ref.remap(src, np.full((h, w), 40000, np.float32), y)                                 # saturates to ix = 32767: outside
        assert not far.any()
        assert not ref.remap(src, x, np.full((h, w), -40000, np.float32)).any()


def test_remap_ties_and_negatives():
    f = lambda v: [int(a[0]) for a in ref.remap_fixed(np.array([v], np.float32), np.array([v], np.float32))[:3:2]]   # (ix, fx)
    assert f(3 + 1 / 64) == [3, 0]       # 96.5 -> 96
    assert f(3 + 3 / 64) == [3, 2]       # 97.5 -> 98
    assert f(-1 / 64) == [0, 0]          # -0.5 -> 0
    assert f(-3 / 64) == [-1, 30]        # -1.5 -> -2: an arithmetic shift and the low five bits
    assert f(40000.0) == [32767, 0] and f(-40000.0) == [-32768, 0]
    # OpenCV's table entry (32767, 0, 0, 1) for fx = fy = 0 gives the byte of the plain weights for every pair of bytes
    a, b = np.meshgrid(np.arange(256), np.arange(256))
    assert np.array_equal((32767 * a + b + 16384) >> 15, a)


def test_resize_against_the_oracle_and_at_2x(oracle):
    rng = np.random.default_rng(3)
    src = rng.integers(0, 256, (60, 90), dtype=np.uint8)
    for dw, dh in ((75, 50), (90, 60), (61, 33), (120, 77)):     # a pyramid ratio (1 / 1.2), the identity, a steeper reduction, enlarging
        assert np.array_equal(ref.resize(src, dw, dh), oracle.resize_linear(src, dw, dh)), (dw, dh)
    s = src.astype(np.int64)
    mean = (s[0::2, 0::2] + s[0::2, 1::2] + s[1::2, 0::2] + s[1::2, 1::2] + 2) >> 2
    assert np.array_equal(ref.resize(src, 45, 30), mean)         # exactly 2 x: cv::resize's area form gives the same byte
    col = rng.integers(0, 256, (60, 90, 3), dtype=np.uint8)
    out = ref.resize(col, 75, 50)                                # every channel on its own
    for c in range(3):
        assert np.array_equal(out[..., c], oracle.resize_linear(np.ascontiguousarray(col[..., c]), 75, 50))
    big = ref.resize(src[:11, :40], 67, 19)                      # a destination larger than the source: inside the source's range, ends kept
    assert big.shape == (19, 67) and big.min() >= src[:11, :40].min() and big.max() <= src[:11, :40].max()
    assert big[0, 0] == src[0, 0] and big[-1, -1] == src[10, 39]


def test_order_of_the_two_steps_matters():
    rng = np.random.default_rng(4)
    src = rng.integers(0, 256, (9, 14, 3), dtype=np.uint8)
    x, y = np.meshgrid(np.arange(14, dtype=np.float32), np.arange(9, dtype=np.float32))
    mx, my = x + np.float32(0.3), y + np.float32(0.6)
    assert not np.array_equal(ref.image_prep(src, ref.RECTIFY, 1, (mx, my)), ref.remap(ref.gray(src, 1), mx, my))


def test_case_list_covers_what_the_issue_names():
    cov = K.coverage()
    assert cov["widths"] == set(K.WIDTHS) and cov["heights"] == set(K.HEIGHTS)
    assert cov["wide"] == {1, 3, 4} and (K.WIDE >> 4) > 64
    assert cov["pads"] == {0, 1, 3} and cov["bases"] == {0, 1, 2, 3} and cov["n"] == {1, 2, 3, 5} and len(cov["gray_pads"]) > 1
    assert cov["kinds"] == set(K.MAP_KINDS) and set(K.RESIZES) <= cov["resizes"]
    assert {(c.mode, c.channels, c.rgb) for c in K.CASES} == {(m, c, r) for m in (0, 1, 2) for c in (1, 3, 4) for r in (0, 1)}
    assert any(c.mode == ref.RECTIFY and c.n > 1 and c.kinds[0] != c.kinds[1] for c in K.CASES)


# ---- the host twin ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,channels,rgb", K.GROUPS)
def test_host_twin_equals_reference(pkg, mode, channels, rgb):
    for case in K.group(mode, channels, rgb):
        assert np.array_equal(K.run_host(pkg, case), case.expected), case.id


def test_host_twin_through_the_array_form(pkg):
    rng = np.random.default_rng(5)
    imgs = rng.integers(0, 256, (3, 19, 65, 3), dtype=np.uint8)
    p = pkg.capi.image_prep_params(65, 19, 3, rgb=False)
    assert np.array_equal(pkg.image_prep_batch(p, imgs, host=True), ref.image_prep_batch(imgs, ref.COPY, 0))
    maps = K.make_map("warp", 65, 19, 40, 11, 1) + K.make_map("borders", 65, 19, 40, 11, 2)
    p = pkg.capi.image_prep_params(65, 19, 3, rgb=True, mode=pkg.IMAGE_PREP_RECTIFY, dst_width=40, dst_height=11)
    assert np.array_equal(pkg.image_prep_batch(p, imgs, maps=maps, host=True), ref.image_prep_batch(imgs, ref.RECTIFY, 1, maps))


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def host_rc(pkg, p, maps=None, n=2, stride=None, gray_stride=None, gray_pitch=None):
    """The host twin's return code on buffers large enough for any of the (small) cases below."""
    src, gray = np.zeros(1 << 16, np.uint8), np.zeros(1 << 16, np.uint8)
    stride = p.src_width * p.channels if stride is None else stride
    gray_stride = p.dst_width if gray_stride is None else gray_stride
    gray_pitch = 4096 if gray_pitch is None else gray_pitch
    try:
        return pkg.capi.host_image_prep_batch_ptr(p, maps, src.ctypes.data, n, stride, 4096, gray.ctypes.data, gray_stride, gray_pitch)
    except pkg.Tc2liError as e:
        return e.code


INVALID = -2


def test_refusals(pkg):
    P = pkg.capi.image_prep_params
    assert host_rc(pkg, P(8, 4, 3)) == 2                                         # the baseline is accepted
    for channels in (0, 2, 5, -1):
        assert host_rc(pkg, P(8, 4, channels)) == INVALID
    for w, h in ((0, 4), (8, 0), (-3, 4), (16385, 4), (8, 16385)):
        assert host_rc(pkg, P(w, h, 1)) == INVALID
        assert host_rc(pkg, P(8, 4, 1, mode=pkg.IMAGE_PREP_RESIZE, dst_width=w, dst_height=h)) == INVALID
    assert host_rc(pkg, P(8, 4, 1, mode=3)) == INVALID and host_rc(pkg, P(8, 4, 1, mode=-1)) == INVALID
    assert host_rc(pkg, P(8, 4, 1, mode=pkg.IMAGE_PREP_COPY, dst_width=9, dst_height=4)) == INVALID
    assert host_rc(pkg, P(8, 4, 3), stride=23) == INVALID and host_rc(pkg, P(8, 4, 3), stride=24) == 2
    assert host_rc(pkg, P(8, 4, 3), gray_stride=7) == INVALID and host_rc(pkg, P(8, 4, 3), gray_stride=8) == 2
    assert host_rc(pkg, P(8, 4, 3), gray_pitch=31) == INVALID and host_rc(pkg, P(8, 4, 3), gray_pitch=32) == 2   # gray images would overlap
    assert host_rc(pkg, P(8, 4, 3), n=-1) == INVALID
    # RECTIFY without the maps of both cameras
    R = P(8, 4, 3, mode=pkg.IMAGE_PREP_RECTIFY)
    good = K.make_map("identity", 8, 4, 8, 4, 0)
    assert host_rc(pkg, R, maps=None) == INVALID
    assert host_rc(pkg, R, maps=good + (None, None)) == INVALID and host_rc(pkg, R, maps=(None, None) + good) == INVALID
    assert host_rc(pkg, R, maps=good + good) == 2
    # a map value cvRound is undefined for
    for bad in (np.nan, np.inf, -np.inf, 16777216.0, -16777216.0, 3e38):
        for slot in range(4):
            maps = [m.copy() for m in good + good]
            maps[slot][3, 7] = bad
            assert host_rc(pkg, R, maps=maps) == INVALID, (bad, slot)
    maps = [m.copy() for m in good + good]
    maps[1][0, 0] = 16777215.0
    assert host_rc(pkg, R, maps=maps) == 2                                       # the largest magnitude that is taken


def test_create_refuses_before_it_looks_for_a_device(pkg):
    """tc2li_image_prep_create validates first: the same codes with and without a GPU."""
    for kw in (dict(channels=2), dict(src_width=0), dict(src_height=16385), dict(mode=7), dict(mode=2, dst_width=0), dict(max_images=0),
               dict(max_images=65536), dict(mode=0, dst_width=9)):
        args = dict(src_width=8, src_height=4, channels=3)
        args.update(kw)
        with pytest.raises(pkg.Tc2liError) as e:
            pkg.ImagePrep(**args)
        assert e.value.code == INVALID, kw
    if pkg.device_count() == 0:
        with pytest.raises(pkg.Tc2liError) as e:
            pkg.ImagePrep(8, 4, 3)
        assert e.value.code == -3   # TC2LI_ERR_NO_DEVICE: the device entry has no fallback


def test_abi_declares_the_ingest(pkg):
    syms = pkg.exported_symbols()
    for s in ("tc2li_image_prep_create", "tc2li_image_prep_destroy", "tc2li_image_prep_set_maps", "tc2li_image_prep_batch",
              "tc2li_host_image_prep_batch"):
        assert s in syms and hasattr(pkg.lib(), s), s
    assert C.sizeof(pkg.capi.ImagePrepParams) == 28
