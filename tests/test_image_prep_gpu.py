"""GPU tests of the image ingest (tc2li_image_prep_batch): the device equals the host twin and the numpy restatement
(tests/image_prep_ref.py) byte for byte on the cases of tests/image_prep_cases.py -- including every byte of the gray buffer the call must
not touch -- from host and from device images, and its output feeds tc2li_orb_extract_batch in place.  torch is the allocator."""
import numpy as np
import pytest

import image_prep_cases as K
import image_prep_ref as ref

pytestmark = pytest.mark.gpu

INVALID = -2


def run_device(pkg, case, on_device):
    import torch
    prep = pkg.ImagePrep(case.sw, case.sh, case.channels, case.rgb, case.mode, case.dw, case.dh, max_images=case.n)
    try:
        if case.mode == ref.RECTIFY:
            prep.set_maps(0, case.maps[0], case.maps[1])
            prep.set_maps(1, case.maps[2], case.maps[3])
        gray = torch.from_numpy(case.gray_buffer()).cuda()
        if on_device:
            src = torch.from_numpy(case.source).cuda()
            ptr = src.data_ptr() + case.base
        else:
            ptr = case.source.ctypes.data + case.base
        stream = torch.cuda.current_stream().cuda_stream
        n = prep.batch_ptr(ptr, on_device, case.n, case.stride, case.pitch, gray.data_ptr() + case.gray_base, case.gray_stride, case.gray_pitch,
                           stream=stream)
        assert n == case.n
        torch.cuda.current_stream().synchronize()
        return gray.cpu().numpy()
    finally:
        prep.close()


@pytest.mark.parametrize("mode,channels,rgb", K.GROUPS)
def test_device_equals_host_twin_and_reference(pkg, mode, channels, rgb):
    assert pkg.device_count() >= 1, "GPU tests need a device; the library has no fallback"
    for i, case in enumerate(K.group(mode, channels, rgb)):
        host = K.run_host(pkg, case)
        assert np.array_equal(host, case.expected), case.id
        for on_device in ((i + channels) % 2 == 0, (i + channels) % 2 != 0) if i % 4 == 0 else ((i + channels) % 2 == 0,):
            got = run_device(pkg, case, on_device)
            assert np.array_equal(got, host), (case.id, on_device)


def test_device_refusals(pkg):
    import torch
    src, gray = torch.zeros(1 << 14, dtype=torch.uint8, device="cuda"), torch.zeros(1 << 14, dtype=torch.uint8, device="cuda")

    def rc(prep, n=2, stride=24, gray_stride=8, gray_pitch=64):
        try:
            return prep.batch_ptr(src.data_ptr(), True, n, stride, 256, gray.data_ptr(), gray_stride, gray_pitch)
        except pkg.Tc2liError as e:
            return e.code

    prep = pkg.ImagePrep(8, 4, 3, max_images=2)
    assert rc(prep) == 2 and rc(prep, n=0) == 0
    assert rc(prep, stride=23) == INVALID and rc(prep, gray_stride=7) == INVALID and rc(prep, gray_pitch=31) == INVALID and rc(prep, n=-1) == INVALID
    assert rc(prep, n=3) == -5                                                   # TC2LI_ERR_CAPACITY: the handle was made for 2 images
    with pytest.raises(pkg.Tc2liError) as e:
        prep.set_maps(0, *K.make_map("identity", 8, 4, 8, 4, 0))                 # not a RECTIFY handle
    assert e.value.code == INVALID
    prep.close()
    prep = pkg.ImagePrep(8, 4, 3, mode=pkg.IMAGE_PREP_RECTIFY, max_images=2)
    good = K.make_map("identity", 8, 4, 8, 4, 0)
    assert rc(prep) == INVALID                                                   # no map yet
    prep.set_maps(0, *good)
    assert rc(prep) == INVALID                                                   # only the left one
    for bad in (np.nan, np.inf, 16777216.0, -16777216.0):
        for which in (0, 1):
            maps = [m.copy() for m in good]
            maps[which][2, 5] = bad
            with pytest.raises(pkg.Tc2liError) as e:
                prep.set_maps(1, *maps)
            assert e.value.code == INVALID
            assert rc(prep) == INVALID                                           # a refused call sets nothing: camera 1 still has no map
    with pytest.raises(pkg.Tc2liError):
        prep.set_maps(2, *good)
    prep.set_maps(1, *good)
    assert rc(prep) == 2
    # ... and changes nothing: after a refused call the accepted maps stay in force, with their bytes
    src.copy_(torch.from_numpy(np.random.default_rng(9).integers(0, 256, 1 << 14, dtype=np.uint8)).cuda())
    torch.cuda.synchronize()
    shifted = K.make_map("shift", 8, 4, 8, 4, 0)
    bad = [m.copy() for m in shifted]
    bad[0][1, 1] = np.nan
    with pytest.raises(pkg.Tc2liError) as e:
        prep.set_maps(1, *bad)
    assert e.value.code == INVALID
    gray.zero_()
    assert rc(prep) == 2
    torch.cuda.synchronize()
    kept = gray.cpu().numpy().copy()
    want = ref.image_prep_batch(np.stack([src.cpu().numpy()[i * 256:i * 256 + 96].reshape(4, 8, 3) for i in range(2)]), ref.RECTIFY, 1, good + good)
    assert np.array_equal(np.stack([kept[i * 64:i * 64 + 32].reshape(4, 8) for i in range(2)]), want)
    # set_maps after a queued batch on device images: the batch reads the maps it was queued with, the next one the new maps
    gray.zero_()
    assert rc(prep) == 2
    prep.set_maps(1, *shifted)
    torch.cuda.synchronize()
    assert np.array_equal(gray.cpu().numpy(), kept)
    assert rc(prep) == 2
    torch.cuda.synchronize()
    want = ref.image_prep_batch(np.stack([src.cpu().numpy()[i * 256:i * 256 + 96].reshape(4, 8, 3) for i in range(2)]), ref.RECTIFY, 1, good + shifted)
    assert np.array_equal(np.stack([gray.cpu().numpy()[i * 64:i * 64 + 32].reshape(4, 8) for i in range(2)]), want)
    prep.close()


FIELDS = ("x", "y", "size", "angle", "response", "octave")


def assert_same_batch(a, b, n):
    ka, da, ca, ma = a
    kb, db, cb, mb = b
    assert np.array_equal(ca[:n], cb[:n]) and np.array_equal(ma[:n], mb[:n]) and ca[:n].min() > 100
    for i in range(n):
        c = int(ca[i])
        for f in FIELDS:
            assert np.array_equal(ka[i, :c][f], kb[i, :c][f]), (i, f)
        assert np.array_equal(da[i, :c], db[i, :c]), i


def test_hand_over_to_the_extractor(pkg, synthetic):
    """At the image size of the ORB GPU tests: the ingest writes straight into a torch device tensor and tc2li_orb_extract_batch reads it in
    place.  An image whose three channels all equal G gives the features of G; a pair with three different channels gives the features of
    the reference's gray."""
    import torch
    left, right = synthetic.stereo_pair(0)
    h, w = left.shape
    stream = torch.cuda.current_stream().cuda_stream
    ext = pkg.OrbExtractor(max_width=w, max_height=h, max_images=2)

    def features(gray_dev):
        out = ext.extract_batch_dev(gray_dev.data_ptr(), 2, w, h, w, w * h, stream=stream)
        return tuple(a.copy() for a in out)

    pair = np.stack([left, right])
    from_gray = features(torch.from_numpy(pair).cuda())
    # all three channels equal: BGR, from host memory
    prep = pkg.ImagePrep(w, h, 3, rgb=False, max_images=2)
    gray_dev = pkg.image_prep_batch(prep, np.repeat(pair[..., None], 3, axis=3), stream=stream)
    assert np.array_equal(gray_dev.cpu().numpy(), pair)
    assert_same_batch(features(gray_dev), from_gray, 2)
    # three different channels: RGB, from device memory
    colour = np.stack([pair, np.roll(pair, 2, axis=2), 255 - np.roll(pair, -3, axis=1) // 2], axis=3)
    want = ref.image_prep_batch(colour, ref.COPY, 1)
    prep_rgb = pkg.ImagePrep(w, h, 3, rgb=True, max_images=2)
    gray_dev = pkg.image_prep_batch(prep_rgb, torch.from_numpy(colour).cuda(), stream=stream)
    assert np.array_equal(gray_dev.cpu().numpy(), want)
    assert_same_batch(features(gray_dev), features(torch.from_numpy(want).cuda()), 2)
    # rectified on the way: a colour pair through different left and right maps
    maps = K.make_map("warp", w, h, w, h, 11) + K.make_map("warp", w, h, w, h, 12)
    want = ref.image_prep_batch(colour, ref.RECTIFY, 1, maps)
    prep_rect = pkg.ImagePrep(w, h, 3, rgb=True, mode=pkg.IMAGE_PREP_RECTIFY, max_images=2)
    prep_rect.set_maps(0, maps[0], maps[1])
    prep_rect.set_maps(1, maps[2], maps[3])
    gray_dev = pkg.image_prep_batch(prep_rect, torch.from_numpy(colour).cuda(), stream=stream)
    assert np.array_equal(gray_dev.cpu().numpy(), want)
    assert_same_batch(features(gray_dev), features(torch.from_numpy(want).cuda()), 2)
    for p in (prep, prep_rgb, prep_rect):
        p.close()
    ext.close()
