"""k_fast_cells with the packed forms of csrc/fast_forms.hpp against the oracle: every case is the smallest image that still takes the named
path.  The same cases run once more in a fresh process with TC2LI_FAST_THREADS=64 (the knob is read at the first launch)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from test_orb_gpu import assert_same_features

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def pinned_noise():
    """120 x 100 noise, a third of the pixels forced to 0 or 255: the sign and saturation edges of the 16-bit differences."""
    rng = np.random.default_rng(11)
    img = rng.integers(0, 256, (100, 120)).astype(np.uint8)
    pin = rng.random(img.shape)
    img[pin < 1 / 6] = 0
    img[pin > 5 / 6] = 255
    return img


def short_wide(synthetic):
    """640 x 120: levels 0 to 2 have two rows or one row of cells taller than 48 (the <76, 80> instantiation), level 3 a row of small ones.
    (Every level keeps a positive height inside its borders, which the reference's keypoint distribution needs.)"""
    return np.ascontiguousarray(synthetic.stereo_pair(4)[0][100:220, 300:940])


def half_flat():
    """Left half flat +-3 grey levels (no corner at either threshold: those cells run both attempts), a band of low contrast (corners only
    at the second threshold), right half textured (corners at the first)."""
    rng = np.random.default_rng(12)
    img = (100 + rng.integers(-3, 4, (150, 250))).astype(np.uint8)
    low = (100 + rng.integers(0, 14, (150, 60))).astype(np.uint8)
    low[::9, ::11] += 16
    img[:, 90:150] = low
    img[:, 150:] = rng.integers(0, 256, (150, 100)).astype(np.uint8)
    return img


def check_single(pkg, oracle, img, ini, mn, nfeatures=500):
    h, w = img.shape
    e = pkg.OrbExtractor(nfeatures=nfeatures, ini_th_fast=ini, min_th_fast=mn, max_width=w, max_height=h, max_images=1)
    o = oracle.OrbOracle(nfeatures=nfeatures, ini_th_fast=ini, min_th_fast=mn)
    want = o.extract(img)
    got = e.extract(img)
    n_cand = 0
    for lvl in range(8):
        c = o.candidates(lvl)
        n_cand += len(c)
        assert np.array_equal(e.candidates(0, lvl), c), "FAST candidates level %d" % lvl
    assert_same_features(got, want)
    e.close()
    return n_cand, len(want[1])


def check_batch(pkg, oracle, imgs, nfeatures=500):
    """Device-resident images of one size in one call against single-image calls and the oracle."""
    import torch
    n = len(imgs)
    h, w = imgs[0].shape
    dev = torch.from_numpy(np.stack(imgs)).cuda()
    e = pkg.OrbExtractor(nfeatures=nfeatures, max_width=w, max_height=h, max_images=n)
    kps, desc, counts, mono = e.extract_batch_dev(dev.data_ptr(), n, w, h, w, w * h, stream=torch.cuda.current_stream().cuda_stream)
    batch_cand = [[e.candidates(i, lvl).copy() for lvl in range(8)] for i in range(n)]
    one = pkg.OrbExtractor(nfeatures=nfeatures, max_width=w, max_height=h, max_images=1)
    o = oracle.OrbOracle(nfeatures=nfeatures)
    seen = {}
    for i, img in enumerate(imgs):
        key = img.tobytes()
        if key not in seen:
            single = one.extract(img)
            seen[key] = (single, [one.candidates(0, lvl).copy() for lvl in range(8)], o.extract(img))
        single, cand, want = seen[key]
        assert_same_features(single, want)
        assert_same_features((int(mono[i]), kps[i, :counts[i]], desc[i, :counts[i]]), single)
        for lvl in range(8):
            assert np.array_equal(batch_cand[i][lvl], cand[lvl]), (i, lvl)
    e.close()
    one.close()


def run_cases(pkg, oracle, synthetic):
    for ini, mn in ((20, 7), (12, 7)):
        n_cand, n_kp = check_single(pkg, oracle, pinned_noise(), ini, mn)
        assert n_cand > 300 and n_kp > 100
    n_cand, _ = check_single(pkg, oracle, short_wide(synthetic), 20, 7)
    assert n_cand > 100
    n_cand, _ = check_single(pkg, oracle, half_flat(), 20, 7)
    assert n_cand > 100
    three = [pinned_noise(), np.ascontiguousarray(half_flat()[:100, 100:220]), np.ascontiguousarray(short_wide(synthetic)[:100, 200:320])]
    check_batch(pkg, oracle, three)
    check_batch(pkg, oracle, [three[k % 3] for k in range(33)])  # 32 images and more: a workgroup walks four cells, the last group is partial


@pytest.mark.gpu
@pytest.mark.parametrize("ini,mn", [(20, 7), (12, 7)])
def test_pinned_noise(pkg, oracle, ini, mn):
    n_cand, n_kp = check_single(pkg, oracle, pinned_noise(), ini, mn)
    assert n_cand > 300 and n_kp > 100


@pytest.mark.gpu
def test_large_tile_instantiation(pkg, oracle, synthetic):
    n_cand, _ = check_single(pkg, oracle, short_wide(synthetic), 20, 7)
    assert n_cand > 100


@pytest.mark.gpu
def test_both_thresholds_in_one_launch(pkg, oracle):
    img = half_flat()
    n_cand, _ = check_single(pkg, oracle, img, 20, 7)
    assert n_cand > 100
    # the three kinds of cells are there: nothing at 7, something only at 7, something at 20
    assert len(oracle.fast9_16(img[:, :90], 7)) == 0
    assert len(oracle.fast9_16(img[:, 93:147], 20)) == 0 and len(oracle.fast9_16(img[:, 93:147], 7)) > 0
    assert len(oracle.fast9_16(img[:, 150:], 20)) > 0


@pytest.mark.gpu
def test_batch_of_three(pkg, oracle, synthetic):
    three = [pinned_noise(), np.ascontiguousarray(half_flat()[:100, 100:220]), np.ascontiguousarray(short_wide(synthetic)[:100, 200:320])]
    check_batch(pkg, oracle, three)


@pytest.mark.gpu
def test_batch_walks_cells_per_workgroup(pkg, oracle, synthetic):
    """From 32 images on a workgroup takes four consecutive cells of its XCD's share: 33 images leave partial groups."""
    three = [pinned_noise(), np.ascontiguousarray(half_flat()[:100, 100:220]), np.ascontiguousarray(short_wide(synthetic)[:100, 200:320])]
    check_batch(pkg, oracle, [three[k % 3] for k in range(33)])


@pytest.mark.gpu
def test_all_cases_at_64_threads(pkg, oracle):
    """TC2LI_FAST_THREADS=64 in a fresh process: the same cases, and the kernels that ran are the 64-wide instantiations."""
    env = dict(os.environ, TC2LI_FAST_THREADS="64")
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    names = [l for l in r.stdout.splitlines() if l.startswith("kernel ")]
    assert len(names) == 2 and all("64>" in l.replace(" ", "") for l in names), r.stdout


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    import tc2li_loader
    pkg_ = tc2li_loader.load()
    from oracle import pyoracle
    from tc2li_slam_amd import synthetic as synthetic_
    pkg_.capi.profile_enable(True)
    run_cases(pkg_, pyoracle, synthetic_)
    pkg_.capi.profile_enable(False)
    for name in sorted(pkg_.capi.profile_report()):
        if "k_fast_cells" in name:
            print("kernel", name)
