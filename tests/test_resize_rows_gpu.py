"""The pyramid resize walks a unit's source rows in groups, with every request of a group in flight before the first is used
(csrc/orb_kernels.hip, resize_strip_unit): every level of the pyramid stays bit for bit the oracle's at the shapes where the walk
takes another path -- destination widths that are no multiple of 4, one column strip and more than one, row ends at every dword
offset, row counts that leave every remainder against the group and the unit, batch units (16 rows, the tail kernel) and
single-image units (4 rows, a launch per level), a caller's image with a pitch, and the tail starting at another level.

Run as a program (`python tests/test_resize_rows_gpu.py WIDTH HEIGHT`) the file checks one batch in a process of its own: the tail
switch TC2LI_RESIZE_TAIL_FROM is read once per process."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTHS = (253, 257, 261, 515)
HEIGHTS = (240, 247)  # 240: the smallest level still has a row of FAST cells; 247: other remainders, an odd row count on most levels
BATCH = 33            # a chunk of 32 or more images takes 16-row units and the tail kernel


def cut_images(synthetic, n, width, height):
    """n distinct windows of one rendered stereo pair, as test_blur_row_ends cuts its image"""
    left, right = synthetic.stereo_pair(3, 1242, 375)
    imgs = np.empty((n, height, width), np.uint8)
    for i in range(n):
        src = left if i % 2 == 0 else right
        x0, y0 = 100 + (37 * i) % (1242 - 100 - width), (11 * i) % (375 - height + 1)
        imgs[i] = src[y0:y0 + height, x0:x0 + width]
    return imgs


def check_levels(ext, pyoracle, imgs, which):
    ora = pyoracle.OrbOracle(nfeatures=300)
    for i in which:
        ora.extract(imgs[i])
        for level in range(8):
            got, want = ext.pyramid_level(i, level), ora.level(level)
            assert got.shape == want.shape, (i, level, got.shape, want.shape)
            assert np.array_equal(got, want), (imgs.shape, i, level, int(np.count_nonzero(got != want)))


def check_batch(pkg, pyoracle, synthetic, width, height, pitch=None):
    import torch
    imgs = cut_images(synthetic, BATCH, width, height)
    pitch = pitch or width
    host = np.zeros((BATCH, height, pitch), np.uint8)
    host[:, :, :width] = imgs
    host[:, :, width:] = 255  # what lies between two rows is not the image
    dev = torch.from_numpy(host).cuda()
    ext = pkg.OrbExtractor(nfeatures=300, max_width=width, max_height=height, max_images=BATCH)
    ext.extract_batch_dev(dev.data_ptr(), BATCH, width, height, pitch, pitch * height)
    check_levels(ext, pyoracle, imgs, (0, BATCH // 2, BATCH - 1))
    ext.close()


@pytest.mark.parametrize("height", HEIGHTS)
@pytest.mark.parametrize("width", WIDTHS)
def test_batch_forms(pkg, oracle, synthetic, width, height):
    check_batch(pkg, oracle, synthetic, width, height)


@pytest.mark.parametrize("height", HEIGHTS)
@pytest.mark.parametrize("width", WIDTHS)
def test_single_image_forms(pkg, oracle, synthetic, width, height):
    imgs = cut_images(synthetic, 3, width, height)
    ext = pkg.OrbExtractor(nfeatures=300, max_width=width, max_height=height, max_images=1)
    for i in range(3):
        ext.extract(imgs[i])
        check_levels(ext, oracle, imgs[i:i + 1], (0,))
    ext.close()


def test_strided_batch(pkg, oracle, synthetic):
    check_batch(pkg, oracle, synthetic, 261, 247, pitch=300)


@pytest.mark.parametrize("tail_from", [1, 8])
def test_tail_switch(tail_from, monkeypatch):
    """every level in the tail kernel (1) and none (8: a launch per level with 16-row units), against the oracle like the default (3)"""
    monkeypatch.setenv("TC2LI_RESIZE_TAIL_FROM", str(tail_from))
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "515", "247"], capture_output=True, text=True, timeout=300, env=dict(os.environ))
    assert r.returncode == 0 and "levels ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    ge.build_native()
    from oracle import pyoracle
    pyoracle.build()
    import tc2li_loader
    pkg_ = tc2li_loader.load()
    from tc2li_slam_amd import synthetic as synthetic_
    check_batch(pkg_, pyoracle, synthetic_, int(sys.argv[1]), int(sys.argv[2]))
    print("levels ok (TC2LI_RESIZE_TAIL_FROM=%s)" % os.environ.get("TC2LI_RESIZE_TAIL_FROM"))
