"""The compact LDS form of the pose optimisation (pose_opt_kernel.hip: 33 bytes per correspondence -- map point, u, v, ur and information held as
floats -- instead of 61) against the 61-byte form, bit for bit.  The compact form is launched only when every one of those seven values of every
correspondence is a float's value; each read widens to double before any arithmetic, so poses, outlier flags and inlier counts must be the same
bytes.  TC2LI_PO_COMPACT=0 (read per call) forces the 61-byte form.

tc2li_pose_optimization_limits()["last_form"]: 1 the 61-byte LDS form, 3 the compact form after the public entry's device-side check.  The
tracking batches know their values to be floats by construction and report 1 in either layout; which kernel they launched is read from the
library's launch profile (k_pose_optimization_lds<true> is the compact instantiation)."""
import numpy as np
import pytest

from matcher_scenario import make, local_map_points
from pose_opt_cases import frame_problem

pytestmark = pytest.mark.gpu

LDS_FORM, COMPACT_FORM = 1, 3
SIZES = (3, 9, 10, 63, 64, 65, 300)


def is_float_exact(a):
    a = np.asarray(a, np.float64)
    return np.array_equal(a.astype(np.float32).astype(np.float64), a)


@pytest.fixture(scope="module")
def frames(synthetic):
    """(window, [(Xw, edges) per keyframe]): 350-374 correspondences per keyframe, every value a float's, 20 % gross outliers, 30 % monocular."""
    w = synthetic.ba_window(7, n_opt=2, n_fix=2, n_points=900, outlier_frac=0.2, mono_frac=0.3)
    out = [frame_problem(w, k, truth_points=False) for k in range(len(w["poses"]))]
    for Xw, ed in out:
        assert len(ed) >= max(SIZES) and is_float_exact(Xw) and is_float_exact(ed[:, 2:6])
    return w, out


def cut(frames, n, k, first):
    """n correspondences of keyframe k from `first` on, renumbered; stereo and monocular both present from 9 on."""
    Xw, ed = frames[k][0][first:first + n], frames[k][1][first:first + n].copy()
    assert len(ed) == n
    ed[:, 0] = np.arange(n)
    if n >= 9:
        assert (ed[:, 4] < 0).any() and (ed[:, 4] >= 0).any()
    return Xw, ed


def both_forms(pkg, monkeypatch, call):
    """-> (result in the compact form, result with the 61-byte form forced); asserts which form each launched."""
    monkeypatch.delenv("TC2LI_PO_COMPACT", raising=False)
    compact = call()
    assert pkg.pose_optimization_limits()["last_form"] == COMPACT_FORM
    monkeypatch.setenv("TC2LI_PO_COMPACT", "0")
    wide = call()
    assert pkg.pose_optimization_limits()["last_form"] == LDS_FORM
    monkeypatch.delenv("TC2LI_PO_COMPACT", raising=False)
    return compact, wide


def same_bits(a, b, tag):
    for x, y, what in zip(a, b, ("poses", "outlier flags", "inliers")):
        assert np.array_equal(np.asarray(x), np.asarray(y)) and np.asarray(x).tobytes() == np.asarray(y).tobytes(), (tag, what)


def test_compact_form_against_the_wide_form(pkg, oracle, frames, monkeypatch):
    w, fr = frames
    reclassified = 0
    for j, n in enumerate(SIZES):
        k = 2 + j % 2                      # the free keyframes: their initial pose carries the window's pose noise
        Xw, ed = cut(fr, n, k, 7 * j)
        e = pkg.pack_ba_edges(ed)
        compact, wide = both_forms(pkg, monkeypatch, lambda: pkg.pose_optimization(w["poses"][k], Xw, e, w["cam"]))
        same_bits(compact, wide, "N = %d" % n)
        print("N = %d: inliers %d, outliers %d" % (n, compact[2], int(compact[1].sum())))
        if n >= 63:
            # an optimisation worth the name, with outliers to classify in every round: the oracle's four rounds each end in a
            # classification, and the final mask is not empty
            want = oracle.pose_optimization(w["poses"][k], Xw, ed, w["cam"])
            assert np.array_equal(compact[1], want[1]) and compact[2] == want[2], n
            assert 0.1 * n <= compact[1].sum() <= 0.4 * n and compact[2] >= 0.6 * n, n
            reclassified += 1
    assert reclassified == 4


def test_batch_of_frames_of_different_sizes(pkg, frames, monkeypatch):
    w, fr = frames
    cuts = [(120, 2, 0), (2, 3, 11), (65, 0, 23), (300, 3, 31), (9, 1, 47), (0, 2, 5), (64, 2, 130)]   # one frame below 3, one empty
    probs = [cut(fr, n, k, o) for n, k, o in cuts]
    offs = np.concatenate([[0], np.cumsum([n for n, _, _ in cuts])])
    poses = np.stack([w["poses"][k] for _, k, _ in cuts])
    Xw, ed = np.concatenate([x for x, _ in probs]), pkg.pack_ba_edges(np.concatenate([e for _, e in probs]))
    monkeypatch.delenv("TC2LI_PO_COMPACT", raising=False)
    alone = {}
    for i in (0, 3, 6):
        alone[i] = pkg.pose_optimization(poses[i], probs[i][0], pkg.pack_ba_edges(probs[i][1]), w["cam"])
        assert pkg.pose_optimization_limits()["last_form"] == COMPACT_FORM
    compact, wide = both_forms(pkg, monkeypatch, lambda: pkg.pose_optimization_batch(poses, offs, Xw, ed, w["cam"]))
    same_bits(compact, wide, "batch")
    assert compact[2][1] == 0 and compact[2][5] == 0 and compact[2][3] > 150
    # a frame does not depend on its batch
    for i, a in alone.items():
        assert a[0].tobytes() == compact[0][i].tobytes() and a[2] == compact[2][i], i
        assert np.array_equal(a[1], compact[1][offs[i]:offs[i + 1]]), i


@pytest.mark.parametrize("field", ["u", "X"])
def test_a_double_that_is_no_float_keeps_the_wide_form(pkg, oracle, frames, monkeypatch, field):
    """One value of one correspondence is not a float's value: the public entry's device-side check must say so, the launch reports the
    61-byte form, and the result meets the oracle at the bar of test_pose_opt_forms_gpu.py."""
    monkeypatch.delenv("TC2LI_PO_COMPACT", raising=False)
    w, fr = frames
    n, k = 300, 3
    Xw, ed = cut(fr, n, k, 17)
    Xw, ed = Xw.copy(), ed.copy()
    if field == "u":
        ed[n - 1, 2] += 2.0 ** -30        # the last correspondence: the check must look at every one
    else:
        Xw[n // 2, 2] *= 1.0 + 2.0 ** -40
    assert not (is_float_exact(Xw) and is_float_exact(ed[:, 2:6]))
    pose, out, inl = pkg.pose_optimization(w["poses"][k], Xw, pkg.pack_ba_edges(ed), w["cam"])
    assert pkg.pose_optimization_limits()["last_form"] == LDS_FORM
    want_pose, want_out, want_inl = oracle.pose_optimization(w["poses"][k], Xw, ed, w["cam"])[:3]
    diff = float(np.abs(pose - want_pose).max())
    print("%s: inliers %d (oracle %d), max |pose - oracle| %.3e" % (field, inl, want_inl, diff))
    assert inl == want_inl and np.array_equal(out, want_out)
    assert np.allclose(pose, want_pose, rtol=1e-4, atol=1e-7) and diff < 1e-6
    # and a NaN is no float's value either: the 61-byte form, as before
    ed[n - 1, 2] = np.nan
    pkg.pose_optimization(w["poses"][k], Xw, pkg.pack_ba_edges(ed), w["cam"])
    assert pkg.pose_optimization_limits()["last_form"] == LDS_FORM


# ---- the tracking entry points --------------------------------------------------------------------------------------------------
W, H, NFEAT = 640, 240, 1000


@pytest.fixture(scope="module")
def tracking(pkg, oracle, synthetic):
    """matcher_scenario.make at its smallest -- one 640 x 240 stereo pair, 1000 features -- with the frame's features on the device."""
    import torch
    sc = make(oracle, synthetic, seed=0, w=W, h=H, nfeat=NFEAT)
    imgs = np.stack(synthetic.stereo_pair(0, W, H))
    dev = torch.from_numpy(imgs).cuda()
    ext = pkg.OrbExtractor(nfeatures=NFEAT, max_width=W, max_height=H, max_images=2)
    kps, desc, counts, _ = ext.extract_batch_dev(dev.data_ptr(), 2, W, H, W, W * H)
    n = int(counts[0])
    assert n == len(sc["keys"]) and np.array_equal(kps[0, :n]["x"], sc["keys"]["x"]) and np.array_equal(kps[0, :n]["y"], sc["keys"]["y"])
    u_right, _, _ = pkg.stereo_match_batch(ext, 1, sc["bf"], sc["b"])
    cam5 = np.float32([sc["cam4"][0], sc["cam4"][1], sc["cam4"][2], sc["cam4"][3], sc["bf"]]).astype(np.float64)
    # TrackLocalMap: the frame's stereo points as local map points, a quarter of the keypoints holding their point already
    rng = np.random.default_rng(3)
    cap = kps.shape[1]
    X_of_key = np.zeros((n, 3), np.float32)
    X_of_key[sc["order"]] = sc["Xw"]
    held, held_Xw = np.zeros((1, cap), np.uint8), np.zeros((1, cap, 3), np.float32)
    hold = (sc["depth"] > 0) & (rng.random(n) < 0.25)
    held[0, :n], held_Xw[0, :n] = hold, X_of_key
    local = np.ascontiguousarray(local_map_points(sc, oracle, rng, n_extra=100)).astype(pkg.MAP_POINT_DTYPE)
    return dict(sc=sc, ext=ext, dev=dev, kps=kps, u_right=u_right, n=n, cam5=cam5, held=held, held_Xw=held_Xw, local=local,
                local_off=np.array([0, len(local)], np.int32))


def pose_kernels(pkg, call):
    """-> (the call's outputs, the pose-optimisation kernels it launched)."""
    pkg.capi.profile_enable(True)
    try:
        pkg.capi.profile_report()
        out = call()
        names = sorted(k for k in pkg.capi.profile_report() if k.startswith("k_pose_optimization"))
    finally:
        pkg.capi.profile_enable(False)
    return out, names


def on_and_off(pkg, monkeypatch, call):
    monkeypatch.delenv("TC2LI_PO_COMPACT", raising=False)
    on, k_on = pose_kernels(pkg, call)
    monkeypatch.setenv("TC2LI_PO_COMPACT", "0")
    off, k_off = pose_kernels(pkg, call)
    monkeypatch.delenv("TC2LI_PO_COMPACT", raising=False)
    assert k_on == ["k_pose_optimization_lds<true>"] and k_off == ["k_pose_optimization_lds<false>"], (k_on, k_off)
    assert len(on) == len(off)
    for i, (a, b) in enumerate(zip(on, off)):
        assert np.array_equal(a, b) and a.tobytes() == b.tobytes(), i
    return on


def test_track_motion_model_batch_in_both_forms(pkg, tracking, monkeypatch):
    t, sc = tracking, tracking["sc"]
    last = dict(has_point=sc["has_point"], outlier=sc["outlier"], Xw=sc["Xw"], keys=sc["last_keys"], descriptors=sc["mp_desc"], pose7=sc["pose_last"])
    packed = pkg.capi.pack_last_frames([last])
    poses, mp, nm, inl = on_and_off(pkg, monkeypatch, lambda: pkg.capi.track_motion_model_batch(t["ext"], 1, t["kps"], t["u_right"], packed,
                                                                                               sc["pose_cur"][None], t["cam5"], sc["b"], 7.0))
    print("TrackWithMotionModel: %d matches, %d inliers" % (nm[0], inl[0]))
    assert nm[0] > 100 and inl[0] > 50
    assert pkg.pose_optimization_limits()["last_form"] == LDS_FORM


def test_track_local_map_batch_in_both_forms(pkg, tracking, monkeypatch):
    t, sc = tracking, tracking["sc"]
    got = on_and_off(pkg, monkeypatch, lambda: pkg.capi.track_local_map_batch(t["ext"], 1, t["kps"], t["u_right"], sc["pose_cur"][None], t["held"],
                                                                              t["held_Xw"], t["local"], t["local_off"], t["cam5"], th=3.0))
    print("TrackLocalMap: %d matches, %d inliers" % (got[3][0], got[4][0]))
    assert got[3][0] > 50 and got[4][0] > 50
    assert pkg.pose_optimization_limits()["last_form"] == LDS_FORM
