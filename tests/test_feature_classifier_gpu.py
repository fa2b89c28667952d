"""GPU parity of the feature branch of Preprocess::velodyne_handler (tc2li_lidar_set_preprocess_features) with the CPU restatement
tests/feature_classifier_ref.py: labels, pl_surf and pl_corn byte for byte on a synthetic HDL-64 scan and on hand-built lines; the
batch entry points with the switch on against the one-scan chain; the switch off again gives the plain preprocess."""
import numpy as np
import pytest

import feature_classifier_ref as ref
from test_feature_classifier import edge_case_scan

pytestmark = pytest.mark.gpu


def as_f32(points):
    return np.ascontiguousarray(points).view(np.float32).reshape(-1, 12)


@pytest.fixture(scope="module")
def fe(pkg):
    assert pkg.device_count() >= 1
    f = pkg.LidarFrontEnd(max_points_per_scan=140000, max_scans=8)
    yield f
    f.close()


@pytest.fixture(scope="module")
def street(synthetic):
    return synthetic.lidar_scan(synthetic.Scene(1), 0)


def check_one(fe, raw, n_lines, dis_b, blind, pfns):
    fe.set_features(n_lines=n_lines, dis_b=dis_b)
    labels = None
    for pfn in pfns:
        surf, corn, lab, off = ref.classify(raw, n_lines, pfn, blind, 1e-3, dis_b)
        got = fe.process(raw, pfn, blind, 1e-3)
        g_lab, g_off = fe.labels(0)
        assert np.array_equal(g_off, off), (n_lines, dis_b, blind, pfn)
        assert g_lab.tobytes() == lab.tobytes(), (n_lines, dis_b, blind, pfn, np.nonzero(g_lab != lab)[0][:10])
        assert len(got) == len(surf) and as_f32(got).tobytes() == surf.tobytes(), (n_lines, dis_b, blind, pfn)
        g_corn = fe.corners(0)
        assert len(g_corn) == len(corn) and as_f32(g_corn).tobytes() == corn.tobytes(), (n_lines, dis_b, blind, pfn)
        labels = lab
    return labels


@pytest.mark.parametrize("n_lines,dis_b", [(64, 0.0), (32, 0.1)])
@pytest.mark.parametrize("blind", [0.0, 2.0, 8.5])
def test_street_scan_equals_restatement(fe, street, n_lines, dis_b, blind):
    lab = check_one(fe, street, n_lines, dis_b, blind, (1, 2, 3, 4) if blind == 2.0 else (1, 3))
    if (n_lines, blind) == (64, 2.0):
        assert set(np.unique(lab)) == set(range(6)), np.bincount(lab)  # every Feature label occurs


@pytest.mark.parametrize("n_lines,dis_b", [(64, 0.0), (32, 0.1), (64, 0.1), (32, 0.0)])
@pytest.mark.parametrize("blind", [0.0, 2.0, 8.5, 0.5])
def test_edge_cases_equal_restatement(fe, n_lines, dis_b, blind):
    check_one(fe, edge_case_scan(), n_lines, dis_b, blind, (1, 2, 3, 4))


def chain(pkg, fe1, raw, tree_map, state, pfn, blind):
    pre = fe1.process(raw, pfn, blind, 1e-3)
    down = fe1.voxel_filter(pre, 0.5)
    fx = fe1.feature_extraction(tree_map, down, state)
    return pre, down, fx


@pytest.mark.parametrize("form", ["0", "1"])
def test_frontend_batch_equals_one_scan_chain(pkg, oracle, synthetic, monkeypatch, form):
    import torch
    monkeypatch.setenv("TC2LI_PRE_STREAM", form)
    scene = synthetic.Scene(2)
    batch = [synthetic.lidar_scan(scene, f % 4) for f in range(7)] + [edge_case_scan()]
    batch[5] = batch[5][:40000].copy()
    down0 = oracle.voxel_grid(oracle.lidar_preprocess(synthetic.lidar_scan(scene, 0)))
    world0 = oracle.feature_extraction(oracle.KdTree(down0[:10]), down0, oracle.pack_state(*synthetic.lidar_state(0)))["world"]
    maps = []
    for _ in batch:
        m = pkg.LidarMap(); m.Build(world0); maps.append(m)
    states = np.stack([oracle.pack_state(*synthetic.lidar_state(f % 4)) for f in range(8)])
    fb = pkg.LidarFrontEnd(max_points_per_scan=140000, max_scans=8)
    fb.set_features(n_lines=64, dis_b=0.0)
    offs = np.concatenate([[0], np.cumsum([len(b) for b in batch])]).astype(np.int32)
    dev = torch.from_numpy(np.concatenate(batch).view(np.uint8)).cuda()
    counts, ori, corr = fb.frontend_batch(dev.data_ptr(), offs, maps, states, point_filter_num=2, blind=2.0)
    fe1 = pkg.LidarFrontEnd(max_points_per_scan=140000, max_scans=1)
    fe1.set_features(n_lines=64, dis_b=0.0)
    for s, raw in enumerate(batch):
        m1 = pkg.LidarMap(); m1.Build(world0)
        pre, down, fx = chain(pkg, fe1, raw, m1, states[s], 2, 2.0)
        assert (counts[0, s], counts[1, s], counts[2, s]) == (len(pre), len(down), fx["effct_feat_num"]), s
        assert len(pre) == len(ref.classify(raw, 64, 2, 2.0, 1e-3)[0]) if s in (0, 7) else True
        k = fx["effct_feat_num"]
        assert ori[s, :k].tobytes() == fx["cloud_ori"].tobytes() and corr[s, :k].tobytes() == fx["corr_normvect"].tobytes(), s
        m1.close()
    assert counts[2, 0] > 100
    for m in maps:
        m.close()
    fb.close(); fe1.close()


def test_inertial_batch_with_features(pkg, oracle, synthetic):
    import torch
    from test_inertial_lidar_gpu import COV12, build_batch
    from test_undistort_gpu import lidar_state24
    seqs = build_batch(pkg, oracle, synthetic, 3)
    S = len(seqs)
    raw = np.concatenate([q["raw"] for q in seqs])
    offs = np.concatenate([[0], np.cumsum([len(q["raw"]) for q in seqs])]).astype(np.int32)
    dev = torch.from_numpy(raw.view(np.uint8)).cuda()
    stream = torch.cuda.current_stream().cuda_stream
    results = []
    for prepared in (False, True):
        fe = pkg.LidarFrontEnd(max_points_per_scan=int(max(len(q["raw"]) for q in seqs)), max_scans=S)
        fe.set_features(n_lines=64)
        maps = []
        for q in seqs:
            m = pkg.LidarMap(); m.Build(q["world0"]); maps.append(m)
        args = (maps, np.stack([q["x"] for q in seqs]), np.stack([q["P"] for q in seqs]), [q["imu"] for q in seqs],
                np.array([q["times"] for q in seqs]), COV12)
        if prepared:
            fe.inertial_prepare_batch(dev.data_ptr(), offs, stream=stream)
            out = fe.inertial_frontend_batch(None, offs, *args, max_iter=3, stream=stream)
        else:
            out = fe.inertial_frontend_batch(dev.data_ptr(), offs, *args, max_iter=3, stream=stream)
        results.append(out)
        for m in maps:
            m.close()
        fe.close()
    (xs, Ps, stats, n_pre, n_down, last), other = results[0], results[1]
    for a, b in zip((xs, Ps, n_pre, n_down, last), (other[0], other[1], other[3], other[4], other[5])):
        assert np.array_equal(a, b)
    for s, q in enumerate(seqs):
        assert n_pre[s] == len(ref.classify(q["raw"], 64, 2, 2.0, 1e-3)[0])
        # one scan at a time with the switch on, in the reference's order
        fe1 = pkg.LidarFrontEnd(max_points_per_scan=len(q["raw"]), max_scans=1)
        fe1.set_features(n_lines=64)
        m1 = pkg.LidarMap(); m1.Build(q["world0"])
        pts = fe1.process(q["raw"])
        x, P, poses, l6 = pkg.capi.lidar_imu_propagate_cov(q["x"], q["P"], COV12, q["imu"], *q["times"], np.zeros(6))
        down = fe1.voxel_filter(fe1.undistort(pts, poses, lidar_state24(x)))
        x2, P2, st = fe1.eskf_update(m1, down, x, P, max_iter=3)
        assert (n_pre[s], n_down[s]) == (len(pts), len(down))
        assert np.array_equal(xs[s], x2) and np.array_equal(Ps[s], P2) and np.array_equal(last[s], l6)
        assert stats[s].effct_feat_num == st.effct_feat_num and stats[s].effct_feat_num > 100
        m1.close(); fe1.close()


def test_switch_off_again_is_the_plain_preprocess(fe, oracle, street):
    fe.set_features(n_lines=64)
    on = fe.process(street, 2, 2.0, 1e-3)
    fe.set_features(None)
    off = fe.process(street, 2, 2.0, 1e-3)
    want = oracle.lidar_preprocess(street, 2, 2.0, 1e-3)
    assert off.tobytes() == want.tobytes() and len(on) != len(off)
    with pytest.raises(Exception):
        fe.corners(0)  # the last preprocess ran with the switch off
