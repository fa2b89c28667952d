"""Writes tests/golden/stereo_points_a.npz: three small frames of tests/stereo_points_cases.py with decisions and the outputs of the
restatement tests/stereo_points_ref.py, so that a change of the restatement itself shows (tests/test_stereo_points.py::test_golden compares
the restatement and the host entries with it).

    python tools/make_golden_stereo_points.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import stereo_points_cases as K  # noqa: E402
import stereo_points_ref as ref  # noqa: E402


def main():
    rng = np.random.default_rng(900)
    cases = [(K.frame(K.depths(40, 90, 20, 900), rng.integers(0, 3, 150), rng.random(150) < 0.2, seed=900), K.decision(frame_id=120)),
             (K.frame(K.depths(130, 60, 10, 901), rng.integers(0, 3, 200), rng.random(200) < 0.2, seed=901),
              K.decision(frame_id=120, mapper_idle=0, keyframes_in_queue=2, ref_nobs=rng.integers(-1, 8, 300).astype(np.int32))),
             (K.frame(K.depths(300, 150, 60, 902), rng.integers(0, 3, 510), rng.random(510) < 0.2, seed=902, mode=ref.ALL),
              K.decision(inertial=1, time_frame=10.5, time_last_kf=10.0))]
    out = dict(n_frames=np.int32(len(cases)), unproject4=K.UNPROJECT4)
    for i, (f, d) in enumerate(cases):
        points = ref.stereo_points(f, K.UNPROJECT4)
        decided = ref.new_keyframe(f, d, K.UNPROJECT4)
        assert points["n_created"] > 0 and decided["need"] == 1 and decided["n_created"] > 0, i
        for k, v in f.items():
            out["f%d_in_%s" % (i, k)] = np.asarray(v)
        for k, v in d.items():
            out["f%d_dec_%s" % (i, k)] = np.asarray(v)
        for k in K.POINT_OUTPUTS:
            out["f%d_points_%s" % (i, k)] = np.asarray(points[k])
        for k in K.POINT_OUTPUTS + K.DECISION_OUTPUTS:
            out["f%d_decided_%s" % (i, k)] = np.asarray(decided[k])
    path = os.path.join(ROOT, "tests", "golden", "stereo_points_a.npz")
    np.savez_compressed(path, **out)
    print("%s: %d bytes" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
