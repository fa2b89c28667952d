"""Writes tests/golden/culling_a.npz: a few culling problems of tests/culling_cases.py with the outputs of the restatement
tests/culling_ref.py, so that a change of the restatement itself shows (tests/test_culling.py::test_golden compares the restatement and the
host entry with it).

    python tools/make_golden_culling.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import culling_cases as K  # noqa: E402
import culling_ref as ref  # noqa: E402


def main():
    problems = [K.make_problem(700, 14, 500, (5, 9)), K.make_problem(701, 30, 1000, (6, 10), inertial=True),
                K.make_problem(702, 26, 700, (7, 12), inertial=True, abort_ba=True), K.make_problem(703, 12, 300, (5, 9), abort_ba=True)]
    out = dict(n_problems=np.int32(len(problems)))
    for i, pr in enumerate(problems):
        want = ref.keyframe_culling(pr)
        assert want["culled"] >= 1, (i, want["culled"])
        for k, v in pr.items():
            out["p%d_in_%s" % (i, k)] = np.asarray(v)
        for k in K.OUTPUTS:
            out["p%d_out_%s" % (i, k)] = np.asarray(want[k])
    pt = K.random_points(704, 2000)
    for k, v in pt.items():
        out["mp_in_" + k] = v
    out["mp_out_action"] = ref.map_point_culling(pt)
    path = os.path.join(ROOT, "tests", "golden", "culling_a.npz")
    np.savez_compressed(path, **out)
    print("%s: %d bytes" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
