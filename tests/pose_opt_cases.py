"""Inputs of the pose-optimisation tests (test_ba_gpu.py, test_pose_opt_forms_gpu.py): one frame of a synthetic.ba_window() as the
arguments of PoseOptimization."""
import numpy as np


def frame_problem(w, k, truth_points=True):
    """Keyframe k of the window -> (Xw [n, 3], edges [n, 6]): its observations with their map points, the edges renumbered 0..n-1."""
    ed = w["edges"][w["edges"][:, 1] == k].copy()
    Xw = (w["points_true"] if truth_points else w["points"])[ed[:, 0].astype(int)]
    ed[:, 0] = np.arange(len(ed)); ed[:, 1] = 0
    return Xw, ed
