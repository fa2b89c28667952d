"""The windows of the inertial-term tests (tc2li_inertial_term_batch), all from synthetic.inertial_window(seed, n_opt=..., n_points=60): a few
keyframes each, the smallest shapes at which each path of the term can go wrong.  A case is the dict form capi.inertial_term_batch takes
(kf33, fixed, has_imu, link4, pre) plus pre298 (the oracle's form of each link's pre-integration) and C (each link's 15 x 15 covariance).

  a        n_opt=1: one link whose kf1 is fixed
  b        the same window with `fixed` all zero: one link, both ends free
  c        n_opt=3 at kf33: the robust, 1e-2-weighted link 0 is far above the Huber threshold
  d        the same window at kf33_true: every link below the threshold (the quadratic branch of a robust link), bias change exactly 0
           (the identity branch of RightJacobianSO3)
  e        c plus a link 0 -> 2 whose pre-integration spans both intervals: keyframe 2 is touched by three links (the order of its sum), the
           link joins keyframes that are not neighbours, and two links leave keyframe 0
  f_empty  c's keyframes without any link: zeros, chi2 = 0
  f_extra  c plus a covisible keyframe (fixed, has_imu = 0) that no link touches: its blocks are zero
  g        n_opt=25: 25 links, 26 keyframes (the reference's bLarge window)
"""
import numpy as np

NAMES = ("a", "b", "c", "d", "e", "f_empty", "f_extra", "g")
_cache = {}


def _window(pkg, oracle, synthetic, seed, n_opt):
    w = synthetic.inertial_window(seed, n_opt=n_opt, n_points=60)
    pre = []
    for s, t1, t2 in w["samples"]:
        p = pkg.capi.Preintegrated(w["bias6"], *synthetic.IMU_NOISE)
        p.preintegrate(s, t1, t2)
        pre.append(p)
    return w, pre


def _case(oracle, w, kf33, fixed, has_imu, link4, pre):
    fields = [p.fields() for p in pre]
    return dict(kf33=np.array(kf33, np.float64), fixed=np.array(fixed, np.uint8), has_imu=np.array(has_imu, np.uint8),
                link4=np.array(link4, np.float64).reshape(-1, 4), pre=list(pre),
                pre298=[oracle.pack_preintegrated(f, w["bias6"]) for f in fields], C=[np.asarray(f["C"], np.float64) for f in fields])


def cases(pkg, oracle, synthetic):
    """name -> case; built once per session."""
    if _cache:
        return _cache
    w1, pre1 = _window(pkg, oracle, synthetic, 1, 1)
    _cache["a"] = _case(oracle, w1, w1["kf33"], w1["fixed"], w1["has_imu"], w1["link4"], pre1)
    _cache["b"] = _case(oracle, w1, w1["kf33"], np.zeros(2), w1["has_imu"], w1["link4"], pre1)
    w3, pre3 = _window(pkg, oracle, synthetic, 0, 3)
    _cache["c"] = _case(oracle, w3, w3["kf33"], w3["fixed"], w3["has_imu"], w3["link4"], pre3)
    _cache["d"] = _case(oracle, w3, w3["kf33_true"], w3["fixed"], w3["has_imu"], w3["link4"], pre3)
    # the link 0 -> 2: the samples of both intervals, every stamp once
    (s0, t0, _), (s1, _, t2) = w3["samples"][0], w3["samples"][1]
    both = np.concatenate([s0, s1])
    both = both[np.unique(both["t"], return_index=True)[1]]
    span = pkg.capi.Preintegrated(w3["bias6"], *synthetic.IMU_NOISE)
    span.preintegrate(both, t0, t2)
    _cache["e"] = _case(oracle, w3, w3["kf33"], w3["fixed"], w3["has_imu"], np.vstack([w3["link4"], [0, 2, 0, 1.0]]), pre3 + [span])
    _cache["f_empty"] = _case(oracle, w3, w3["kf33"], w3["fixed"], w3["has_imu"], np.zeros((0, 4)), [])
    _cache["f_extra"] = _case(oracle, w3, np.vstack([w3["kf33"], w3["kf33_true"][2:3]]), np.append(w3["fixed"], 1), np.append(w3["has_imu"], 0),
                              w3["link4"], pre3)
    w25, pre25 = _window(pkg, oracle, synthetic, 2, 25)
    _cache["g"] = _case(oracle, w25, w25["kf33"], w25["fixed"], w25["has_imu"], w25["link4"], pre25)
    return _cache


def sentinel_outputs(case, value=-7.25):
    """The four output arrays of a case filled with a sentinel (what a call must leave alone)."""
    K, L = len(case["kf33"]), len(case["link4"])
    return [np.full(1, value), np.full((K, 15, 15), value), np.full((L, 15, 15), value), np.full((K, 15), value)]
