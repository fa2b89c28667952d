"""Reference assembly of a window's inertial term in numpy, from the oracle's edge (oracle.inertial_edge: error and 9 x 24 Jacobian of
EdgeInertial, columns P1 6 | V1 3 | G1 3 | A1 3 | P2 6 | V2 3) -- what tc2li_inertial_term_batch is compared with.
Information: inv(C[:9, :9]) symmetrised, eigenvalues below 1e-12 set to zero, times info_scale; Huber with sqrt(16.92); random-walk terms
from inv(C[9:12, 9:12]) and inv(C[12:15, 12:15]), never robust; the blocks summed in link order, in double."""
import numpy as np

HUBER_DELTA = np.sqrt(16.92)
RTOL = 1e-4  # the project's bar for a Hessian against the oracle; b in the same units (max |H_ref|), chi2 relative
_cache = {}


def information(C15, info_scale):
    inv = np.linalg.inv(C15[:9, :9])
    w, V = np.linalg.eigh((inv + inv.T) / 2)
    w[w < 1e-12] = 0.0
    return (V * w) @ V.T * info_scale, np.linalg.inv(C15[9:12, 9:12]), np.linalg.inv(C15[12:15, 12:15])


def assemble(oracle, case):
    """-> dict(chi2, H_diag [K, 15, 15], H_link [L, 15, 15], b [K, 15], c2 [L] (e' Omega e of each inertial edge))."""
    kf, fixed, link4 = case["kf33"], case["fixed"], case["link4"]
    K, L = len(kf), len(link4)
    H_diag, H_link, b, c2s, chi2 = np.zeros((K, 15, 15)), np.zeros((L, 15, 15)), np.zeros((K, 15)), np.zeros(L), 0.0
    for l, (k1, k2, robust, scale) in enumerate(link4):
        k1, k2 = int(k1), int(k2)
        err, J = oracle.inertial_edge(kf[k1], kf[k2], case["pre298"][l])
        Om, Og, Oa = information(case["C"][l], scale)
        c2 = float(err @ Om @ err)
        c2s[l] = c2
        rho0, rho1 = c2, 1.0
        if robust and c2 > HUBER_DELTA ** 2:
            rho0, rho1 = 2 * np.sqrt(c2) * HUBER_DELTA - HUBER_DELTA ** 2, HUBER_DELTA / np.sqrt(c2)
        # the edge's 24 columns and the two random-walk edges (error kf2 - kf1, Jacobians -I / +I) on 30 unknowns: kf1's 15, then kf2's
        J30 = np.zeros((9, 30))
        J30[:, :15], J30[:, 15:24] = J[:, :15], J[:, 15:]
        H30 = J30.T @ (rho1 * Om) @ J30
        g30 = -J30.T @ (rho1 * Om) @ err
        for o, info, e in ((9, Og, kf[k2][27:30] - kf[k1][27:30]), (12, Oa, kf[k2][30:33] - kf[k1][30:33])):
            Jw = np.zeros((3, 30))
            Jw[:, o:o + 3], Jw[:, 15 + o:15 + o + 3] = -np.eye(3), np.eye(3)
            H30 += Jw.T @ info @ Jw
            g30 -= Jw.T @ info @ e
            rho0 += float(e @ info @ e)
        chi2 += rho0
        if not fixed[k1]:
            H_diag[k1] += H30[:15, :15]
            b[k1] += g30[:15]
        if not fixed[k2]:
            H_diag[k2] += H30[15:, 15:]
            b[k2] += g30[15:]
        if not fixed[k1] and not fixed[k2]:
            H_link[l] = H30[:15, 15:]
    return dict(chi2=chi2, H_diag=H_diag, H_link=H_link, b=b, c2=c2s)


def reference(oracle, all_cases):
    """name -> assemble(case); computed once per session and left unchanged."""
    if not _cache:
        for name, case in all_cases.items():
            r = assemble(oracle, case)
            for a in r.values():
                if isinstance(a, np.ndarray):
                    a.setflags(write=False)
            _cache[name] = r
    return _cache


def deviations(got, want):
    """(H, b, chi2): max |dH| / max |H_ref| over the window's blocks, max |db| / max |H_ref|, |dchi2| / |chi2_ref|.  `got` is the tuple
    capi.inertial_term_batch returns or a dict as `want`.  A reference that is all zero asks for exact zeros (deviation 0 or inf)."""
    if isinstance(got, dict):
        got = (got["chi2"], got["H_diag"], got["H_link"], got["b"])
    chi2, H_diag, H_link, b = got
    scale = max(np.abs(want["H_diag"]).max(initial=0.0), np.abs(want["H_link"]).max(initial=0.0))
    dH = max(np.abs(H_diag - want["H_diag"]).max(initial=0.0), np.abs(H_link - want["H_link"]).max(initial=0.0))
    db = np.abs(b - want["b"]).max(initial=0.0)
    dc = abs(chi2 - want["chi2"])
    ratio = lambda d, s: 0.0 if d == 0 else (d / s if s > 0 else np.inf)
    return ratio(dH, scale), ratio(db, scale), ratio(dc, abs(want["chi2"]))
