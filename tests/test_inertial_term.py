"""tc2li_host_inertial_term_batch (the host twin of the device entry: the same per-link function, the same link-order sums) against the
numpy assembly of the oracle's edge, its validation, its linearize == 0 path and the structure of its blocks.  Needs no GPU.

Metrics (inertial_term_ref.deviations): H and b in units of max |H_ref| of the window, chi2 relative; bound 1e-4 each -- the project's bar
for a Hessian against the oracle.  chi2 is compared with the oracle where the residual is large (c, e, f_extra, g: c2 1e3 - 1e6, and a, b);
at the true state (d) the error vector is a few float ulps of the pre-integrated deltas, which the reference keeps in float, and a
relative chi2 means nothing.
Measured, host twin against the oracle (H, b, chi2): a 1.9e-11 6.0e-13 1.2e-7 | b the same | c 1.5e-8 1.7e-9 1.1e-6 | d 1.5e-8 3.6e-11 (4.6e-7) |
e 1.2e-8 1.3e-9 1.0e-6 | f_extra as c | g 3.0e-8 1.9e-9 2.6e-8."""
import copy

import numpy as np
import pytest

import inertial_term_cases as tc
import inertial_term_ref as tr

ERR_INVALID = -2
CHI2_VS_ORACLE = ("a", "b", "c", "e", "f_extra", "g")


@pytest.fixture(scope="module")
def cases(pkg, oracle, synthetic):
    return tc.cases(pkg, oracle, synthetic)


@pytest.fixture(scope="module")
def ref(oracle, cases):
    return tr.reference(oracle, cases)


@pytest.fixture(scope="module")
def host(pkg, cases):
    """every case through the host twin, each alone"""
    return {n: pkg.capi.inertial_term_batch([cases[n]], host=True)[0] for n in tc.NAMES}


def test_the_cases_take_the_branches_they_are_for(cases, ref):
    huber = tr.HUBER_DELTA ** 2
    assert ref["c"]["c2"][0] > huber and cases["c"]["link4"][0, 2] == 1             # Huber branch of the robust link
    assert np.all(ref["d"]["c2"] < 1.0) and ref["d"]["c2"][0] < huber                # quadratic branch of the robust link
    assert np.array_equal(np.float32(cases["d"]["kf33"][:, 27:33]), np.tile(np.float32(cases["d"]["pre298"][0][-6:])[[3, 4, 5, 0, 1, 2]], (4, 1)))  # dbg == 0
    assert sorted(np.concatenate([cases["e"]["link4"][:, 0], cases["e"]["link4"][:, 1]]).tolist()).count(2.0) == 3
    assert len(cases["g"]["link4"]) == 25 and len(cases["g"]["kf33"]) == 26


@pytest.mark.parametrize("name", tc.NAMES)
def test_host_twin_equals_the_reference_assembly(host, ref, name):
    dH, db, dc = tr.deviations(host[name], ref[name])
    print("%s: host twin vs oracle  H %.3g  b %.3g  chi2 %.3g" % (name, dH, db, dc))
    assert dH < tr.RTOL and db < tr.RTOL
    if name in CHI2_VS_ORACLE:
        assert dc < tr.RTOL
    if name == "f_empty":
        assert host[name][0] == 0.0 and not host[name][1].any() and not host[name][3].any()


@pytest.mark.parametrize("name", tc.NAMES)
def test_structure_of_the_blocks(cases, host, name):
    case = cases[name]
    chi2, H_diag, H_link, b = host[name]
    touched = np.zeros(len(case["kf33"]), bool)
    for l, (k1, k2, _, _) in enumerate(case["link4"]):
        touched[[int(k1), int(k2)]] = True
        if case["fixed"][int(k1)] or case["fixed"][int(k2)]:
            assert not H_link[l].any()
        else:
            # kf2 has no bias columns in the inertial edge: only the random-walk edges write there, -information on the two bias blocks
            _, Og, Oa = tr.information(case["C"][l], 1.0)
            walk = np.zeros((6, 6))
            walk[:3, :3], walk[3:, 3:] = Og, Oa
            assert H_link[l][:9, :9].any() and not H_link[l][:9, 9:].any()
            assert np.abs(H_link[l][9:, 9:] + walk).max() <= 1e-9 * np.abs(walk).max()
    for k in range(len(case["kf33"])):
        if case["fixed"][k] or not touched[k]:
            assert not H_diag[k].any() and not b[k].any()
        else:
            assert H_diag[k].any() and b[k].any()
        # Symmetric to rounding, not to the last bit: entry (i, j) is sum_k J_ki (Omega J)_kj and entry (j, i) sum_k J_kj (Omega J)_ki, two
        # different 9-term sums of doubles (2^-53 each, the products up to the block's largest entry): 1e-12 of that entry is ample, and a
        # misplaced block misses it by twelve orders.
        assert np.abs(H_diag[k] - H_diag[k].T).max(initial=0.0) <= 1e-12 * np.abs(H_diag[k]).max(initial=0.0)


def test_limits(pkg):
    lim = pkg.capi.inertial_term_limits()
    assert lim["max_keyframes"] >= 64 and lim["max_links"] >= 64


@pytest.mark.parametrize("name", tc.NAMES)
def test_cost_only_is_the_same_chi2_and_leaves_the_arrays_alone(pkg, cases, host, name):
    out = tc.sentinel_outputs(cases[name])
    before = copy.deepcopy(out)
    chi2 = pkg.capi.inertial_term_batch([cases[name]], linearize=False, host=True, out=[out])[0][0]
    assert chi2 == host[name][0]                                                    # bit for bit
    assert all(np.array_equal(out[j], before[j]) for j in (1, 2, 3))
    assert pkg.capi.inertial_term_batch([cases[name]], linearize=False, host=True)[0][1:] == (None, None, None)   # NULL arrays are fine


def test_a_window_in_a_batch_is_the_window_alone(pkg, cases, host):
    got = pkg.capi.inertial_term_batch([cases[n] for n in tc.NAMES], host=True)
    for n, g in zip(tc.NAMES, got):
        assert g[0] == host[n][0] and all(np.array_equal(g[j], host[n][j]) for j in (1, 2, 3)), n
    assert pkg.capi.inertial_term_batch([], host=True) == []


class NotPositiveDefinite:
    """a pre-integration whose covariance has a negative pivot"""

    def __init__(self, pkg, pre):
        self.p = pkg.capi.PreintegratedPOD.from_buffer_copy(pre.p)
        self.p.C[0] = -1.0


def _broken(pkg, cases):
    c, g = cases["c"], cases["g"]
    lim = pkg.capi.inertial_term_limits()

    def with_link(row, value):
        link4 = c["link4"].copy()
        link4[row[0], row[1]] = value
        return dict(c, link4=link4)

    too_many_kf = dict(g, kf33=np.tile(g["kf33"], (lim["max_keyframes"] // 26 + 1, 1)), fixed=np.tile(g["fixed"], lim["max_keyframes"] // 26 + 1),
                       has_imu=np.tile(g["has_imu"], lim["max_keyframes"] // 26 + 1))
    reps = lim["max_links"] // 25 + 1
    too_many_links = dict(g, link4=np.tile(g["link4"], (reps, 1)), pre=g["pre"] * reps)
    return [("kf2 out of range", with_link((1, 1), 4), "link 1"), ("kf1 negative", with_link((2, 0), -1), "link 2"),
            ("kf1 == kf2", with_link((1, 0), 2), "link 1"), ("no IMU state", dict(c, has_imu=np.array([1, 1, 0, 1], np.uint8)), "link 1"),
            ("null pre-integration", dict(c, pre=[c["pre"][0], None, c["pre"][2]]), "link 1"),
            ("covariance not positive definite", dict(c, pre=[c["pre"][0], c["pre"][1], NotPositiveDefinite(pkg, c["pre"][2])]), "link 2"),
            ("too many keyframes", too_many_kf, "limits"), ("too many links", too_many_links, "limits")]


@pytest.mark.parametrize("linearize", [True, False])
def test_validation_errors_name_the_window_and_the_link_and_write_nothing(pkg, cases, linearize):
    good = cases["c"]
    for what, bad, names in _broken(pkg, cases):
        outs = [tc.sentinel_outputs(good), tc.sentinel_outputs(bad)]
        before = copy.deepcopy(outs)
        with pytest.raises(pkg.capi.Tc2liError) as e:
            pkg.capi.inertial_term_batch([good, bad], linearize=linearize, host=True, out=outs)
        assert e.value.code == ERR_INVALID, what
        assert "window 1" in str(e.value) and names in str(e.value), (what, str(e.value))
        assert all(np.array_equal(a, b) for o, bo in zip(outs, before) for a, b in zip(o, bo)), what
