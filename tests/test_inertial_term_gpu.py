"""tc2li_inertial_term_batch on the device against the numpy assembly of the oracle's edge and against the host twin, every case alone; then
batches of mixed sizes, in which every window must have the bits it has alone, from call to call; and the linearize == 0 path.

Metrics and bound as tests/test_inertial_term.py: H and b in units of max |H_ref| of the window, chi2 relative, 1e-4 each; chi2 against the
oracle on the large-residual cases only, on d between device and host twin only.  The device and the host twin run the same per-link
function, so they differ by contraction and libm alone.
Measured on an MI355X (H, b, chi2): see DESIGN.md section 4, "Inertial term on the device"."""
import copy

import numpy as np
import pytest

import inertial_term_cases as tc
import inertial_term_ref as tr

pytestmark = pytest.mark.gpu
CHI2_VS_ORACLE = ("a", "b", "c", "e", "f_extra", "g")


@pytest.fixture(scope="module")
def cases(pkg, oracle, synthetic):
    return tc.cases(pkg, oracle, synthetic)


@pytest.fixture(scope="module")
def ref(oracle, cases):
    return tr.reference(oracle, cases)


@pytest.fixture(scope="module")
def alone(pkg, cases):
    """every case through the device entry, each in a call of its own"""
    return {n: pkg.capi.inertial_term_batch([cases[n]])[0] for n in tc.NAMES}


@pytest.fixture(scope="module")
def host(pkg, cases):
    return {n: pkg.capi.inertial_term_batch([cases[n]], host=True)[0] for n in tc.NAMES}


def same_bits(x, y):
    return x[0] == y[0] and all(np.array_equal(x[j], y[j]) for j in (1, 2, 3))


@pytest.mark.parametrize("name", tc.NAMES)
def test_device_equals_the_reference_assembly_and_the_host_twin(alone, host, ref, name):
    dH, db, dc = tr.deviations(alone[name], ref[name])
    hH, hb, hc = tr.deviations(alone[name], dict(zip(("chi2", "H_diag", "H_link", "b"), host[name])))
    print("%s: device vs oracle  H %.3g  b %.3g  chi2 %.3g | device vs host twin  H %.3g  b %.3g  chi2 %.3g" % (name, dH, db, dc, hH, hb, hc))
    assert dH < tr.RTOL and db < tr.RTOL
    if name in CHI2_VS_ORACLE:
        assert dc < tr.RTOL
    assert hH < tr.RTOL and hb < tr.RTOL and hc < tr.RTOL
    if name == "f_empty":
        assert alone[name][0] == 0.0 and not alone[name][1].any() and not alone[name][3].any()


def _batches(cases):
    """Mixed sizes, and 70 copies of c; one more one-link window ends each, which makes the links 41 and 211: odd, so no power of two that a
    workgroup may take divides them and the grid's last workgroup is partly filled."""
    mixed = ["g", "a", "e", "c", "f_empty", "d", "b", "f_extra", "a"]
    many = ["c"] * 70 + ["a"]
    assert sum(len(cases[n]["link4"]) for n in mixed) == 41 and sum(len(cases[n]["link4"]) for n in many) == 211
    return mixed, many


def test_every_window_of_a_batch_has_the_bits_it_has_alone(pkg, cases, alone):
    for names in _batches(cases):
        got = pkg.capi.inertial_term_batch([cases[n] for n in names])
        for i, (n, g) in enumerate(zip(names, got)):
            assert same_bits(g, alone[n]), (i, n)
        again = pkg.capi.inertial_term_batch([cases[n] for n in names])
        assert all(same_bits(x, y) for x, y in zip(got, again))
    assert pkg.capi.inertial_term_batch([]) == []


def test_cost_only_is_the_same_chi2_and_leaves_the_arrays_alone(pkg, cases, alone):
    for names in _batches(cases):
        outs = [tc.sentinel_outputs(cases[n]) for n in names]
        before = copy.deepcopy(outs)
        got = pkg.capi.inertial_term_batch([cases[n] for n in names], linearize=False, out=outs)
        for n, g, o, bo in zip(names, got, outs, before):
            assert g[0] == alone[n][0], n                                           # bit for bit
            assert all(np.array_equal(o[j], bo[j]) for j in (1, 2, 3)), n
    assert [g[0] for g in pkg.capi.inertial_term_batch([cases[n] for n in tc.NAMES], linearize=False)] == [alone[n][0] for n in tc.NAMES]   # NULL arrays


def test_validation_comes_before_any_launch(pkg, cases):
    c = cases["c"]
    bad = dict(c, pre=[c["pre"][0], None, c["pre"][2]])
    outs = [tc.sentinel_outputs(c), tc.sentinel_outputs(bad)]
    before = copy.deepcopy(outs)
    with pytest.raises(pkg.capi.Tc2liError) as e:
        pkg.capi.inertial_term_batch([c, bad], out=outs)
    assert e.value.code == -2 and "window 1" in str(e.value) and "link 1" in str(e.value)
    assert all(np.array_equal(a, b) for o, bo in zip(outs, before) for a, b in zip(o, bo))
