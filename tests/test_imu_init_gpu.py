"""The batched inertial optimisation of the IMU initialisation on the device (tc2li_inertial_optimization_batch,
tc2li_inertial_scale_refinement_batch; k_ii_optimize / k_ii_refine, csrc/imu_init_kernels.hip) against the oracle at the bars
test_imu_init.py applies to the host entry, against the host entry where the control flow must be the same, and against itself: a map's
results are the same bits alone, in any batch, from call to call and from two threads.  The problems are imu_init_cases.py's; that they
reach the branches they were designed for is settled on the CPU (test_imu_init_batch.py)."""
import ctypes as C
import threading

import numpy as np
import pytest

import imu_init_cases as ic

pytestmark = pytest.mark.gpu


def device(pkg, problems):
    return pkg.capi.inertial_optimization_batch(problems)


def host(pkg, p):
    return ic.plain(pkg.capi.inertial_optimization_batch([p], host=True)[0])


def solo(pkg, oracle, synthetic, name):
    """The device's result of one form run alone (once per session)."""
    return ic.shared(("solo", name), lambda: ic.plain(device(pkg, [ic.case(pkg, oracle, synthetic, name)])[0]))


def figures(what, got, want):
    got, want = ic.plain(got), ic.plain(want)
    print("%s: iterations %s / %s, trials %s / %s, chi2 %r / %r, lambda %r / %r, largest state difference %.3e" % (
        what, got["iterations"], want["iterations"], got.get("trials"), want.get("trials"), tuple(got["chi2"]), tuple(want["chi2"]), got.get("final_lambda"),
        want.get("final_lambda"), ic.state_difference(got, want)))


@pytest.mark.parametrize("name", ic.FORMS)
def test_against_the_oracle(pkg, oracle, synthetic, name):
    """default: the knife-edge tail, states only; mild: iterations within 2; mono; fixed_vel; mono + fixed_vel (m = 3, no velocity blocks);
    prior_g = 0 (lambda_0 from the largest diagonal entry); the refinement form (the same number of Gauss-Newton steps)."""
    p = ic.case(pkg, oracle, synthetic, name)
    got, want = solo(pkg, oracle, synthetic, name), ic.shared(("oracle", name), lambda: ic.oracle_result(oracle, p))
    figures(name, got, want)
    assert ic.within_bars(got, want, iterations={"mild": 2, "refine": 0}.get(name)) == []
    if name == "fixed_vel" or name == "mono_fixed_vel":
        assert np.array_equal(got["vel"], np.asarray(p["vel"], np.float64)) and np.array_equal(got["bg"], p["bg"]) and np.array_equal(got["ba"], p["ba"])
    if name != "refine":
        assert got["stats_iterations"] == got["iterations"] and got["trials"] >= got["iterations"]


@pytest.mark.parametrize("name", ic.EXACT)
def test_exact_control_flow(pkg, oracle, synthetic, name):
    """Capped at 1, 2 and 3 iterations, far from convergence: the same iterations and trials as the host entry, lambda to 1e-9 relative (it is
    a product of the same few factors: only a different decision moves it)."""
    p = ic.case(pkg, oracle, synthetic, name)
    caps = [dict(p, iterations=cap) for cap in (1, 2, 3)]
    for cap, got in zip((1, 2, 3), device(pkg, caps)):
        got, want = ic.plain(got), host(pkg, dict(p, iterations=cap))
        figures("%s capped at %d" % (name, cap), got, want)
        assert (got["iterations"], got["trials"]) == (want["iterations"], want["trials"])
        assert abs(got["final_lambda"] - want["final_lambda"]) <= 1e-9 * want["final_lambda"]
        assert ic.within_bars(got, want) == []


@pytest.mark.parametrize("name", ic.FORMS)
def test_zero_iterations_return_the_inputs(pkg, oracle, synthetic, name):
    p = ic.case(pkg, oracle, synthetic, name)
    got = ic.plain(device(pkg, [dict(p, iterations=0)])[0])
    assert got["iterations"] == 0 and got["chi2"][0] == got["chi2"][1] and got["chi2"][0] > 0
    assert np.array_equal(got["Rwg"], np.asarray(p["Rwg"], np.float64)) and got["scale"] == p["scale"]
    if name != "refine":
        assert got["trials"] == 0
        assert np.array_equal(got["vel"], np.asarray(p["vel"], np.float64)) and np.array_equal(got["bg"], p["bg"]) and np.array_equal(got["ba"], p["ba"])


@pytest.mark.parametrize("name", ic.SHAPES)
def test_shapes(pkg, oracle, synthetic, name):
    """One link; two; 64 and 65 links (sixteen links per pass, 256 lanes per cost sum: four full passes, and one link into a fifth); a NULL
    link in the middle; a keyframe with no link on either side (its S is lambda I); a NULL link at pre[1].  Against the oracle, and against
    the host entry where the oracle cannot run (it has no notion of a missing link)."""
    p = ic.shape_case(pkg, oracle, synthetic, name)
    got = ic.plain(device(pkg, [p])[0])
    want = host(pkg, p) if any(q is None for q in p["pres"][1:]) else ic.oracle_result(oracle, p)
    figures(name, got, want)
    assert ic.within_bars(got, want) == []


def test_a_mixed_batch_equals_the_solo_runs(pkg, oracle, synthetic):
    """The seven forms in one call -- two launches, one per overload -- and in another order."""
    problems = [ic.case(pkg, oracle, synthetic, n) for n in ic.FORMS]
    for order in (list(range(7)), [6, 2, 5, 0, 4, 1, 3]):
        for k, got in zip(order, device(pkg, [problems[k] for k in order])):
            assert ic.same_bits(got, solo(pkg, oracle, synthetic, ic.FORMS[k])), ic.FORMS[k]
    # the refinement entry: the same kernel, flag or no flag
    refine = dict(problems[6])
    for flag in (True, False):
        refine["refine"] = flag
        assert ic.same_bits(pkg.capi.inertial_scale_refinement_batch([refine])[0], solo(pkg, oracle, synthetic, "refine"))


def test_more_workgroups_than_compute_units(pkg, oracle, synthetic):
    names = ("mild", "mono", "prior_g_zero")
    problems = [ic.case(pkg, oracle, synthetic, n) for n in names]
    got = device(pkg, [problems[i % 3] for i in range(258)])
    assert len(got) == 258
    for i, g in enumerate(got):
        assert ic.same_bits(g, solo(pkg, oracle, synthetic, names[i % 3])), i


def test_call_to_call_and_two_threads(pkg, oracle, synthetic):
    names = ("default", "mono", "refine", "n66")
    problems = [ic.case(pkg, oracle, synthetic, n) for n in names[:3]] + [ic.shape_case(pkg, oracle, synthetic, "n66")]
    first = device(pkg, problems)
    for a, b in zip(first, device(pkg, problems)):
        assert ic.same_bits(a, b)
    out = [None, None]

    def work(k):
        out[k] = [device(pkg, problems if k == 0 else problems[::-1]) for _ in range(3)]
    threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for t in threads: t.start()
    for t in threads: t.join()
    for k in range(2):
        assert out[k] is not None
        for res in out[k]:
            for a, b in zip(first, res if k == 0 else res[::-1]):
                assert ic.same_bits(a, b)


def test_the_keyframe_limit(pkg, oracle, synthetic):
    """A map at the first form's limit runs and agrees with the host entry (three iterations keep it short); one keyframe more is refused
    with nothing written."""
    n = pkg.capi.inertial_init_limits()["max_keyframes"]
    w = ic.world(pkg, oracle, synthetic, 9, n)
    p = ic.first_form(w, prior_g=1.0, prior_a=1e3, iterations=3)
    got, want = ic.plain(device(pkg, [p])[0]), host(pkg, p)
    figures("%d keyframes" % n, got, want)
    assert got["iterations"] == 3 and ic.within_bars(got, want) == []
    more = dict(p, Rwb=np.concatenate([p["Rwb"], p["Rwb"][-1:]]), twb=np.concatenate([p["twb"], p["twb"][-1:]]), vel=np.concatenate([p["vel"], p["vel"][-1:]]),
                pres=p["pres"] + [p["pres"][-1]])
    arr, outs, keep = pkg.capi.pack_inertial_init_problems([p, more])
    before = [{k: (bytes(v) if k == "stats" else v.tobytes()) for k, v in o.items() if v is not None} for o in outs]
    f = pkg.lib().tc2li_inertial_optimization_batch
    f.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    assert f(C.addressof(arr), 2, None) == -2 and "problem 1" in pkg.lib().tc2li_last_error().decode()
    assert before == [{k: (bytes(v) if k == "stats" else v.tobytes()) for k, v in o.items() if v is not None} for o in outs]
    del keep
