"""The batched inertial optimisation of the IMU initialisation (include/tc2li_hip.h "IMU initialisation: the inertial optimisation,
batched"; Optimizer::InertialOptimization, both overloads, SF/src/Optimizer.cc:2169-2356 and 2359-2466), the part that needs no GPU: the
host batch entries against the single-problem entries, the limits, every refusal of the host and of the device entries (a device entry
validates before it looks for a device), the shared chain step, and that the designed cases of imu_init_cases.py reach the branches they
were designed for."""
import ctypes as C

import numpy as np
import pytest

import imu_init_cases as ic

ERR_INVALID = -2


def single(pkg, p):
    """The single-problem entry on a problem of the batch layout -> the batch entries' result layout."""
    if p.get("refine"):
        R, s, it, chi = pkg.capi.inertial_scale_refinement(p["Rwb"], p["twb"], p["vel"], p["bg3"], p["ba3"], p["pres"], p["Rwg"], p["scale"],
                                                           iterations=p.get("iterations", 10))
        return dict(Rwg=R, scale=s, iterations=it, chi2=chi)
    v, R, s, g, a, st = pkg.capi.inertial_optimization(p["Rwb"], p["twb"], p["vel"], p["pres"], p["Rwg"], p["scale"], p["bg"], p["ba"], mono=p.get("mono", False),
                                                       fixed_vel=p.get("fixed_vel", False), prior_g=p.get("prior_g", 1e2), prior_a=p.get("prior_a", 1e6),
                                                       iterations=p.get("iterations", 200))
    return dict(Rwg=R, scale=s, iterations=st.iterations, vel=v, bg=g, ba=a, stats=st)


@pytest.fixture(scope="module")
def problems(pkg, oracle, synthetic):
    return [ic.case(pkg, oracle, synthetic, n) for n in ic.FORMS] + [ic.shape_case(pkg, oracle, synthetic, n) for n in ic.SHAPES]


def test_host_batch_equals_the_single_entries(pkg, problems):
    """Mixed forms and sizes (2 .. 66 keyframes, NULL links, both overloads) in one call; then more problems than the pool has threads."""
    want = [single(pkg, p) for p in problems]
    got = pkg.capi.inertial_optimization_batch(problems, host=True)
    assert len(got) == len(problems)
    for p, g, w in zip(problems, got, want):
        assert ic.same_bits(g, w), ic.plain(g)
    many = [problems[i % 5] for i in range(3 * pkg.capi.host_threads()["budget"] + 5)]
    for i, g in enumerate(pkg.capi.inertial_optimization_batch(many, host=True)):
        assert ic.same_bits(g, want[i % 5]), i
    # the refinement entry takes every problem in the second form, flag or no flag
    refine = dict(problems[ic.FORMS.index("refine")])
    for flag in (True, False):
        refine["refine"] = flag
        got = pkg.capi.inertial_scale_refinement_batch([refine], host=True)[0]
        assert ic.same_bits(got, want[ic.FORMS.index("refine")])


def test_empty_batch(pkg):
    assert pkg.capi.inertial_optimization_batch([], host=True) == [] and pkg.capi.inertial_scale_refinement_batch([], host=True) == []
    for name in ("tc2li_host_inertial_optimization_batch", "tc2li_host_inertial_scale_refinement_batch"):
        f = getattr(pkg.lib(), name)
        f.argtypes = [C.c_void_p, C.c_int]
        assert f(None, 0) == 0 and f(None, 1) == ERR_INVALID and f(None, -1) == ERR_INVALID


def test_limits(pkg):
    for name in ("tc2li_inertial_optimization_batch", "tc2li_inertial_scale_refinement_batch", "tc2li_host_inertial_optimization_batch",
                 "tc2li_host_inertial_scale_refinement_batch", "tc2li_inertial_init_limits", "tc2li_inertial_init_arrow_pivot"):
        assert name in pkg.exported_symbols() and hasattr(pkg.lib(), name), name
    lim = pkg.capi.inertial_init_limits()
    assert lim["max_keyframes"] >= 256 and lim["max_refine_keyframes"] >= 4096 and lim["max_iterations"] >= 200
    f = pkg.lib().tc2li_inertial_init_limits
    f.argtypes = [C.c_void_p, C.c_int]
    out = (C.c_int32 * 3)()
    assert f(out, 2) == ERR_INVALID and f(None, 3) == ERR_INVALID and f(out, 3) == 3


def _bad_covariance(pkg, p, link):
    """The problem with a copy of one link whose covariance is not positive definite."""
    q = dict(p, pres=list(p["pres"]))
    bad = pkg.capi.Preintegrated(np.zeros(6), 1.0, 1.0, 1.0, 1.0)
    C.memmove(C.addressof(bad.p), C.addressof(p["pres"][link].p), C.sizeof(bad.p))
    bad.p.C[0] = -1.0
    q["pres"][link] = bad
    return q


def _refusals(pkg, oracle, synthetic, device):
    first, refine = ic.case(pkg, oracle, synthetic, "mild"), ic.case(pkg, oracle, synthetic, "refine")
    lim = pkg.capi.inertial_init_limits()
    out = [("one keyframe", dict(first, n_keyframes=1)), ("negative iterations", dict(first, iterations=-1)),
           ("bad covariance", _bad_covariance(pkg, first, 4)), ("refine bad covariance", _bad_covariance(pkg, refine, 2))]
    for key in ("Rwb", "twb", "vel", "pres", "Rwg", "scale", "bg", "ba"):
        out.append(("null " + key, dict(first, **{key: None}, n_keyframes=len(first["Rwb"]))))
    for key in ("bg3", "ba3"):
        out.append(("null " + key, dict(refine, **{key: None})))
    if device:
        out.append(("iterations beyond the limit", dict(first, iterations=lim["max_iterations"] + 1)))
        out.append(("refine iterations beyond the limit", dict(refine, iterations=lim["max_iterations"] + 1)))
        n = lim["max_refine_keyframes"] + 1
        w = ic.world(pkg, oracle, synthetic, 7, 3)
        big = dict(Rwb=np.tile(np.eye(3).reshape(1, 9), (n, 1)), twb=np.zeros((n, 3)), vel=np.zeros((n, 3)), pres=[None] + [w["pres"][1]] * (n - 1), Rwg=np.eye(3),
                   scale=1.0, bg3=np.zeros((n, 3)), ba3=np.zeros((n, 3)), refine=True)
        out.append(("refine keyframes beyond the limit", big))
        # (the first form's keyframe limit + 1 is refused in test_imu_init_gpu.py beside the run at the limit)
    return first, out


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_refusals_write_nothing(pkg, oracle, synthetic, device):
    """TC2LI_ERR_INVALID naming the problem, before any launch (the device entries need no device to refuse), every output as it was."""
    good, cases = _refusals(pkg, oracle, synthetic, device)
    f = getattr(pkg.lib(), "tc2li_inertial_optimization_batch" if device else "tc2li_host_inertial_optimization_batch")
    f.argtypes = [C.c_void_p, C.c_int] + ([C.c_void_p] if device else [])
    for what, bad in cases:
        arr, outs, keep = pkg.capi.pack_inertial_init_problems([good, bad])
        for o in outs:  # what the call could write, marked
            o["stats"].iterations, o["stats"].final_chi2 = -77, -77.0
            o["chi2"][:] = -77.0
            o["iterations_run"][:] = -77
        before = [{k: (bytes(v) if k == "stats" else None if v is None else v.tobytes()) for k, v in o.items()} for o in outs]
        rc = f(C.addressof(arr), 2, None) if device else f(C.addressof(arr), 2)
        text = pkg.lib().tc2li_last_error().decode()
        assert rc == ERR_INVALID, (what, rc, text)
        assert "problem 1" in text, (what, text)
        after = [{k: (bytes(v) if k == "stats" else None if v is None else v.tobytes()) for k, v in o.items()} for o in outs]
        assert before == after, what
        del keep


def test_chain_step_refuses_a_singular_block(pkg):
    """ii_arrow_pivot, the step of the block factorisation that the kernel's chain and the host entry's ArrowSystem::solve both run: a
    singular or non-finite S makes the trial fail (ok2 == false) instead of producing a NaN state."""
    piv = pkg.capi.inertial_init_arrow_pivot
    assert piv(np.zeros((3, 3)), None, None, 0.0) is None
    assert piv(np.ones((3, 3)), None, None, 0.0) is None                                   # rank 1
    assert piv(np.diag([1.0, np.inf, 1.0]), None, None, 0.0) is None and piv(np.diag([1.0, np.nan, 1.0]), None, None, 0.0) is None
    # D - L Sinv_prev L' cancels exactly: singular through the block above
    assert piv(np.eye(3), np.eye(3), np.eye(3), 0.0) is None
    assert np.array_equal(piv(np.zeros((3, 3)), None, None, 2.0), np.eye(3) / 2)           # a keyframe without links: S = lambda I
    rng = np.random.default_rng(11)
    A = rng.normal(size=(3, 3)); D = A @ A.T + 3 * np.eye(3)
    L = rng.normal(size=(3, 3)) * 0.3
    B = rng.normal(size=(3, 3)); Sp = np.linalg.inv(B @ B.T + 2 * np.eye(3))
    assert np.allclose(piv(D, L, Sp, 0.5), np.linalg.inv(D + 0.5 * np.eye(3) - L @ Sp @ L.T), rtol=1e-12, atol=1e-14)


def test_designed_cases_reach_their_branches(pkg, oracle, synthetic):
    """Conditions on the INPUTS of test_imu_init_gpu.py, settled on the CPU: host entry and oracle run here."""
    host = lambda p: ic.plain(pkg.capi.inertial_optimization_batch([p], host=True)[0])
    # the exact-count cases: host entry and oracle take the same decisions at 1, 2 and 3 iterations, and a rejected trial is among them
    rejected = 0
    for name in ic.EXACT:
        p = ic.case(pkg, oracle, synthetic, name)
        for cap in (1, 2, 3):
            h, o = host(dict(p, iterations=cap)), ic.oracle_result(oracle, dict(p, iterations=cap))
            assert (h["iterations"], h["trials"]) == (o["iterations"], o["trials"]) and h["iterations"] == cap, (name, cap, h, o)
            rejected += h["trials"] > h["iterations"]
        # far from convergence: the full run goes on for longer
        assert host(p)["iterations"] > 3, name
    assert rejected >= 2
    # every form against the oracle at the bars, so that what the GPU tests compare with is a well-posed problem
    for name in ic.FORMS:
        p = ic.case(pkg, oracle, synthetic, name)
        assert ic.within_bars(host(p), ic.oracle_result(oracle, p)) == [], name
    p = ic.case(pkg, oracle, synthetic, "mono")
    h = host(p)
    assert h["scale"] != 1.0 and not np.array_equal(h["vel"], p["vel"])
    p = ic.case(pkg, oracle, synthetic, "fixed_vel")
    h = host(p)
    assert np.array_equal(h["vel"], p["vel"]) and np.array_equal(h["bg"], p["bg"]) and h["scale"] == 1.0 and not np.array_equal(h["Rwg"], p["Rwg"])
    p = ic.case(pkg, oracle, synthetic, "mono_fixed_vel")
    h = host(p)
    assert np.array_equal(h["vel"], p["vel"]) and h["scale"] != 1.0
    # prior_g == 0: lambda_0 is 1e-5 of the largest diagonal entry, not 1e3 -- one accepted step leaves lambda_0 / 3
    h = host(dict(ic.case(pkg, oracle, synthetic, "prior_g_zero"), iterations=1))
    assert h["trials"] == 1 and abs(h["final_lambda"] - 1e3 / 3) > 1.0
    h = host(dict(ic.case(pkg, oracle, synthetic, "mild"), iterations=1))
    assert h["trials"] == 1 and h["final_lambda"] == 1e3 / 3
    p = ic.case(pkg, oracle, synthetic, "refine")
    h = host(p)
    assert h["iterations"] == 10 and h["chi2"][1] < h["chi2"][0]
    # the shapes: sizes, where the links are missing, and that each is a problem the reference solves to the bars where it can run
    sizes = {n: len(ic.shape_case(pkg, oracle, synthetic, n)["Rwb"]) for n in ic.SHAPES}
    assert (sizes["n2"], sizes["n3"], sizes["n65"], sizes["n66"]) == (2, 3, 65, 66)
    missing = {n: [i for i, q in enumerate(ic.shape_case(pkg, oracle, synthetic, n)["pres"]) if i and q is None] for n in ic.SHAPES}
    assert missing["null_middle"] == [6] and missing["lonely_keyframe"] == [5, 6] and missing["null_first"] == [1]
    for name in ic.SHAPES:
        p = ic.shape_case(pkg, oracle, synthetic, name)
        h = host(p)
        assert h["iterations"] >= 1 and h["chi2"][1] < h["chi2"][0], name
        # (one link: the initial cost is a single edge's rotation error, where the host entry's float normalisation of dR and the oracle's
        # already differ by 1e-5 of it -- a property of the host entry, not of the input)
        if not missing[name] and name != "n2":
            assert ic.within_bars(h, ic.oracle_result(oracle, p)) == [], name
