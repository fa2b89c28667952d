"""GPU tests of the inertial local-BA window: tc2li_inertial_window_batch against the host entry and the restatement
tests/inertial_window_ref.py, on every graph of tests/test_inertial_window.py, in several batch compositions, and one window carried
through tc2li_local_inertial_bundle_adjustment.  All outputs are integers or floats widened to double: the criterion is equality, nothing
is left out."""
import functools

import numpy as np
import pytest

import inertial_window_cases as K
import inertial_window_ref as ref
import test_inertial_window as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def store(pkg):
    """the world of ba_window_cases.py resident on the device; slot EMPTY_SLOT stays empty"""
    with pkg.KeyframeStore(K.WORLD_SLOTS, 64) as s:
        slots = [i for i, v in enumerate(K.WORLD) if v is not None]
        s.put_batch(slots, [K.WORLD[i] for i in slots], K.BOUNDS, n_levels=K.N_LEVELS)
        yield s


def device_run(pkg, store):
    return lambda problems, **kw: pkg.inertial_window_batch(problems, K.SIGMA, store=store, **kw)


@functools.lru_cache(maxsize=None)
def _host_family(pkg):
    return T.host_run(pkg)(T.family_of(pkg)[0])


def _check(run, problems, want, host, what):
    got = run(problems)
    assert len(got) == len(problems)
    for i, (g, h, w) in enumerate(zip(got, host, want)):
        K.assert_equal(g, h, "%s: problem %d, device against host" % (what, i))
        K.assert_equal(g, w, "%s: problem %d, device against the restatement" % (what, i))
    return got


def test_device_one_batch(pkg, store):
    problems, want = T.family_of(pkg)
    _check(device_run(pkg, store), problems, want, _host_family(pkg), "one batch")


def test_device_batches_of_one(pkg, store):
    problems, want = T.family_of(pkg)
    run = device_run(pkg, store)
    for i, (p, w, h) in enumerate(zip(problems, want, _host_family(pkg))):
        _check(run, [p], [w], [h], "problem %d alone" % i)


def test_device_shuffled_batch(pkg, store):
    problems, want = T.family_of(pkg)
    host, run = _host_family(pkg), device_run(pkg, store)
    order = np.random.default_rng(5).permutation(len(problems))
    _check(run, [problems[i] for i in order], [want[i] for i in order], [host[i] for i in order], "shuffled")
    _check(run, problems[::-1], want[::-1], host[::-1], "reversed")


def test_device_batch_of_512(pkg, store):
    """512 problems picked from the family in one call, every one at least once (the four large graphs once, the small ones often); that
    the family holds every branch is test_family_reaches_every_branch."""
    problems, want = T.family_of(pkg)
    host = _host_family(pkg)
    small = [i for i, p in enumerate(problems) if len(p["kf_slot"]) <= 40 and len(p["point_flags"]) <= 400]
    pick = np.array(small)[np.random.default_rng(6).integers(0, len(small), 512)]
    pick[:len(problems)] = np.arange(len(problems))
    got = _check(device_run(pkg, store), [problems[i] for i in pick], [want[i] for i in pick], [host[i] for i in pick], "512")
    assert len(got) == 512


@pytest.mark.parametrize("rule", T.RULES, ids=lambda r: r.__name__)
def test_device_rule(pkg, store, rule):
    """The rules one by one go through the same kernels: the hand-made graphs of test_inertial_window.py with the device entry."""
    rule(device_run(pkg, store))


def test_device_contracts(pkg, store):
    run = device_run(pkg, store)
    assert run([T._base()])[0]["status"] == ref.OK
    for what, pr, views in T.invalid_problems():
        if views is not None:                                                          # the store refuses such a keyframe at put
            continue
        for batch in ([pr], [T._base(), pr]):
            with pytest.raises(pkg.Tc2liError) as e:
                run(batch)
            assert e.value.code == T.INVALID, what
    with pytest.raises(pkg.Tc2liError) as e:                                           # slot 2 holds a higher octave than this table has
        pkg.inertial_window_batch([T._base()], K.SIGMA[:int(K.WORLD[2]["keys"]["octave"].max())], store=store)
    assert e.value.code == T.INVALID
    T.capacity_contract(run)
    assert run([]) == []


def test_device_slot_shared_by_problems_with_other_flags(pkg, store):
    """One store slot under several problems of a batch, and under several rows of one problem, with flags of their own each"""
    kfs = [dict(slot=0, id=4, prev=1, holds=[0, 1]), dict(slot=0, id=3, prev=2, holds=[1, 2]), dict(slot=0, id=2), dict(slot=0, id=1)]
    points = [dict(obs={0: 5, 1: 6, 2: 7, 3: 8}), dict(obs={0: 9, 1: -1, 3: 10}), dict(obs={1: 11, 2: 12, 3: 13})]
    batch = []
    for flags in ((12, 12, 12, 12), (12, 13, 12, 4), (4, 4, 1, 2), (3, 12, 12, 12), (12, 14, 2, 13), (8, 12, 13, 12)):
        for k, f in zip(kfs, flags):
            k["flags"] = f
        batch += [K.hand(kfs, points, 0), K.hand(kfs, points, 0, in_map=3, rec_init=True), K.hand(kfs, points, 1, in_map=2)]
    want = [ref.gather(p, K.WORLD, K.SIGMA) for p in batch]
    assert len({w["edges"].tobytes() for w in want}) > 6 and len({w["link4"].tobytes() for w in want}) > 3
    _check(device_run(pkg, store), batch, want, T.host_run(pkg)(batch), "shared slot")


def test_visual_and_inertial_gathers_in_turn(pkg, store):
    """Both entries list their points with the same code and end with the same edge kernel: on one store and in one process the visual
    gather, the inertial one and the visual one again -- with a batch of another size -- each give what their host entry gives.  Guards
    scratch or state that the two paths would share by mistake.  Hand-made graphs of 4 keyframes and 3 points, with flags that make the
    windows differ."""
    import ba_window_cases as KV
    kfs = [dict(slot=0, id=4, prev=1, holds=[0, 1]), dict(slot=0, id=3, prev=2, holds=[1, 2]), dict(slot=0, id=2), dict(slot=0, id=1)]
    points = [dict(obs={0: 5, 1: 6, 2: 7, 3: 8}), dict(obs={0: 9, 1: -1, 3: 10}), dict(obs={1: 11, 2: 12, 3: 13})]
    visual, inertial = [], []
    for vf, nf in (((0, 0, 0, 0), (12, 12, 12, 12)), ((4, 4, 1, 2), (12, 13, 12, 4)), ((0, 2, 4, 0), (8, 12, 13, 12))):
        vk, nk = [dict(k, flags=f) for k, f in zip(kfs, vf)], [dict(k, flags=f) for k, f in zip(kfs, nf)]
        visual += [KV.hand(vk, points, 0, [1]), KV.hand(vk, points, 1, [2, 0], init=2)]
        inertial += [K.hand(nk, points, 0), K.hand(nk, points, 1, in_map=3, rec_init=True)]
    host_v = pkg.ba_window_batch(visual, K.SIGMA, views=K.WORLD)
    host_i = T.host_run(pkg)(inertial)
    assert len({h["edges"].tobytes() for h in host_v}) > 2 and len({h["edges"].tobytes() for h in host_i}) > 2
    first = pkg.ba_window_batch(visual, K.SIGMA, store=store)
    second = pkg.inertial_window_batch(inertial, K.SIGMA, store=store)
    third = pkg.ba_window_batch(visual[2:], K.SIGMA, store=store)
    for i, (g, h) in enumerate(zip(first, host_v)):
        KV.assert_equal(g, h, "visual gather, problem %d" % i)
    for i, (g, h) in enumerate(zip(second, host_i)):
        K.assert_equal(g, h, "inertial gather after the visual one, problem %d" % i)
    assert len(third) == 4
    for i, (g, h) in enumerate(zip(third, host_v[2:])):
        KV.assert_equal(g, h, "visual gather after the inertial one, problem %d" % i)


def test_gathered_window_through_the_inertial_bundle_adjustment(pkg, synthetic):
    """A window gathered on the device goes into tc2li_local_inertial_bundle_adjustment and comes out as the window gathered by the
    restatement does, bit for bit -- and the optimiser accepts the arrays as they are.  The links get their preintegration through
    link_kf2_row, as INTEGRATION.md tells the shim to."""
    w = synthetic.inertial_window(seed=3, n_opt=8, n_points=300)
    views, pr, sigma = K.from_inertial_window(w)
    with pkg.KeyframeStore(len(views), max(len(v["keys"]) for v in views)) as s:
        s.put_batch(list(range(len(views))), views, K.BOUNDS, n_levels=K.N_LEVELS)
        got = pkg.inertial_window_batch([pr], sigma, store=s)[0]
    want = ref.gather(pr, views, sigma)
    K.assert_equal(got, want)
    assert got["status"] == ref.OK and got["n_points_without_edge"] == 0 and len(got["edges"]) > 400
    assert np.array_equal(got["fixed"], w["fixed"]) and np.array_equal(got["has_imu"], w["has_imu"])
    assert np.array_equal(got["link4"][::-1], w["link4"])                              # the window lists its links oldest first
    pre_of_row = {}
    for (samples, t1, t2), link in zip(w["samples"], w["link4"]):                       # the link into keyframe link[1]
        pre = pkg.capi.Preintegrated(w["bias6"], *synthetic.IMU_NOISE)
        pre.preintegrate(samples, t1, t2)
        pre_of_row[int(link[1])] = pre
    run = lambda g: pkg.capi.local_inertial_bundle_adjustment(g["kf33"], g["fixed"], g["has_imu"], w["calib24"], g["points3"],
                                                              g["edges"].astype(pkg.BA_EDGE_DTYPE), g["link4"],
                                                              [pre_of_row[int(r)] for r in g["link_kf2_row"]], w["cam"])
    a, b = run(got), run(want)
    assert a[4].iterations > 0 and a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    assert np.abs(a[0] - got["kf33"]).max() > 0                                        # the optimiser moved something
