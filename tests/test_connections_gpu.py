"""GPU tests of the covisibility update: tc2li_update_connections_batch and tc2li_update_best_covisibles_batch against the host entries and
the restatement tests/connections_ref.py, on every problem of tests/test_connections.py, in several batch compositions.  All outputs are
integers: the criterion is equality, nothing is left out."""
import functools

import numpy as np
import pytest

import connections_cases as K
import connections_ref as ref
import test_connections as T

pytestmark = pytest.mark.gpu


def _family(pkg):
    return T.family(pkg.connections_limits()["lds_keyframes"])


@functools.lru_cache(maxsize=None)
def _host_family(pkg):
    return pkg.update_connections_batch(_family(pkg)[0], host=True)


def _check(pkg, problems, want, host, what):
    got = pkg.update_connections_batch(problems)
    assert len(got) == len(problems)
    for i, (g, h, w) in enumerate(zip(got, host, want)):
        K.assert_equal(g, h, "%s: problem %d, device against host" % (what, i))
        K.assert_equal(g, w, "%s: problem %d, device against the restatement" % (what, i))
    return got


def test_device_one_batch(pkg):
    problems, want = _family(pkg)
    _check(pkg, problems, want, _host_family(pkg), "one batch")


def test_device_batches_of_one(pkg):
    problems, want = _family(pkg)
    for i, (p, w, h) in enumerate(zip(problems, want, _host_family(pkg))):
        _check(pkg, [p], [w], [h], "problem %d alone" % i)


def test_device_shuffled_batch(pkg):
    problems, want = _family(pkg)
    host = _host_family(pkg)
    order = np.random.default_rng(5).permutation(len(problems))
    _check(pkg, [problems[i] for i in order], [want[i] for i in order], [host[i] for i in order], "shuffled")
    _check(pkg, problems[::-1], want[::-1], host[::-1], "reversed")


def test_device_batch_of_512(pkg):
    """512 problems picked from the family in one call, every one at least once; the family holds every branch."""
    problems, want = _family(pkg)
    host = _host_family(pkg)
    assert any(w["status"] == ref.UNCHANGED for w in want)                            # an empty counter
    assert any(w["by_max"] for w in want)                                             # connected by the maximum rule
    assert any(w["n_unchanged"] for w in want)                                        # a neighbour that holds the weight already
    assert any(w["parent"] >= 0 for w in want)                                        # a first connection
    # the big graphs once, the others often: the call stays small
    small = [i for i, p in enumerate(problems) if len(p["kf_flags"]) <= 300]
    pick = np.array(small)[np.random.default_rng(6).integers(0, len(small), 512)]
    pick[:len(problems)] = np.arange(len(problems))
    got = _check(pkg, [problems[i] for i in pick], [want[i] for i in pick], [host[i] for i in pick], "512")
    assert len(got) == 512


def test_device_hand_made_cases(pkg):
    """The rules one by one go through the same kernels: the hand-made graphs of test_connections.py with the device entries."""
    real = pkg.update_connections_batch, pkg.update_best_covisibles_batch

    class Device:
        def __getattr__(self, name):
            return getattr(pkg, name)

        @staticmethod
        def update_connections_batch(problems, host=False, **kw):
            return real[0](problems, host=False, **kw)

        @staticmethod
        def update_best_covisibles_batch(rows, bad, host=False, **kw):
            return real[1](rows, bad, host=False, **kw)

    dev = Device()
    for name in T.HAND_MADE:
        getattr(T, name)(dev)
    for slots in ([], [-1, -1, -1], [0, 1]):
        T.test_nothing_counted_leaves_everything_as_it_was(dev, slots)
    for first, init in ((0, 0), (0, 1), (1, 0), (1, 1)):
        T.test_parent(dev, first, init)


def test_device_empty_batch(pkg):
    assert pkg.update_connections_batch([]) == []
    none = pkg.update_best_covisibles_batch(dict(offsets=[0], kf=[], weight=[]), [])
    assert none["offsets"].tolist() == [0] and len(none["kf"]) == 0


def test_device_best_covisibles(pkg):
    """10^5 rows of mixed length, 0 to 1100 entries"""
    rows, bad = K.random_rows(4, 100000, 300000)
    want = ref.update_best_covisibles(rows, bad)
    got = pkg.update_best_covisibles_batch(rows, bad)
    host = pkg.update_best_covisibles_batch(rows, bad, host=True)
    for k in want:
        assert np.array_equal(got[k], host[k]), k
        assert np.array_equal(got[k], want[k]), k
    assert len(want["kf"]) < len(rows["kf"]) and {0, 1} <= set(np.diff(rows["offsets"]).tolist()) and int(np.diff(want["offsets"]).max()) > 900


# ---- the buffers kept between calls -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _tiny():
    """Problems of the family's smallest sizes: 12 keyframes and 63 slots, counts on both sides of the threshold."""
    return [K.make_problem(900 + i, 12, 63, 8, ("high", "mixed")[i % 2], (0, 1, 5), first=bool(i % 3 == 0)) for i in range(16)]


def _equals_host(pkg, problems, what):
    got = pkg.update_connections_batch(problems)
    host = pkg.update_connections_batch(problems, host=True)
    assert len(got) == len(host) == len(problems)
    for i, (g, h) in enumerate(zip(got, host)):
        K.assert_equal(g, h, "%s: problem %d, device against host" % (what, i))
    return got


def _rows_equal_host(pkg, rows, bad, what):
    got, host = pkg.update_best_covisibles_batch(rows, bad), pkg.update_best_covisibles_batch(rows, bad, host=True)
    for k in host:
        assert np.array_equal(got[k], host[k]), (what, k)
    return got


def test_device_reuses_its_buffers_across_batch_sizes(pkg):
    """8 problems, then 1 other, then the 8 again through the same buffers: nothing of an earlier call shows in a later one."""
    tiny = _tiny()
    eight, one = tiny[:8], [tiny[8]]
    _equals_host(pkg, tiny, "fill")                                                  # whatever the tests before left, the buffers are larger than the calls below need
    first = _equals_host(pkg, eight, "8")
    assert any(g["status"] == ref.UPDATED and len(g["changed_kf"]) for g in first)
    _equals_host(pkg, one, "1")
    again = _equals_host(pkg, eight, "8 again")
    for i, (a, b) in enumerate(zip(first, again)):
        K.assert_equal(a, b, "problem %d, first against third call" % i)
    rows, bad = K.random_rows(8, 300, 4000, long_rows=(63, 65))
    one_row = dict(offsets=rows["offsets"][:2], kf=rows["kf"], weight=rows["weight"])
    for r, what in ((rows, "300 rows"), (one_row, "1 row"), (rows, "300 rows again")):
        _rows_equal_host(pkg, r, bad, what)


def test_device_empty_problem_inside_a_batch(pkg):
    """The emptiest problem the validation admits -- the current keyframe alone: no slots, no points, no weight rows -- between two
    ordinary ones: its tables are empty places in the concatenation.  A problem without any keyframe has no current one and is refused."""
    tiny = _tiny()
    alone = K.hand([dict()], [], [], 0)
    got = _equals_host(pkg, [tiny[0], alone, tiny[1]], "empty in the middle")
    assert got[1]["status"] == ref.UNCHANGED and len(got[1]["counter_kf"]) == 0
    _equals_host(pkg, [alone, tiny[0], alone], "empty at both ends")
    _equals_host(pkg, [alone], "empty alone")
    for host in (True, False):
        with pytest.raises(pkg.Tc2liError) as e:
            pkg.update_connections_batch([tiny[0], K.hand([], [], [], 0), tiny[1]], host=host)
        assert e.value.code == -2 and "problem 1" in str(e.value) and "current" in str(e.value), e.value
    # UpdateBestCovisibles: rows without entries between rows with some, and rows without any entry at all
    got = _rows_equal_host(pkg, dict(offsets=[0, 2, 2, 2, 3], kf=[1, 3, 2], weight=[5, 7, 9]), [0, 0, 1, 0], "empty rows in the middle")
    assert got["offsets"].tolist() == [0, 2, 2, 2, 2] and got["kf"].tolist() == [3, 1]
    got = _rows_equal_host(pkg, dict(offsets=[0, 0, 0, 0], kf=[], weight=[]), [], "three empty rows")
    assert got["offsets"].tolist() == [0, 0, 0, 0] and len(got["kf"]) == 0


def test_device_two_callers_at_once(pkg):
    """Two threads, four calls each on batches of four of their own: each gets its own results."""
    import two_callers
    tiny = _tiny()
    batches = [[[tiny[8 * t + (2 * s + i) % 8] for i in range(4)] for s in range(4)] for t in (0, 1)]
    want = [[pkg.update_connections_batch(b, host=True) for b in side] for side in batches]
    got = two_callers.run(pkg.update_connections_batch, batches[0], batches[1])
    for t in (0, 1):
        for c, (g, w) in enumerate(zip(got[t], want[t])):
            assert len(g) == len(w) == 4
            for i in range(4):
                K.assert_equal(g[i], w[i], "thread %d, call %d, problem %d" % (t, c, i))
    rows = [[K.random_rows(50 + 4 * t + c, 100 + 20 * c, 2000, long_rows=(64,)) for c in range(4)] for t in (0, 1)]
    got = two_callers.run(lambda rb: pkg.update_best_covisibles_batch(*rb), rows[0], rows[1])
    for t in (0, 1):
        for c in range(4):
            host = pkg.update_best_covisibles_batch(*rows[t][c], host=True)
            for k in host:
                assert np.array_equal(got[t][c][k], host[k]), (t, c, k)
