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
