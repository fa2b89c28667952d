"""CPU tests of the covisibility update: tc2li_host_update_connections_batch and tc2li_host_update_best_covisibles_batch against the
restatement tests/connections_ref.py, on generated graphs and on hand-made graphs, one per rule, whose expected lists are written out
here so that the restatement cannot drift.  Every output is an integer, so the criterion is equality.  No GPU needed."""
import functools

import numpy as np
import pytest

import connections_cases as K
import connections_ref as ref

SENTINEL = -77


@functools.lru_cache(maxsize=None)
def family(lds_keyframes):
    problems = K.family(lds_keyframes)
    return problems, [ref.update_connections(p) for p in problems]


def _one(pkg, pr):
    got = pkg.update_connections_batch([pr], host=True)[0]
    K.assert_equal(got, ref.update_connections(pr))
    return got


def _lists(got):
    """the changed neighbours' lists as {keyframe: (keyframes, weights)}"""
    ks = [int(k) for k, c in zip(got["touched_kf"], got["touched_changed"]) if c]
    off = got["changed_offsets"]
    assert len(off) == len(ks) + 1
    return {k: (got["changed_kf"][off[i]:off[i + 1]].tolist(), got["changed_weight"][off[i]:off[i + 1]].tolist()) for i, k in enumerate(ks)}


# ---- generated graphs ----------------------------------------------------------------------------------------------------------------
def test_family_reaches_every_rule(pkg):
    """The restatement alone: the generated graphs contain what the device tests count on."""
    lim = pkg.connections_limits()
    problems, want = family(lim["lds_keyframes"])
    sizes = {len(p["kf_flags"]) for p in problems}
    assert len(problems) >= 38 and {1, lim["lds_keyframes"] - 1, lim["lds_keyframes"], lim["lds_keyframes"] + 1, 3000} <= sizes
    assert {0, 1, 63, 64, 65, 2000} <= {len(p["slot_point"]) for p in problems}
    assert any(w["status"] == ref.UNCHANGED for w in want)
    assert any(w["by_max"] for w in want)
    assert any(w["n_unchanged"] for w in want)
    assert any(w["parent"] >= 0 for w in want) and any(w["status"] and w["parent"] < 0 for w in want)
    assert max(len(w["ordered_kf"]) for w in want) > 256
    assert {63, 64, 65, 255, 257} <= {len(w["ordered_kf"]) for w in want}
    lens = {int(n) for w in want for n in np.diff(w["changed_offsets"])}
    assert {1, 2, 64, 65, 256, 258} & lens and max(lens) > 1000, sorted(lens)
    # equal weights inside one list
    assert any(len(set(w["ordered_weight"].tolist())) < len(w["ordered_weight"]) for w in want)
    assert any((w["counter_weight"] < ref.TH).any() and (w["counter_weight"] >= ref.TH).any() for w in want)


def test_host_equals_restatement_on_generated_problems(pkg):
    problems, want = family(pkg.connections_limits()["lds_keyframes"])
    batch = pkg.update_connections_batch(problems, host=True)
    for i, (g, w) in enumerate(zip(batch, want)):
        K.assert_equal(g, w, "problem %d in the batch" % i)
    for i in (0, 3, 10, 19, 24):
        K.assert_equal(pkg.update_connections_batch([problems[i]], host=True)[0], batch[i], "problem %d alone" % i)


# ---- hand-made graphs, one per rule --------------------------------------------------------------------------------------------------
def test_counts_of_14_and_15(pkg):
    kfs, points, slots = K.votes(4, 0, {1: 14, 2: 15, 3: 16})
    got = _one(pkg, K.hand(kfs, points, slots, 0))
    assert got["status"] == 1
    assert got["counter_kf"].tolist() == [1, 2, 3] and got["counter_weight"].tolist() == [14, 15, 16]      # the whole counter (:473)
    assert got["ordered_kf"].tolist() == [3, 2] and got["ordered_weight"].tolist() == [16, 15]
    assert got["touched_kf"].tolist() == [2, 3] and got["touched_changed"].tolist() == [1, 1]
    assert _lists(got) == {2: ([0], [15]), 3: ([0], [16])}


def test_nobody_reaches_15(pkg):
    """the maximum is connected alone; equal maxima: the lowest row (`>` at :443)"""
    kfs, points, slots = K.votes(5, 4, {0: 3, 1: 9, 2: 9, 3: 2})
    got = _one(pkg, K.hand(kfs, points, slots, 4))
    assert got["counter_kf"].tolist() == [0, 1, 2, 3] and got["counter_weight"].tolist() == [3, 9, 9, 2]
    assert got["ordered_kf"].tolist() == [1] and got["ordered_weight"].tolist() == [9]
    assert got["touched_kf"].tolist() == [1] and _lists(got) == {1: ([4], [9])}


def test_equal_weights_go_by_row_descending(pkg):
    kfs, points, slots = K.votes(6, 2, {0: 20, 1: 17, 3: 20, 4: 17, 5: 20})
    got = _one(pkg, K.hand(kfs, points, slots, 2))
    assert got["ordered_kf"].tolist() == [5, 3, 0, 4, 1] and got["ordered_weight"].tolist() == [20, 20, 20, 17, 17]
    assert got["touched_kf"].tolist() == [0, 1, 3, 4, 5]


def test_votes_that_do_not_count(pkg):
    """self, a bad keyframe, a keyframe of another map, a bad point"""
    kfs = [dict(), dict(flags=1), dict(flags=2), dict(), dict(flags=3)]
    points = [dict(obs=[0, 1, 2, 3, 4]) for _ in range(16)] + [dict(obs=[3], bad=1) for _ in range(5)]
    got = _one(pkg, K.hand(kfs, points, list(range(21)), 0))
    assert got["counter_kf"].tolist() == [3] and got["counter_weight"].tolist() == [16]
    assert got["ordered_kf"].tolist() == [3]


def test_point_in_two_slots_votes_twice(pkg):
    points = [dict(obs=[0, 1]) for _ in range(8)]
    got = _one(pkg, K.hand([dict(), dict()], points, list(range(8)) + list(range(7)), 0))
    assert got["counter_weight"].tolist() == [15] and got["ordered_weight"].tolist() == [15]
    got = _one(pkg, K.hand([dict(), dict(), dict()], points + [dict(obs=[2]) for _ in range(15)], list(range(8)) + list(range(6)) + list(range(8, 23)), 0))
    assert got["counter_weight"].tolist() == [14, 15] and got["ordered_kf"].tolist() == [2]


@pytest.mark.parametrize("slots", [[], [-1, -1, -1], [0, 1]])
def test_nothing_counted_leaves_everything_as_it_was(pkg, slots):
    """no slots, all slots NULL, points seen by nobody else: the reference returns at :426-427; nothing but counts is written"""
    pr = K.hand([dict(conn={1: 5}), dict(conn={0: 5})], [dict(obs=[0]), dict(obs=[0, 1], bad=1)], slots, 0, first_connection=1)
    raw = pkg.update_connections_batch([pr], host=True, raw=True, fill=SENTINEL)[0]
    assert raw["counts"].tolist() == [0, 0, 0, 0, 0, -1, 0, 0]
    for k, v in raw.items():
        if k != "counts":
            assert len(v) and (v == np.array(SENTINEL).astype(v.dtype)).all(), k
    _one(pkg, pr)


def test_outputs_beyond_the_counts_stay_untouched(pkg):
    kfs, points, slots = K.votes(6, 0, {1: 15, 2: 3, 4: 30})
    raw = pkg.update_connections_batch([K.hand(kfs, points, slots, 0)], host=True, raw=True, fill=SENTINEL)[0]
    assert raw["counts"].tolist() == [1, 3, 2, 2, 2, -1, 0, 0]
    assert raw["counter_kf"].tolist() == [1, 2, 4] + [SENTINEL] * 3 and raw["ordered_kf"].tolist() == [4, 1] + [SENTINEL] * 4
    assert raw["touched_changed"].tolist() == [1, 1] + [SENTINEL & 0xff] * 4 and raw["changed_offsets"].tolist() == [0, 1, 2] + [SENTINEL] * 4
    assert raw["changed_kf"].tolist() == [0, 0] + [SENTINEL] * 4


@pytest.mark.parametrize("first,init", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_parent(pkg, first, init):
    kfs, points, slots = K.votes(4, 3, {0: 15, 1: 40, 2: 22})
    got = _one(pkg, K.hand(kfs, points, slots, 3, first_connection=first, is_init_kf=init))
    assert got["ordered_kf"].tolist() == [1, 2, 0]
    assert got["parent"] == (1 if first and not init else -1)


def test_neighbour_that_holds_the_same_weight_is_unchanged(pkg):
    """AddConnection returns at :210: no list is given, the neighbour's (possibly stale) lists are not refreshed"""
    kfs, points, slots = K.votes(4, 0, {1: 15, 2: 16})
    kfs[1]["conn"] = {0: 15, 3: 99}
    kfs[2]["conn"] = {3: 99}
    got = _one(pkg, K.hand(kfs, points, slots, 0))
    assert got["touched_kf"].tolist() == [1, 2] and got["touched_changed"].tolist() == [0, 1]
    assert got["changed_offsets"].tolist() == [0, 2] and _lists(got) == {2: ([3, 0], [99, 16])}


def test_neighbour_that_holds_another_weight_has_it_overwritten(pkg):
    kfs, points, slots = K.votes(5, 0, {1: 15, 2: 16})
    kfs[1]["conn"] = {0: 16, 3: 99, 4: 15}    # 16 -> 15: the entry moves behind keyframe 4
    kfs[2]["conn"] = {0: 15, 3: 9}            # 15 -> 16
    got = _one(pkg, K.hand(kfs, points, slots, 0))
    assert got["touched_changed"].tolist() == [1, 1]
    assert _lists(got) == {1: ([3, 4, 0], [99, 15, 15]), 2: ([0, 3], [16, 9])}


def test_neighbour_list_keeps_weights_below_15_and_drops_bad(pkg):
    kfs, points, slots = K.votes(7, 1, {0: 15})
    kfs[0]["conn"] = {2: 3, 3: 50, 4: 15, 5: 3, 6: 15}
    kfs[3]["flags"] = 1
    got = _one(pkg, K.hand(kfs, points, slots, 1))
    assert _lists(got) == {0: ([6, 4, 1, 5, 2], [15, 15, 15, 3, 3])}
    kfs[1]["flags"] = 1                        # the current keyframe itself is bad: it gets its votes, the neighbour's list leaves it out
    got = _one(pkg, K.hand(kfs, points, slots, 1))
    assert got["touched_changed"].tolist() == [1] and _lists(got) == {0: ([6, 4, 5, 2], [15, 15, 3, 3])}


def test_invalid_problems_are_refused(pkg):
    kfs, points, slots = K.votes(4, 0, {1: 15, 2: 16})
    kfs[1]["conn"] = {0: 1, 2: 2, 3: 3}
    good = K.hand(kfs, points, slots, 0)
    _one(pkg, good)

    def refused(**change):
        pr = dict(good, **{k: np.array(v, good[k].dtype) if k != "current" else v for k, v in change.items()})
        with pytest.raises(pkg.Tc2liError) as e:
            pkg.update_connections_batch([good, pr], host=True)
        assert e.value.code == -2, e.value
        return str(e.value)

    off = good["obs_offsets"].copy(); off[3] = off[2] - 1
    assert "obs_offsets" in refused(obs_offsets=off)
    assert "conn_offsets" in refused(conn_offsets=[0, 0, 3, 2, 3])
    assert "conn_offsets" in refused(conn_offsets=[1, 1, 3, 3, 3])
    obs = good["obs_kf"].copy(); obs[5] = 4
    assert "obs_kf" in refused(obs_kf=obs)
    assert "slot_point" in refused(slot_point=[0, 1, len(points)])
    assert "slot_point" in refused(slot_point=[0, -2])
    assert "current" in refused(current=4)
    assert "out of range" in refused(conn_kf=[0, 2, 4])
    assert "ascend strictly" in refused(conn_kf=[0, 3, 2])
    assert "ascend strictly" in refused(conn_kf=[0, 2, 2])


def test_capacity_one_short(pkg):
    kfs, points, slots = K.votes(5, 0, {1: 15, 2: 3, 4: 30})
    kfs[4]["conn"] = {2: 7, 3: 8}
    good = K.hand(kfs, points, slots, 0)
    need = dict(counter_capacity=3, ordered_capacity=2, changed_capacity=4)
    got = pkg.update_connections_batch([dict(good, **need)], host=True)[0]
    K.assert_equal(got, ref.update_connections(good))
    assert _lists(got) == {1: ([0], [15]), 4: ([0, 3, 2], [30, 8, 7])}
    for k, v in need.items():
        with pytest.raises(pkg.Tc2liError) as e:
            pkg.update_connections_batch([good, dict(good, **dict(need, **{k: v - 1}))], host=True)
        assert e.value.code == -5 and "problem 1" in str(e.value), e.value


# ---- UpdateBestCovisibles alone ------------------------------------------------------------------------------------------------------
def test_best_covisibles_rules(pkg):
    rows = dict(offsets=[0, 0, 2, 7, 7, 8], kf=[1, 3, 0, 1, 2, 4, 5, 2], weight=[5, 6, 9, 20, 9, 20, 9, 1])
    bad = [0, 1, 0, 1, 0, 0]
    got = pkg.update_best_covisibles_batch(rows, bad, host=True)
    # an empty row, an all-bad row, ties by row descending with a bad keyframe dropped, an empty row, one entry
    assert got["offsets"].tolist() == [0, 0, 0, 4, 4, 5]
    assert got["kf"].tolist() == [4, 5, 2, 0, 2] and got["weight"].tolist() == [20, 9, 9, 9, 1]
    want = ref.update_best_covisibles(rows, bad)
    assert all(np.array_equal(got[k], want[k]) for k in want)
    none = pkg.update_best_covisibles_batch(dict(offsets=[0], kf=[], weight=[]), [], host=True)
    assert none["offsets"].tolist() == [0] and len(none["kf"]) == 0
    with pytest.raises(pkg.Tc2liError) as e:
        pkg.update_best_covisibles_batch(dict(offsets=[0, 2], kf=[3, 1], weight=[1, 1]), [0] * 4, host=True)
    assert e.value.code == -2
    with pytest.raises(pkg.Tc2liError) as e:
        pkg.update_best_covisibles_batch(dict(offsets=[0, 2], kf=[1, 4], weight=[1, 1]), [0] * 4, host=True)
    assert e.value.code == -2


def test_best_covisibles_on_generated_rows(pkg):
    rows, bad = K.random_rows(3, 3000, 20000)
    got = pkg.update_best_covisibles_batch(rows, bad, host=True)
    want = ref.update_best_covisibles(rows, bad)
    assert all(np.array_equal(got[k], want[k]) for k in want)
    assert len(want["kf"]) < len(rows["kf"]) and int(np.diff(want["offsets"]).max()) > 900


# the tests that tests/test_connections_gpu.py sends through the device entries
HAND_MADE = ("test_counts_of_14_and_15", "test_nobody_reaches_15", "test_equal_weights_go_by_row_descending", "test_votes_that_do_not_count",
             "test_point_in_two_slots_votes_twice", "test_outputs_beyond_the_counts_stay_untouched", "test_neighbour_that_holds_the_same_weight_is_unchanged",
             "test_neighbour_that_holds_another_weight_has_it_overwritten",
             "test_neighbour_list_keeps_weights_below_15_and_drops_bad", "test_invalid_problems_are_refused", "test_capacity_one_short",
             "test_best_covisibles_rules")
