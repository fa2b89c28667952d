"""CPU tests of relocalisation: the restatement's quirks on hand-built cases, the ordering-key claim the device design rests on, and the
host logic of the keyframe database handle through the ABI (no GPU needed); the computing entries refuse to run without a GPU."""
import ctypes as C

import numpy as np
import pytest

import bow_ref as B
import reloc_ref as R


def _uniform(words):
    return list(words), [1.0 / len(words)] * len(words)


def _tiny_voc(pkg, scoring=R.L1_NORM, k=10, L=2):
    p, lf, d, w = B.random_tree(k, L, seed=1, stop_frac=0.0)
    return pkg.Vocabulary.from_arrays(k, L, scoring, B.TF_IDF, p, lf, d, w)


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
def test_list_order_after_add_add_erase_add():
    db = R.KeyFrameDatabase()
    db.add(1, 0, *_uniform([3, 5]))
    db.add(2, 0, *_uniform([3, 5, 7]))
    db.erase(1)
    db.add(1, 0, *_uniform([3, 5]))
    assert [kf.kf_id for kf in db.inverted[3]] == [2, 1] and [kf.kf_id for kf in db.inverted[5]] == [2, 1]
    assert [kf.kf_id for kf in db.sharing_words(1, [3, 5, 7])] == [2, 1]
    assert R.order_by_key(db, [3, 5, 7]) == [2, 1]
    assert db.live[1].sequence == 2 and db.live[1].reloc_score == 0


def test_min_common_words_float_form_equals_integer_form():
    """(int)(maxCommonWords * 0.8f) (KeyFrameDatabase.cc:778) over the whole capacity range of a BowVector."""
    for m in range(1, 4097):
        assert int(np.float32(m) * np.float32(0.8)) == 4 * m // 5, m


def _gate_case():
    """Keyframe 1 shares 10 words with the frame, keyframe 2 one word (fails the gate: 1 <= (int)(10 * 0.8f)) and is 1's neighbour."""
    db = R.KeyFrameDatabase()
    db.add(1, 0, *_uniform(range(10)))
    db.add(2, 0, *_uniform([9, 50, 51, 52]))
    db.set_covisibility(1, [2])
    return db


def test_neighbour_below_the_word_gate_contributes_its_stored_score():
    frame = _uniform(range(10))
    fresh = _gate_case()
    cands, scored = fresh.detect_relocalization_candidates(0, *frame)
    assert [s[0] for s in scored] == [1] and scored[0][3] == scored[0][2]       # accScore = si + 0.0f on a fresh database
    assert cands == [1] and fresh.live[2].reloc_score == 0
    db = _gate_case()
    _, first = db.detect_relocalization_candidates(0, *_uniform([50, 51, 52]))  # an earlier query scores keyframe 2
    stale = db.live[2].reloc_score
    assert [s[0] for s in first] == [2] and stale > 0
    _, scored = db.detect_relocalization_candidates(0, *frame)
    assert [s[0] for s in scored] == [1]
    assert scored[0][3] == np.float32(scored[0][2] + stale) and scored[0][3] != scored[0][2]
    assert db.live[2].reloc_score == stale                                        # not rescored: it failed the gate


def test_first_occurrence_and_map_filter():
    db = R.KeyFrameDatabase()
    words = list(range(20))
    db.add(1, 0, *_uniform(words))                   # the best keyframe of all three
    db.add(2, 0, *_uniform(words[:18] + [30, 31]))
    db.add(3, 1, *_uniform(words[:17] + [40, 41, 42]))
    db.set_covisibility(2, [1])
    db.set_covisibility(3, [1, 2])
    cands, scored = db.detect_relocalization_candidates(0, *_uniform(words))
    assert [s[0] for s in scored] == [1, 2, 3] and [s[4] for s in scored] == [1, 1, 1]
    assert cands == [1]                               # keyframe 1 once, not three times
    db.set_covisibility(2, [])
    db.set_covisibility(3, [])
    cands, scored = db.detect_relocalization_candidates(0, *_uniform(words))
    assert [s[4] for s in scored] == [1, 2, 3] and cands == [1, 2]              # keyframe 3 belongs to map 1
    assert db.detect_relocalization_candidates(1, *_uniform(words))[0] == [3]
    assert db.detect_relocalization_candidates(0, *_uniform([60, 61]))[0] == []  # no keyframe shares a word


def test_score_quirks():
    a = ([1, 2, 3], [0.6, 0.6, 0.6])
    assert R.score_l2(a, a) == 1.0                                               # 1.08 >= 1: the clamp (:114-115)
    half = ([1, 2], [0.5, 0.5])
    assert R.score_l2(half, half) == 1.0 - np.sqrt(0.5)
    v, w = ([1, 2], [0.5, -0.25]), ([1, 2], [-0.5, 0.75])
    assert R.score_chi_square(v, w) == 2.0 * (-0.25 * 0.75 / 0.5)                # word 1: vi + wi == 0 is skipped (:148)
    assert R.score_l1(([1], [1.0]), ([2], [1.0])) == 0.0 and np.signbit(R.score_l1(([1], [1.0]), ([2], [1.0])))  # -0.0 / 2
    assert R.score_l1(([], []), ([], [])) == 0.0
    t = 0.0 - 0.6 - 0.6                                                         # fabs(vi - wi) - fabs(vi) - fabs(wi)
    assert R.score_l1(a, a) == -(((0.0 + t) + t) + t) / 2.0
    assert R.score_bhattacharyya(half, half) == np.sqrt(0.25) + np.sqrt(0.25)
    assert R.score_dot_product(half, ([2, 9], [4.0, 1.0])) == 2.0


def test_order_of_sharing_keyframes_is_first_common_word_then_sequence():
    """The one claim the device design rests on: the order in which the inverted file's lists meet the keyframes equals the order by
    (smallest word shared with the frame, sequence number of the add call), whatever the add / erase history."""
    rng = np.random.default_rng(7)
    for history in range(300):
        n_voc = int(rng.integers(20, 200))
        db = R.KeyFrameDatabase()
        next_id = 0
        erased = []
        for _ in range(int(rng.integers(1, 60))):
            op = rng.random()
            if op < 0.6 or not db.live:
                if erased and rng.random() < 0.3:
                    kf_id = erased.pop(int(rng.integers(len(erased))))     # an erased keyframe comes back
                else:
                    kf_id, next_id = next_id, next_id + 1
                words = np.unique(rng.integers(0, n_voc, int(rng.integers(1, 25))))
                db.add(kf_id, int(rng.integers(2)), words, np.ones(len(words)))
            elif op < 0.9:
                kf_id = list(db.live)[int(rng.integers(len(db.live)))]
                db.erase(kf_id)
                erased.append(kf_id)
            else:
                m = int(rng.integers(2))
                erased += [k for k, kf in db.live.items() if kf.map_id == m]
                db.clear_map(m)
        for query in range(3):
            words = np.unique(rng.integers(0, n_voc, int(rng.integers(1, 30))))
            got = [kf.kf_id for kf in db.sharing_words(1000 * history + query, words)]
            assert got == R.order_by_key(db, words), history
            for kf in db.live.values():
                if kf.kf_id in got:
                    assert kf.reloc_words == len(set(kf.words) & set(int(w) for w in words))


# ---- the handle through the ABI, without a device ------------------------------------------------------------------------------------
def test_database_host_logic(pkg):
    voc = _tiny_voc(pkg)
    assert voc.info()["words"] == 100
    db = pkg.KeyFrameDatabase(voc)
    assert len(db) == 0
    assert db.add(7, 0, [1, 5, 9], [0.2, 0.3, 0.5]) == 0
    assert db.add(3, 1, [], []) == 1
    assert db.add(11, 0, [0, 99], [0.5, 0.5]) == 2
    e = db.entries()
    assert e["kf_id"].tolist() == [7, 3, 11] and e["map_id"].tolist() == [0, 1, 0] and e["sequence"].tolist() == [0, 1, 2]
    assert e["score"].dtype == np.float32 and e["score"].tobytes() == np.zeros(3, np.float32).tobytes()
    assert db.erase(7) == 1 and db.erase(7) == 0 and db.erase(12345) == 0        # an unknown id is a no-op
    assert len(db) == 2
    assert db.add(7, 0, [2], [1.0]) == 3                                          # a new entry with a new sequence number
    assert db.entries()["kf_id"].tolist() == [3, 11, 7] and db.entries()["sequence"].tolist() == [1, 2, 3]
    assert db.set_covisibility(7, [3, 11, 555]) == 3                              # ids that are no entries are allowed
    assert db.clear_map(0) == 2 and db.entries()["kf_id"].tolist() == [3]
    assert db.clear_map(5) == 0
    assert db.clear() == 1 and len(db) == 0 and db.entries()["kf_id"].tolist() == []
    assert db.add(3, 0, [4], [1.0]) == 4


def test_database_compacts_and_keeps_sequence_order(pkg):
    voc = _tiny_voc(pkg)
    db = pkg.KeyFrameDatabase(voc)
    rng = np.random.default_rng(3)
    want = []
    seq = 0
    for step in range(400):
        if want and rng.random() < 0.55:
            k = want.pop(int(rng.integers(len(want))))
            assert db.erase(k[0]) == 1
        else:
            kf_id = step
            w = np.unique(rng.integers(0, 100, 10)).astype(np.int32)
            assert db.add(kf_id, step % 3, w, np.ones(len(w))) == seq
            want.append((kf_id, step % 3, seq))
            seq += 1
        e = db.entries()
        assert list(zip(e["kf_id"].tolist(), e["map_id"].tolist(), e["sequence"].tolist())) == want
    assert len(db) == len(want)


def test_database_rejects(pkg):
    voc = _tiny_voc(pkg)
    db = pkg.KeyFrameDatabase(voc)
    db.add(1, 0, [1, 2], [0.5, 0.5])
    for what, call, needle in [
        ("live duplicate", lambda: db.add(1, 0, [3], [1.0]), "already"),
        ("not ascending", lambda: db.add(2, 0, [5, 5], [0.5, 0.5]), "ascending"),
        ("descending", lambda: db.add(2, 0, [5, 4], [0.5, 0.5]), "ascending"),
        ("outside the vocabulary", lambda: db.add(2, 0, [5, 100], [0.5, 0.5]), "vocabulary"),
        ("negative word", lambda: db.add(2, 0, [-1, 5], [0.5, 0.5]), "vocabulary"),
        ("eleven neighbours", lambda: db.set_covisibility(1, list(range(11))), "neighbours"),
        ("unknown keyframe", lambda: db.set_covisibility(9, [1]), "not in the database"),
    ]:
        with pytest.raises(pkg.Tc2liError) as e:
            call()
        assert e.value.code == -2 and needle in str(e.value), (what, str(e.value))
    assert len(db) == 1 and db.entries()["sequence"].tolist() == [0]
    assert db.add(2, 0, [5, 99], [0.5, 0.5]) == 1                                 # a rejected add takes no sequence number
    with pytest.raises(pkg.Tc2liError) as e:
        db.add(3, 0, np.arange(4097) % 100, np.ones(4097))                        # not ascending comes first
    assert e.value.code == -2


def test_reloc_entries_need_a_device(pkg):
    if pkg.device_count() > 0:
        pytest.skip("GPU present")
    voc = _tiny_voc(pkg)
    db = pkg.KeyFrameDatabase(voc)
    db.add(1, 0, [1, 2], [0.5, 0.5])
    for call in (lambda: pkg.detect_relocalization_candidates_batch([(db, 0, [1, 2], [0.5, 0.5])]),
                 lambda: voc.score([(([1], [1.0]), ([1], [1.0]))])):
        with pytest.raises(pkg.Tc2liError) as e:
            call()
        assert e.value.code == -3  # TC2LI_ERR_NO_DEVICE
    assert db.entries()["score"].tolist() == [0.0]
    keys = np.zeros(3, pkg.capi.KEYPOINT_DTYPE)
    item = dict(keys=keys, descriptors=np.zeros((3, 32), np.uint8), held=np.zeros(3, np.uint8), pose7=[0, 0, 0, 1, 0, 0, 0], bounds=[0, 640, 0, 480],
                has_point=np.ones(2, np.uint8), found=np.zeros(2, np.uint8), Xw=np.ones((2, 3), np.float32), point_descriptors=np.zeros((2, 32), np.uint8),
                min_distance=np.zeros(2, np.float32), max_distance=np.full(2, 10, np.float32), max_distance_raw=np.full(2, 8, np.float32),
                angle=np.zeros(2, np.float32))
    with pytest.raises(pkg.Tc2liError) as e:
        pkg.search_by_projection_keyframe_batch([item], [500, 500, 320, 240], [1.0, 1.2], np.log(1.2), 10, 100)
    assert e.value.code == -3
    f = pkg.lib().tc2li_relocalization_refine_batch     # the extractor handle itself cannot be made without a device
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int] + [C.c_void_p] * 8
    assert f(None, None, 0, 0, None, 0, None, None, None, None, None, None, None, None) == -3
