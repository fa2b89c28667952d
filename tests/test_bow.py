"""CPU tests of the ORB vocabulary: the text loader (DBoW2's loadFromTextFile format) and its readback, the loader's rejections,
the restatement's quirks on hand-built trees, and that every compute entry refuses to run without a GPU."""
import ctypes as C

import numpy as np
import pytest

import bow_ref as R


def _voc_from_ref(pkg, v):
    return pkg.Vocabulary.from_arrays(v.k, v.L, v.scoring, v.weighting, v.file_parent, v.file_leaf, v.desc[1:], v.weight[1:])


def _small(seed=0, k=3, L=3, scoring=R.L1_NORM, weighting=R.TF_IDF):
    p, lf, d, w = R.random_tree(k, L, seed=seed, flips=20, stop_frac=0.2)
    return R.Voc(k, L, scoring, weighting, p, lf, d, w)


def _check_nodes(h, v, weights=None):
    parent, word, desc, weight = h.nodes()
    assert np.array_equal(parent, v.parent)
    assert np.array_equal(word, v.word)
    assert np.array_equal(desc, v.desc)
    assert np.array_equal(weight, v.weight if weights is None else weights)


@pytest.mark.parametrize("newline,sep", [("\n", " "), ("\r\n", " "), ("\n", "  \t ")])
def test_loader_round_trip(pkg, tmp_path, newline, sep):
    v = _small(seed=1, scoring=R.L2_NORM, weighting=R.IDF)
    v.weight[1:] = np.where(v.file_leaf > 0, v.weight[1:] * 1.2345678901, 0.0)   # more digits than the file keeps
    path = tmp_path / "voc.txt"
    R.write_text(path, v, newline=newline, sep=sep)
    h = pkg.Vocabulary.load_text(str(path))
    info = h.info()
    assert info == dict(k=3, L=3, scoring=R.L2_NORM, weighting=R.IDF, nodes=len(v.parent), words=v.n_words)
    _check_nodes(h, v, np.array([R.read_weight_6(x) for x in v.weight]))   # 6 significant digits, as saveToTextFile wrote them
    h2 = _voc_from_ref(pkg, v)
    assert h2.info() == info
    _check_nodes(h2, v)


def test_loader_blank_lines_and_byte_wrap(pkg, tmp_path):
    v = _small(seed=2)
    path = tmp_path / "voc.txt"
    R.write_text(path, v)
    text = path.read_text().splitlines()
    text.insert(3, "   ")
    fields = text[1].split()
    fields[2] = str(int(fields[2]) + 256)     # read as int, cast to unsigned char
    text[1] = " ".join(fields)
    path.write_text("\n".join(text) + "\n\n\n")
    h = pkg.Vocabulary.load_text(str(path))
    _check_nodes(h, v, np.array([R.read_weight_6(x) for x in v.weight]))


def _bad(tmp_path, lines, name="bad.txt"):
    p = tmp_path / name
    p.write_text("\n".join(lines) + "\n")
    return str(p)


def _line(parent, leaf, w=1.0):
    return " ".join([str(parent), str(leaf)] + ["7"] * 32 + [str(w)])


@pytest.mark.parametrize("case,lines,needle", [
    ("header_k", ["21 2 0 0", _line(0, 1)], "header"),
    ("header_L", ["2 0 0 0", _line(0, 1)], "header"),
    ("header_L11", ["2 11 0 0", _line(0, 1)], "header"),
    ("header_scoring", ["2 2 6 0", _line(0, 1)], "header"),
    ("header_weighting", ["2 2 0 4", _line(0, 1)], "header"),
    ("header_short", ["2 2 0", _line(0, 1)], "header"),
    ("short_line", ["2 2 0 0", _line(0, 1), "0 1 " + " ".join(["1"] * 31) + " 1.0"], "line 3"),
    ("parent_later", ["2 2 0 0", _line(0, 0), _line(3, 1), _line(1, 1)], "line 3"),
    ("parent_negative", ["2 2 0 0", _line(-1, 1)], "line 2"),
    ("word_with_children", ["2 2 0 0", _line(0, 1), _line(1, 1)], "line 3"),
    ("childless_not_word", ["2 2 0 0", _line(0, 0), _line(0, 1)], "line 2"),
    ("not_a_number", ["2 2 0 0", _line(0, 1).replace(" 7 ", " x ", 1)], "line 2"),
])
def test_loader_rejects(pkg, tmp_path, case, lines, needle):
    with pytest.raises(pkg.Tc2liError) as e:
        pkg.Vocabulary.load_text(_bad(tmp_path, lines))
    assert e.value.code == -2 and needle in str(e.value), str(e.value)


def test_loader_rejects_too_many_children(pkg):
    n = 65536  # the descent keeps a child's position in 16 bits
    with pytest.raises(pkg.Tc2liError) as e:
        pkg.Vocabulary.from_arrays(20, 1, 0, 0, np.zeros(n, np.int32), np.ones(n, np.int32), np.zeros((n, 32), np.uint8), np.ones(n))
    assert e.value.code == -2 and "65535" in str(e.value)
    assert pkg.Vocabulary.from_arrays(20, 1, 0, 0, np.zeros(n - 1, np.int32), np.ones(n - 1, np.int32), np.zeros((n - 1, 32), np.uint8),
                                      np.ones(n - 1)).info()["words"] == n - 1


def test_loader_rejects_missing_file_and_arrays(pkg, tmp_path):
    with pytest.raises(pkg.Tc2liError) as e:
        pkg.Vocabulary.load_text(str(tmp_path / "missing.txt"))
    assert e.value.code == -2
    z = np.zeros((1, 32), np.uint8)
    with pytest.raises(pkg.Tc2liError):
        pkg.Vocabulary.from_arrays(10, 6, 0, 0, [1], [1], z, [1.0])          # parent not earlier
    with pytest.raises(pkg.Tc2liError):
        pkg.Vocabulary.from_arrays(10, 6, 0, 0, [0, 1], [1, 1], np.zeros((2, 32), np.uint8), [1.0, 1.0])  # word with a child
    with pytest.raises(pkg.Tc2liError):
        pkg.Vocabulary.from_arrays(10, 6, 0, 0, [0], [0], z, [1.0])          # childless, not a word
    with pytest.raises(pkg.Tc2liError):
        pkg.Vocabulary.from_arrays(30, 6, 0, 0, [0], [1], z, [1.0])          # header
    assert pkg.Vocabulary.from_arrays(10, 6, 0, 0, [], [], np.zeros((0, 32), np.uint8), []).info()["words"] == 0


# ---- the restatement's quirks on hand-built trees ---------------------------------------------------------------------------------------
def _hand_tree():
    """root -> A (1), B (2);  A -> a0 (3), a1 (4);  B -> b0 (5, word);  a0 / a1 words;  plus C (6) a word directly under the root."""
    d = np.zeros((6, 32), np.uint8)
    d[0, 0] = 0x0F; d[1, 0] = 0x0F          # A and B equally far from 0x00: the first child (A) wins
    d[2, 1] = 0x03; d[3, 1] = 0x03          # a0 / a1 tie again: a0
    d[4, 0] = 0xFF
    d[5, :] = 0xFF                          # C far away
    parent = [0, 0, 1, 1, 2, 0]
    leaf = [0, 0, 1, 1, 1, 1]
    return parent, leaf, d


def test_ref_ties_go_to_first_child():
    p, lf, d = _hand_tree()
    v = R.Voc(3, 2, R.L1_NORM, R.TF_IDF, p, lf, d, [0, 0, 1.0, 2.0, 3.0, 4.0])
    q = np.zeros(32, np.uint8)
    assert R.transform_one(v, q, 0) == (0, 1.0, 3)          # A over B, a0 over a1
    q2 = np.full(32, 0xFF, np.uint8)
    assert R.transform_one(v, q2, 0)[0] == 3                 # C: a leaf directly below the root
    assert R.transform_one(v, q2, 1)[2] == 6                 # leaf above nid_level (1 = L - 1 reached at C itself: C)
    v3 = R.Voc(3, 3, R.L1_NORM, R.TF_IDF, p, lf, d, [0, 0, 1.0, 2.0, 3.0, 4.0])
    assert R.transform_one(v3, q2, 1)[2] == 6                # nid_level 2 never reached: the leaf's own id
    assert R.transform_one(v3, q, 1)[2] == 3                 # nid_level 2 = a0
    assert R.transform_one(v3, q, 2)[2] == 1                 # nid_level 1 = A
    for lu in (3, 4, 10):
        assert R.transform_one(v3, q, lu)[2] == 0            # levelsup >= L: the root


def test_ref_stopped_words_absent():
    p, lf, d = _hand_tree()
    v = R.Voc(3, 2, R.L1_NORM, R.TF_IDF, p, lf, d, [0, 0, 0.0, 2.0, 3.0, 4.0])   # a0 stopped
    out = R.transform(v, np.stack([np.zeros(32, np.uint8), np.full(32, 0xFF, np.uint8)]), 1)
    assert list(out["word"]) == [-1, 3] and list(out["node"]) == [-1, 6]
    assert list(out["bow_word"]) == [3] and list(out["fv_node"]) == [6] and list(out["fv_index"]) == [1]


@pytest.mark.parametrize("scoring", range(6))
@pytest.mark.parametrize("weighting", range(4))
def test_ref_scoring_weighting(scoring, weighting):
    p, lf, d = _hand_tree()
    w = [0, 0, 0.3, 2.0, 3.0, 0.7]
    v = R.Voc(3, 2, scoring, weighting, p, lf, d, w)
    q = np.stack([np.zeros(32, np.uint8)] * 3 + [np.full(32, 0xFF, np.uint8)])
    out = R.transform(v, q, 4)
    vals = [0.3 + 0.3 + 0.3, 0.7] if weighting in (R.TF, R.TF_IDF) else [0.3, 0.7]
    if scoring == R.DOT_PRODUCT:
        if weighting in (R.TF, R.TF_IDF):
            vals = [x / 2.0 for x in vals]
    elif scoring == R.L2_NORM:
        n = np.sqrt(vals[0] * vals[0] + vals[1] * vals[1]); vals = [x / n for x in vals]
    else:
        n = abs(vals[0]) + abs(vals[1]); vals = [x / n for x in vals]
    assert list(out["bow_word"]) == [0, 3]
    assert np.array_equal(out["bow_value"], np.array(vals))
    assert list(out["fv_node"]) == [0] and list(out["fv_offset"]) == [0, 4] and list(out["fv_index"]) == [0, 1, 2, 3]


def _kfv(descs, angles, nodes, has_point=None):
    descs = np.asarray(descs, np.uint8)
    order = sorted(set(nodes))
    idx = [i for n in order for i in range(len(nodes)) if nodes[i] == n]
    off = np.concatenate([[0], np.cumsum([nodes.count(n) for n in order])]).astype(np.int32)
    return dict(descriptors=descs, angle=np.float32(angles), fv_node=np.int32(order), fv_offset=off, fv_index=np.int32(idx),
                has_point=np.ones(len(descs), np.uint8) if has_point is None else np.uint8(has_point))


def _d(nbits):
    d = np.zeros(32, np.uint8)
    bits = np.unpackbits(d)
    bits[:nbits] = 1
    return np.packbits(bits)


def test_ref_search_taken_and_edges():
    z = np.zeros(32, np.uint8)
    # two keyframe features want the same frame feature: the second takes the next one (taken-skip)
    kf = _kfv([z, z], [10, 10], [5, 5])
    fr = _kfv([_d(3), _d(20)], [10, 10], [5, 5])
    m, n = R.search_by_bow(kf, fr, 0.7, False)
    assert list(m) == [0, 1] and n == 2
    # equal best and second: best < 0.7 * best fails
    fr = _kfv([_d(3), _d(3)], [10, 10], [5, 5])
    m, n = R.search_by_bow(_kfv([z], [0], [5]), fr, 0.7, False)
    assert n == 0
    # TH_LOW: 50 passes, 51 does not (second = 256)
    assert R.search_by_bow(_kfv([z], [0], [5]), _kfv([_d(50)], [0], [5]), 0.7, False)[1] == 1
    assert R.search_by_bow(_kfv([z], [0], [5]), _kfv([_d(51)], [0], [5]), 0.7, False)[1] == 0
    # strict ratio: 35 < 0.7 * 50 is false (float 35.0 == 35.0), 34 passes
    assert R.search_by_bow(_kfv([z], [0], [5]), _kfv([_d(35), _d(50)], [0, 0], [5, 5]), 0.7, False)[1] == 0
    assert R.search_by_bow(_kfv([z], [0], [5]), _kfv([_d(34), _d(50)], [0, 0], [5, 5]), 0.7, False)[1] == 1
    # no map point / other node
    assert R.search_by_bow(_kfv([z], [0], [5], has_point=[0]), _kfv([_d(3)], [0], [5]), 0.7, False)[1] == 0
    assert R.search_by_bow(_kfv([z], [0], [5]), _kfv([_d(3)], [0], [6]), 0.7, False)[1] == 0


def test_ref_rotation_bins():
    assert {R.rot_bin(a, 0.0) for a in np.arange(0, 360, 0.25)} == set(range(13))   # roundf(rot / 30): bins 0 .. 12 only
    assert R.rot_bin(0.0, 1.0) == 12 and R.rot_bin(14.9, 0.0) == 0 and R.rot_bin(15.0, 0.0) == 1
    assert R.compute_three_maxima([10, 1, 0, 5, 2]) == (0, 3, 4)
    assert R.compute_three_maxima([100, 9, 0, 5]) == (0, -1, -1)
    assert R.compute_three_maxima([100, 10, 9]) == (0, 1, -1)


def test_bow_entries_without_device(pkg):
    if pkg.device_count() > 0:
        pytest.skip("GPU present")
    v = _small(seed=3)
    h = _voc_from_ref(pkg, v)
    with pytest.raises(pkg.Tc2liError) as e:
        h.transform([np.zeros((4, 32), np.uint8)])
    assert e.value.code == -3
    out = pkg.capi.BowOut()
    f = pkg.lib().tc2li_orb_compute_bow_batch
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    buf = np.zeros(64, np.int64)
    for name, _ in pkg.capi.BowOut._fields_:
        setattr(out, name, buf.ctypes.data)
    assert f(None, h._h, 1, 4, 8, C.byref(out), None) == -3       # without a device nothing else is looked at
    g = pkg.lib().tc2li_track_reference_keyframe_batch
    g.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 9
    assert g(None, h._h, 1, None, None, 8, None, None, None, None, None, None, None, None, None) == -3
    kf = dict(keys=np.zeros(1, pkg.capi.KEYPOINT_DTYPE), descriptors=np.zeros((1, 32), np.uint8), has_point=np.ones(1, np.uint8),
              fv_node=[0], fv_offset=[0, 1], fv_index=[0])
    with pytest.raises(pkg.Tc2liError) as e:
        pkg.search_by_bow_batch([dict(keyframe=kf, frame=kf, nn_ratio=0.7, check_orientation=True)])
    assert e.value.code == -3
