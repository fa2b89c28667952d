"""Keyframe store and the batch entries of local mapping's geometric front half: tc2li_keyframe_store_*,
tc2li_create_new_map_points_batch, tc2li_fuse_search_batch.  Every batch result is compared with the CPU oracle
(oracle.create_new_map_points / oracle.fuse_search) problem by problem and, bit for bit, with the single-keyframe entries.
The keyframes are those of tests/test_mapping.py (five along the synthetic drive, 800 x 300, 1200 features, extracted by the oracle);
its small helpers are restated here."""
import threading

import numpy as np
import pytest

W, H = 800, 300
NFEAT = 1200
ERR_INVALID, ERR_CAPACITY = -2, -5
BOUNDS = (0.0, float(W), 0.0, float(H))


def camera_position(k):
    return np.array([0.25 * k + 0.05 * np.sin(1.3 * k), 0.0, 0.45 * k])


def make_keyframes(oracle, synthetic, n_kf, seed=5, mono_fraction=0.3, with_points=0.45):
    """Keyframe dicts, newest first (as tests/test_mapping.py builds them)."""
    ol, orr = oracle.OrbOracle(nfeatures=NFEAT), oracle.OrbOracle(nfeatures=NFEAT)
    bf = float(np.float32(synthetic.BF)); b = float(np.float32(synthetic.BF) / np.float32(synthetic.FX))
    scene = synthetic.Scene(seed)
    rng = np.random.default_rng(100 + seed)
    kfs = []
    for k in range(n_kf):
        c = camera_position(k)
        left, _ = scene.render(c[0], W, H, noise_seed=2 * k + 1, cam_z=c[2])
        right, _ = scene.render(c[0] + synthetic.BASELINE, W, H, noise_seed=2 * k + 2, cam_z=c[2])
        _, keys, desc = ol.extract(left)
        _, kr, dr = orr.extract(right)
        u_right, depth, _ = oracle.stereo_match(ol, orr, keys, desc, kr, dr, bf, b)
        n = len(keys)
        drop = rng.random(n) < mono_fraction
        u_right = np.where(drop, np.float32(-1), u_right).astype(np.float32)
        depth = np.where(drop, np.float32(-1), depth).astype(np.float32)
        node = (desc[:, 0] & 1).astype(np.int32) | ((desc[:, 5] & 1) << 1) | ((desc[:, 9] & 1) << 2) | ((desc[:, 14] & 1) << 3) | \
               ((desc[:, 21] & 1).astype(np.int32) << 4) | ((desc[:, 27] & 1).astype(np.int32) << 5)
        node = node * 7 + 3
        ids = np.unique(node)
        order = np.argsort(node, kind="stable")
        off = np.concatenate([[0], np.cumsum([(node == i).sum() for i in ids])]).astype(np.int32)
        kfs.append(dict(keys=keys, descriptors=desc, u_right=u_right, depth=depth, has_point=(rng.random(n) < with_points).astype(np.uint8),
                        fv_node=ids.astype(np.int32), fv_offset=off, fv_index=order.astype(np.int32),
                        pose7=np.concatenate([[0, 0, 0, 1], -c]).astype(np.float32), centre=c))
    return kfs[::-1]


def tables(n_levels=8):
    sf = np.cumprod(np.concatenate([[np.float32(1)], np.full(n_levels - 1, np.float32(1.2))])).astype(np.float32)
    return sf, (sf * sf).astype(np.float32)


def cam_of(synthetic):
    bf = np.float32(synthetic.BF)
    return np.float32([synthetic.FX, synthetic.FY, synthetic.CX, synthetic.CY]), float(bf), float(bf / np.float32(synthetic.FX))


def cam5_of(synthetic):
    cam4, mbf, _ = cam_of(synthetic)
    return np.float32([cam4[0], cam4[1], cam4[2], cam4[3], mbf]).astype(np.float64)


BARE, EMPTY = 5, 6  # slots beside the five keyframes: keyframe 0 without vocabulary entries, a keyframe without keypoints


@pytest.fixture(scope="module")
def stored(oracle, synthetic):
    """What goes into the store, slot by slot (never modified by a test)."""
    kfs = make_keyframes(oracle, synthetic, 5)
    bare = dict(kfs[0]); bare["fv_node"] = np.zeros(0, np.int32); bare["fv_offset"] = np.zeros(1, np.int32); bare["fv_index"] = np.zeros(0, np.int32)
    empty = dict(keys=kfs[0]["keys"][:0], descriptors=kfs[0]["descriptors"][:0], u_right=np.zeros(0, np.float32), depth=np.zeros(0, np.float32),
                 has_point=np.zeros(0, np.uint8), fv_node=np.zeros(0, np.int32), fv_offset=np.zeros(1, np.int32), fv_index=np.zeros(0, np.int32),
                 pose7=kfs[4]["pose7"].copy(), centre=kfs[4]["centre"])
    return kfs + [bare, empty]


def the_problems(stored, synthetic):
    """Seven CreateNewMapPoints problems over the stored keyframes: (store-level problem dicts, the same as (current, neighbours, flags) of
    keyframe dicts for the oracle and the single call)."""
    _, _, mb = cam_of(synthetic)
    rng = np.random.default_rng(77)
    other_hp = (rng.random(len(stored[0]["keys"])) < 0.6).astype(np.uint8)   # slot 0 again, with other map points
    near_pose = stored[0]["pose7"].copy(); near_pose[4] -= 0.5 * mb            # half the stereo baseline from keyframe 0 (LocalMapping.cc:456-460)
    spec = [
        (0, [1, 2, 3, 4], {}, {}, {}),
        (2, [4], {}, {}, {}),
        (1, [], {}, {}, {}),
        (0, [2, 3, EMPTY], dict(inertial=True), {0: other_hp}, {2: near_pose}),
        (3, [4, 2, 1, 0], dict(far_points=True, th_far_points=15.0), {}, {}),
        (4, [3, 2], dict(coarse=True), {}, {}),
        (BARE, [1, 2], {}, {}, {}),
    ]
    problems, views = [], []
    for cur, nbs, flags, hp_of, pose_of in spec:
        slots = [cur] + nbs
        kds = []
        for s in slots:
            kd = dict(stored[s])
            kd["has_point"] = hp_of.get(s, stored[s]["has_point"])
            kd["pose7"] = pose_of.get(s, stored[s]["pose7"])
            kds.append(kd)
        problems.append(dict(current=cur, neighbours=nbs, poses7=np.stack([k["pose7"] for k in kds]), has_point=[k["has_point"] for k in kds], **flags))
        views.append((kds[0], kds[1:], flags))
    return problems, views


DEGENERATE = (2, 6)  # no neighbours; a current keyframe without vocabulary entries


@pytest.fixture(scope="module")
def new_points_reference(oracle, synthetic, stored):
    cam4, mbf, mb = cam_of(synthetic)
    sf, sg = tables()
    problems, views = the_problems(stored, synthetic)
    want = [oracle.create_new_map_points(cur, nbs, cam4, mb, mbf, sf, sg, **flags) for cur, nbs, flags in views]
    return problems, views, want


def fuse_points(oracle, stored, synthetic, src, seed):
    """Map points = the stereo points of keyframe `src` (as tests/test_mapping.py makes them) and a valid mask."""
    cam4, _, _ = cam_of(synthetic)
    sf, _ = tables()
    rng = np.random.default_rng(seed)
    A = stored[src]
    sel = np.nonzero(A["depth"] > 0)[0]
    z = A["depth"][sel]
    Xc = np.stack([(A["keys"]["x"][sel] - cam4[2]) * z / cam4[0], (A["keys"]["y"][sel] - cam4[3]) * z / cam4[1], z], 1).astype(np.float32)
    Xw = (Xc + A["centre"].astype(np.float32)).astype(np.float32)
    pts = np.zeros(len(sel), oracle.MAP_POINT_DTYPE)
    pts["pos"] = Xw
    v = Xw - A["centre"].astype(np.float32)
    dist = np.linalg.norm(v, axis=1).astype(np.float32)
    pts["normal"] = v / dist[:, None]
    raw = (dist * sf[A["keys"]["octave"][sel]]).astype(np.float32)
    pts["max_distance_raw"] = raw
    pts["max_distance"] = np.float32(1.2) * raw
    pts["min_distance"] = np.float32(0.8) * (raw / sf[-1])
    pts["descriptor"] = A["descriptors"][sel]
    return pts, (rng.random(len(sel)) < 0.85).astype(np.uint8)


def the_fuse_items(oracle, stored, synthetic):
    """(items, points, valid, per item (dst keyframe dict, pose, points, valid, th) for the oracle and the single call)."""
    lists = {src: fuse_points(oracle, stored, synthetic, src, seed=src) for src in (2, 0, 1)}
    first = {}
    at = 0
    for src in (2, 0, 1):
        first[src] = at
        at += len(lists[src][0])
    points = np.concatenate([lists[src][0] for src in (2, 0, 1)])
    rng = np.random.default_rng(9)
    back = stored[0]["pose7"].copy(); back[6] -= 500.0
    #        src dst th   valid                                                     pose
    spec = [(2, 0, 3.0, lists[2][1], None), (0, 3, 3.0, lists[0][1], None), (1, 4, 6.0, lists[1][1], None),
            (2, 1, 3.0, (rng.random(len(lists[2][0])) < 0.5).astype(np.uint8), None),    # the point range of the first item, another valid
            (0, 2, 3.0, lists[0][1][:0], None),                                            # n_points = 0
            (1, 0, 3.0, lists[1][1], back)]                                                # every point behind the camera
    items, singles, valid = [], [], []
    nv = 0
    for src, dst, th, val, pose in spec:
        pose = stored[dst]["pose7"] if pose is None else pose
        n = len(val)
        items.append(dict(keyframe=dst, first_point=first[src], first_valid=nv, n_points=n, pose7=pose, th=th))
        singles.append((stored[dst], pose, lists[src][0][:n], val, th))
        valid.append(val)
        nv += n
    return items, points, np.concatenate(valid), singles


NON_DEGENERATE_ITEMS = (0, 1, 2, 3)


@pytest.fixture(scope="module")
def fuse_reference(oracle, synthetic, stored):
    cam4, mbf, _ = cam_of(synthetic)
    sf, sg = tables()
    isg, logsf = (np.float32(1) / sg).astype(np.float32), float(np.log(np.float32(1.2)))
    items, points, valid, singles = the_fuse_items(oracle, stored, synthetic)
    want = [oracle.fuse_search(B["keys"], B["descriptors"], B["u_right"], W, H, pose, cam4, mbf, sf, isg, logsf, pts, val, th=th)
            for B, pose, pts, val, th in singles]
    return items, points, valid, singles, want, (cam4, mbf, sf, isg, logsf)


@pytest.fixture(scope="module")
def store(pkg, stored):
    with pkg.KeyframeStore(8, 1500) as s:
        s.put_batch(list(range(len(stored))), stored, BOUNDS)
        yield s


def run_batch(pkg, synthetic, store, problems, **kw):
    _, _, mb = cam_of(synthetic)
    sf, sg = tables()
    return pkg.capi.create_new_map_points_batch(store, problems, cam5_of(synthetic), mb, sf, sg, **kw)


def check_against_oracle(got, want):
    assert len(got) == len(want)
    for p, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g[0], w[0]), p
        stereo = w[0][:, 3] == 1
        assert np.array_equal(g[1][stereo], w[1][stereo]), p                              # un-projections: bit for bit
        assert np.allclose(g[1][~stereo], w[1][~stereo], rtol=1e-4, atol=1e-5), p         # triangulations: Jacobi against SVD


# ---- CPU: the cases are worth comparing, and argument checks that come before any device work ------------------------------------------
def test_oracle_problems_are_not_trivial(new_points_reference, fuse_reference):
    _, _, want = new_points_reference
    assert len(want) == 7
    for p, (idx, _) in enumerate(want):
        assert (len(idx) == 0) if p in DEGENERATE else (len(idx) >= 20), (p, len(idx))
    assert any((idx[:, 3] == 1).any() for idx, _ in want) and any((idx[:, 3] == 0).any() for idx, _ in want)
    assert not (want[3][0][:, 1] == 0).any() and not (want[3][0][:, 1] == 2).any()       # the near and the empty neighbour give nothing
    assert not np.array_equal(want[0][0], want[3][0])                                     # slot 0 twice, different results
    fwant = fuse_reference[4]
    for k, (nf, bi, _) in enumerate(fwant):
        assert (nf > 50) if k in NON_DEGENERATE_ITEMS else (nf == 0), (k, nf)
    assert len(fwant[4][1]) == 0


def test_arguments_refused_before_any_device_work(pkg):
    import ctypes as C
    L = pkg.lib()
    h = C.c_void_p()
    L.tc2li_keyframe_store_create.argtypes = [C.c_int, C.c_int, C.c_void_p]
    assert L.tc2li_keyframe_store_create(0, 100, C.byref(h)) == ERR_INVALID
    assert L.tc2li_keyframe_store_create(4, 0, C.byref(h)) == ERR_INVALID
    assert L.tc2li_keyframe_store_create(4, 100, None) == ERR_INVALID
    P, I, F = C.c_void_p, C.c_int, C.c_float
    for name, argtypes in (("tc2li_keyframe_store_put_batch", [P, I, P, P, P, I, P]),
                           ("tc2li_create_new_map_points_batch", [P, P, I, P, F, P, P, I, F, P, P, P, P]),
                           ("tc2li_fuse_search_batch", [P, P, I, P, F, P, P, I, F, P, I, P, I, P, P, P, P]),
                           ("tc2li_keyframe_store_erase", [P, I]), ("tc2li_keyframe_store_info", [P, I, P, P])):
        f = getattr(L, name)
        f.argtypes = argtypes
        assert f(*[None if t is P else t(1) for t in argtypes]) == ERR_INVALID, name   # no store


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def batch_result(pkg, synthetic, store, new_points_reference):
    return run_batch(pkg, synthetic, store, new_points_reference[0])


@pytest.mark.gpu
def test_new_points_batch_matches_the_oracle(new_points_reference, batch_result):
    _, _, want = new_points_reference
    for p, (idx, _) in enumerate(want):
        assert (len(idx) == 0) if p in DEGENERATE else (len(idx) >= 20), (p, len(idx))
    assert any((idx[:, 3] == 1).any() for idx, _ in want) and any((idx[:, 3] == 0).any() for idx, _ in want)
    check_against_oracle(batch_result, want)


@pytest.mark.gpu
def test_new_points_batch_equals_the_single_call(pkg, synthetic, store, new_points_reference, batch_result):
    problems, views, _ = new_points_reference
    _, _, mb = cam_of(synthetic)
    sf, sg = tables()
    for p, (cur, nbs, flags) in enumerate(views):
        one = pkg.capi.create_new_map_points(cur, nbs, cam5_of(synthetic), mb, sf, sg, **flags)
        assert np.array_equal(batch_result[p][0], one[0]), p                              # records in creation order
        assert batch_result[p][1].tobytes() == one[1].tobytes(), p                        # every x3D bit
    a = run_batch(pkg, synthetic, store, problems, raw=True)
    b = run_batch(pkg, synthetic, store, problems, raw=True)
    assert a[0] == b[0] >= 0 and np.array_equal(a[1], b[1])
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a[2], b[2]))
    assert [len(x) for x in a[2]] == [len(r[0]) for r in batch_result]


@pytest.mark.gpu
def test_new_points_batch_capacity(pkg, synthetic, store, new_points_reference, batch_result):
    problems = new_points_reference[0]
    counts = [len(r[0]) for r in batch_result]
    caps = list(counts)
    caps[4] -= 1
    rc, n_points, _ = run_batch(pkg, synthetic, store, problems, capacities=caps, raw=True)
    assert rc == ERR_CAPACITY and list(n_points) == counts
    rc, n_points, recs = run_batch(pkg, synthetic, store, problems, capacities=counts, raw=True)  # exactly enough room
    assert rc == sum(counts) and list(n_points) == counts and [len(r) for r in recs] == counts


@pytest.mark.gpu
def test_fuse_batch_matches_the_oracle_and_the_single_call(pkg, store, fuse_reference):
    items, points, valid, singles, want, (cam4, mbf, sf, isg, logsf) = fuse_reference
    nf, bi, bd = pkg.capi.fuse_search_batch(store, items, cam4, mbf, sf, isg, logsf, points, valid)
    assert len(bi) == len(valid) == sum(it["n_points"] for it in items)
    for k, (it, (B, pose, pts, val, th)) in enumerate(zip(items, singles)):
        r = slice(it["first_valid"], it["first_valid"] + it["n_points"])
        assert (want[k][0] > 50) if k in NON_DEGENERATE_ITEMS else (want[k][0] == 0), k
        assert nf[k] == want[k][0] and np.array_equal(bi[r], want[k][1]) and np.array_equal(bd[r], want[k][2]), k
        one = pkg.capi.fuse_search(B["keys"], B["descriptors"], B["u_right"], W, H, pose, cam4, mbf, sf, isg, logsf, pts, val, th=th)
        assert nf[k] == one[0] and np.array_equal(bi[r], one[1]), k
        if it["n_points"]:
            assert np.array_equal(bd[r], one[2]), k
    assert not np.array_equal(bi[:items[0]["n_points"]], bi[items[3]["first_valid"]:items[3]["first_valid"] + items[3]["n_points"]])
    with pytest.raises(pkg.capi.Tc2liError) as e:
        pkg.capi.fuse_search_batch(store, items, cam4, mbf, sf, isg, 0.0, points, valid)
    assert e.value.code == ERR_INVALID
    for bad in (dict(items[0], first_point=len(points) - 1), dict(items[0], first_valid=len(valid) - 1), dict(items[0], keyframe=7), dict(items[0], keyframe=99)):
        with pytest.raises(pkg.capi.Tc2liError) as e:
            pkg.capi.fuse_search_batch(store, [bad], cam4, mbf, sf, isg, logsf, points, valid)
        assert e.value.code == ERR_INVALID


@pytest.mark.gpu
def test_store_semantics(pkg, oracle, synthetic, stored, fuse_reference):
    cam4, mbf, mb = cam_of(synthetic)
    sf, sg = tables()
    items, points, valid, _, _, (_, _, _, isg, logsf) = fuse_reference
    with pkg.KeyframeStore(4, 1400) as s:
        assert s.info(0) == (-1, -1)
        s.put_batch([0, 1, 2], [stored[2], stored[4], stored[0]], BOUNDS)
        assert [s.info(k) for k in range(4)] == [(len(stored[2]["keys"]), len(stored[2]["fv_node"])), (len(stored[4]["keys"]), len(stored[4]["fv_node"])),
                                                 (len(stored[0]["keys"]), len(stored[0]["fv_node"])), (-1, -1)]

        def both(slot0):  # keyframe `slot0` of the list sits in slot 0: points of keyframe 2's list fused into it, and it as the current keyframe against slot 1 (keyframe 4)
            it = dict(items[0], keyframe=0, pose7=stored[slot0]["pose7"])
            f = pkg.capi.fuse_search_batch(s, [it], cam4, mbf, sf, isg, logsf, points, valid[:it["n_points"]])
            pr = dict(current=0, neighbours=[1], poses7=np.stack([stored[slot0]["pose7"], stored[4]["pose7"]]), has_point=[stored[slot0]["has_point"], stored[4]["has_point"]])
            c = pkg.capi.create_new_map_points_batch(s, [pr], cam5_of(synthetic), mb, sf, sg)
            B = stored[slot0]
            fw = oracle.fuse_search(B["keys"], B["descriptors"], B["u_right"], W, H, B["pose7"], cam4, mbf, sf, isg, logsf, points[:it["n_points"]], valid[:it["n_points"]], th=3.0)
            cw = oracle.create_new_map_points(B, [stored[4]], cam4, mb, mbf, sf, sg)
            assert len(cw[0]) >= 20
            assert f[0][0] == fw[0] and np.array_equal(f[1], fw[1]) and np.array_equal(f[2], fw[2])
            check_against_oracle(c, [cw])
            return f, c

        f2, c2 = both(2)
        s.erase(0)
        assert s.info(0) == (-1, -1)
        for call in (lambda: pkg.capi.fuse_search_batch(s, [dict(items[0], keyframe=0)], cam4, mbf, sf, isg, logsf, points, valid),
                     lambda: pkg.capi.create_new_map_points_batch(s, [dict(current=1, neighbours=[0], poses7=np.zeros((2, 7), np.float32),
                                                                      has_point=[stored[4]["has_point"], stored[2]["has_point"]])], cam5_of(synthetic), mb, sf, sg)):
            with pytest.raises(pkg.capi.Tc2liError) as e:     # an empty slot named in an item / a problem
                call()
            assert e.value.code == ERR_INVALID
        s.put_batch([0], [stored[0]], BOUNDS)                  # another keyframe into the same slot: no stale grid or descriptors
        assert s.info(0) == (len(stored[0]["keys"]), len(stored[0]["fv_node"]))
        f0, c0 = both(0)
        assert not np.array_equal(f0[1], f2[1]) and not np.array_equal(c0[0][0], c2[0][0])
        # refused puts leave the store as it was
        before = [s.info(k) for k in range(4)]
        big = {k: (np.concatenate([v, v]) if k in ("keys", "descriptors", "u_right", "depth", "has_point") else v) for k, v in stored[0].items()}
        assert len(big["keys"]) > 1400
        bad = dict(stored[1]); bad["fv_index"] = stored[1]["fv_index"].copy(); bad["fv_index"][0] = 10 ** 6
        for slots, kfs, code in (([3], [big], ERR_CAPACITY), ([3, 3], [stored[3], stored[4]], ERR_INVALID), ([3, 0], [stored[3], bad], ERR_INVALID),
                                 ([4], [stored[3]], ERR_INVALID)):
            with pytest.raises(pkg.capi.Tc2liError) as e:
                s.put_batch(slots, kfs, BOUNDS)
            assert e.value.code == code
        with pytest.raises(pkg.capi.Tc2liError) as e:          # an octave the level tables do not have
            s.put_batch([3], [stored[3]], BOUNDS, n_levels=int(stored[3]["keys"]["octave"].max()))
        assert e.value.code == ERR_INVALID
        assert [s.info(k) for k in range(4)] == before
        f0b, c0b = both(0)
        assert np.array_equal(f0b[1], f0[1]) and c0b[0][1].tobytes() == c0[0][1].tobytes()


@pytest.mark.gpu
def test_concurrent_callers_share_one_store(pkg, synthetic, stored, store, new_points_reference, batch_result):
    problems = new_points_reference[0]
    out, errors = {}, []
    start = threading.Barrier(3)

    def search(name):
        try:
            start.wait()
            out[name] = [run_batch(pkg, synthetic, store, problems) for _ in range(3)]
        except Exception as e:  # noqa: BLE001 -- reported below
            errors.append(e)

    def put():
        try:
            start.wait()
            for _ in range(3):
                store.put_batch([7], [stored[3]], BOUNDS)
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=search, args=("a",)), threading.Thread(target=search, args=("b",)), threading.Thread(target=put)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    filled = store.info(7)
    store.erase(7)
    assert filled == (len(stored[3]["keys"]), len(stored[3]["fv_node"]))
    for name in ("a", "b"):
        for got in out[name]:
            for g, w in zip(got, batch_result):
                assert np.array_equal(g[0], w[0]) and g[1].tobytes() == w[1].tobytes()
    check_against_oracle(out["a"][0], new_points_reference[2])
