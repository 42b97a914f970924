"""ycnr_als_recommend: top-N for users of a resident trainer handle, from the factor matrices on the device.

The parity contract is bit equality with ycnr_recommend_items on the same rows (the fused kernel keeps that entry's
MFMA operand order, so every predict has the same bits, and both rank equal predicts by item id): ids, predicts and
counts are compared with np.array_equal, no tolerances.  float64 is also checked against the oracle directly.
"""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from helpers import make_problem
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
ADDON = os.path.join(ROOT, "you-can-not-recommend_amd", "addon", "ycnr_als.node")


@pytest.fixture(scope="module")
def als():
    import ycnr_als
    L = ycnr_als._lib.load()  # raises if libycnr_als.so is missing: no fallback
    assert L.ycnr_device_count() >= 1, L.ycnr_last_error()
    return ycnr_als


def problem(users, items, k, seed, dt=np.float32, skip_frac=0.1):
    rng = np.random.default_rng(seed)
    U = (rng.standard_normal((users, k)) * 0.8).astype(dt)
    V = (rng.standard_normal((items, k)) * 0.8).astype(dt)
    skips = [np.sort(rng.choice(items, rng.integers(0, max(2, int(items * skip_frac))), replace=False)).astype(np.int32) for _ in range(users)]
    ptr = np.zeros(users + 1, np.int64)
    ptr[1:] = np.cumsum([len(x) for x in skips])
    return U, V, ptr, (np.concatenate(skips) if users else np.zeros(0, np.int32)), skips


def device_with(als, U, V):
    dev = als.AlsDevice(U.shape[1], U.shape[0], V.shape[0], useDoublePrecision=(U.dtype == np.float64))
    dev.set_factors("byUser", U)
    dev.set_factors("byItem", V)
    return dev


def request(skips, uid):
    """skip CSR relative to the request"""
    ptr = np.zeros(len(uid) + 1, np.int64)
    ptr[1:] = np.cumsum([len(skips[u]) for u in uid])
    sk = np.concatenate([skips[u] for u in uid]) if len(uid) else np.zeros(0, np.int32)
    return ptr, sk.astype(np.int32)


def assert_same(got, want):
    for g, w, name in zip(got[:3], want[:3], ("ids", "predicts", "counts")):
        assert g.shape == w.shape and np.array_equal(g, w), name


LIMITS = (1, 2, 20, 64, 65, 400)  # 64 / 65: the last fused limit and the first that goes through the score matrix


@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("users,items,k", [(40, 1234, 100), (3, 50, 8), (17, 17, 7), (5, 5000, 20), (64, 700, 256)])
def test_bits_equal_recommend_items(als, users, items, k, dt):
    U, V, _, _, skips = problem(users, items, k, 100 + k, dt)
    rng = np.random.default_rng(k)
    uid = np.concatenate([rng.permutation(users), rng.integers(0, users, 5)]).astype(np.int32)  # permuted, with repeats
    ptr, sk = request(skips, uid)
    dev = device_with(als, U, V)
    try:
        for limit in LIMITS:
            want = als.recommend_items(U[uid], V, ptr, sk, globalAvgShift=0.2, minRecommendRating=1.0, limit=limit)
            got = dev.recommend(uid, ptr, sk, globalAvgShift=0.2, minRecommendRating=1.0, limit=limit)
            assert_same(got, want)
            assert got[3] >= 0
            if limit in (20, 400):
                assert got[2].max() > 1  # (the case is not vacuous)
    finally:
        dev.destroy()


def test_bits_equal_beyond_the_lds_bound(als):
    # k = 1000 float32: sixteen padded user rows are 64 KB, more than the 48 KB the MFMA kernels use -> the 16-lane-group score kernel
    U, V, _, _, skips = problem(20, 700, 1000, 5)
    uid = np.array([3, 19, 0, 3, 7], np.int32)
    ptr, sk = request(skips, uid)
    dev = device_with(als, U, V)
    try:
        for limit in (20, 65):
            assert_same(dev.recommend(uid, ptr, sk, 0.0, 1.0, limit), als.recommend_items(U[uid], V, ptr, sk, 0.0, 1.0, limit))
    finally:
        dev.destroy()


def test_float64_against_the_oracle(als):
    # the shape and seed of tests/test_recommend.py::test_gpu_float64_exact: no near-ties
    U, V, ptr, sk, skips = problem(40, 1234, 100, 3, np.float64)
    dev = device_with(als, U, V)
    try:
        ids, pred, cnt, _ = dev.recommend(np.arange(40, dtype=np.int32), ptr, sk, globalAvgShift=0.3, minRecommendRating=2.0, limit=20)
    finally:
        dev.destroy()
    for u in range(40):
        oid, opr = orc.recommend(U[u], V, skips[u], 0.3, 2.0, 20)
        assert cnt[u] == len(oid) <= 19
        assert np.array_equal(ids[u, :cnt[u]], oid) and np.allclose(pred[u, :cnt[u]], opr, rtol=1e-12, atol=0)
        assert (ids[u, cnt[u]:] == -1).all() and (pred[u, cnt[u]:] == 0).all()


@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("limit", [6, 40])
def test_ties_rank_by_item_id(als, limit, dt):
    # 8 distinct item rows tiled to 400 items: every predict occurs 50 times, in different tiles, waves and workgroups
    rng = np.random.default_rng(21)
    U = (rng.standard_normal((6, 12)) * 0.8).astype(dt)
    V = np.tile((rng.standard_normal((8, 12)) * 0.8).astype(dt), (50, 1))
    uid = np.arange(6, dtype=np.int32)
    best = int(np.argmax(V[:8].astype(np.float64) @ U[0].astype(np.float64)))  # user 0's best row: its tie group leads the list
    skips = [np.array([best + 16], np.int32)] + [np.zeros(0, np.int32)] * 5        # one skipped id inside that group
    ptr, sk = request(skips, uid)
    dev = device_with(als, U, V)
    try:
        got = dev.recommend(uid, ptr, sk, 0.0, -1e9, limit)
    finally:
        dev.destroy()
    assert_same(got, als.recommend_items(U, V, ptr, sk, 0.0, -1e9, limit))
    ids, pred, cnt = got[:3]
    assert (cnt == limit - 1).all()
    for u in range(6):
        p, i = pred[u, :cnt[u]], ids[u, :cnt[u]]
        assert (np.diff(p) <= 0).all()
        same = np.diff(p) == 0
        assert same.any() and (np.diff(i)[same] > 0).all()  # equal predicts: ascending ids
    want0 = [i for i in range(best, 400, 8) if i != best + 16][:limit - 1]
    assert ids[0, :min(limit - 1, 49)].tolist() == want0[:49]


def test_edges(als):
    U, V, ptr, sk, skips = problem(3, 50, 8, 11)
    uid = np.arange(3, dtype=np.int32)
    dev = device_with(als, U, V)
    try:
        # everything skipped for user 0
        ptr2, sk2 = np.array([0, 50, 50, 50], np.int64), np.arange(50, dtype=np.int32)
        ids, pred, cnt, _ = dev.recommend(uid, ptr2, sk2, 0.0, -1e9, 10)
        assert cnt[0] == 0 and cnt[1] == 9 and (ids[0] == -1).all() and (pred[0] == 0).all()
        # a threshold above every predict
        ids, pred, cnt, _ = dev.recommend(uid, ptr, sk, 0.0, 1e9, 10)
        assert (cnt == 0).all() and (ids == -1).all()
        # a skip id outside the catalogue matches nothing
        free = dev.recommend(uid, np.zeros(4, np.int64), np.zeros(0, np.int32), 0.0, -1e9, 10)
        far = dev.recommend(uid, np.array([0, 1, 2, 2], np.int64), np.array([50, 1 << 30], np.int32), 0.0, -1e9, 10)
        assert_same(far, free)
        # nUsers == 0
        ids, pred, cnt, _ = dev.recommend(np.zeros(0, np.int32), np.zeros(1, np.int64), np.zeros(0, np.int32))
        assert ids.shape == (0, 20) and cnt.shape == (0,)
        # invalid requests: ERR_INVALID, outputs untouched
        L, h = dev._L, dev._h
        good_ptr = np.array([0, 2, 2, 2], np.int64)
        for what, u, p, s, limit in (("descending skip ids", uid, good_ptr, np.array([5, 4], np.int32), 10),
                                     ("repeated skip id", uid, good_ptr, np.array([4, 4], np.int32), 10),
                                     ("user id == totalUsersCount", np.array([0, 3, 1], np.int32), good_ptr, np.array([4, 5], np.int32), 10),
                                     ("user id -1", np.array([0, -1, 1], np.int32), good_ptr, np.array([4, 5], np.int32), 10),
                                     ("limit 0", uid, good_ptr, np.array([4, 5], np.int32), 0),
                                     ("limit 4097", uid, good_ptr, np.array([4, 5], np.int32), 4097)):
            oi, op, oc = np.full((3, 10), 77, np.int32), np.full((3, 10), 7.5), np.full(3, 77, np.int32)
            rc = L.ycnr_als_recommend(h, 3, u.ctypes.data, p.ctypes.data, s.ctypes.data, 0.0, -1e9, limit, oi.ctypes.data, op.ctypes.data,
                                      oc.ctypes.data, None)
            assert rc == als._lib.ERR_INVALID, what
            assert (oi == 77).all() and (op == 7.5).all() and (oc == 77).all(), what
        with pytest.raises(als.YcnrError) as e:
            dev.recommend(uid, ptr2, sk2[::-1].copy(), 0.0, 0.0, 10)
        assert e.value.code == als._lib.ERR_INVALID
        with pytest.raises(als.YcnrError) as e:
            dev.recommend(uid, ptr, sk, 0.0, 0.0, 0)
        assert e.value.code == als._lib.ERR_INVALID
    finally:
        dev.destroy()
    # a NaN in one item row: that item never competes
    V2 = V.copy()
    V2[7, 3] = np.nan
    dev = device_with(als, U, V2)
    try:
        none = (np.zeros(4, np.int64), np.zeros(0, np.int32))
        got = dev.recommend(uid, *none, 0.0, -1e9, 50)
        assert (got[2] == 49).all() and not (got[0] == 7).any() and np.isfinite(got[1]).all()
        assert_same(got, als.recommend_items(U, V2, *none, 0.0, -1e9, 50))
    finally:
        dev.destroy()


@pytest.mark.parametrize("k", [20, 7])  # 7: float32 half-steps work on padded copies, recommend reads the masters
def test_ordered_behind_the_half_steps_in_flight(als, k):
    users, items = 200, 150
    bu, bi, U, V = make_problem(users, items, k, density=0.2, seed=1)
    dev = als.AlsDevice(k, users, items)
    try:
        dev.set_ratings("byUser", bu.rowPtr, bu.indx, bu.vals)
        dev.set_ratings("byItem", bi.rowPtr, bi.indx, bi.vals)
        dev.set_factors("byUser", U)
        dev.set_factors("byItem", V)
        uid = np.array([199, 0, 17, 4, 17, 100], np.int32)
        skips = [bu.indx[bu.rowPtr[u]:bu.rowPtr[u + 1]].astype(np.int32) for u in range(users)]
        ptr, sk = request(skips, uid)
        dev.step_async("byUser")
        dev.step_async("byItem")
        first = dev.recommend(uid, ptr, sk, 3.0, 3.2, 10)   # no sync in between
        dev.sync()
        U1, V1 = dev.get_factors("byUser"), dev.get_factors("byItem")
        assert not np.array_equal(U1, U) and not np.array_equal(V1, V)
        assert_same(first, als.recommend_items(U1[uid], V1, ptr, sk, 3.0, 3.2, 10))
        assert first[2].max() > 0
        assert_same(dev.recommend(uid, ptr, sk, 3.0, 3.2, 10), first)
    finally:
        dev.destroy()


def split_dataset(seed, users, items, dt):
    """train (types 1, 2) by user and by item, validate (2) and test (3) by user, like tests/test_node_host.py builds them"""
    from ycnr_als.data import Csr
    from ycnr_als.emf import Dataset
    bu, _, U, V = make_problem(users, items, 8, density=0.35, seed=seed, min_per_row=1, empty_rows=(3,))
    bu.vals = bu.vals.astype(dt)
    user = np.repeat(np.arange(users), bu.counts()).astype(np.int32)
    typ = np.random.default_rng(seed).choice([1, 1, 1, 1, 1, 1, 2, 3], size=bu.nnz).astype(np.int8)

    def sub(mask):
        rp = np.zeros(bu.rows + 1, np.int64)
        rp[1:] = np.cumsum(np.bincount(user[mask], minlength=bu.rows))
        return Csr(bu.rows, bu.cols, rp, bu.indx[mask].copy(), bu.vals[mask].copy())

    tu, ti, tv = user[typ <= 2], bu.indx[typ <= 2], bu.vals[typ <= 2]
    o = np.lexsort((tu, ti))
    rp = np.zeros(bu.cols + 1, np.int64)
    rp[1:] = np.cumsum(np.bincount(ti, minlength=bu.cols))
    tri = Csr(bu.cols, bu.rows, rp, tu[o].astype(np.int32), tv[o].copy())
    ds = Dataset(sub(typ <= 2), tri, sub(typ == 2), sub(typ == 3), float(bu.vals.astype(np.float64).mean()))
    return ds, bu, user, typ, U.astype(dt), V.astype(dt)


def test_python_host_recommends_from_the_trained_handle(als, tmp_path):
    # float64, so that the oracle's dot and the kernel's agree to rounding and the order is the oracle's (rtol 1e-12 as above)
    from ycnr_als.emf import EmfLord
    ds, bu, _, _, U, V = split_dataset(6, 60, 45, np.float64)
    lord = EmfLord(options={"factorsCount": 8, "trainIters": 2, "useDoublePrecision": True, "dbType": "ml", "dataDir": str(tmp_path),
                            "ratingsInPortionForRmse": 30, "numThreadsForTrain": {"als": 2}})
    try:
        lord.prepareToTrain(ds, U, V)
        lord.train()
        uid, unrated = [17, 4, 59, 3, 17], [None, [0, 1, 2], None, None, [44]]
        recs = lord.recommendItemsForUsers(uid, limit=6, minRecommendRating=2.5, unratedItems=unrated)
        U1, V1 = lord.backend.get_factors(0), lord.backend.get_factors(1)
        shift = lord.globalAvgShift
    finally:
        lord.destroy()
    assert len(recs) == 5 and any(len(r) > 0 for r in recs)
    for u, extra, rec in zip(uid, unrated, recs):
        rated = bu.indx[bu.rowPtr[u]:bu.rowPtr[u + 1]]  # every rating of the user: train, validate and test
        skip = np.unique(np.concatenate([rated, np.asarray(extra or [], np.int64)])).astype(np.int32)
        oid, opr = orc.recommend(U1[u], V1, skip, shift, 2.5, 6)
        assert len(rec) == len(oid) < 6
        assert [r["id"] for r in rec] == (oid + 1).tolist()  # 1-based
        assert np.allclose([r["predict"] for r in rec], opr, rtol=1e-12, atol=0)
        assert not np.isin(np.array([r["id"] - 1 for r in rec], np.int64), skip).any()


@pytest.mark.skipif(shutil.which("node") is None or not os.path.exists(ADDON), reason="node or the built addon is missing")
def test_js_host_recommends_like_the_python_host(als, tmp_path):
    """Driven like tests/test_node_host.py::test_js_train_matches_python_host: both hosts warm-start from the same factor
    files and train through the same library, so their factors -- and with them ids and predicts -- are the same bits."""
    from ycnr_als.emf import EmfLord
    ds, bu, user, typ, U, V = split_dataset(6, 60, 45, np.float32)
    pydir, jsdir = tmp_path / "py", tmp_path / "js"
    opts = {"factorsCount": 8, "trainIters": 2, "useDoublePrecision": False, "dbType": "ml", "ratingsInPortionForRmse": 30,
            "numThreadsForTrain": {"als": 2}}
    seedlord = EmfLord(options=dict(opts, dataDir=str(jsdir), trainIters=0))
    seedlord.prepareToTrain(ds, U, V)
    seedlord.train()  # zero iterations: writes the starting factors as ml_factors_ready
    seedlord.destroy()
    uid, unrated = [17, 4, 59, 3, 17], [None, [0, 1, 2], None, None, [44]]
    lord = EmfLord(options=dict(opts, dataDir=str(pydir)))
    try:
        lord.prepareToTrain(ds, U, V)
        lord.train()
        want = lord.recommendItemsForUsers(uid, limit=6, minRecommendRating=2.5, unratedItems=unrated)
    finally:
        lord.destroy()
    inp = {"dir": str(jsdir), "k": 8, "iters": 2, "rip": 30, "threads": 2, "useDoublePrecision": False, "users": bu.rows, "items": bu.cols,
           "user": user.tolist(), "item": bu.indx.tolist(), "rating": bu.vals.tolist(), "type": typ.tolist(),
           "userIds": uid, "unratedItems": unrated, "limit": 6, "minRecommendRating": 2.5}
    (tmp_path / "in.json").write_text(json.dumps(inp))
    r = subprocess.run(["node", os.path.join(HERE, "js", "recommend_gpu.js"), str(tmp_path / "in.json")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert any(len(x) > 0 for x in want)
    assert [[x["id"] for x in rec] for rec in out["recs"]] == [[x["id"] for x in rec] for rec in want]
    assert [[x["predict"] for x in rec] for rec in out["recs"]] == [[x["predict"] for x in rec] for rec in want]
    assert "itemStepSharding" in out["bandsError"]
