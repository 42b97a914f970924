"""EmfLord.recommendItemsForUsers (YcnrController.recommendItemsForUser, lib/YcnrController.js:227-284) on the CPU: the
host logic -- skip lists, 1-based ids, the limit - 1 rule, refusals -- with a test-only backend whose recommend() is the
oracle's restatement of the reference loop.  The package itself has no CPU path: a backend without recommend() raises."""
import numpy as np
import pytest

from helpers import OracleBackend, make_problem
from oracle import oracle as orc
from ycnr_als.data import Csr
from ycnr_als.emf import Dataset, EmfLord

USERS, ITEMS, K = 30, 40, 6


class RecommendingOracle(OracleBackend):
    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.requests = []

    def recommend(self, user_ids, skip_ptr, skip_ids, shift, min_rating, limit):
        self.requests.append((np.array(user_ids), np.array(skip_ptr), np.array(skip_ids), shift, min_rating, limit))
        n = len(user_ids)
        ids, pred, cnt = np.full((n, limit), -1, np.int32), np.zeros((n, limit)), np.zeros(n, np.int32)
        for i, u in enumerate(user_ids):
            oid, opr = orc.recommend(self.fac_np[0][u], self.fac_np[1], skip_ids[skip_ptr[i]:skip_ptr[i + 1]], shift, min_rating, limit)
            cnt[i] = len(oid)
            ids[i, :len(oid)], pred[i, :len(oid)] = oid, opr
        return ids, pred, cnt


def dataset(seed=2):
    bu, _, U, V = make_problem(USERS, ITEMS, K, density=0.3, seed=seed, min_per_row=2, dtype=np.float64)
    user = np.repeat(np.arange(USERS), bu.counts()).astype(np.int32)
    typ = np.random.default_rng(seed).choice([1, 1, 1, 1, 2, 3], size=bu.nnz).astype(np.int8)

    def sub(mask):
        rp = np.zeros(USERS + 1, np.int64)
        rp[1:] = np.cumsum(np.bincount(user[mask], minlength=USERS))
        return Csr(USERS, ITEMS, rp, bu.indx[mask].copy(), bu.vals[mask].copy())

    tu, ti, tv = user[typ <= 2], bu.indx[typ <= 2], bu.vals[typ <= 2]
    o = np.lexsort((tu, ti))
    rp = np.zeros(ITEMS + 1, np.int64)
    rp[1:] = np.cumsum(np.bincount(ti, minlength=ITEMS))
    tri = Csr(ITEMS, USERS, rp, tu[o].astype(np.int32), tv[o].copy())
    return Dataset(sub(typ <= 2), tri, sub(typ == 2), sub(typ == 3)), bu, typ, user, U, V


def lord_with(backend_cls, tmp_path, ds, U, V):
    lord = EmfLord(options={"factorsCount": K, "trainIters": 1, "useDoublePrecision": True, "dataDir": str(tmp_path),
                            "numThreadsForTrain": {"als": 1}, "numThreadsForRmse": 1},
                   backend_factory=lambda o, u, i, d: backend_cls(o, u, i, d))
    lord.prepareToTrain(ds, U, V)
    return lord


def test_skip_lists_ids_and_the_limit_rule(tmp_path):
    ds, bu, typ, user, U, V = dataset()
    assert (typ == 3).any() and (typ == 2).any()
    lord = lord_with(RecommendingOracle, tmp_path, ds, U, V)
    lord.globalAvgShift = 0.25
    uid = [7, 0, 29, 7]
    unrated = [None, [5, 5, 3, 39], [], [bu.indx[bu.rowPtr[7]]]]  # duplicates, and an id the user has rated anyway
    recs = lord.recommendItemsForUsers(uid, limit=5, minRecommendRating=-100.0, unratedItems=unrated)
    got_u, ptr, skip, shift, thr, limit = lord.backend.requests[-1]
    assert got_u.tolist() == uid and shift == 0.25 and thr == -100.0 and limit == 5 and ptr[0] == 0 and len(ptr) == 5
    for i, u in enumerate(uid):
        rated = bu.indx[bu.rowPtr[u]:bu.rowPtr[u + 1]]  # train, validate and test ratings of the user
        want = sorted(set(rated.tolist()) | set(unrated[i] or []))
        mine = skip[ptr[i]:ptr[i + 1]]
        assert mine.tolist() == want and mine.dtype == np.int32          # the union, sorted, unique
        oid, opr = orc.recommend(U[u], V, np.array(want, np.int32), 0.25, -100.0, 5)
        assert len(recs[i]) == 4 == len(oid)                               # the reference never returns `limit` items
        assert [r["id"] for r in recs[i]] == (oid + 1).tolist()            # 1-based (YcnrController.js:261-266)
        assert [r["predict"] for r in recs[i]] == opr.tolist()
        assert not set(r["id"] - 1 for r in recs[i]) & set(want)
    # the test set's ratings are skipped, not only the train set's
    u3 = int(user[np.flatnonzero(typ == 3)[0]])
    i3 = int(bu.indx[np.flatnonzero(typ == 3)[0]])
    lord.recommendItemsForUsers([u3], limit=ITEMS + 1, minRecommendRating=-100.0)
    _, ptr, skip, _, _, _ = lord.backend.requests[-1]
    assert i3 in skip.tolist()
    # the threshold of the reference's getter: 3.5 for 'ml' (0.7 maxRating)
    lord.recommendItemsForUsers([0])
    assert lord.backend.requests[-1][4] == 3.5 and lord.backend.requests[-1][5] == 20
    assert lord.recommendItemsForUsers([]) == []
    with pytest.raises(ValueError):
        lord.recommendItemsForUsers([USERS])
    with pytest.raises(ValueError):
        lord.recommendItemsForUsers([0, 1], unratedItems=[[1]])
    lord.destroy()


def test_refused_where_the_user_matrix_is_not_replicated(tmp_path):
    ds, _, _, _, U, V = dataset()
    lord = lord_with(RecommendingOracle, tmp_path, ds, U, V)
    lord.bands, lord.world = np.array([0, USERS], np.int64), 2   # what prepareToTrain leaves with itemStepSharding='bands' on 2 ranks
    with pytest.raises(RuntimeError, match="itemStepSharding"):
        lord.recommendItemsForUsers([0])
    assert lord.backend.requests == []
    lord.bands, lord.world = None, 1
    assert len(lord.recommendItemsForUsers([0], minRecommendRating=-100.0)) == 1
    lord.destroy()


def test_a_backend_without_recommend_raises_instead_of_computing(tmp_path):
    ds, _, _, _, U, V = dataset()
    lord = lord_with(OracleBackend, tmp_path, ds, U, V)
    with pytest.raises(RuntimeError, match="no recommend"):
        lord.recommendItemsForUsers([0])
    lord.destroy()
    with pytest.raises(RuntimeError, match="prepareToTrain"):
        EmfLord(options={"dataDir": str(tmp_path)}).recommendItemsForUsers([0])
