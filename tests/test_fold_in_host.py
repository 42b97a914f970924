"""Fold-in on the CPU: the new C entry points are exported and bound, and the host logic of EmfLord.recommendItemsForRatings /
EmfLord.foldIn -- 1-based ids, skip lists, defaults, refusals -- runs over a test-only backend that answers fold_in and
recommend_for_ratings from the oracle and numpy.  The package itself has no CPU path."""
import ctypes as C

import numpy as np
import pytest

import ycnr_als
from helpers import OracleBackend, make_problem, numpy_row_solve
from oracle import oracle as orc
from ycnr_als import _lib
from ycnr_als.emf import Dataset, EmfLord

USERS, ITEMS, K = 30, 40, 6


def test_symbols_are_exported_and_bound():
    L = _lib.load()
    assert "ycnr_als_fold_in" in _lib.EXPORTS and "ycnr_als_recommend_for_ratings" in _lib.EXPORTS
    assert len(L.ycnr_als_fold_in.argtypes) == 10 and len(L.ycnr_als_recommend_for_ratings.argtypes) == 16
    assert L.ycnr_version() == 4  # additions only
    for name in ("fold_in", "recommend_for_ratings"):
        assert callable(getattr(ycnr_als.AlsDevice, name)) and callable(getattr(ycnr_als.emf.HipBackend, name))
    # a null handle is refused before anything else is looked at
    assert L.ycnr_als_fold_in(None, 0, 1, None, None, None, None, None, None, None) == _lib.ERR_INVALID
    assert L.ycnr_als_recommend_for_ratings(None, 1, None, None, None, None, None, 0.0, 0.0, 5, None, None, None, None, None, None) == _lib.ERR_INVALID


def test_no_device_no_fold_in():
    """Without a GPU there is no handle to fold into: creating one fails with YCNR_ERR_HIP, nothing is computed on the host."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present: covered by the -m gpu suite")
    with pytest.raises(ycnr_als.YcnrError) as e:
        ycnr_als.AlsDevice(8, 4, 4).fold_in("byUser", [0, 1], [0], [1.0])
    assert e.value.code == _lib.ERR_HIP


class FoldingOracle(OracleBackend):
    """fold_in: float64 LAPACK per row; recommend_for_ratings: that + the oracle's restatement of the reference loop"""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.folds, self.requests = [], []

    def fold_in(self, side, row_ptr, indx, vals, store_ids=None):
        self.folds.append((side, np.array(row_ptr), np.array(indx), np.array(vals), None if store_ids is None else np.array(store_ids)))
        n = len(row_ptr) - 1
        rows, status = np.zeros((n, self.k)), np.zeros(n, np.int32)
        for r in range(n):
            b, e = row_ptr[r], row_ptr[r + 1]
            if e == b:
                status[r] = 2
                continue
            rows[r] = numpy_row_solve(self.lam[side], self.k, indx[b:e], np.asarray(vals[b:e]), self.fac_np[1 - side])[0]
            if store_ids is not None:
                self.fac_np[side][store_ids[r]] = rows[r]
        return rows, status

    def recommend_for_ratings(self, rat_ptr, rat_ids, rat_vals, skip_ptr, skip_ids, shift, min_rating, limit):
        self.requests.append((np.array(rat_ptr), np.array(rat_ids), np.array(rat_vals), np.array(skip_ptr), np.array(skip_ids), shift, min_rating, limit))
        rows, status = self.fold_in(0, rat_ptr, rat_ids, rat_vals)
        self.folds.pop()
        n = len(rat_ptr) - 1
        ids, pred, cnt = np.full((n, limit), -1, np.int32), np.zeros((n, limit)), np.zeros(n, np.int32)
        for i in range(n):
            if status[i]:
                continue
            oid, opr = orc.recommend(rows[i], self.fac_np[1], skip_ids[skip_ptr[i]:skip_ptr[i + 1]], shift, min_rating, limit)
            cnt[i] = len(oid)
            ids[i, :len(oid)], pred[i, :len(oid)] = oid, opr
        return ids, pred, cnt, rows, status


def lord_with(backend_cls, tmp_path):
    bu, bi, U, V = make_problem(USERS, ITEMS, K, density=0.3, seed=2, min_per_row=2, dtype=np.float64)
    lord = EmfLord(options={"factorsCount": K, "trainIters": 1, "useDoublePrecision": True, "dataDir": str(tmp_path),
                            "numThreadsForTrain": {"als": 1}, "numThreadsForRmse": 1},
                   backend_factory=lambda o, u, i, d: backend_cls(o, u, i, d))
    lord.prepareToTrain(Dataset(bu, bi), U, V)
    return lord, U, V


def test_recommend_items_for_ratings(tmp_path):
    lord, U, V = lord_with(FoldingOracle, tmp_path)
    lord.globalAvgShift = 0.25
    ratings = [[(3, 4.0), (17, 2.0), (40, 5.0)], [], [(1, 1.0)]]  # 1-based item ids; a user without ratings
    unrated = [[5, 5, 2, 39], None, [0]]  # 0-based; 2 = item id 3, rated anyway; duplicates
    recs = lord.recommendItemsForRatings(ratings, limit=5, minRecommendRating=-100.0, unratedItems=unrated)
    rp, ri, rv, sp, sk, shift, thr, limit = lord.backend.requests[-1]
    assert rp.tolist() == [0, 3, 3, 4] and ri.tolist() == [2, 16, 39, 0] and rv.tolist() == [4.0, 2.0, 5.0, 1.0]  # 0-based on the device
    assert ri.dtype == np.int32 and sk.dtype == np.int32 and shift == 0.25 and thr == -100.0 and limit == 5
    assert sp.tolist() == [0, 4, 4, 5]  # skip list = rated | unratedItems, sorted, unique
    assert sk[sp[0]:sp[1]].tolist() == [2, 5, 16, 39] and sk[sp[1]:sp[2]].tolist() == [] and sk[sp[2]:sp[3]].tolist() == [0]
    # the return shape of recommendItemsForUsers: per user a list of {id (1-based), predict}, at most limit - 1, best first
    assert len(recs) == 3 and recs[1] == []
    lam = lord.options["als"]["userFactReg"]
    x = numpy_row_solve(lam, K, np.array([2, 16, 39]), np.array([4.0, 2.0, 5.0]), V)[0]
    oid, opr = orc.recommend(x, V, np.array([2, 5, 16, 39], np.int32), 0.25, -100.0, 5)
    assert len(recs[0]) == 4 == len(oid)
    assert [r["id"] for r in recs[0]] == (oid + 1).tolist() and [r["predict"] for r in recs[0]] == opr.tolist()
    assert not {r["id"] - 1 for r in recs[0]} & {2, 5, 16, 39}
    # defaults: the reference's threshold getter (3.5 for 'ml') and limit 20, the Lord's shift
    lord.recommendItemsForRatings([[(1, 5.0)]])
    assert lord.backend.requests[-1][6] == 3.5 and lord.backend.requests[-1][7] == 20 and lord.backend.requests[-1][5] == 0.25
    assert lord.recommendItemsForRatings([]) == []
    with pytest.raises(ValueError):
        lord.recommendItemsForRatings([[(ITEMS + 1, 3.0)]])
    with pytest.raises(ValueError):
        lord.recommendItemsForRatings([[(0, 3.0)]])
    with pytest.raises(ValueError):
        lord.recommendItemsForRatings([[(1, 3.0)], []], unratedItems=[[1]])
    # the user side needs only the item matrix: allowed where the user matrix is not replicated
    lord.bands, lord.world = np.array([0, USERS], np.int64), 2
    assert len(lord.recommendItemsForRatings([[(1, 5.0)]], minRecommendRating=-100.0)) == 1
    lord.destroy()


def test_fold_in(tmp_path):
    lord, U, V = lord_with(FoldingOracle, tmp_path)
    rows, status = lord.foldIn("byUser", [[(3, 4.0), (17, 2.0)], []])
    side, rp, ri, rv, st = lord.backend.folds[-1]
    assert side == 0 and rp.tolist() == [0, 2, 2] and ri.tolist() == [2, 16] and rv.tolist() == [4.0, 2.0] and st is None
    assert rows.shape == (2, K) and status.tolist() == [0, 2]
    assert np.array_equal(rows[0], numpy_row_solve(lord.options["als"]["userFactReg"], K, np.array([2, 16]), np.array([4.0, 2.0]), V)[0])
    # a new item, stored: ids of the rows are USER ids here, the store ids 0-based rows of the item matrix
    rows, status = lord.foldIn("byItem", [[(1, 5.0), (USERS, 1.0)]], storeIds=[7])
    side, rp, ri, rv, st = lord.backend.folds[-1]
    assert side == 1 and ri.tolist() == [0, USERS - 1] and st.tolist() == [7] and st.dtype == np.int32
    assert np.array_equal(lord.backend.fac_np[1][7], rows[0])
    with pytest.raises(ValueError):
        lord.foldIn("byItem", [[(USERS + 1, 5.0)]])
    with pytest.raises(ValueError):
        lord.foldIn("byRow", [[(1, 5.0)]])
    # bands on several ranks: the user matrix is not replicated, so no item can be folded in; users can
    lord.bands, lord.world = np.array([0, USERS], np.int64), 2
    n = len(lord.backend.folds)
    with pytest.raises(RuntimeError, match="itemStepSharding"):
        lord.foldIn("byItem", [[(1, 5.0)]])
    assert len(lord.backend.folds) == n
    assert lord.foldIn("byUser", [[(1, 5.0)]])[1].tolist() == [0]
    lord.destroy()


def test_refusals(tmp_path):
    lord, _, _ = lord_with(OracleBackend, tmp_path)
    with pytest.raises(RuntimeError, match="no recommend_for_ratings"):
        lord.recommendItemsForRatings([[(1, 5.0)]])
    with pytest.raises(RuntimeError, match="no fold_in"):
        lord.foldIn("byUser", [[(1, 5.0)]])
    lord.destroy()
    fresh = EmfLord(options={"dataDir": str(tmp_path)})
    with pytest.raises(RuntimeError, match="prepareToTrain"):
        fresh.recommendItemsForRatings([[(1, 5.0)]])
    with pytest.raises(RuntimeError, match="prepareToTrain"):
        fresh.foldIn("byUser", [[(1, 5.0)]])
