"""ycnr_als_fold_in / ycnr_als_recommend_for_ratings: factor rows solved from ratings that arrive in the call, against the
fixed matrix a resident handle holds, and the top-N of such rows.

Up to 128 factors the kernel works in float64 whatever the handle's dtype, so the reference is helpers.numpy_row_solve
(float64 LAPACK on the handle's own inputs) with the project's bound form, 8 amp eps64; a float32 handle adds the one rounding
of the store: at most half an ulp per element = EPS32 / 2 row-relative, allowed as EPS32 (a factor of 2).
"""
import ctypes as C

import numpy as np
import pytest

from helpers import EPS32, make_problem, numpy_row_solve, row_rel_err

pytestmark = pytest.mark.gpu

EPS64 = float(np.finfo(np.float64).eps)
LAM = (0.05, 0.07)  # userFactReg, itemFactReg: different, so that a test sees which one a side uses


@pytest.fixture(scope="module")
def als():
    import ycnr_als
    L = ycnr_als._lib.load()  # raises if libycnr_als.so is missing: no fallback
    assert L.ycnr_device_count() >= 1, L.ycnr_last_error()
    return ycnr_als


def factors(rng, rows, k, dt):
    return (rng.standard_normal((rows, k)) / np.sqrt(k)).astype(dt)  # the pattern of helpers.make_problem


def make_request(rng, counts, fixed_rows, dt):
    """CSR relative to the request: row r has counts[r] distinct column ids, ratings 1..5"""
    ptr = np.zeros(len(counts) + 1, np.int64)
    ptr[1:] = np.cumsum(counts)
    idx = np.concatenate([rng.choice(fixed_rows, c, replace=False) for c in counts] + [np.zeros(0, np.int64)]).astype(np.int32)
    vals = rng.integers(1, 6, int(ptr[-1])).astype(dt)
    return ptr, idx, vals


def device(als, k, dt, side, fixed, solved_rows=8, solved=None):
    """a handle whose FIXED side (the opposite of `side`) holds `fixed`"""
    n = [0, 0]
    n[1 - side], n[side] = fixed.shape[0], solved_rows
    dev = als.AlsDevice(k, n[0], n[1], useDoublePrecision=(dt == np.float64), userFactReg=LAM[0], itemFactReg=LAM[1])
    dev.set_factors(1 - side, fixed)
    dev.set_factors(side, np.zeros((solved_rows, k), dt) if solved is None else solved)
    return dev


def reference(side, k, ptr, idx, vals, fixed):
    want = np.zeros((len(ptr) - 1, k))
    amp = np.ones(len(ptr) - 1)
    for r in range(len(ptr) - 1):
        if ptr[r + 1] > ptr[r]:
            want[r], amp[r] = numpy_row_solve(LAM[side], k, idx[ptr[r]:ptr[r + 1]], vals[ptr[r]:ptr[r + 1]], fixed)
    return want, amp


def bound(amp, dt):
    return 8 * amp * EPS64 + (EPS32 if dt == np.float32 else 0.0)


def check_rows(rows, status, side, k, ptr, idx, vals, fixed, dt, what):
    want, amp = reference(side, k, ptr, idx, vals, fixed)
    live = np.diff(ptr) > 0
    assert np.array_equal(status, np.where(live, 0, 2)), status
    assert not rows[~live].any()
    err = row_rel_err(rows[live], want[live])
    tol = bound(amp[live], dt)
    print(f"{what}: max err {err.max():.3e}, max err / bound {np.max(err / tol):.3f}, max amp {amp.max():.3e}")
    assert (err <= tol).all(), (err.max(), np.max(err / tol))


@pytest.mark.parametrize("side", [0, 1])
@pytest.mark.parametrize("k", [7, 20, 100, 128])
@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_parity_numpy(als, dt, k, side):
    rng = np.random.default_rng(1000 + k + side)
    fixed = factors(rng, 400, k, dt)
    counts = [1, 2, 3, 15, 16, 17, 0, 31, 32, 33, k - 1, k, k + 1, 300]  # the empty row in the middle
    ptr, idx, vals = make_request(rng, counts, 400, dt)
    dev = device(als, k, dt, side, fixed)
    try:
        rows, status, ms = dev.fold_in(side, ptr, idx, vals)
        assert rows.dtype == dt and rows.shape == (len(counts), k) and ms >= 0
        check_rows(rows, status, side, k, ptr, idx, vals, fixed, dt, f"parity {np.dtype(dt).name} k={k} side={side}")
    finally:
        dev.destroy()


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_one_long_row(als, dt):
    k = 100
    rng = np.random.default_rng(7)
    fixed = factors(rng, 6000, k, dt)
    ptr, idx, vals = make_request(rng, [5000], 6000, dt)
    dev = device(als, k, dt, 0, fixed)
    try:
        rows, status, _ = dev.fold_in("byUser", ptr, idx, vals)
        check_rows(rows, status, 0, k, ptr, idx, vals, fixed, dt, f"long row {np.dtype(dt).name}")
    finally:
        dev.destroy()


def sub_request(ptr, idx, vals, order):
    counts = [int(ptr[r + 1] - ptr[r]) for r in order]
    p = np.zeros(len(order) + 1, np.int64)
    p[1:] = np.cumsum(counts)
    i = np.concatenate([idx[ptr[r]:ptr[r + 1]] for r in order] + [idx[:0]])
    v = np.concatenate([vals[ptr[r]:ptr[r + 1]] for r in order] + [vals[:0]])
    return p, i, v


@pytest.mark.parametrize("dt,k", [(np.float32, 100), (np.float64, 20)])
def test_row_does_not_depend_on_the_batch(als, dt, k):
    rng = np.random.default_rng(11)
    fixed = factors(rng, 500, k, dt)
    counts = list(rng.integers(0, 200, 257))
    counts[0], counts[100], counts[256] = 1, 333, 17
    ptr, idx, vals = make_request(rng, counts, 500, dt)
    dev = device(als, k, dt, 0, fixed)
    try:
        whole, st, _ = dev.fold_in(0, ptr, idx, vals)
        order = list(range(257))[::-1]
        rev, strev, _ = dev.fold_in(0, *sub_request(ptr, idx, vals, order))
        assert np.array_equal(rev[::-1], whole) and np.array_equal(strev[::-1], st)
        for r in (0, 100, 128, 255, 256):
            alone, sta, _ = dev.fold_in(0, *sub_request(ptr, idx, vals, [r]))
            assert np.array_equal(alone[0], whole[r]) and sta[0] == st[r], r
    finally:
        dev.destroy()


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_agrees_with_training(als, dt):
    k, users, items = 20, 300, 200
    bu, _, U, V = make_problem(users, items, k, density=0.1, seed=5, dtype=dt, empty_rows=(17,))
    dev = als.AlsDevice(k, users, items, useDoublePrecision=(dt == np.float64), userFactReg=LAM[0], itemFactReg=LAM[1])
    try:
        dev.set_factors("byUser", U)
        dev.set_factors("byItem", V)
        dev.set_ratings("byUser", bu.rowPtr, bu.indx, bu.vals)
        dev.step("byUser")
        trained = dev.get_factors("byUser")
        rows, status, _ = dev.fold_in("byUser", bu.rowPtr, bu.indx, bu.vals)
        assert np.array_equal(dev.get_factors("byUser"), trained)  # storeIds=None: nothing is written
        live = np.diff(bu.rowPtr) > 0
        assert status[17] == 2 and np.array_equal(status, np.where(live, 0, 2))
        _, amp = reference(0, k, bu.rowPtr, bu.indx, bu.vals, V)
        err = row_rel_err(rows[live], trained[live])
        tol = 8 * amp[live] * float(np.finfo(dt).eps)  # the trainer works in the handle's precision
        print(f"training {np.dtype(dt).name}: max err {err.max():.3e}, max err / bound {np.max(err / tol):.3f}")
        assert (err <= tol).all()
    finally:
        dev.destroy()


@pytest.mark.parametrize("dt,k", [(np.float32, 160), (np.float32, 130), (np.float64, 136)])
def test_more_than_128_factors(als, dt, k):
    rng = np.random.default_rng(k)
    fixed = factors(rng, 500, k, dt)
    ptr, idx, vals = make_request(rng, [1, 50, 0, 200, 400], 500, dt)
    dev = device(als, k, dt, 0, fixed)
    try:
        rows, status, _ = dev.fold_in(0, ptr, idx, vals)
        want, amp = reference(0, k, ptr, idx, vals, fixed)
        live = np.diff(ptr) > 0
        assert np.array_equal(status, np.where(live, 0, 2)) and not rows[~live].any()
        err = row_rel_err(rows[live], want[live])
        tol = 8 * amp[live] * EPS32 if dt == np.float32 else np.full(live.sum(), 1e-5)
        print(f"k={k} {np.dtype(dt).name}: max err {err.max():.3e}, max err / bound {np.max(err / tol):.3f}")
        assert (err <= tol).all()
        # stored where asked, rows without ratings left alone
        rows2, status2, _ = dev.fold_in(0, ptr, idx, vals, storeIds=[4, 0, 7, 2, 5])
        assert np.array_equal(rows2, rows) and np.array_equal(status2, status)
        m = dev.get_factors(0)
        assert np.array_equal(m[[4, 0, 2, 5]], rows[[0, 1, 3, 4]]) and not m[[1, 3, 6, 7]].any()
    finally:
        dev.destroy()


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_status_of_a_nan_row(als, dt):
    k = 20
    rng = np.random.default_rng(3)
    fixed = factors(rng, 100, k, dt)
    counts = [5, 40, 0, 17, 64, 1, 33]
    ptr, idx, vals = make_request(rng, counts, 100, dt)
    poison = int(idx[ptr[1] + 3])  # an id row 1 refers to
    old = rng.standard_normal((8, k)).astype(dt)
    dev = device(als, k, dt, 0, fixed, solved=old)
    try:
        clean, st0, _ = dev.fold_in(0, ptr, idx, vals)
        bad = fixed.copy()
        bad[poison] = np.nan
        dev.set_factors(1, bad)
        rows, status, _ = dev.fold_in(0, ptr, idx, vals, storeIds=np.arange(len(counts)))
        hit = np.array([poison in idx[ptr[r]:ptr[r + 1]] for r in range(len(counts))])
        assert hit[1] and not hit.all()
        assert np.array_equal(status, np.where(hit, 1, st0)), status
        assert not rows[hit].any()
        assert np.array_equal(rows[~hit], clean[~hit])
        # rows with status 1 / 2 are not stored
        want = old.copy()
        ok = status == 0
        want[np.arange(len(counts))[ok]] = rows[ok]
        assert np.array_equal(dev.get_factors(0), want)
    finally:
        dev.destroy()


@pytest.mark.parametrize("side", [0, 1])
@pytest.mark.parametrize("dt,k", [(np.float32, 100), (np.float32, 7), (np.float64, 20)])
def test_store_ids(als, dt, k, side):
    rng = np.random.default_rng(21 + side)
    fixed = factors(rng, 300, k, dt)
    old = rng.standard_normal((50, k)).astype(dt)
    counts = [3, 0, 120, 16, 80]
    ptr, idx, vals = make_request(rng, counts, 300, dt)
    dev = device(als, k, dt, side, fixed, solved_rows=50, solved=old)
    try:
        store = np.array([49, 7, 0, 23, 8], np.int32)
        rows, status, _ = dev.fold_in(side, ptr, idx, vals, storeIds=store)
        assert list(status) == [0, 2, 0, 0, 0]
        want = old.copy()
        want[store[status == 0]] = rows[status == 0]
        assert np.array_equal(dev.get_factors(side), want)
        assert np.array_equal(dev.get_factors(1 - side), fixed)
        plain, _, _ = dev.fold_in(side, ptr, idx, vals)
        assert np.array_equal(plain, rows)
    finally:
        dev.destroy()


def test_runs_behind_a_half_step_in_flight(als):
    k, users, items = 100, 3000, 2000
    bu, bi, U, V = make_problem(users, items, k, density=0.05, seed=9)
    rng = np.random.default_rng(9)
    ptr, idx, vals = make_request(rng, [40, 3, 200, 64], items, np.float32)
    got = []
    for wait in (False, True):
        dev = als.AlsDevice(k, users, items)
        try:
            dev.set_factors("byUser", U)
            dev.set_factors("byItem", V)
            dev.set_ratings("byItem", bi.rowPtr, bi.indx, bi.vals)
            dev.step_async("byItem")  # rewrites the item matrix the fold-in reads
            if wait:
                dev.sync()
            got.append(dev.fold_in("byUser", ptr, idx, vals)[0])
            dev.sync()
            assert not np.array_equal(dev.get_factors("byItem"), V)
        finally:
            dev.destroy()
    assert np.array_equal(got[0], got[1])


def test_invalid_arguments(als):
    k, dt = 20, np.float32
    rng = np.random.default_rng(2)
    fixed = factors(rng, 60, k, dt)
    old = rng.standard_normal((9, k)).astype(dt)
    dev = device(als, k, dt, 0, fixed, solved_rows=9, solved=old)
    L, INV = dev._L, als._lib.ERR_INVALID
    ptr, idx, vals = make_request(rng, [4, 0, 9], 60, dt)
    rows = np.full((3, k), 77, dt)
    status = np.full(3, 77, np.int32)
    ms = C.c_double(-1.0)
    good = dict(rowPtr=ptr, indx=idx, vals=vals, storeIds=None, outRows=rows, outStatus=status)

    def call(**kw):
        a = dict(good, **kw)
        p = lambda x: None if x is None else x.ctypes.data  # noqa: E731
        return L.ycnr_als_fold_in(dev._h, 0, 3, p(a["rowPtr"]), p(a["indx"]), p(a["vals"]), p(a["storeIds"]), p(a["outRows"]),
                                  p(a["outStatus"]), C.byref(ms))

    def bumped(a, pos, v):
        b = a.copy()
        b[pos] = v
        return b

    try:
        cases = {
            "null rowPtr": dict(rowPtr=None), "null indx": dict(indx=None), "null vals": dict(vals=None),
            "null outRows": dict(outRows=None), "null outStatus": dict(outStatus=None),
            "rowPtr[0] != 0": dict(rowPtr=ptr + 1), "negative rowPtr": dict(rowPtr=bumped(ptr, 0, -1)),
            "decreasing rowPtr": dict(rowPtr=np.array([0, 4, 3, 13], np.int64)),
            "column id too large": dict(indx=bumped(idx, 5, 60)), "negative column id": dict(indx=bumped(idx, 0, -1)),
            "store id too large": dict(storeIds=np.array([0, 1, 9], np.int32)), "negative store id": dict(storeIds=np.array([-1, 1, 2], np.int32)),
            "repeated store id": dict(storeIds=np.array([2, 1, 2], np.int32)),
        }
        for name, kw in cases.items():
            assert call(**kw) == INV, name
            assert L.ycnr_last_error(), name
        assert L.ycnr_als_fold_in(dev._h, 2, 3, ptr.ctypes.data, idx.ctypes.data, vals.ctypes.data, None, rows.ctypes.data, status.ctypes.data, None) == INV
        assert L.ycnr_als_fold_in(dev._h, 0, -1, ptr.ctypes.data, idx.ctypes.data, vals.ctypes.data, None, rows.ctypes.data, status.ctypes.data, None) == INV
        # recommend_for_ratings: the same request checks, and those of ycnr_als_recommend
        ids = np.full((3, 5), 77, np.int32)
        pred = np.full((3, 5), 77.0)
        cnt = np.full(3, 77, np.int32)
        sp = np.zeros(4, np.int64)

        def rcall(rp=ptr, ix=idx, sptr=sp, limit=5, oi=ids):
            return L.ycnr_als_recommend_for_ratings(dev._h, 3, rp.ctypes.data, ix.ctypes.data, vals.ctypes.data, None if sptr is None else sptr.ctypes.data,
                                                    None, 0.0, 0.0, limit, None if oi is None else oi.ctypes.data, pred.ctypes.data, cnt.ctypes.data,
                                                    rows.ctypes.data, status.ctypes.data, None)
        assert rcall(rp=np.array([0, 4, 3, 13], np.int64)) == INV
        assert rcall(ix=bumped(idx, 2, 60)) == INV
        assert rcall(sptr=None) == INV and rcall(oi=None) == INV and rcall(limit=0) == INV and rcall(limit=4097) == INV
        assert rcall(sptr=np.array([0, 2, 2, 2], np.int64)) == INV  # skips without skipIds
        # nothing was touched
        assert (rows == 77).all() and (status == 77).all() and (ids == 77).all() and (pred == 77).all() and (cnt == 77).all()
        assert np.array_equal(dev.get_factors(0), old) and np.array_equal(dev.get_factors(1), fixed)
        # nRows == 0 is fine, and the good request still works
        assert L.ycnr_als_fold_in(dev._h, 0, 0, None, None, None, None, None, None, None) == 0
        assert call() == 0 and list(status) == [0, 2, 0] and ms.value >= 0
    finally:
        dev.destroy()


@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("users,items,k", [(40, 1234, 100), (3, 50, 8)])
def test_recommend_for_ratings(als, users, items, k, dt):
    rng = np.random.default_rng(100 + k)
    V = (rng.standard_normal((items, k)) * 0.8).astype(dt)
    counts = list(rng.integers(1, min(items, 150), users))
    counts[1] = 0  # a user without ratings
    ptr, idx, vals = make_request(rng, counts, items, dt)
    # skip list = the rated items (ascending, as the Lord builds it)
    sk = np.concatenate([np.sort(idx[ptr[u]:ptr[u + 1]]) for u in range(users)]).astype(np.int32)
    dev = device(als, k, dt, 0, V)
    try:
        rows, status, _ = dev.fold_in(0, ptr, idx, vals)
        assert status[1] == 2 and (np.delete(status, 1) == 0).all()
        several = False
        for limit in (1, 2, 20, 64, 65):
            ids, pred, cnt, rows2, status2, ms = dev.recommend_for_ratings(ptr, idx, vals, ptr, sk, globalAvgShift=0.2, minRecommendRating=0.5, limit=limit)
            assert np.array_equal(rows2, rows) and np.array_equal(status2, status) and ms >= 0
            want = als.recommend_items(rows2, V, ptr, sk, globalAvgShift=0.2, minRecommendRating=0.5, limit=limit)
            # (the zero row of the user without ratings predicts the shift everywhere, below the threshold: count 0 both ways)
            for g, w, name in zip((ids, pred, cnt), want[:3], ("ids", "predicts", "counts")):
                assert g.shape == w.shape and np.array_equal(g, w), (name, limit)
            assert cnt[1] == 0 and (ids[1] == -1).all()
            several = several or cnt.max() > 1
        assert several  # not vacuous
        # a threshold the shift alone passes: the user without ratings still gets nothing
        ids, pred, cnt, _, _, _ = dev.recommend_for_ratings(ptr, idx, vals, ptr, sk, globalAvgShift=0.2, minRecommendRating=0.1, limit=20)
        assert cnt[1] == 0 and (ids[1] == -1).all() and not pred[1].any() and cnt[0] > 0
    finally:
        dev.destroy()
