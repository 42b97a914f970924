"""ycnr_als_fold_in_implicit / ycnr_als_recommend_for_observations (csrc/foldin_implicit_kernels.hip.h): rows of the implicit
model solved from observations given in the call, in dual form (n <= 32) and by the exact k x k solve, against a plain float64
numpy solve of the primal formula (the reference() of tests/test_gpu_implicit.py, restated) with that file's bounds: 8 amp eps64
for float64 handles, max(8 amp EPS32, 1e-6) for float32.  Observed worst err / bound: DESIGN.md 16."""
import functools

import numpy as np
import pytest

import ycnr_als
from helpers import EPS32, row_rel_err
from ycnr_als import _lib

pytestmark = pytest.mark.gpu

EPS64 = float(np.finfo(np.float64).eps)
LAM = (0.05, 0.07)  # user, item: different, so that a test sees which one a side uses
FIXED, SOLVED = 2069, 16  # two Gramian slices, the second ending on a partial panel; the request has 15 rows, row 15 is never touched


def reference(alpha, lam, idx, r, Y):
    """x and amp = cond(A) max(1, || |Y|^T c || / ||b||) of one row, float64"""
    Y = Y.astype(np.float64)
    Ys, r = Y[idx], r.astype(np.float64)
    c = 1.0 + alpha * r
    A = Y.T @ Y + (Ys.T * (alpha * r)) @ Ys + lam * np.eye(Y.shape[1])
    b = Ys.T @ c
    amp = np.linalg.cond(A) * max(1.0, np.linalg.norm(np.abs(Ys).T @ c) / max(np.linalg.norm(b), 1e-300))
    return np.linalg.solve(A, b), amp


@functools.lru_cache(maxsize=None)
def problem(k, alpha, side):
    """float32 inputs (a float64 handle gets them widened, so both share this reference): the request, the fixed matrix, the
    start of the solved one, want / amp per row.  Row 3 (dual) has a zero value; the last row has a negative one: primal."""
    rng = np.random.default_rng(2000 * k + side)
    counts = [0, 1, 2, 15, 16, 17, 31, 32, 33, k - 1, k, k + 1, 64, 300, 5]
    ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    idx = np.concatenate([np.sort(rng.choice(FIXED, n, replace=False)) for n in counts]).astype(np.int32)
    vals = rng.integers(1, 6, len(idx)).astype(np.float32)
    vals[ptr[3] + 7] = 0.0
    vals[ptr[14] + 2] = -0.25  # G's smallest eigenvalue is about FIXED / k >= 16: A stays definite
    Y = (rng.standard_normal((FIXED, k)) / np.sqrt(k)).astype(np.float32)
    X0 = (rng.standard_normal((SOLVED, k)) / np.sqrt(k)).astype(np.float32)
    want, amp = np.zeros((len(counts), k)), np.ones(len(counts))
    for u in range(1, len(counts)):
        want[u], amp[u] = reference(alpha, LAM[side], idx[ptr[u]:ptr[u + 1]], vals[ptr[u]:ptr[u + 1]], Y)
    return ptr, idx, vals, Y, X0, want, amp


def device(dt, k, side, Y, X0):
    rows = (SOLVED, FIXED) if side == 0 else (FIXED, SOLVED)
    dev = ycnr_als.AlsDevice(k, rows[0], rows[1], useDoublePrecision=dt == np.float64, userFactReg=LAM[0], itemFactReg=LAM[1])
    dev.set_factors(1 - side, Y.astype(dt))
    dev.set_factors(side, X0.astype(dt))
    return dev


def bound(amp, dt):
    return 8 * amp * EPS64 if dt == np.float64 else np.maximum(8 * amp * EPS32, 1e-6)


def check(dt, k, alpha, side):
    ptr, idx, vals, Y, X0, want, amp = problem(k, alpha, side)
    dev = device(dt, k, side, Y, X0)
    for primal_only in (False, True):
        rows, status, ms = dev.fold_in_implicit(side, alpha, ptr, idx, vals.astype(dt), primal_only=primal_only)
        assert rows.dtype == dt and len(ms) == 3 and ms[2] > 0
        assert list(status) == [2] + [0] * 14 and not rows[0].any()
        err, tol = row_rel_err(rows[1:], want[1:]), bound(amp[1:], dt)
        print(f"fold-in implicit {np.dtype(dt).name} k={k} alpha={alpha} side={side} primal_only={primal_only}: "
              f"max err {err.max():.3e}, worst err / bound {np.max(err / tol):.3f}")
        assert (err <= tol).all(), float(np.max(err / tol))
    assert np.array_equal(dev.get_factors(side), X0.astype(dt))  # storeIds=None: nothing is written
    dev.destroy()


@pytest.mark.parametrize("side", [0, 1])
@pytest.mark.parametrize("k", [7, 20, 100, 128])
@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_parity_with_float64_numpy(dt, k, side):
    check(dt, k, 0.5, side)


@pytest.mark.parametrize("alpha", [0.0, 40.0])
def test_alpha_cases(alpha):
    check(np.float32, 20, alpha, 0)


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_agrees_with_training_and_stores_where_asked(dt):
    k, alpha, side = 20, 0.5, 1
    ptr, idx, vals, Y, X0, _, amp = problem(k, alpha, side)
    dev = device(dt, k, side, Y, X0)
    dev.set_ratings(side, np.append(ptr, ptr[-1]), idx, vals.astype(dt))  # 16 rows: the request's and an empty one
    assert dev.step_implicit(side, alpha)[0] == 0
    trained = dev.get_factors(side)
    dev.set_factors(side, X0.astype(dt))
    store = np.arange(15, dtype=np.int32)[::-1].copy()  # request row r -> row 14 - r
    rows, status, _ = dev.fold_in_implicit(side, alpha, ptr, idx, vals.astype(dt), storeIds=store)
    err, tol = row_rel_err(rows[1:], trained[1:15]), 2 * bound(amp[1:], dt)  # the sum of both bounds
    print(f"training {np.dtype(dt).name}: worst err / bound {np.max(err / tol):.3f}")
    assert list(status) == [2] + [0] * 14 and (err <= tol).all()
    want = X0.astype(dt)
    want[store[1:]] = rows[1:]  # the empty row's target (14) and row 15 keep what they held
    assert np.array_equal(dev.get_factors(side), want)
    dev.destroy()


def reverse(ptr, idx, vals):
    order = range(len(ptr) - 2, -1, -1)
    p = np.concatenate([[0], np.cumsum([ptr[r + 1] - ptr[r] for r in order])]).astype(np.int64)
    return p, np.concatenate([idx[ptr[r]:ptr[r + 1]] for r in order]), np.concatenate([vals[ptr[r]:ptr[r + 1]] for r in order])


@pytest.mark.parametrize("primal_only", [False, True])
def test_bits_do_not_depend_on_the_company(primal_only):
    ptr, idx, vals, Y, X0, _, _ = problem(100, 0.5, 0)
    dev = device(np.float32, 100, 0, Y, X0)
    rows, status, _ = dev.fold_in_implicit(0, 0.5, ptr, idx, vals, primal_only=primal_only)
    rev, strev, _ = dev.fold_in_implicit(0, 0.5, *reverse(ptr, idx, vals), primal_only=primal_only)
    assert np.array_equal(rev[::-1], rows) and np.array_equal(strev[::-1], status) and rows[1:].all(axis=1).any()
    dev.destroy()


def test_recommend_for_observations_is_fold_in_then_recommend():
    ptr, idx, vals, Y, X0, _, _ = problem(20, 0.5, 0)
    dev = device(np.float32, 20, 0, Y, X0)
    args = dict(globalAvgShift=0.1, minRecommendRating=-1e30, limit=10)
    rows, status, _ = dev.fold_in_implicit(0, 0.5, ptr, idx, vals, storeIds=np.arange(15, dtype=np.int32))
    want = dev.recommend(np.arange(15), ptr, idx, **args)  # skip list: the observed items (ascending per user)
    ids, pred, cnt, rows2, status2, ms = dev.recommend_for_observations(0.5, ptr, idx, vals, ptr, idx, **args)
    assert np.array_equal(rows2, rows) and np.array_equal(status2, status) and status[0] == 2 and ms >= 0
    assert cnt[0] == 0 and (ids[0] == -1).all() and (cnt[1:] == 9).all()
    assert np.array_equal(ids[1:], want[0][1:]) and np.array_equal(pred[1:], want[1][1:]) and np.array_equal(cnt[1:], want[2][1:])
    dev.destroy()


@pytest.mark.parametrize("k,kw,code", [(129, {}, _lib.ERR_UNSUPPORTED), (20, dict(alpha=-1.0), _lib.ERR_INVALID),
                                       (20, dict(alpha=float("nan")), _lib.ERR_INVALID), (20, dict(bad_column=True), _lib.ERR_INVALID),
                                       (20, dict(store=[3] * 15), _lib.ERR_INVALID), (20, dict(flags=2), _lib.ERR_INVALID)])
def test_refusals_leave_outputs_and_matrices_alone(k, kw, code):
    ptr, idx, vals, Y, X0, _, _ = problem(k, 0.5, 0)
    dev = device(np.float32, k, 0, Y, X0)
    if kw.get("bad_column"):
        idx = idx.copy()
        idx[5] = FIXED
    store = None if "store" not in kw else np.array(kw["store"], np.int32)
    rows, status = np.full((15, k), 77, np.float32), np.full(15, 77, np.int32)
    rc = dev._L.ycnr_als_fold_in_implicit(dev._h, 0, kw.get("alpha", 0.5), 15, ptr.ctypes.data, idx.ctypes.data, vals.ctypes.data,
                                          None if store is None else store.ctypes.data, kw.get("flags", 0), rows.ctypes.data,
                                          status.ctypes.data, None)
    assert rc == code
    assert (rows == 77).all() and (status == 77).all()
    assert np.array_equal(dev.get_factors(0), X0) and np.array_equal(dev.get_factors(1), Y)
    dev.destroy()
