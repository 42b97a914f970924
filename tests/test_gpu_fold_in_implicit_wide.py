"""ycnr_als_fold_in_implicit_wide (csrc/foldin_wide_kernels.hip.h): rows of the implicit model for up to 512 factors, every
served row (1 .. 128 non-negative observations) in dual form, against the plain float64 numpy solve of the primal formula and the
bounds of tests/test_gpu_fold_in_implicit.py: 8 amp eps64 for float64 handles, max(8 amp EPS32, 1e-6) for float32.  The row
lengths are the kernel's edges: one observation, both sides of a 16-group, of the launch classes' boundary (32 / 33), of the last
full tile count (127 / 128) and the first unserved length.  Observed worst err / bound: DESIGN.md 16."""
import functools

import numpy as np
import pytest

from helpers import row_rel_err
from test_gpu_fold_in_implicit import FIXED, LAM, bound, device, reference, reverse
from ycnr_als import _lib

pytestmark = pytest.mark.gpu

COUNTS = [0, 1, 15, 16, 17, 32, 33, 64, 100, 127, 128, 129, 5]
STATUS = [2] + [0] * 10 + [3, 3]
SERVED = slice(1, 11)


@functools.lru_cache(maxsize=None)
def problem(k, alpha, side):
    """float32 inputs shared by both handle types.  Row 4 (served) has a zero value; the last row has a negative one."""
    rng = np.random.default_rng(3000 * k + side)
    ptr = np.concatenate([[0], np.cumsum(COUNTS)]).astype(np.int64)
    idx = np.concatenate([np.sort(rng.choice(FIXED, n, replace=False)) for n in COUNTS]).astype(np.int32)
    vals = rng.integers(1, 6, len(idx)).astype(np.float32)
    vals[ptr[4] + 7] = 0.0
    vals[ptr[12] + 2] = -0.25
    Y = (rng.standard_normal((FIXED, k)) / np.sqrt(k)).astype(np.float32)
    X0 = (rng.standard_normal((16, k)) / np.sqrt(k)).astype(np.float32)
    want, amp = np.zeros((len(COUNTS), k)), np.ones(len(COUNTS))
    for u in range(SERVED.start, SERVED.stop):
        want[u], amp[u] = reference(alpha, LAM[side], idx[ptr[u]:ptr[u + 1]], vals[ptr[u]:ptr[u + 1]], Y)
    return ptr, idx, vals, Y, X0, want, amp


def check(dt, k, alpha, side):
    ptr, idx, vals, Y, X0, want, amp = problem(k, alpha, side)
    dev = device(dt, k, side, Y, X0)
    rows, status, ms = dev.fold_in_implicit_wide(side, alpha, ptr, idx, vals.astype(dt))
    assert rows.dtype == dt and len(ms) == 3 and ms[2] > 0
    assert list(status) == STATUS and not rows[[0, 11, 12]].any()
    err, tol = row_rel_err(rows[SERVED], want[SERVED]), bound(amp[SERVED], dt)
    print(f"fold-in implicit wide {np.dtype(dt).name} k={k} alpha={alpha} side={side}: max err {err.max():.3e}, "
          f"worst err / bound {np.max(err / tol):.3f}")
    assert (err <= tol).all(), float(np.max(err / tol))
    assert np.array_equal(dev.get_factors(side), X0.astype(dt))  # storeIds=None: nothing is written
    dev.destroy()


@pytest.mark.parametrize("k,side", [(20, 0), (128, 0), (144, 0), (144, 1), (200, 0), (512, 0)])
@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_parity_with_float64_numpy(dt, k, side):
    check(dt, k, 0.5, side)


@pytest.mark.parametrize("alpha", [0.0, 40.0])
def test_alpha_cases(alpha):
    check(np.float32, 144, alpha, 0)


def test_agrees_with_fold_in_implicit_on_short_rows():
    ptr, idx, vals, Y, X0, _, amp = problem(100, 0.5, 0)
    dev = device(np.float32, 100, 0, Y, X0)
    rows, status, _ = dev.fold_in_implicit_wide(0, 0.5, ptr, idx, vals)
    old, _, _ = dev.fold_in_implicit(0, 0.5, ptr, idx, vals)
    short = slice(1, 6)  # lengths 1 .. 32
    err, tol = row_rel_err(rows[short], old[short]), 2 * bound(amp[short], np.float32)  # the sum of both bounds
    print(f"against fold_in_implicit: worst err / bound {np.max(err / tol):.3f}")
    assert list(status) == STATUS and (err <= tol).all()
    dev.destroy()


def test_bits_do_not_depend_on_the_company():
    ptr, idx, vals, Y, X0, _, _ = problem(144, 0.5, 0)
    dev = device(np.float32, 144, 0, Y, X0)
    rows, status, _ = dev.fold_in_implicit_wide(0, 0.5, ptr, idx, vals)
    rev, strev, _ = dev.fold_in_implicit_wide(0, 0.5, *reverse(ptr, idx, vals))
    assert np.array_equal(rev[::-1], rows) and np.array_equal(strev[::-1], status) and rows[SERVED].all(axis=1).all()
    dev.destroy()


def test_stores_where_asked_and_recommend_serves_the_stored_rows():
    ptr, idx, vals, Y, X0, _, _ = problem(144, 0.5, 0)
    dev = device(np.float32, 144, 0, Y, X0)
    store = np.arange(13, dtype=np.int32)[::-1].copy()  # request row r -> row 12 - r
    rows, status, _ = dev.fold_in_implicit_wide(0, 0.5, ptr, idx, vals, storeIds=store)
    want = X0.copy()
    want[store[SERVED]] = rows[SERVED]  # the targets of the rows with status 2 / 3 (12, 1, 0) and rows 13 .. 15 keep what they held
    assert list(status) == STATUS and np.array_equal(dev.get_factors(0), want)
    users, args = store[SERVED].copy(), dict(globalAvgShift=0.1, minRecommendRating=-1e30, limit=10)
    got = dev.recommend(users, ptr[SERVED.start:SERVED.stop + 1] - ptr[SERVED.start], idx[ptr[SERVED.start]:ptr[SERVED.stop]], **args)
    dev.set_factors(0, want)
    ref = dev.recommend(users, ptr[SERVED.start:SERVED.stop + 1] - ptr[SERVED.start], idx[ptr[SERVED.start]:ptr[SERVED.stop]], **args)
    assert all(np.array_equal(g, r) for g, r in zip(got[:3], ref[:3])) and (got[2] == 9).all()  # (limit - 1, as everywhere)
    dev.destroy()


@pytest.mark.parametrize("k,kw,code", [(513, {}, _lib.ERR_UNSUPPORTED), (144, dict(alpha=-1.0), _lib.ERR_INVALID),
                                       (144, dict(alpha=float("nan")), _lib.ERR_INVALID), (144, dict(bad_column=True), _lib.ERR_INVALID),
                                       (144, dict(store=[3] * 13), _lib.ERR_INVALID)])
def test_refusals_leave_outputs_and_matrices_alone(k, kw, code):
    ptr, idx, vals, Y, X0, _, _ = problem(144, 0.5, 0)
    rng = np.random.default_rng(k)
    Y, X0 = rng.standard_normal((FIXED, k)).astype(np.float32), rng.standard_normal((16, k)).astype(np.float32)
    dev = device(np.float32, k, 0, Y, X0)
    if kw.get("bad_column"):
        idx = idx.copy()
        idx[5] = FIXED
    store = None if "store" not in kw else np.array(kw["store"], np.int32)
    rows, status = np.full((13, k), 77, np.float32), np.full(13, 77, np.int32)
    rc = dev._L.ycnr_als_fold_in_implicit_wide(dev._h, 0, kw.get("alpha", 0.5), 13, ptr.ctypes.data, idx.ctypes.data, vals.ctypes.data,
                                               None if store is None else store.ctypes.data, rows.ctypes.data, status.ctypes.data, None)
    assert rc == code
    assert (rows == 77).all() and (status == 77).all()
    assert np.array_equal(dev.get_factors(0), X0) and np.array_equal(dev.get_factors(1), Y)
    dev.destroy()
