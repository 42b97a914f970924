"""ycnr_als_step_implicit (csrc/implicit_kernels.hip.h): the implicit-feedback half-step of Hu, Koren, Volinsky against a plain
float64 numpy solve of the same formula, with the bounds of tests/test_gpu_parity.py (8 amp eps of the handle's precision,
floor 1e-6 for float32).  Observed worst err / bound: DESIGN.md 14."""
import functools

import numpy as np
import pytest

import ycnr_als
from helpers import EPS32, make_problem, numpy_step, row_rel_err
from ycnr_als import _lib
from ycnr_als.data import init_factors

pytestmark = pytest.mark.gpu

EPS64 = float(np.finfo(np.float64).eps)
LAM = (0.05, 0.07)  # user, item: different, so that a test sees which one a side uses
FIXED, SOLVED, SHARD = 2069, 16, (1, 15)  # two Gramian slices, the second ending on a partial panel; rows 0 and 15 lie outside the shard


def reference(alpha, lam, idx, r, Y):
    """x and amp = cond(A) max(1, || |Y|^T c || / ||b||) of one row, float64 (the form of helpers.numpy_row_solve)."""
    Y = Y.astype(np.float64)
    Ys, r = Y[idx], r.astype(np.float64)
    c = 1.0 + alpha * r
    A = Y.T @ Y + (Ys.T * (alpha * r)) @ Ys + lam * np.eye(Y.shape[1])
    b = Ys.T @ c
    amp = np.linalg.cond(A) * max(1.0, np.linalg.norm(np.abs(Ys).T @ c) / max(np.linalg.norm(b), 1e-300))
    return np.linalg.solve(A, b), amp


@functools.lru_cache(maxsize=None)
def problem(k, alpha, side):
    """float32 inputs (a float64 handle gets them widened, so both share this reference): CSR over all SOLVED rows, the fixed
    matrix, the start of the solved one, and want / amp per row."""
    rng = np.random.default_rng(1000 * k + side)
    counts = [3, 1, 2, 15, 16, 17, 0, 31, 33, k - 1, k, k + 1, 64, 65, 300, 3]  # chunkRatings = 64: 65 and 300 take 2 and 5 slabs
    ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    idx = np.concatenate([np.sort(rng.choice(FIXED, n, replace=False)) for n in counts]).astype(np.int32)
    vals = rng.integers(1, 6, len(idx)).astype(np.float32)
    Y = (rng.standard_normal((FIXED, k)) / np.sqrt(k)).astype(np.float32)
    X0 = (rng.standard_normal((SOLVED, k)) / np.sqrt(k)).astype(np.float32)
    want, amp = np.zeros((SOLVED, k)), np.ones(SOLVED)
    for u in range(*SHARD):
        if counts[u]:
            want[u], amp[u] = reference(alpha, LAM[side], idx[ptr[u]:ptr[u + 1]], vals[ptr[u]:ptr[u + 1]], Y)
    return ptr, idx, vals, Y, X0, want, amp


def device(dt, k, side, ptr, idx, vals, Y, X0, upload=True):
    rows = (SOLVED, FIXED) if side == 0 else (FIXED, SOLVED)
    dev = ycnr_als.AlsDevice(k, rows[0], rows[1], useDoublePrecision=dt == np.float64, userFactReg=LAM[0], itemFactReg=LAM[1], chunkRatings=64)
    if upload:
        dev.set_ratings(side, ptr, idx, vals.astype(dt), *SHARD)
    dev.set_factors(1 - side, Y.astype(dt))
    dev.set_factors(side, X0.astype(dt))
    return dev


def check(dt, k, alpha, side):
    ptr, idx, vals, Y, X0, want, amp = problem(k, alpha, side)
    dev = device(dt, k, side, ptr, idx, vals, Y, X0)
    bad, ms = dev.step_implicit(side, alpha)
    got = dev.get_factors(side)
    dev.destroy()
    assert bad == 0 and len(ms) == 3 and ms[2] > 0
    assert np.array_equal(got[[0, 15]], X0[[0, 15]].astype(dt))  # outside the shard: untouched
    assert not got[6].any()                                     # no observations: exactly zero
    live = [u for u in range(*SHARD) if u != 6]
    err = row_rel_err(got[live], want[live])
    tol = 8 * amp[live] * EPS64 if dt == np.float64 else np.maximum(8 * amp[live] * EPS32, 1e-6)
    print(f"implicit {np.dtype(dt).name} k={k} alpha={alpha} side={side}: max err {err.max():.3e}, worst err / bound {np.max(err / tol):.3f}")
    assert (err <= tol).all(), float(np.max(err / tol))


@pytest.mark.parametrize("side", [0, 1])
@pytest.mark.parametrize("k", [7, 20, 100, 128])
@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_parity_with_float64_numpy(dt, k, side):
    check(dt, k, 0.5, side)


@pytest.mark.parametrize("alpha", [0.0, 40.0])  # 0: every row solves (G + lambda I) x = sum y, the shared Gramian alone; 40: the paper's
def test_alpha_cases(alpha):
    check(np.float32, 20, alpha, 0)


def objective(alpha, R, mask, X, Y):
    X, Y = X.astype(np.float64), Y.astype(np.float64)
    return ((1.0 + alpha * R) * (mask - X @ Y.T) ** 2).sum() + LAM[0] * (X * X).sum() + LAM[1] * (Y * Y).sum()


def test_every_half_step_descends_and_leaves_the_explicit_step_intact():
    users, items, k, alpha = 60, 45, 8, 0.5
    bu, bi, _, _ = make_problem(users, items, k, density=0.3, seed=3)
    mask = np.zeros((users, items))
    mask[np.repeat(np.arange(users), bu.counts()), bu.indx] = 1.0
    R = np.zeros((users, items))
    R[mask > 0] = bu.vals
    dev = ycnr_als.AlsDevice(k, users, items, userFactReg=LAM[0], itemFactReg=LAM[1])
    dev.set_ratings("byUser", bu.rowPtr, bu.indx, bu.vals)
    dev.set_ratings("byItem", bi.rowPtr, bi.indx, bi.vals)
    dev.set_factors("byUser", init_factors(users, k, 1))
    dev.set_factors("byItem", init_factors(items, k, 2))
    last = objective(alpha, R, mask, dev.get_factors(0), dev.get_factors(1))
    for side in (0, 1, 0, 1):
        assert dev.step_implicit(side, alpha)[0] == 0
        now = objective(alpha, R, mask, dev.get_factors(0), dev.get_factors(1))
        assert now <= last, (side, now, last)  # an exact minimiser over one side; float32's excess is second order
        last = now
    U, V = dev.get_factors(0), dev.get_factors(1)
    dev.step("byUser")  # the explicit path on the same handle: its padded copies and planes are rebuilt from these matrices
    want, conds = numpy_step(LAM[0], k, bu, V, U)
    assert (row_rel_err(dev.get_factors(0), want) <= np.maximum(8 * conds * EPS32, 1e-6)).all()
    dev.destroy()


@pytest.mark.parametrize("k,alpha,upload,code", [(129, 0.5, True, _lib.ERR_UNSUPPORTED), (20, -1.0, True, _lib.ERR_INVALID),
                                                 (20, float("nan"), True, _lib.ERR_INVALID), (20, 0.5, False, _lib.ERR_STATE)])
def test_refusals_leave_the_matrices_alone(k, alpha, upload, code):
    ptr, idx, vals, Y, X0, _, _ = problem(k, 0.5, 0)
    dev = device(np.float32, k, 0, ptr, idx, vals, Y, X0, upload)
    with pytest.raises(ycnr_als.YcnrError) as e:
        dev.step_implicit(0, alpha)
    assert e.value.code == code
    assert np.array_equal(dev.get_factors(0), X0) and np.array_equal(dev.get_factors(1), Y)
    dev.destroy()


def test_same_request_same_bits():
    ptr, idx, vals, Y, X0, _, _ = problem(100, 0.5, 1)
    dev = device(np.float32, 100, 1, ptr, idx, vals, Y, X0)
    dev.step_implicit(1, 0.5)
    first = dev.get_factors(1)
    dev.set_factors(1, X0)
    dev.step_implicit(1, 0.5)
    assert np.array_equal(first, dev.get_factors(1)) and first[1:15].any()
    dev.destroy()
