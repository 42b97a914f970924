"""ycnr_als_step_implicit_wide (csrc/implicit_wide_kernels.hip.h): the exact implicit half-step up to 512 factors.  Dual rows
(1 .. 128 non-negative observations) bit for bit against fold_in_implicit_wide on the same handle; primal rows against the plain
float64 numpy solve and the bounds of tests/test_gpu_implicit.py (8 amp eps of the handle's precision, floor 1e-6 for float32).
chunkRatings = 64: 129 observations are three slabs with a last chunk of one, 192 exactly three, 193 four, 700 eleven.
Observed worst err / bound: DESIGN.md 14."""
import functools

import numpy as np
import pytest

import ycnr_als
from helpers import EPS32, row_rel_err
from test_gpu_implicit import EPS64, FIXED, LAM, reference
from ycnr_als import _lib

pytestmark = pytest.mark.gpu

ALPHA = 0.5


def make(counts, k, seed):
    """float32 inputs shared by both handle types; the first and the last row lie outside the shard."""
    rng = np.random.default_rng(seed)
    ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    idx = np.concatenate([np.sort(rng.choice(FIXED, n, replace=False)) for n in counts]).astype(np.int32)
    vals = rng.integers(1, 6, len(idx)).astype(np.float32)
    Y = (rng.standard_normal((FIXED, k)) / np.sqrt(k)).astype(np.float32)
    X0 = (rng.standard_normal((len(counts), k)) / np.sqrt(k)).astype(np.float32)
    return ptr, idx, vals, Y, X0


def device(dt, k, side, ptr, idx, vals, Y, X0, upload=True):
    rows = (len(X0), FIXED) if side == 0 else (FIXED, len(X0))
    dev = ycnr_als.AlsDevice(k, rows[0], rows[1], useDoublePrecision=dt == np.float64, userFactReg=LAM[0], itemFactReg=LAM[1], chunkRatings=64)
    if upload:
        dev.set_ratings(side, ptr, idx, vals.astype(dt), 1, len(X0) - 1)
    dev.set_factors(1 - side, Y.astype(dt))
    dev.set_factors(side, X0.astype(dt))
    return dev


@functools.lru_cache(maxsize=None)
def problem(k, side):
    counts = [3, 1, 3, 127, 128, 129, 130, 192, 193, 700, k - 1, k, k + 1, 0, 5, 128, 3]
    ptr, idx, vals, Y, X0 = make(counts, k, 7000 * k + side)
    vals[ptr[14] + 2] = vals[ptr[15] + 77] = -0.25  # primal by value
    dual = [u for u in range(1, 16) if 1 <= counts[u] <= 128 and u not in (14, 15)]
    primal = [u for u in range(1, 16) if counts[u] and u not in dual]
    want, amp = np.zeros((len(counts), k)), np.ones(len(counts))
    for u in primal:
        want[u], amp[u] = reference(ALPHA, LAM[side], idx[ptr[u]:ptr[u + 1]], vals[ptr[u]:ptr[u + 1]], Y)
    for u in (14, 15):  # the rows with a negative weight are still well posed
        Yd, sl = Y.astype(np.float64), slice(ptr[u], ptr[u + 1])
        A = Yd.T @ Yd + (Yd[idx[sl]].T * (ALPHA * vals[sl])) @ Yd[idx[sl]] + LAM[side] * np.eye(k)
        assert np.isfinite(amp[u]) and np.linalg.eigvalsh(A).min() > 0
    return ptr, idx, vals, Y, X0, want, amp, dual, primal


@pytest.mark.parametrize("k,side", [(40, 0), (129, 0), (144, 0), (144, 1), (256, 0), (512, 0)])
@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_parity(dt, k, side):
    ptr, idx, vals, Y, X0, want, amp, dual, primal = problem(k, side)
    dev = device(dt, k, side, ptr, idx, vals, Y, X0)
    bad, ms = dev.step_implicit_wide(side, ALPHA)
    got = dev.get_factors(side)
    dptr = np.concatenate([[0], np.cumsum([ptr[u + 1] - ptr[u] for u in dual])]).astype(np.int64)
    take = np.concatenate([np.arange(ptr[u], ptr[u + 1]) for u in dual])
    rows, status, _ = dev.fold_in_implicit_wide(side, ALPHA, dptr, idx[take], vals[take].astype(dt))
    dev.destroy()
    assert bad == 0 and len(ms) == 3 and ms[2] > 0
    assert np.array_equal(got[[0, -1]], X0[[0, -1]].astype(dt))  # outside the shard: untouched
    assert not got[13].any()                                     # no observations: exactly zero
    assert not status.any() and np.array_equal(got[dual], rows) and rows.all(axis=1).all()  # the fold-in's bits
    err = row_rel_err(got[primal], want[primal])
    tol = 8 * amp[primal] * EPS64 if dt == np.float64 else np.maximum(8 * amp[primal] * EPS32, 1e-6)
    print(f"implicit wide {np.dtype(dt).name} k={k} side={side}: max err {err.max():.3e}, worst err / bound {np.max(err / tol):.3f}")
    assert (err <= tol).all(), float(np.max(err / tol))


@pytest.mark.parametrize("case", ["indefinite", "nan value", "nan in the fixed matrix"])
def test_bad_rows_stay_alone(case):
    k, counts = 144, [3, 200, 10, 5, 130, 0, 64, 3]
    ptr, idx, vals, Y, X0 = make(counts, k, 11)
    row = {"indefinite": 1, "nan value": 2}.get(case)

    def run(vals, Y):
        dev = device(np.float32, k, 0, ptr, idx, vals, Y, X0)
        bad, _ = dev.step_implicit_wide(0, ALPHA)
        got = dev.get_factors(0)
        dev.destroy()
        return bad, got

    hurt, Yh = vals.copy(), Y.copy()
    if case == "indefinite":
        hurt[ptr[1]:ptr[2]] = -50.0
    elif case == "nan value":
        hurt[ptr[2] + 4] = np.nan
    else:
        Yh[1000, 77] = np.nan
    bad, got = run(hurt, Yh)
    assert np.array_equal(got[[0, -1]], X0[[0, -1]])
    if row is None:
        assert bad == 5 and not got[1:-1].any()
        return
    clean = vals.copy()
    clean[ptr[row]:ptr[row + 1]] = 1.0
    bad0, ref = run(clean, Y)
    others = [u for u in range(len(counts)) if u != row]
    assert bad == 1 and bad0 == 0 and not got[row].any() and ref[row].any()
    assert np.array_equal(got[others], ref[others])


@pytest.mark.parametrize("k,alpha,upload,code", [(513, 0.5, True, _lib.ERR_UNSUPPORTED), (20, -1.0, True, _lib.ERR_INVALID),
                                                 (20, 0.5, False, _lib.ERR_STATE)])
def test_refusals_leave_the_matrices_alone(k, alpha, upload, code):
    ptr, idx, vals, Y, X0 = make([3, 5, 0, 140, 3], k, k)
    dev = device(np.float32, k, 0, ptr, idx, vals, Y, X0, upload)
    with pytest.raises(ycnr_als.YcnrError) as e:
        dev.step_implicit_wide(0, alpha)
    assert e.value.code == code
    assert np.array_equal(dev.get_factors(0), X0) and np.array_equal(dev.get_factors(1), Y)
    dev.destroy()
