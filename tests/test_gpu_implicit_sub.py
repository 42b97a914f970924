"""ycnr_als_step_implicit_sub (csrc/implicit_sub_kernels.hip.h): sweeps of 16-wide subspace solves per row from a warm start,
against a numpy restatement of the method in the widest float numpy has, with the bounds of tests/test_gpu_implicit.py
(8 amp eps of the handle's precision, floor 1e-6 for float32).  Observed worst err / bound: DESIGN.md 14."""
import functools

import numpy as np
import pytest

import ycnr_als
from helpers import EPS32, make_problem, row_rel_err
from test_gpu_implicit import EPS64, FIXED, LAM, objective, reference
from ycnr_als import _lib
from ycnr_als.data import init_factors

pytestmark = pytest.mark.gpu

LD = np.longdouble if np.finfo(np.longdouble).eps < EPS64 else np.float64
WIDE = 256  # kSubWideRow: a longer row is walked by all four waves
SOLVED, SHARD, EMPTY = 36, (1, 35), 6  # 33 rows with observations in the shard: three batches of 16, the last one a single row


def ldl_solve(H, g, pivots=None):
    """pivots: a list that receives d_0 .. d_{n-1} as they are met (tests/test_gpu_implicit_edges.py decides bad rows from them)"""
    n = len(g)
    L, d, z = np.eye(n, dtype=H.dtype), np.zeros(n, H.dtype), g.copy()
    for j in range(n):
        d[j] = H[j, j] - (L[j, :j] * L[j, :j]) @ d[:j]
        if pivots is not None:
            pivots.append(d[j])
        for i in range(j + 1, n):
            L[i, j] = (H[i, j] - (L[i, :j] * L[j, :j]) @ d[:j]) / d[j]
        z[j] -= L[j, :j] @ z[:j]
    z /= d
    for j in range(n - 1, -1, -1):
        z[j] -= L[j + 1:, j] @ z[j + 1:]
    return z


def sub_reference(alpha, lam, G, Ys, r, x, sweeps):
    w, x = alpha * r, x.copy()
    e = Ys @ x
    for _ in range(sweeps):
        for b in range(0, len(x), 16):
            pi = slice(b, min(b + 16, len(x)))
            Yp = Ys[:, pi]
            g = G[pi] @ x + lam * x[pi] + Yp.T @ (w * e - (1 + w))
            H = G[pi, pi] + lam * np.eye(Yp.shape[1], dtype=LD) + (Yp.T * w) @ Yp
            delta = ldl_solve(H, g)
            x[pi] -= delta
            e -= Yp @ delta
    return x


@functools.lru_cache(maxsize=None)
def inputs(k, side):
    rng = np.random.default_rng(1000 * k + side)
    counts = [3, 1, 2, 15, 16, 17, 0, 31, 33, k - 1, k, k + 1, WIDE, WIDE + 1, 1000, 3] + list(range(1, 21))
    ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    idx = np.concatenate([np.sort(rng.choice(FIXED, n, replace=False)) for n in counts]).astype(np.int32)
    vals = rng.integers(1, 6, len(idx)).astype(np.float32)
    Y = (rng.standard_normal((FIXED, k)) / np.sqrt(k)).astype(np.float32)
    X0 = (rng.standard_normal((SOLVED, k)) / np.sqrt(k)).astype(np.float32)
    return ptr, idx, vals, Y, X0


@functools.lru_cache(maxsize=None)
def problem(k, alpha, side, sweeps):
    """float32 inputs shared by both handle types: CSR over all SOLVED rows, the fixed matrix, the warm start (the exact solution
    moved by 10 % of its norm in a random direction), the exact solutions, and want / amp per row."""
    ptr, idx, vals, Y, X0 = inputs(k, side)
    rng = np.random.default_rng(k + side)
    X0 = X0.copy()
    Yl = Y.astype(LD)
    G = Yl.T @ Yl
    want, exact, amp = np.zeros((SOLVED, k)), np.zeros((SOLVED, k)), np.ones(SOLVED)
    for u in range(*SHARD):
        if u != EMPTY:
            sl = slice(ptr[u], ptr[u + 1])
            exact[u], amp[u] = reference(alpha, LAM[side], idx[sl], vals[sl], Y)
            d = rng.standard_normal(k)
            X0[u] = (exact[u] + 0.1 * np.linalg.norm(exact[u]) * d / np.linalg.norm(d)).astype(np.float32)
            want[u] = sub_reference(LD(alpha), LD(LAM[side]), G, Yl[idx[sl]], vals[sl].astype(LD), X0[u].astype(LD), sweeps)
    return ptr, idx, vals, Y, X0, want, amp, exact


def device(dt, k, side, ptr, idx, vals, Y, X0, upload=True):
    rows = (SOLVED, FIXED) if side == 0 else (FIXED, SOLVED)
    dev = ycnr_als.AlsDevice(k, rows[0], rows[1], useDoublePrecision=dt == np.float64, userFactReg=LAM[0], itemFactReg=LAM[1], chunkRatings=64)
    if upload:
        dev.set_ratings(side, ptr, idx, vals.astype(dt), *SHARD)
    dev.set_factors(1 - side, Y.astype(dt))
    dev.set_factors(side, X0.astype(dt))
    return dev


def run_and_check(dt, k, alpha, side, sweeps, X0, want, amp, what):
    ptr, idx, vals, Y, _ = inputs(k, side)
    dev = device(dt, k, side, ptr, idx, vals, Y, X0)
    bad, ms = dev.step_implicit(side, alpha, sweeps=sweeps)
    got = dev.get_factors(side)
    dev.destroy()
    assert bad == 0 and len(ms) == 3 and ms[2] > 0
    outside = [0, SOLVED - 1]
    assert np.array_equal(got[outside], X0[outside].astype(dt))  # outside the shard: untouched
    assert not got[EMPTY].any()                                  # no observations: exactly zero
    live = [u for u in range(*SHARD) if u != EMPTY]
    err = row_rel_err(got[live], want[live])
    tol = 8 * amp[live] * EPS64 if dt == np.float64 else np.maximum(8 * amp[live] * EPS32, 1e-6)
    print(f"implicit sub {what} {np.dtype(dt).name} k={k} alpha={alpha} side={side} sweeps={sweeps}: max err {err.max():.3e}, "
          f"worst err / bound {np.max(err / tol):.3f}")
    assert (err <= tol).all(), float(np.max(err / tol))


# 7: a lone partial block; 20: a partial second block; 128: the last k on the narrow Gramian; 144: the first on the wide one, one
# pair of column blocks; 260: several pairs and a partial block; 512: the maximum
CASES = [(dt, k, 0.5, side, 1) for dt in (np.float32, np.float64) for k in (7, 20, 128, 144, 260, 512) for side in (0, 1)]
CASES += [(np.float32, 20, alpha, 0, 3) for alpha in (0.5, 0.0, 40.0)]


@pytest.mark.parametrize("dt,k,alpha,side,sweeps", CASES)
def test_parity_with_the_method_in_numpy(dt, k, alpha, side, sweeps):
    _, _, _, _, X0, want, amp, _ = problem(k, alpha, side, sweeps)
    run_and_check(dt, k, alpha, side, sweeps, X0, want, amp, "parity")


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_the_exact_solution_is_a_fixed_point(dt):
    _, _, _, _, X0, _, amp, exact = problem(144, 0.5, 0, 1)
    start = X0.astype(np.float64)
    start[SHARD[0]:SHARD[1]] = exact[SHARD[0]:SHARD[1]]
    run_and_check(dt, 144, 0.5, 0, 1, start.astype(dt), exact, amp, "fixed point")


def test_every_sub_half_step_descends_and_leaves_the_exact_step_intact():
    users, items, k, alpha = 60, 45, 8, 0.5
    bu, bi, _, _ = make_problem(users, items, k, density=0.3, seed=3)
    mask = np.zeros((users, items))
    mask[np.repeat(np.arange(users), bu.counts()), bu.indx] = 1.0
    R = np.zeros((users, items))
    R[mask > 0] = bu.vals
    devs = [ycnr_als.AlsDevice(k, users, items, userFactReg=LAM[0], itemFactReg=LAM[1]) for _ in range(2)]
    for dev in devs:
        dev.set_ratings("byUser", bu.rowPtr, bu.indx, bu.vals)
        dev.set_ratings("byItem", bi.rowPtr, bi.indx, bi.vals)
    dev, fresh = devs
    dev.set_factors("byUser", init_factors(users, k, 1))
    dev.set_factors("byItem", init_factors(items, k, 2))
    last = objective(alpha, R, mask, dev.get_factors(0), dev.get_factors(1))
    for side in (0, 1, 0, 1):
        assert dev.step_implicit(side, alpha, sweeps=1)[0] == 0
        now = objective(alpha, R, mask, dev.get_factors(0), dev.get_factors(1))
        assert now <= last, (side, now, last)  # an exact minimisation over a block never raises the row's quadratic
        last = now
    fresh.set_factors(0, dev.get_factors(0))
    fresh.set_factors(1, dev.get_factors(1))
    for d in devs:  # the exact call on the used handle: its plan, G and slabs are intact
        assert d.step_implicit(0, alpha)[0] == 0
    assert np.array_equal(dev.get_factors(0), fresh.get_factors(0))
    for d in devs:
        d.destroy()


@pytest.mark.parametrize("k,sweeps,upload,code", [(20, 0, True, _lib.ERR_INVALID), (20, 17, True, _lib.ERR_INVALID),
                                                  (513, 1, True, _lib.ERR_UNSUPPORTED), (20, 1, False, _lib.ERR_STATE)])
def test_refusals_leave_the_matrices_alone(k, sweeps, upload, code):
    ptr, idx, vals, Y, X0 = inputs(k, 0)
    dev = device(np.float32, k, 0, ptr, idx, vals, Y, X0, upload)
    with pytest.raises(ycnr_als.YcnrError) as e:
        dev.step_implicit(0, 0.5, sweeps=sweeps)
    assert e.value.code == code
    with pytest.raises(ValueError):
        dev.step_implicit(0, 0.5, cg_steps=3, sweeps=1)
    assert np.array_equal(dev.get_factors(0), X0) and np.array_equal(dev.get_factors(1), Y)
    dev.destroy()


def test_same_request_same_bits():
    ptr, idx, vals, Y, X0 = inputs(260, 1)
    dev = device(np.float32, 260, 1, ptr, idx, vals, Y, X0)
    dev.step_implicit(1, 0.5, sweeps=1)
    first = dev.get_factors(1)
    dev.set_factors(1, X0)
    dev.step_implicit(1, 0.5, sweeps=1)
    assert np.array_equal(first, dev.get_factors(1)) and not np.array_equal(first[1:35], X0[1:35])
    dev.destroy()
