"""ycnr_als_step_implicit_cg (csrc/implicit_cg_kernels.hip.h): a fixed number of conjugate-gradient steps per row from a warm
start, against a numpy restatement of the method in the widest float numpy has, with the bounds of tests/test_gpu_implicit.py
(8 amp eps of the handle's precision, floor 1e-6 for float32).  Rows longer than chunkRatings are split and solved exactly:
their reference is the exact solve.  Observed worst err / bound: DESIGN.md 14."""
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
SOLVED, SHARD, CHUNK, EMPTY = 36, (1, 35), 64, 6  # 32 whole rows with observations: two batches of 16, the second one short


def cg_reference(alpha, lam, G, Ys, r, x, steps, trace=None):
    """trace: a list that receives (d, p . p) of every step the row takes (tests/test_gpu_implicit_edges.py checks d's margin)"""
    w = alpha * r
    op = lambda v: G @ v + lam * v + Ys.T @ (w * (Ys @ v))
    res = Ys.T @ (1 + w) - op(x)
    p, rho = res.copy(), res @ res
    for _ in range(steps):
        q = op(p)
        d = p @ q
        if trace is not None:
            trace.append((d, p @ p))
        if rho == 0 or not d > 0:
            break
        a = rho / d
        x, res = x + a * p, res - a * q
        rho, old = res @ res, rho
        p = res + (rho / old) * p
    return x


@functools.lru_cache(maxsize=None)
def problem(k, alpha, side, steps):
    """float32 inputs shared by both handle types: CSR over all SOLVED rows, the fixed matrix, the warm start (the exact solution
    moved by 10 % of its norm in a random direction), and want / amp per row."""
    rng = np.random.default_rng(1000 * k + side)
    counts = [3, 1, 2, 15, 16, 17, 0, 31, 33, k - 1, k, k + 1, 64, 65, 300, 3] + list(range(1, 21))
    ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    idx = np.concatenate([np.sort(rng.choice(FIXED, n, replace=False)) for n in counts]).astype(np.int32)
    vals = rng.integers(1, 6, len(idx)).astype(np.float32)
    Y = (rng.standard_normal((FIXED, k)) / np.sqrt(k)).astype(np.float32)
    X0 = (rng.standard_normal((SOLVED, k)) / np.sqrt(k)).astype(np.float32)
    Yl = Y.astype(LD)
    G = Yl.T @ Yl
    want, amp = np.zeros((SOLVED, k)), np.ones(SOLVED)
    for u in range(*SHARD):
        if counts[u]:
            sl = slice(ptr[u], ptr[u + 1])
            exact, amp[u] = reference(alpha, LAM[side], idx[sl], vals[sl], Y)
            d = rng.standard_normal(k)
            X0[u] = (exact + 0.1 * np.linalg.norm(exact) * d / np.linalg.norm(d)).astype(np.float32)
            want[u] = exact if counts[u] > CHUNK else cg_reference(LD(alpha), LD(LAM[side]), G, Yl[idx[sl]], vals[sl].astype(LD), X0[u].astype(LD), steps)
    return ptr, idx, vals, Y, X0, want, amp


def device(dt, k, side, ptr, idx, vals, Y, X0, upload=True):
    rows = (SOLVED, FIXED) if side == 0 else (FIXED, SOLVED)
    dev = ycnr_als.AlsDevice(k, rows[0], rows[1], useDoublePrecision=dt == np.float64, userFactReg=LAM[0], itemFactReg=LAM[1], chunkRatings=CHUNK)
    if upload:
        dev.set_ratings(side, ptr, idx, vals.astype(dt), *SHARD)
    dev.set_factors(1 - side, Y.astype(dt))
    dev.set_factors(side, X0.astype(dt))
    return dev


CASES = [(dt, k, 0.5, side, 3) for dt in (np.float32, np.float64) for k in (7, 20, 100, 128) for side in (0, 1)]
CASES += [(np.float32, 20, 0.5, 0, 1), (np.float32, 20, 0.0, 0, 3), (np.float32, 20, 40.0, 0, 3)]


@pytest.mark.parametrize("dt,k,alpha,side,steps", CASES)
def test_parity_with_the_method_in_numpy(dt, k, alpha, side, steps):
    ptr, idx, vals, Y, X0, want, amp = problem(k, alpha, side, steps)
    dev = device(dt, k, side, ptr, idx, vals, Y, X0)
    bad, ms = dev.step_implicit(side, alpha, cg_steps=steps)
    got = dev.get_factors(side)
    dev.destroy()
    assert bad == 0 and len(ms) == 3 and ms[2] > 0
    outside = [0, SOLVED - 1]
    assert np.array_equal(got[outside], X0[outside].astype(dt))  # outside the shard: untouched
    assert not got[EMPTY].any()                                  # no observations: exactly zero
    live = [u for u in range(*SHARD) if u != EMPTY]
    err = row_rel_err(got[live], want[live])
    tol = 8 * amp[live] * EPS64 if dt == np.float64 else np.maximum(8 * amp[live] * EPS32, 1e-6)
    print(f"implicit cg {np.dtype(dt).name} k={k} alpha={alpha} side={side} steps={steps}: max err {err.max():.3e}, "
          f"worst err / bound {np.max(err / tol):.3f}")
    assert (err <= tol).all(), float(np.max(err / tol))


def test_every_cg_half_step_descends_and_leaves_the_exact_step_intact():
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
        assert dev.step_implicit(side, alpha, cg_steps=2)[0] == 0
        now = objective(alpha, R, mask, dev.get_factors(0), dev.get_factors(1))
        assert now <= last, (side, now, last)  # a CG iterate from a warm start never raises the row's quadratic
        last = now
    fresh.set_factors(0, dev.get_factors(0))
    fresh.set_factors(1, dev.get_factors(1))
    for d in devs:  # the exact call on the used handle: the shared plan, G and slabs are intact
        assert d.step_implicit(0, alpha)[0] == 0
    assert np.array_equal(dev.get_factors(0), fresh.get_factors(0))
    for d in devs:
        d.destroy()


@pytest.mark.parametrize("k,steps,upload,code", [(20, 0, True, _lib.ERR_INVALID), (20, 65, True, _lib.ERR_INVALID),
                                                 (129, 3, True, _lib.ERR_UNSUPPORTED), (20, 3, False, _lib.ERR_STATE)])
def test_refusals_leave_the_matrices_alone(k, steps, upload, code):
    ptr, idx, vals, Y, X0, _, _ = problem(k, 0.5, 0, 3)
    dev = device(np.float32, k, 0, ptr, idx, vals, Y, X0, upload)
    with pytest.raises(ycnr_als.YcnrError) as e:
        dev.step_implicit(0, 0.5, cg_steps=steps)
    assert e.value.code == code
    assert np.array_equal(dev.get_factors(0), X0) and np.array_equal(dev.get_factors(1), Y)
    dev.destroy()


def test_same_request_same_bits():
    ptr, idx, vals, Y, X0, _, _ = problem(100, 0.5, 1, 3)
    dev = device(np.float32, 100, 1, ptr, idx, vals, Y, X0)
    dev.step_implicit(1, 0.5, cg_steps=3)
    first = dev.get_factors(1)
    dev.set_factors(1, X0)
    dev.step_implicit(1, 0.5, cg_steps=3)
    assert np.array_equal(first, dev.get_factors(1)) and not np.array_equal(first[1:35], X0[1:35])
    dev.destroy()
