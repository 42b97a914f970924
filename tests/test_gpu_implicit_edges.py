"""The implicit-feedback entries (ycnr_als_step_implicit, _cg, _sub, ycnr_als_fold_in_implicit, ycnr_als_recommend_for_observations)
where their own files do not go:
  1. the row-count edges of the fixed side, i.e. of implicit_gram_kernel / implicit_gram_wide_kernel (one row, one panel +- 1, one
     MFMA chain +- 1, one slice +- 1, three slices), seen through the solved rows: a lost or doubled fixed row moves every row by
     about 1 / m, the bounds are those of tests/test_gpu_implicit.py (8 amp eps64 for float64 handles, max(8 amp EPS32, 1e-6) for
     float32) and every one of them is asserted to be <= 1e-2;
  2. bad rows: an indefinite row, a NaN row and a NaN in G are counted, zeroed, kept away from the rows beside them and forgotten by
     the next call;
  3. matrices bound at an address that is no multiple of 16 bytes: the element-load Gramian gives the bits of the vector-load one.
The references are imported from the entries' own files.  Observed worst err / bound: DESIGN.md 14 and 16."""
import functools

import numpy as np
import pytest

import ycnr_als
from helpers import EPS32, row_rel_err
from test_gpu_implicit import EPS64, LAM, reference
from test_gpu_implicit_cg import LD, cg_reference
from test_gpu_implicit_sub import device as sub_device, inputs as sub_inputs, ldl_solve, sub_reference

pytestmark = pytest.mark.gpu

ALPHA, CG_STEPS, SWEEPS = 0.5, 3, 1
F32, F64 = np.float32, np.float64


def bound(amp, dt):
    return 8 * amp * EPS64 if dt == np.float64 else np.maximum(8 * amp * EPS32, 1e-6)


def nudged(rng, exact):
    """the warm start of the CG and subspace files: the exact solution moved by 10 % of its norm in a random direction"""
    d = rng.standard_normal(len(exact))
    return (exact + 0.1 * np.linalg.norm(exact) * d / np.linalg.norm(d)).astype(np.float32)


def iterate(method, G, Yl, idx, vals, x0):
    ref, n = (cg_reference, CG_STEPS) if method == "cg" else (sub_reference, SWEEPS)
    return ref(LD(ALPHA), LD(LAM[0]), G, Yl[idx], vals.astype(LD), x0.astype(LD), n)


def judge(what, dt, got, want, amp):
    tol = bound(amp, dt)
    assert (tol <= 1e-2).all(), float(tol.max())  # else the comparison below says nothing
    err = row_rel_err(got, want)
    print(f"implicit edges {what} {np.dtype(dt).name}: max err {err.max():.3e}, worst err / bound {np.max(err / tol):.3f}")
    assert (err <= tol).all(), float(np.max(err / tol))


# ---------------------------------------------------------------------------------------------- 1. row counts of the fixed side
EDGE_LIVE = [0, 1, 2, 4]  # row 3 has no observations; row 4 observes EVERY fixed row: its sums touch every panel


@functools.lru_cache(maxsize=None)
def edge_problem(m, k, method):
    """float32 inputs shared by both handle types, user side: five rows of 1, min(m, 3), min(m, 17), 0 and m observations with
    continuous values (one exact zero), the fixed matrix of m rows, the start (for "cg" / "sub": the warm start), want / amp."""
    rng = np.random.default_rng(100000 * k + m)
    counts = [1, min(m, 3), min(m, 17), 0, m]
    ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    idx = np.concatenate([np.sort(rng.choice(m, n, replace=False)) for n in counts]).astype(np.int32)
    vals = rng.gamma(2.0, 1.0, len(idx)).astype(np.float32)
    vals[ptr[2]] = 0.0
    Y = (rng.standard_normal((m, k)) / np.sqrt(k)).astype(np.float32)
    X0 = (rng.standard_normal((5, k)) / np.sqrt(k)).astype(np.float32)
    Yl = Y.astype(LD)
    G = Yl.T @ Yl if method != "exact" else None
    want, amp = np.zeros((5, k)), np.ones(5)
    for u in EDGE_LIVE:
        sl = slice(ptr[u], ptr[u + 1])
        want[u], amp[u] = reference(ALPHA, LAM[0], idx[sl], vals[sl], Y)
        if method != "exact":
            X0[u] = nudged(rng, want[u])
            want[u] = iterate(method, G, Yl, idx[sl], vals[sl], X0[u])
    return ptr, idx, vals, Y, X0, want, amp


def edge_device(dt, m, k, ptr, idx, vals, Y, X0):
    dev = ycnr_als.AlsDevice(k, 5, m, useDoublePrecision=dt == np.float64, userFactReg=LAM[0], itemFactReg=LAM[1])
    dev.set_ratings(0, ptr, idx, vals.astype(dt))  # the whole matrix is the shard
    dev.set_factors(1, Y.astype(dt))
    dev.set_factors(0, X0.astype(dt))
    return dev


def check_edge_step(dt, m, k, method, **how):
    ptr, idx, vals, Y, X0, want, amp = edge_problem(m, k, method)
    dev = edge_device(dt, m, k, ptr, idx, vals, Y, X0)
    bad, _ = dev.step_implicit(0, ALPHA, **how)
    got = dev.get_factors(0)
    dev.destroy()
    assert bad == 0 and not got[3].any()
    judge(f"{method} m={m} k={k}", dt, got[EDGE_LIVE], want[EDGE_LIVE], amp[EDGE_LIVE])


# 1: a lone row (nPanels == 1, one live row); 15 / 16 / 17: a panel less one, whole, plus one; 63 / 64 / 65: the same for an MFMA
# chain of four panels; 2047 / 2048 / 2049: for a slice; 4097: three slices, and the all-observing row takes two chunks of 4096
NARROW_M = [1, 15, 16, 17, 63, 64, 65, 2047, 2048, 2049, 4097]


@pytest.mark.parametrize("m", NARROW_M)
@pytest.mark.parametrize("k", [7, 20])  # 7: element loads in both types; 20: 16-byte loads in both
@pytest.mark.parametrize("dt", [F32, F64])
def test_narrow_gramian_row_counts(dt, k, m):
    check_edge_step(dt, m, k, "exact")


WIDE_CASES = [(F32, k, m) for k in (144, 260) for m in (1, 17, 64, 65, 2048, 2049)] + [(F64, k, m) for k in (144, 260) for m in (17, 2049)]


@pytest.mark.parametrize("dt,k,m", WIDE_CASES)
def test_wide_gramian_row_counts(dt, k, m):
    check_edge_step(dt, m, k, "sub", sweeps=SWEEPS)


@pytest.mark.parametrize("m", [17, 2049])
@pytest.mark.parametrize("dt", [F32, F64])
def test_cg_launch_site_row_counts(dt, m):
    check_edge_step(dt, m, 20, "cg", cg_steps=CG_STEPS)


@pytest.mark.parametrize("m", [17, 2049])
@pytest.mark.parametrize("dt", [F32, F64])
def test_fold_in_launch_site_row_counts(dt, m):
    ptr, idx, vals, Y, X0, want, amp = edge_problem(m, 20, "exact")
    dev = edge_device(dt, m, 20, ptr, idx, vals, Y, X0)
    rows, status, _ = dev.fold_in_implicit(0, ALPHA, ptr, idx, vals.astype(dt))  # m = 17: every row dual; 2049: the last one primal
    dev.destroy()
    assert list(status) == [0, 0, 0, 2, 0] and not rows[3].any()
    judge(f"fold-in m={m} k=20", dt, rows[EDGE_LIVE], want[EDGE_LIVE], amp[EDGE_LIVE])


# ---------------------------------------------------------------------------------------------- 2. bad rows
# 36 rows, shard [1, 35), 33 of its rows with observations: three batches of 16 in the CG and subspace kernels; chunkRatings = 64,
# so the rows of 65 and 200 are split and solved exactly by every entry but the subspace one.  Float32 handles.
BK, BM, BSOLVED, BSHARD, BEMPTY, BCHUNK = 20, 300, 36, (1, 35), 6, 64
BCOUNTS = [3, 1, 2, 15, 16, 17, 0, 31, 33, 19, 20, 21, 64, 65, 200, 3] + list(range(1, 21))
ROW_A, ROW_B, ROW_C = 20, 25, 30  # A: one strongly negative value (indefinite); B: one NaN; C: one mildly negative value (healthy)
HOSTILE = [ROW_A, ROW_B]
OUTSIDE = [0, BSOLVED - 1]
LIVE = [u for u in range(*BSHARD) if u != BEMPTY]
STEPS = {"exact": {}, "cg": dict(cg_steps=CG_STEPS), "sub": dict(sweeps=SWEEPS)}


@functools.lru_cache(maxsize=None)
def bad_inputs(k):
    """CSR over all 36 rows, its values twice -- `hostile`, and `benign` = the same with the bad values of rows A and B replaced --,
    the fixed matrix, and the warm start (nudged from the exact solution under the hostile values; row B: random).  Nobody
    observes the last fixed row: the tests of a poisoned G put their NaN there."""
    rng = np.random.default_rng(424242 + k)
    ptr = np.concatenate([[0], np.cumsum(BCOUNTS)]).astype(np.int64)
    idx = np.concatenate([np.sort(rng.choice(BM - 1, n, replace=False)) for n in BCOUNTS]).astype(np.int32)
    benign = rng.gamma(2.0, 1.0, len(idx)).astype(np.float32)
    benign[ptr[ROW_C] + 7] = -1.0
    hostile = benign.copy()
    hostile[ptr[ROW_A] + 2] = -200.0
    hostile[ptr[ROW_B] + 4] = np.nan
    Y = (rng.standard_normal((BM, k)) / np.sqrt(k)).astype(np.float32)
    X0 = (rng.standard_normal((BSOLVED, k)) / np.sqrt(k)).astype(np.float32)
    for u in range(BSOLVED):
        if u not in (BEMPTY, ROW_B):
            X0[u] = nudged(rng, reference(ALPHA, LAM[0], idx[ptr[u]:ptr[u + 1]], hostile[ptr[u]:ptr[u + 1]], Y)[0])
    return ptr, idx, benign, hostile, Y, X0


def row_matrix(Y, idx, r):
    Y = Y.astype(np.float64)
    return Y.T @ Y + (Y[idx].T * (ALPHA * r.astype(np.float64))) @ Y[idx] + LAM[0] * np.eye(Y.shape[1])


def sub_verdict(G, Ys, w):
    """(bad, decided) of one row by the pivots of its 16 x 16 systems in the widest float (they do not depend on x): bad when a
    block meets a pivot <= 0 with every |pivot| / |H_jj| up to it above 1e-6; good when every pivot of every block is positive with
    that margin; anything else is not decided."""
    k, allGood = G.shape[0], True
    for b in range(0, k, 16):
        pi = slice(b, min(b + 16, k))
        H = G[pi, pi] + LD(LAM[0]) * np.eye(pi.stop - pi.start, dtype=LD) + (Ys[:, pi].T * w) @ Ys[:, pi]
        pivots, margin = [], np.inf
        with np.errstate(all="ignore"):
            ldl_solve(H, np.zeros(pi.stop - pi.start, LD), pivots=pivots)
        for j, d in enumerate(pivots):
            margin = min(margin, abs(d) / abs(H[j, j]))
            if not d > 0:
                break
        if not margin > 1e-6:
            allGood = False
        elif not pivots[j] > 0:
            return True, True
    return False, allGood


@functools.lru_cache(maxsize=None)
def bad_facts():
    """What the float64 / long-double references say about the hostile request, with the margins that make it a decision:
    want per entry and amp for every row but B, and the set of rows the subspace entry must flag."""
    ptr, idx, _, hostile, Y, X0 = bad_inputs(BK)
    Yl = Y.astype(LD)
    G = Yl.T @ Yl
    want = {e: np.zeros((BSOLVED, BK)) for e in STEPS}
    amp, subBad = np.ones(BSOLVED), {ROW_B}
    for u in range(BSOLVED):
        if u in (BEMPTY, ROW_B):
            continue
        sl = slice(ptr[u], ptr[u + 1])
        want["exact"][u], amp[u] = reference(ALPHA, LAM[0], idx[sl], hostile[sl], Y)
        eig = np.linalg.eigvalsh(row_matrix(Y, idx[sl], hostile[sl]))
        norm = np.abs(eig).max()
        if u == ROW_A:
            assert eig[0] < -0.1 * norm, (eig[0], norm)  # clearly indefinite: a pivot <= 0 in any elimination order
        else:
            assert eig[0] > 0.1 * LAM[0], (u, eig[0])     # definite, row C with its negative value included
        trace = []
        split = BCOUNTS[u] > BCHUNK  # solved exactly by the CG entry
        want["cg"][u] = want["exact"][u] if split else cg_reference(LD(ALPHA), LD(LAM[0]), G, Yl[idx[sl]], hostile[sl].astype(LD),
                                                                    X0[u].astype(LD), CG_STEPS, trace=trace)
        for d, pp in trace:  # the stop rule !(d > 0) is decided with room, for row A above all
            assert abs(d) > 1e-6 * pp * norm, (u, float(d), float(pp), norm)
        if u == ROW_A:
            print("row A under cg: d / (p.p ||A||) =", [float(d / (pp * norm)) for d, pp in trace])
        isBad, decided = sub_verdict(G, Yl[idx[sl]], LD(ALPHA) * hostile[sl].astype(LD))
        assert decided and isBad == (u == ROW_A), (u, isBad, decided)
        if isBad:
            subBad.add(u)
        else:
            want["sub"][u] = sub_reference(LD(ALPHA), LD(LAM[0]), G, Yl[idx[sl]], hostile[sl].astype(LD), X0[u].astype(LD), SWEEPS)
    return want, amp, frozenset(subBad)


def bad_device(k, vals, Y, shard=BSHARD):
    ptr, idx, _, _, _, X0 = bad_inputs(k)
    dev = ycnr_als.AlsDevice(k, BSOLVED, BM, userFactReg=LAM[0], itemFactReg=LAM[1], chunkRatings=BCHUNK)
    dev.set_ratings(0, ptr, idx, vals, *shard)
    dev.set_factors(1, Y)
    dev.set_factors(0, X0)
    return dev


def run_step(entry, k, vals, Y, shard=BSHARD):
    dev = bad_device(k, vals, Y, shard)
    bad, _ = dev.step_implicit(0, ALPHA, **STEPS[entry])
    got = dev.get_factors(0)
    dev.destroy()
    return bad, got


def run_fold(k, vals, Y, primal_only=False):
    ptr, idx, _, _, _, _ = bad_inputs(k)
    dev = bad_device(k, vals, Y)
    rows, status, _ = dev.fold_in_implicit(0, ALPHA, ptr, idx, vals, primal_only=primal_only)
    dev.destroy()
    return rows, status


def poisoned(Y):
    Y = Y.copy()
    Y[BM - 1, 3] = np.nan  # a fixed row that no observation names: only G carries it
    return Y


@pytest.mark.parametrize("entry", ["exact", "cg", "sub"])
def test_bad_rows_are_counted_and_zeroed(entry):
    _, _, _, hostile, Y, X0 = bad_inputs(BK)
    want, amp, subBad = bad_facts()
    flagged = {"exact": {ROW_A, ROW_B}, "cg": {ROW_B}, "sub": set(subBad)}[entry]
    assert ROW_B in flagged and (entry == "cg" or ROW_A in flagged)
    bad, got = run_step(entry, BK, hostile, Y)
    assert bad == len(flagged), (bad, sorted(flagged))
    assert not got[sorted(flagged)].any() and not got[BEMPTY].any()
    assert np.array_equal(got[OUTSIDE], X0[OUTSIDE])
    rest = [u for u in LIVE if u not in flagged]  # row C among them, and row A for cg: it follows the method, stop rule included
    judge(f"bad rows {entry}", F32, got[rest], want[entry][rest], amp[rest])


FOLD_STATUS = [2 if u == BEMPTY else 1 if u in HOSTILE else 0 for u in range(BSOLVED)]
FOLD_REST = [u for u in range(BSOLVED) if FOLD_STATUS[u] == 0]


@pytest.mark.parametrize("primal_only", [False, True])  # rows A and B are primal by rule either way
def test_fold_in_status_of_bad_rows(primal_only):
    _, _, _, hostile, Y, _ = bad_inputs(BK)
    want, amp, _ = bad_facts()
    rows, status = run_fold(BK, hostile, Y, primal_only)
    assert list(status) == FOLD_STATUS
    assert not rows[HOSTILE + [BEMPTY]].any()
    judge(f"bad rows fold-in primal_only={primal_only}", F32, rows[FOLD_REST], want["exact"][FOLD_REST], amp[FOLD_REST])


def test_recommend_for_observations_gives_bad_rows_nothing():
    ptr, idx, _, hostile, Y, _ = bad_inputs(BK)
    dev = bad_device(BK, hostile, Y)
    rows, status, _ = dev.fold_in_implicit(0, ALPHA, ptr, idx, hostile)
    ids, _, cnt, rows2, status2, _ = dev.recommend_for_observations(ALPHA, ptr, idx, hostile, np.zeros(BSOLVED + 1, np.int64), np.zeros(0, np.int32),
                                                                    minRecommendRating=-1e30, limit=10)
    dev.destroy()
    assert list(status2) == FOLD_STATUS and np.array_equal(rows2, rows) and np.array_equal(status2, status)
    none = HOSTILE + [BEMPTY]
    assert (cnt[none] == 0).all() and (ids[none] == -1).all()
    assert (cnt[FOLD_REST] == 9).all() and (ids[FOLD_REST][:, :9] >= 0).all()  # limit - 1 items, as the reference serves them


@pytest.mark.parametrize("entry", ["exact", "cg", "sub", "fold"])
def test_bad_rows_leave_their_neighbours_bits_alone(entry):
    """the same request on two fresh handles, rows A and B hostile / benign: every other row has the same bits"""
    _, _, benign, hostile, Y, X0 = bad_inputs(BK)
    if entry == "fold":
        (foul, st), (fair, st2) = run_fold(BK, hostile, Y), run_fold(BK, benign, Y)
        assert list(st) == FOLD_STATUS and list(st2) == [2 if u == BEMPTY else 0 for u in range(BSOLVED)]
    else:
        (bad, foul), (bad2, fair) = run_step(entry, BK, hostile, Y), run_step(entry, BK, benign, Y)
        assert bad > 0 and bad2 == 0
    others = [u for u in range(BSOLVED) if u not in HOSTILE]
    assert np.array_equal(foul[others], fair[others])
    assert fair[HOSTILE].all(axis=1).all() and not np.array_equal(fair[LIVE], X0[LIVE])  # (the benign run did solve them)


@pytest.mark.parametrize("entry", ["cg", "sub"])
def test_bits_do_not_depend_on_the_batch(entry):
    """the same CSR as shard [1, 35) and as shard [8, 27): other rows share the 16-row batches of rows 8 .. 26, bad ones included"""
    _, _, _, hostile, Y, X0 = bad_inputs(BK)
    _, wide = run_step(entry, BK, hostile, Y)
    bad, narrow = run_step(entry, BK, hostile, Y, (8, 27))
    assert bad >= 1 and ROW_A < 27 and ROW_B < 27
    assert np.array_equal(wide[8:27], narrow[8:27]) and not np.array_equal(narrow[8:27], X0[8:27])
    assert np.array_equal(narrow[:8], X0[:8]) and np.array_equal(narrow[27:], X0[27:])


@pytest.mark.parametrize("entry,k", [("exact", BK), ("cg", BK), ("sub", BK), ("sub", 144)])  # 144: the wide Gramian
def test_a_poisoned_gramian_fails_every_row(entry, k):
    _, _, benign, _, Y, X0 = bad_inputs(k)
    bad, got = run_step(entry, k, benign, poisoned(Y))
    assert bad == len(LIVE), bad
    assert not got[BSHARD[0]:BSHARD[1]].any()  # the empty row too
    assert np.array_equal(got[OUTSIDE], X0[OUTSIDE])


@pytest.mark.parametrize("primal_only", [False, True])
def test_a_poisoned_gramian_fails_every_fold_in_row(primal_only):
    _, _, benign, _, Y, _ = bad_inputs(BK)
    rows, status = run_fold(BK, benign, poisoned(Y), primal_only)
    assert list(status) == [2 if u == BEMPTY else 1 for u in range(BSOLVED)]
    assert not rows.any()


@pytest.mark.parametrize("entry", ["exact", "cg", "sub"])
def test_the_next_call_forgets_the_bad_rows(entry):
    """a call with bad rows (hostile values AND a poisoned G), then the inputs repaired on the same handle: no bad row is left in
    the count, and the result has the bits of a fresh handle"""
    ptr, idx, benign, hostile, Y, X0 = bad_inputs(BK)
    dev = bad_device(BK, hostile, poisoned(Y))
    assert dev.step_implicit(0, ALPHA, **STEPS[entry])[0] == len(LIVE)
    dev.set_ratings(0, ptr, idx, benign, *BSHARD)
    dev.set_factors(1, Y)
    dev.set_factors(0, X0)
    bad, _ = dev.step_implicit(0, ALPHA, **STEPS[entry])
    got = dev.get_factors(0)
    dev.destroy()
    badFresh, fresh = run_step(entry, BK, benign, Y)
    assert bad == 0 and badFresh == 0
    assert np.array_equal(got, fresh) and fresh[LIVE].all(axis=1).all()


# ---------------------------------------------------------------------------------------------- 3. misaligned bound matrices
def offset_view(a):
    """`a` on the device as a view that starts one element into its allocation: 4 or 8 bytes past a 16-byte boundary"""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a))
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device="cuda")
    view = buf[1:].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and buf.data_ptr() % 16 == 0 and view.data_ptr() % 16 == a.itemsize
    return view


@pytest.mark.parametrize("entry", ["exact", "cg", "sub", "fold"])
@pytest.mark.parametrize("dt", [F32, F64])
def test_misaligned_bound_matrices_give_the_same_bits(dt, entry):
    """k = 20 takes the 16-byte Gramian loads for an aligned fixed matrix and the element loads for this one: G's bits depend on
    the row count alone, so the two results are the same.  Both sides are bound; every other kernel reads them by elements."""
    import torch
    ptr, idx, vals, Y, X0 = sub_inputs(20, 0)
    seen = []
    for bind in (False, True):
        dev = sub_device(dt, 20, 0, ptr, idx, vals, Y, X0)
        if bind:
            fixed, solved = offset_view(Y.astype(dt)), offset_view(X0.astype(dt))
            torch.cuda.synchronize()
            dev.bind_factors(1, fixed)
            dev.bind_factors(0, solved)
        if entry == "fold":
            rows, status, _ = dev.fold_in_implicit(0, ALPHA, ptr, idx, vals.astype(dt), storeIds=np.arange(len(ptr) - 1, dtype=np.int32))
            out = [rows, status]
        else:
            out = [np.array(dev.step_implicit(0, ALPHA, **STEPS[entry])[0])]
        out.append(dev.get_factors(0))
        if bind:  # solved in place, in the caller's memory; the fixed side is only read
            assert np.array_equal(solved.cpu().numpy(), out[-1]) and np.array_equal(fixed.cpu().numpy(), Y.astype(dt))
        dev.destroy()
        seen.append(out)
    for a, b in zip(*seen):
        assert np.array_equal(a, b)
    assert seen[0][0].size and not np.array_equal(seen[0][-1][1:35], X0[1:35].astype(dt))
