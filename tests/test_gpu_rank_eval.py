"""ycnr_als_rank_eval: for every held-out pair (u, i), the number of competing items the resident factors place ahead of i.

The reference is `reference` below: scores in long double, the total order of ycnr_als_recommend (higher score first, equal
scores by lower id), skipped items out.  Integer-valued factors make every score exact in any summation order, so there the
device must equal it; on random floats the device must equal the recommend path bit for bit and lie inside the bracket that
the rounding of a k-term dot product allows.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPES = [(3, 50, 8), (17, 17, 7), (40, 1234, 100), (20, 700, 256)]
DTYPES = [np.float32, np.float64]


@pytest.fixture(scope="module")
def als():
    import ycnr_als
    assert ycnr_als._lib.load().ycnr_device_count() >= 1
    return ycnr_als


def scores_and_competitors(U, V, req, q):
    uid, _, _, sptr, sids = req
    s = V.astype(np.longdouble) @ U[uid[q]].astype(np.longdouble)
    skip = sids[sptr[q]:sptr[q + 1]]
    comp = np.ones(len(V), bool)
    comp[skip[(skip >= 0) & (skip < len(V))]] = False
    return s, comp


def reference(U, V, req):
    ranks, cand, ids = [], [], np.arange(len(V))
    for q in range(len(req[0])):
        s, comp = scores_and_competitors(U, V, req, q)
        cand.append(comp.sum())
        for i in req[2][req[1][q]:req[1][q + 1]]:
            ranks.append(int((comp & ((s > s[i]) | ((s == s[i]) & (ids < i)))).sum()) if comp[i] else -1)
    return np.array(ranks, np.int32), np.array(cand, np.int32)


def csr(lists):
    ptr = np.zeros(len(lists) + 1, np.int64)
    ptr[1:] = np.cumsum([len(x) for x in lists])
    return ptr, np.concatenate(lists + [np.zeros(0, np.int32)]).astype(np.int32)


def make_request(users, items, seed, counts):
    """Request users 0, 1, ... hold counts[.] held-out items (then 1 .. 11); user ids repeat; request user 1 has an empty skip
    list, user 2's holds ids outside the catalogue, and the first held-out item of the last user is in its skip list too."""
    rng = np.random.default_rng(seed)
    counts = [c for c in counts if c <= items]
    n = max(users, len(counts)) + 2
    counts += list(rng.integers(1, min(12, items + 1), n - len(counts)))
    uid = (rng.permutation(n) % users).astype(np.int32)
    tests = [np.sort(rng.choice(items, c, replace=False)).astype(np.int32) for c in counts]
    skips = [np.sort(rng.choice(items, rng.integers(0, items // 3 + 1), replace=False)).astype(np.int32) for _ in range(n)]
    skips[1] = np.zeros(0, np.int32)
    skips[2] = np.concatenate([[-2], skips[2], [items, items + 5]]).astype(np.int32)
    skips[-1] = np.union1d(skips[-1], tests[-1][:1]).astype(np.int32)
    return (uid,) + csr(tests) + csr(skips)


def device_with(als, U, V):
    dev = als.AlsDevice(U.shape[1], U.shape[0], V.shape[0], useDoublePrecision=(U.dtype == np.float64))
    dev.set_factors("byUser", U)
    dev.set_factors("byItem", V)
    return dev


def run(als, U, V, req):
    dev = device_with(als, U, V)
    try:
        return dev.rank_eval(*req)[:2]
    finally:
        dev.destroy()


def floats(users, items, k, dt, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((users, k)) * 0.8).astype(dt), (rng.standard_normal((items, k)) * 0.8).astype(dt)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("users,items,k", SHAPES)
def test_exact_on_integer_valued_factors(als, users, items, k, dt):
    rng = np.random.default_rng(k)
    U, V = rng.integers(-2, 3, (users, k)).astype(dt), rng.integers(-2, 3, (items, k)).astype(dt)
    req = make_request(users, items, 7 + k, [0, 1, 63, 64, 65, 130])
    ranks, cand = run(als, U, V, req)
    want_ranks, want_cand = reference(U, V, req)
    assert (want_ranks == -1).any()
    assert np.array_equal(cand, want_cand)
    assert np.array_equal(ranks, want_ranks)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("users,items,k", [(40, 1234, 100), (5, 3000, 20)])
def test_same_bits_as_the_recommend_path_whatever_the_grid(als, users, items, k, dt):
    U, V = floats(users, items, k, dt, 31 + k)
    req = make_request(users, items, 5 + k, [0, 1, 64, 65, 130])
    uid, tptr, tids, sptr, sids = req
    dev = device_with(als, U, V)
    try:
        ranks, _, _ = dev.rank_eval(*req)
        few = dev.rank_eval(uid[:3], tptr[:4], tids[:tptr[3]], sptr[:4], sids[:sptr[3]])[0]  # one slot group: another grid
        lists = dev.recommend(uid, sptr, sids, globalAvgShift=0.0, minRecommendRating=-1e300, limit=4096)[0]
    finally:
        dev.destroy()
    for q in range(len(uid)):
        for p in range(tptr[q], tptr[q + 1]):
            at = np.flatnonzero(lists[q] == tids[p])
            assert ranks[p] == (at[0] if len(at) else -1), (q, p)
    assert np.array_equal(few, ranks[:tptr[3]])


@pytest.mark.parametrize("dt,users,items,k", [(np.float64,) + s for s in SHAPES] + [(np.float32, 17, 300, 20), (np.float32, 33, 2000, 7)])
def test_random_floats_inside_the_rounding_bracket(als, dt, users, items, k):
    U, V = floats(users, items, k, dt, 77 + k)
    rng = np.random.default_rng(k)
    req = make_request(users, items, 9 + k, list(rng.integers(1, min(12, items), users)))
    ranks, _ = run(als, U, V, req)
    lo, hi = [], []
    for q in range(len(req[0])):
        s, comp = scores_and_competitors(U, V, req, q)
        d = 2 * k * np.finfo(dt).eps * (np.abs(V).astype(np.longdouble) @ np.abs(U[req[0][q]]).astype(np.longdouble))
        for i in req[2][req[1][q]:req[1][q + 1]]:
            others = comp & (np.arange(items) != i)
            lo.append(int((others & (s - d > s[i] + d[i])).sum()) if comp[i] else -1)
            hi.append(int((others & (s + d >= s[i] - d[i])).sum()) if comp[i] else -1)
    lo, hi = np.array(lo), np.array(hi)
    print("brackets of width 0: %.4f, widest %d" % ((lo == hi).mean(), (hi - lo).max()))
    assert (lo == hi).mean() >= (1.0 if dt == np.float64 else 0.95)  # else the check below would be vacuous
    assert ((lo <= ranks) & (ranks <= hi)).all()


def test_refusals_leave_the_outputs_untouched(als):
    U, V = floats(6, 40, 8, np.float32, 1)
    dev = device_with(als, U, V)

    def call(uid, tptr, tids):
        a = [np.asarray(x, t) for x, t in ((uid, np.int32), (tptr, np.int64), (tids, np.int32), (np.zeros(len(uid) + 1), np.int64))]
        ranks, cand = np.full(8, 77, np.int32), np.full(8, 77, np.int32)
        rc = dev._L.ycnr_als_rank_eval(dev._h, len(uid), a[0].ctypes.data, a[1].ctypes.data, a[2].ctypes.data, a[3].ctypes.data, None,
                                       ranks.ctypes.data, cand.ctypes.data, None)
        return rc, ranks, cand
    try:
        for uid, tptr, tids in (([0, 1], [0, 2, 3], [5, 4, 1]), ([0, 1], [0, 2, 3], [4, 40, 1]), ([0, 6], [0, 2, 3], [4, 5, 1])):
            rc, ranks, cand = call(uid, tptr, tids)
            assert rc == als._lib.ERR_INVALID and (ranks == 77).all() and (cand == 77).all()
        assert call([], [0], [])[0] == als._lib.OK
        rc, ranks, cand = call([0, 1], [0, 2, 3], [4, 5, 1])
        assert rc == als._lib.OK and (ranks[:3] != 77).all() and (cand[:2] == 40).all()
    finally:
        dev.destroy()
