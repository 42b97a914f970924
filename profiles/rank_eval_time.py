"""Time of ycnr_als_rank_eval beside ycnr_als_recommend at limit = 20 for the same users and skip lists on the same handle: the
existing kernel that also streams the catalogue's scores once per user.  float32, one device, two shapes of bench.py's table.
The data set is synthetic: every user gets nnz / users distinct random items, split 90 / 10 per user; the train items are the
skip list, the rest are held out.  The factors are random (init_factors): the time of neither kernel depends on what they mean,
and the expected percentile rank of a random model, 0.5, is recorded as a sanity check.  Both calls are warmed up, then 10 of
each alternate in one process; prints and writes profiles/rank_eval_time.json: median and min .. max deviceMs and their ratio.
  python profiles/rank_eval_time.py [ml1m c3]"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "you-can-not-recommend_amd", "python"))
from ycnr_als import AlsDevice, ranking_metrics  # noqa: E402
from ycnr_als.data import init_factors  # noqa: E402

# (users, items, nnz, k) as in bench.py's WORKLOADS
SHAPES = {"ml1m": (6040, 3883, 1_000_209, 100), "c3": (200_000, 20_000, 20_000_000, 64)}
CALLS = 10


def stats(ms):
    return {"median": float(np.median(ms)), "min": float(np.min(ms)), "max": float(np.max(ms))}


def split_lists(users, items, nnz, seed):
    """(trainPtr, trainIds, testPtr, testIds): per user, every tenth of its distinct ascending items is held out"""
    rng = np.random.default_rng(seed)
    ids = np.sort(rng.integers(0, items, (users, max(2, nnz // users)), dtype=np.int32), axis=1)
    keep = np.ones(ids.shape, bool)
    keep[:, 1:] = ids[:, 1:] != ids[:, :-1]
    held = keep & ((np.cumsum(keep, axis=1) % 10) == 0)
    out = []
    for m in (keep & ~held, held):
        ptr = np.zeros(users + 1, np.int64)
        ptr[1:] = np.cumsum(m.sum(axis=1))
        out += [ptr, ids[m]]
    return out


def run(name):
    users, items, nnz, k = SHAPES[name]
    sptr, sids, tptr, tids = split_lists(users, items, nnz, 7)
    uid = np.arange(users, dtype=np.int32)
    dev = AlsDevice(k, users, items)
    dev.set_factors("byUser", init_factors(users, k, 1))
    dev.set_factors("byItem", init_factors(items, k, 2))
    for _ in range(2):
        ranks, cand, _ = dev.rank_eval(uid, tptr, tids, sptr, sids)
        dev.recommend(uid, sptr, sids, globalAvgShift=0.0, minRecommendRating=-1e300, limit=20)
    rk, rc = [], []
    for _ in range(CALLS):
        rk.append(dev.rank_eval(uid, tptr, tids, sptr, sids)[2])
        rc.append(dev.recommend(uid, sptr, sids, globalAvgShift=0.0, minRecommendRating=-1e300, limit=20)[3])
    dev.destroy()
    m = ranking_metrics(ranks, cand, tptr)
    out = {"shape": name, "users": users, "items": items, "k": k, "dtype": "float32", "held_out_pairs": int(tptr[-1]), "skip_ids": int(sptr[-1]),
           "calls": CALLS, "rank_eval_ms": stats(rk), "recommend_limit20_ms": stats(rc), "rank_eval_over_recommend": float(np.median(rk) / np.median(rc)),
           "expected_percentile_rank_of_random_factors": m["expected_percentile_rank"], "skipped_pairs": m["skipped_pairs"]}
    print(json.dumps(out), flush=True)
    return out


if __name__ == "__main__":
    res = [run(n) for n in (sys.argv[1:] or ["ml1m", "c3"])]
    with open(os.path.join(ROOT, "profiles", "rank_eval_time.json"), "w") as f:
        json.dump(res, f, indent=1)
