"""Time of ycnr_als_fold_in_implicit by its default route (rows of <= 32 observations in dual form) beside YCNR_FOLD_PRIMAL_ONLY
(every row by the exact k x k solve) on the same handle and request: the item matrices of two shapes of bench.py's table as the
fixed side, requests of 1, 256 and 16 384 new users of 8 and of 24 observations.  Both routes are warmed up, then 10 calls of each
alternate in one process; prints and writes profiles/foldin_implicit_time.json: median (min .. max) of msOut3 = {G + factor,
rows, total} per route, and the ratios dual / primal.
  python profiles/foldin_implicit_time.py [ml1m c3]"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "you-can-not-recommend_amd", "python"))
from ycnr_als import AlsDevice  # noqa: E402
from ycnr_als.data import init_factors  # noqa: E402

# (items, k, max_rating) as in bench.py's WORKLOADS
SHAPES = {"ml1m": (3883, 100, 5), "c3": (20_000, 64, 10)}
ALPHA, ITERS, WARM = 40.0, 10, 3


def stats(ms):
    ms = np.array(ms)
    return {"median": [float(v) for v in np.median(ms, axis=0)], "min": [float(v) for v in ms.min(axis=0)], "max": [float(v) for v in ms.max(axis=0)]}


def run(name):
    items, k, mx = SHAPES[name]
    dev = AlsDevice(k, 1, items)
    dev.set_factors("byItem", init_factors(items, k, 2))
    rng = np.random.default_rng(7)
    out = []
    for users in (1, 256, 16384):
        for n in (8, 24):
            ptr = np.arange(users + 1, dtype=np.int64) * n
            idx = np.sort(rng.integers(0, items, (users, n)), axis=1).astype(np.int32).reshape(-1)  # (a repeated id is a repeated observation)
            vals = rng.integers(1, mx + 1, users * n).astype(np.float32)
            ms, bad = {False: [], True: []}, 0
            for it in range(WARM + ITERS):
                for primal in (False, True):
                    _, status, t = dev.fold_in_implicit("byUser", ALPHA, ptr, idx, vals, primal_only=primal)
                    bad += int((status != 0).sum())
                    if it >= WARM:
                        ms[primal].append(t)
            d, p = stats(ms[False]), stats(ms[True])
            res = {"shape": name, "items": items, "k": k, "alpha": ALPHA, "users": users, "observations": n, "iterations": ITERS, "badRows": bad,
                   "dual_gram_rows_total_ms": d, "primal_gram_rows_total_ms": p,
                   "dual_over_primal_rows": d["median"][1] / p["median"][1], "dual_over_primal_total": d["median"][2] / p["median"][2]}
            print(json.dumps(res), flush=True)
            out.append(res)
    dev.destroy()
    return out


if __name__ == "__main__":
    res = [r for n in (sys.argv[1:] or ["ml1m", "c3"]) for r in run(n)]
    with open(os.path.join(ROOT, "profiles", "foldin_implicit_time.json"), "w") as f:
        json.dump(res, f, indent=1)
