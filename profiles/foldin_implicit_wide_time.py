"""Time of ycnr_als_fold_in_implicit_wide.  (1) k = 100 (the ml1m shape of profiles/foldin_implicit_time.py, its requests of 1, 256
and 16 384 new users of 8 and of 24 observations): the new entry beside ycnr_als_fold_in_implicit by its default route and with
YCNR_FOLD_PRIMAL_ONLY, the three alternating in one process on one handle.  (2) The new entry alone at k = 256 and 512 against
20 000 items, the same user counts with 8, 24 and 100 observations.  Every route is warmed up; prints and writes
profiles/foldin_implicit_wide_time.json: median (min .. max) of msOut3 = {G + factor, rows, total} per route.
  python profiles/foldin_implicit_wide_time.py [compare] [alone]"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "you-can-not-recommend_amd", "python"))
from ycnr_als import AlsDevice  # noqa: E402
from ycnr_als.data import init_factors  # noqa: E402

ALPHA, ITERS, WARM = 40.0, 10, 3


def stats(ms):
    ms = np.array(ms)
    return {"median": [float(v) for v in np.median(ms, axis=0)], "min": [float(v) for v in ms.min(axis=0)], "max": [float(v) for v in ms.max(axis=0)]}


def request(rng, items, users, n, mx):
    ptr = np.arange(users + 1, dtype=np.int64) * n
    idx = np.sort(rng.integers(0, items, (users, n)), axis=1).astype(np.int32).reshape(-1)  # (a repeated id is a repeated observation)
    return ptr, idx, rng.integers(1, mx + 1, users * n).astype(np.float32)


def run(items, k, mx, observations, compare):
    dev = AlsDevice(k, 1, items)
    dev.set_factors("byItem", init_factors(items, k, 2))
    rng = np.random.default_rng(7)
    routes = {"wide": lambda *a: dev.fold_in_implicit_wide("byUser", ALPHA, *a)}
    if compare:
        routes["dual"] = lambda *a: dev.fold_in_implicit("byUser", ALPHA, *a)
        routes["primal"] = lambda *a: dev.fold_in_implicit("byUser", ALPHA, *a, primal_only=True)
    out = []
    for users in (1, 256, 16384):
        for n in observations:
            req = request(rng, items, users, n, mx)
            ms, bad = {r: [] for r in routes}, 0
            for it in range(WARM + ITERS):
                for name, call in routes.items():
                    _, status, t = call(*req)
                    bad += int((status != 0).sum())
                    if it >= WARM:
                        ms[name].append(t)
            res = {"items": items, "k": k, "alpha": ALPHA, "users": users, "observations": n, "iterations": ITERS, "badRows": bad}
            res.update({name + "_gram_rows_total_ms": stats(v) for name, v in ms.items()})
            print(json.dumps(res), flush=True)
            out.append(res)
    dev.destroy()
    return out


if __name__ == "__main__":
    what = sys.argv[1:] or ["compare", "alone"]
    res = []
    if "compare" in what:
        res += run(3883, 100, 5, (8, 24), True)
    if "alone" in what:
        for k in (256, 512):
            res += run(20_000, k, 10, (8, 24, 100), False)
    with open(os.path.join(ROOT, "profiles", "foldin_implicit_wide_time.json"), "w") as f:
        json.dump(res, f, indent=1)
