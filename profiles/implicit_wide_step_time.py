"""Time of the exact implicit half-step up to 512 factors (ycnr_als_step_implicit_wide) beside the entries it can be compared
with, on one handle and one set of ratings per shape, as profiles/implicit_step_time.py does: every party is warmed up, then
the parties alternate for ITERS iterations in one process; per party and side the median ms of msOut3's total (HIP events
around the kernels), min .. max, and the median split {G and the factorisation of M, rows, total} for the wide entry.
  c3 at k = 256: wide against the subspace half-step (ycnr_als_step_implicit_sub) with 1 and 3 sweeps
  c3 at k = 128: wide against the exact half-step of the narrow path (ycnr_als_step_implicit)
Writes profiles/implicit_wide_step_time.json.
  python profiles/implicit_wide_step_time.py [c3k256 c3k128]"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "you-can-not-recommend_amd", "python"))
from ycnr_als import AlsDevice  # noqa: E402
from ycnr_als.data import init_factors, synth_ratings  # noqa: E402

# (users, items, nnz, k, max_rating): the c3 shape of bench.py's table at two k
SHAPES = {"c3k256": (200_000, 20_000, 20_000_000, 256, 10), "c3k128": (200_000, 20_000, 20_000_000, 128, 10)}
ALPHA, WARMUP, ITERS = 40.0, 2, 5


def stats(ms):
    return {"median": float(np.median(ms)), "min": float(np.min(ms)), "max": float(np.max(ms))}


def run(name):
    users, items, nnz, k, mx = SHAPES[name]
    bu, bi = synth_ratings(users, items, nnz, max_rating=mx, device="cuda")
    dev = AlsDevice(k, users, items)
    dev.set_ratings("byUser", bu.rowPtr, bu.indx, bu.vals)
    dev.set_ratings("byItem", bi.rowPtr, bi.indx, bi.vals)
    start = init_factors(users, k, 1), init_factors(items, k, 2)
    parties = {"wide": lambda s: dev.step_implicit_wide(s, ALPHA)}
    if k <= 128:
        parties["exact"] = lambda s: dev.step_implicit(s, ALPHA)
    else:
        parties["sub1"] = lambda s: dev.step_implicit(s, ALPHA, sweeps=1)
        parties["sub3"] = lambda s: dev.step_implicit(s, ALPHA, sweeps=3)
    times = {p: ([], []) for p in parties}
    split, bad = ([], []), 0
    for it in range(WARMUP + ITERS):
        for p, step in parties.items():  # every party solves the same system: both matrices go back to the start
            for side in (0, 1):
                dev.set_factors("byUser", start[0])
                dev.set_factors("byItem", start[1])
                b, ms = step(side)
                if it >= WARMUP:
                    bad += b
                    times[p][side].append(ms[2])
                    if p == "wide":
                        split[side].append(ms)
    out = {"shape": name, "users": users, "items": items, "nnz": int(bu.nnz), "k": k, "alpha": ALPHA, "warmup": WARMUP, "iterations": ITERS,
           "badRows": int(bad)}
    for side, sn in ((0, "byUser"), (1, "byItem")):
        out[sn] = {p + "_ms": stats(times[p][side]) for p in parties}
        out[sn]["wide_gram_rows_total_ms"] = [float(v) for v in np.median(np.array(split[side]), axis=0)]
    dev.destroy()
    print(json.dumps(out), flush=True)
    return out


if __name__ == "__main__":
    res = [run(n) for n in (sys.argv[1:] or ["c3k256", "c3k128"])]
    with open(os.path.join(ROOT, "profiles", "implicit_wide_step_time.json"), "w") as f:
        json.dump(res, f, indent=1)
