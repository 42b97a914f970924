"""Time of the implicit half-step (ycnr_als_step_implicit) beside the explicit one on the same handle and ratings, at two shapes
of bench.py's table.  Both paths are warmed up, then 10 explicit and 10 implicit iterations alternate in one process; prints and
writes profiles/implicit_step_time.json: median ms per half-step and side, the spread (min .. max), and the median msOut3.
With --cg-steps N the conjugate-gradient half-step (ycnr_als_step_implicit_cg, N steps) alternates with the two in the same
process, and the result goes to profiles/implicit_cg_step_time.json instead (the other file stays).
  python profiles/implicit_step_time.py [--cg-steps N] [ml1m c3]"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "you-can-not-recommend_amd", "python"))
from ycnr_als import AlsDevice  # noqa: E402
from ycnr_als.data import init_factors, synth_ratings  # noqa: E402

# (users, items, nnz, k, max_rating) as in bench.py's WORKLOADS
SHAPES = {"ml1m": (6040, 3883, 1_000_209, 100, 5), "c3": (200_000, 20_000, 20_000_000, 64, 10)}
ALPHA, ITERS = 40.0, 10


def stats(ms):
    return {"median": float(np.median(ms)), "min": float(np.min(ms)), "max": float(np.max(ms))}


def run(name, cg_steps=None):
    users, items, nnz, k, mx = SHAPES[name]
    bu, bi = synth_ratings(users, items, nnz, max_rating=mx, device="cuda")
    dev = AlsDevice(k, users, items)
    dev.set_ratings("byUser", bu.rowPtr, bu.indx, bu.vals)
    dev.set_ratings("byItem", bi.rowPtr, bi.indx, bi.vals)
    dev.set_factors("byUser", init_factors(users, k, 1))
    dev.set_factors("byItem", init_factors(items, k, 2))
    for _ in range(3):  # warm-up of both paths (the explicit one captures its graph on the third half-step of a small upload)
        for side in (0, 1):
            dev.step(side)
            dev.step_implicit(side, ALPHA)
            if cg_steps:
                dev.step_implicit(side, ALPHA, cg_steps)
    ex, im, parts, bad = ([], []), ([], []), ([], []), 0
    cg, cgparts = ([], []), ([], [])
    for _ in range(ITERS):
        for side in (0, 1):
            ex[side].append(dev.step(side).totalMs)
        for side in (0, 1):
            b, ms = dev.step_implicit(side, ALPHA)
            bad += b
            im[side].append(ms[2])
            parts[side].append(ms)
        for side in (0, 1) if cg_steps else ():
            b, ms = dev.step_implicit(side, ALPHA, cg_steps)
            bad += b
            cg[side].append(ms[2])
            cgparts[side].append(ms)
    out = {"shape": name, "users": users, "items": items, "nnz": int(bu.nnz), "k": k, "alpha": ALPHA, "iterations": ITERS, "badRows": int(bad)}
    for side, sn in ((0, "byUser"), (1, "byItem")):
        out[sn] = {"explicit_ms": stats(ex[side]), "implicit_ms": stats(im[side]),
                   "implicit_gram_rows_total_ms": [float(v) for v in np.median(np.array(parts[side]), axis=0)],
                   "implicit_over_explicit": float(np.median(im[side]) / np.median(ex[side]))}
        if cg_steps:
            out[sn].update({"cg_steps": cg_steps, "cg_ms": stats(cg[side]),
                            "cg_gram_rows_total_ms": [float(v) for v in np.median(np.array(cgparts[side]), axis=0)],
                            "cg_over_explicit": float(np.median(cg[side]) / np.median(ex[side])),
                            "exact_over_cg": float(np.median(im[side]) / np.median(cg[side]))})
    dev.destroy()
    print(json.dumps(out), flush=True)
    return out


if __name__ == "__main__":
    args, steps = sys.argv[1:], None
    if args[:1] == ["--cg-steps"]:
        steps, args = int(args[1]), args[2:]
    res = [run(n, steps) for n in (args or ["ml1m", "c3"])]
    with open(os.path.join(ROOT, "profiles", "implicit_cg_step_time.json" if steps else "implicit_step_time.json"), "w") as f:
        json.dump(res, f, indent=1)
