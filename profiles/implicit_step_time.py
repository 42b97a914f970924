"""Time of the implicit half-step (ycnr_als_step_implicit) beside the explicit one on the same handle and ratings, at two shapes
of bench.py's table.  Both paths are warmed up, then 10 explicit and 10 implicit iterations alternate in one process; prints and
writes profiles/implicit_step_time.json: median ms per half-step and side, the spread (min .. max), and the median msOut3.
With --cg-steps N the conjugate-gradient half-step (ycnr_als_step_implicit_cg, N steps) alternates with the two in the same
process, and the result goes to profiles/implicit_cg_step_time.json instead (the other file stays).
With --sweeps N the subspace half-step (ycnr_als_step_implicit_sub, N sweeps) is a further party beside explicit, exact and
CG(3) at ml1m and c3, and beside the explicit one alone at c3k256, where no other implicit entry exists; it also records the
Hu-Koren-Volinsky objective at the ml1m shape after 5 iterations from one seeded start for exact, CG(3) and sub(1).  That result
goes to profiles/implicit_sub_step_time.json.
  python profiles/implicit_step_time.py [--cg-steps N | --sweeps N] [ml1m c3]"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "you-can-not-recommend_amd", "python"))
from ycnr_als import AlsDevice  # noqa: E402
from ycnr_als.data import init_factors, synth_ratings  # noqa: E402

# (users, items, nnz, k, max_rating) as in bench.py's WORKLOADS
SHAPES = {"ml1m": (6040, 3883, 1_000_209, 100, 5), "c3": (200_000, 20_000, 20_000_000, 64, 10),
          "c3k256": (200_000, 20_000, 20_000_000, 256, 10)}
ALPHA, ITERS = 40.0, 10


def stats(ms):
    return {"median": float(np.median(ms)), "min": float(np.min(ms)), "max": float(np.max(ms))}


def run(name, cg_steps=None, sweeps=None):
    users, items, nnz, k, mx = SHAPES[name]
    old = k <= 128  # the exact and CG entries stop there
    bu, bi = synth_ratings(users, items, nnz, max_rating=mx, device="cuda")
    dev = AlsDevice(k, users, items)
    dev.set_ratings("byUser", bu.rowPtr, bu.indx, bu.vals)
    dev.set_ratings("byItem", bi.rowPtr, bi.indx, bi.vals)
    dev.set_factors("byUser", init_factors(users, k, 1))
    dev.set_factors("byItem", init_factors(items, k, 2))
    for _ in range(3):  # warm-up of both paths (the explicit one captures its graph on the third half-step of a small upload)
        for side in (0, 1):
            dev.step(side)
            if old:
                dev.step_implicit(side, ALPHA)
            if cg_steps and old:
                dev.step_implicit(side, ALPHA, cg_steps)
            if sweeps:
                dev.step_implicit(side, ALPHA, sweeps=sweeps)
    ex, im, parts, bad = ([], []), ([], []), ([], []), 0
    cg, cgparts = ([], []), ([], [])
    sub, subparts = ([], []), ([], [])
    for _ in range(ITERS):
        for side in (0, 1):
            ex[side].append(dev.step(side).totalMs)
        for side in (0, 1) if old else ():
            b, ms = dev.step_implicit(side, ALPHA)
            bad += b
            im[side].append(ms[2])
            parts[side].append(ms)
        for side in (0, 1) if sweeps else ():
            b, ms = dev.step_implicit(side, ALPHA, sweeps=sweeps)
            bad += b
            sub[side].append(ms[2])
            subparts[side].append(ms)
        for side in (0, 1) if cg_steps and old else ():
            b, ms = dev.step_implicit(side, ALPHA, cg_steps)
            bad += b
            cg[side].append(ms[2])
            cgparts[side].append(ms)
    out = {"shape": name, "users": users, "items": items, "nnz": int(bu.nnz), "k": k, "alpha": ALPHA, "iterations": ITERS, "badRows": int(bad)}
    for side, sn in ((0, "byUser"), (1, "byItem")):
        out[sn] = {"explicit_ms": stats(ex[side])}
        if old:
            out[sn].update({"implicit_ms": stats(im[side]),
                            "implicit_gram_rows_total_ms": [float(v) for v in np.median(np.array(parts[side]), axis=0)],
                            "implicit_over_explicit": float(np.median(im[side]) / np.median(ex[side]))})
        if sweeps:
            out[sn].update({"sweeps": sweeps, "sub_ms": stats(sub[side]),
                            "sub_gram_rows_total_ms": [float(v) for v in np.median(np.array(subparts[side]), axis=0)],
                            "sub_over_explicit": float(np.median(sub[side]) / np.median(ex[side]))})
        if cg_steps and old:
            out[sn].update({"cg_steps": cg_steps, "cg_ms": stats(cg[side]),
                            "cg_gram_rows_total_ms": [float(v) for v in np.median(np.array(cgparts[side]), axis=0)],
                            "cg_over_explicit": float(np.median(cg[side]) / np.median(ex[side])),
                            "exact_over_cg": float(np.median(im[side]) / np.median(cg[side]))})
    dev.destroy()
    print(json.dumps(out), flush=True)
    return out


def quality(iters=5):
    """The Hu-Koren-Volinsky objective at the ml1m shape after `iters` iterations from one seeded start, per trainer."""
    users, items, nnz, k, mx = SHAPES["ml1m"]
    bu, bi = synth_ratings(users, items, nnz, max_rating=mx, device="cuda")
    ptr, idx, vals = (np.asarray(a.cpu()) if hasattr(a, "cpu") else np.asarray(a) for a in (bu.rowPtr, bu.indx, bu.vals))
    C1 = np.zeros((users, items))  # alpha r on the observations
    C1[np.repeat(np.arange(users), np.diff(ptr)), idx] = ALPHA * vals
    out = {"shape": "ml1m", "alpha": ALPHA, "iterations": iters, "lambda": 0.05}
    for name, kw in (("exact", {}), ("cg3", {"cg_steps": 3}), ("sub1", {"sweeps": 1})):
        dev = AlsDevice(k, users, items, userFactReg=0.05, itemFactReg=0.05)
        dev.set_ratings("byUser", bu.rowPtr, bu.indx, bu.vals)
        dev.set_ratings("byItem", bi.rowPtr, bi.indx, bi.vals)
        dev.set_factors("byUser", init_factors(users, k, 1))
        dev.set_factors("byItem", init_factors(items, k, 2))
        for _ in range(iters):
            for side in (0, 1):
                dev.step_implicit(side, ALPHA, **kw)
        X, Y = dev.get_factors(0).astype(np.float64), dev.get_factors(1).astype(np.float64)
        dev.destroy()
        out[name] = float(((1.0 + C1) * ((C1 > 0) - X @ Y.T) ** 2).sum() + 0.05 * ((X * X).sum() + (Y * Y).sum()))
    print(json.dumps(out), flush=True)
    return out


if __name__ == "__main__":
    args, steps, sweeps = sys.argv[1:], None, None
    if args[:1] == ["--cg-steps"]:
        steps, args = int(args[1]), args[2:]
    if args[:1] == ["--sweeps"]:
        sweeps, steps, args = int(args[1]), 3, args[2:]
    res = [run(n, steps, sweeps) for n in (args or (["ml1m", "c3", "c3k256"] if sweeps else ["ml1m", "c3"]))]
    if sweeps:
        res.append({"quality": quality()})
    name = "implicit_sub_step_time.json" if sweeps else "implicit_cg_step_time.json" if steps else "implicit_step_time.json"
    with open(os.path.join(ROOT, "profiles", name), "w") as f:
        json.dump(res, f, indent=1)
