"""The NodeJS host's EmfLord.recommendItemsForRatings / EmfLord.foldIn against the Python host's, bit for bit: both warm-start
from the same factor files and train through the same library (as tests/test_gpu_recommend_resident.py does for
recommendItemsForUsers), so their factor matrices -- and every row folded in against them -- are the same bits."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from test_gpu_recommend_resident import split_dataset

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
ADDON = os.path.join(ROOT, "you-can-not-recommend_amd", "addon", "ycnr_als.node")


@pytest.mark.skipif(shutil.which("node") is None or not os.path.exists(ADDON), reason="node or the built addon is missing")
def test_js_host_folds_in_like_the_python_host(tmp_path):
    import ycnr_als
    from ycnr_als.emf import EmfLord
    assert ycnr_als._lib.load().ycnr_device_count() >= 1
    ds, bu, user, typ, U, V = split_dataset(6, 60, 45, np.float32)
    pydir, jsdir = tmp_path / "py", tmp_path / "js"
    opts = {"factorsCount": 8, "trainIters": 2, "useDoublePrecision": False, "dbType": "ml", "ratingsInPortionForRmse": 30,
            "numThreadsForTrain": {"als": 2}}
    seedlord = EmfLord(options=dict(opts, dataDir=str(jsdir), trainIters=0))
    seedlord.prepareToTrain(ds, U, V)
    seedlord.train()  # zero iterations: writes the starting factors as ml_factors_ready
    seedlord.destroy()
    ratings = [[[5, 4.0], [12, 2.0], [45, 5.0], [1, 3.0]], [], [[7, 1.0]], [[i, float(1 + i % 5)] for i in range(1, 41)]]
    unrated = [None, [0, 1], None, [44]]
    item_rows = [[[1, 5.0], [60, 1.0], [17, 4.0]]]
    lord = EmfLord(options=dict(opts, dataDir=str(pydir)))
    try:
        lord.prepareToTrain(ds, U, V)
        lord.train()
        recs = lord.recommendItemsForRatings(ratings, limit=6, minRecommendRating=2.5, unratedItems=unrated)
        users = lord.foldIn("byUser", ratings)
        item = lord.foldIn("byItem", item_rows, storeIds=[44])
        stored = lord.foldIn("byUser", ratings[:1], storeIds=[3])
        after = lord.recommendItemsForUsers([3], limit=6, minRecommendRating=2.5)
    finally:
        lord.destroy()
    assert any(len(r) > 1 for r in recs) and recs[1] == [] and users[1].tolist() == [0, 2, 0, 0] and len(after[0]) > 0
    inp = {"dir": str(jsdir), "k": 8, "iters": 2, "rip": 30, "threads": 2, "useDoublePrecision": False, "users": bu.rows, "items": bu.cols,
           "user": user.tolist(), "item": bu.indx.tolist(), "rating": bu.vals.tolist(), "type": typ.tolist(),
           "ratings": ratings, "unratedItems": unrated, "limit": 6, "minRecommendRating": 2.5, "itemRows": item_rows, "itemStore": [44],
           "userStore": [3]}
    (tmp_path / "in.json").write_text(json.dumps(inp))
    r = subprocess.run(["node", os.path.join(HERE, "js", "foldin_gpu.js"), str(tmp_path / "in.json")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    out = json.loads(r.stdout.strip().splitlines()[-1])
    for got, want in ((out["recs"], recs), (out["after"], after)):
        assert [[x["id"] for x in rec] for rec in got] == [[x["id"] for x in rec] for rec in want]
        assert [[x["predict"] for x in rec] for rec in got] == [[x["predict"] for x in rec] for rec in want]
    for got, want in ((out["users"], users), (out["item"], item), (out["stored"], stored)):
        assert got["status"] == want[1].tolist()
        assert np.array_equal(np.array(got["rows"], np.float32).reshape(want[0].shape), want[0])
    assert "itemStepSharding" in out["bandsError"] and out["bandsUsers"] == [0, 2, 0, 0]
