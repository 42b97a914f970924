"""Ranking measures from the output of AlsDevice.rank_eval: plain numpy on the host, nothing here touches the device."""
import numpy as np


def ranking_metrics(ranks, candidates, testPtr, weights=None, n=10):
    """ranks [one per held-out pair], candidates [one per request user] and testPtr as AlsDevice.rank_eval takes and returns
    them; weights: one per pair (default 1; Hu, Koren and Volinsky weight by the held-out observation's value).  Pairs of
    rank -1 (the item is in the user's own skip list) are left out and counted in "skipped_pairs".  Returns a dict:
      expected_percentile_rank  sum w rank / max(candidates_u - 1, 1) / sum w: 0 is best, 0.5 what a random order gives
      hit_rate_at_n             the weighted share of pairs with rank < n
      mrr                       mean over users of 1 / (1 + the user's best rank)
      auc                       mean over users of the share of (held-out item, competing item that is not held out) pairs the
                                model orders correctly; users all of whose competing items are held out are left out
      n, pairs, skipped_pairs, users   n as given, the pairs and users that entered the measures, the pairs left out
    The measures of an empty selection are nan."""
    ranks = np.asarray(ranks, np.int64).reshape(-1)
    cand = np.asarray(candidates, np.int64).reshape(-1)
    ptr = np.asarray(testPtr, np.int64).reshape(-1)
    if len(ptr) != len(cand) + 1 or ptr[-1] != len(ranks):
        raise ValueError("testPtr does not describe ranks / candidates")
    w = np.ones(len(ranks)) if weights is None else np.asarray(weights, np.float64).reshape(-1)
    if len(w) != len(ranks):
        raise ValueError("weights needs one entry per held-out pair")
    user = np.repeat(np.arange(len(cand)), np.diff(ptr))
    keep = ranks >= 0
    r, w, user = ranks[keep], w[keep], user[keep]
    out = {"n": int(n), "pairs": int(keep.sum()), "skipped_pairs": int((~keep).sum()), "users": int(len(np.unique(user)))}
    wsum = w.sum()
    nan = float("nan")
    out["expected_percentile_rank"] = float((w * r / np.maximum(cand[user] - 1, 1)).sum() / wsum) if wsum > 0 else nan
    out["hit_rate_at_n"] = float(w[r < n].sum() / wsum) if wsum > 0 else nan
    rr, aucs = [], []
    for u in np.unique(user):
        ru = np.sort(r[user == u])
        rr.append(1.0 / (1 + ru[0]))
        m, neg = len(ru), cand[u] - len(ru)  # ru[i] - i of the items ahead of the i-th best held-out item are not held out
        if neg > 0:
            aucs.append(float((neg - (ru - np.arange(m))).sum()) / (m * neg))
    out["mrr"] = float(np.mean(rr)) if rr else nan
    out["auc"] = float(np.mean(aucs)) if aucs else nan
    return out
