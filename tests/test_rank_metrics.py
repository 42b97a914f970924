"""ranking_metrics: the four measures on a handful of ranks, worked out by hand."""
import pytest

from ycnr_als import ranking_metrics


def test_measures_of_a_hand_written_case():
    # user 0: 11 candidates, held-out ranks 0 and 4          user 1: 5 candidates, ranks 2 and -1 (left out)
    # user 2: 1 candidate (the held-out item itself), rank 0  user 3: nothing held out
    m = ranking_metrics(ranks=[0, 4, 2, -1, 0], candidates=[11, 5, 1, 7], testPtr=[0, 2, 4, 5, 5], weights=[1, 2, 1, 9, 4], n=3)
    assert (m["pairs"], m["skipped_pairs"], m["users"], m["n"]) == (4, 1, 3, 3)
    # rank-bar: (1 * 0 / 10 + 2 * 4 / 10 + 1 * 2 / 4 + 4 * 0 / max(0, 1)) / (1 + 2 + 1 + 4) = 1.3 / 8
    assert m["expected_percentile_rank"] == pytest.approx(1.3 / 8)
    # ranks below 3: the pairs of weight 1, 1 and 4
    assert m["hit_rate_at_n"] == pytest.approx(6 / 8)
    # best ranks 0, 2, 0
    assert m["mrr"] == pytest.approx((1 + 1 / 3 + 1) / 3)
    # user 0: 9 other items; nothing is ahead of the first held-out item, 4 - 1 = 3 other items ahead of the second: (9 + 6) / 18
    # user 1: 4 other items, 2 ahead: 2 / 4.  user 2 has no other item and is left out.
    assert m["auc"] == pytest.approx((15 / 18 + 0.5) / 2)
    unweighted = ranking_metrics([0, 4, 2, -1, 0], [11, 5, 1, 7], [0, 2, 4, 5, 5], n=3)
    assert unweighted["expected_percentile_rank"] == pytest.approx((0.4 + 0.5) / 4) and unweighted["hit_rate_at_n"] == pytest.approx(3 / 4)
