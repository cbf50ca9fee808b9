"""Clusters against labels, the host side: the pandas oracle of spk_cluster_agreement's fields against enumeration,
and labels.cluster_truth_rows.  No device."""
import numpy as np
import pytest

from agreement_common import FIELDS, agreement_brute, agreement_oracle, labels_of_edges

F = {name: i for i, name in enumerate(FIELDS)}


def random_labeling(rng, n):
    """n nodes: clusters from a few random edges, ids from a few values, a fifth NULL (any negative value)."""
    m = int(rng.integers(0, n + 1))
    labels = labels_of_edges(n, rng.integers(0, max(n, 1), m), rng.integers(0, max(n, 1), m)) if n else np.zeros(0, np.int64)
    ids = rng.integers(0, max(1, n // 3) + 1, n).astype(np.int64)
    ids[rng.random(n) < 0.2] = -int(rng.integers(1, 1 << 40))
    return labels, ids


def test_oracle_equals_enumeration():
    rng = np.random.Generator(np.random.PCG64(11))
    mixed = split = recovered = 0
    for case in range(300):
        n = int(rng.integers(0, 41))
        labels, ids = random_labeling(rng, n)
        for cross, n_left in [(0, 0), (1, 0), (1, n), (1, n // 2), (1, int(rng.integers(0, n + 1)))]:
            want = agreement_brute(labels, ids, n_left, cross)
            got = agreement_oracle(labels, ids, n_left, cross)
            assert got.dtype == np.int64 and np.array_equal(got, want), (case, cross, n_left, got, want)
            if cross and n_left in (0, n):
                assert got[F["pairs_total"]] == got[F["predicted_pairs"]] == got[F["true_pairs"]] == 0
        mixed += want[F["clusters_mixed"]] > 0
        split += want[F["entities_split"]] > 0
        recovered += want[F["entities_recovered"]] > 0
    assert mixed > 50 and split > 50 and recovered > 50  # the cases reach every field


def test_oracle_by_hand():
    # clusters {0, 1, 2} {3, 4} {5}; ids a a b | b NULL | c
    labels, ids = [0, 0, 0, 3, 3, 5], [7, 7, 9, 9, -1, 4]
    got = dict(zip(FIELDS, agreement_oracle(labels, ids, 0, 0).tolist()))
    assert got == {"records_labelled": 5, "clusters_labelled": 3, "entities": 3, "predicted_pairs": 3, "true_pairs": 2,
                   "tp": 1, "clusters_mixed": 1, "entities_split": 1, "entities_recovered": 1, "pairs_total": 10}
    # left = nodes 0..2: the pair (2, 3) is the only true cross pair, and no cluster spans the sides
    got = dict(zip(FIELDS, agreement_oracle(labels, ids, 3, 1).tolist()))
    assert (got["predicted_pairs"], got["true_pairs"], got["tp"], got["pairs_total"]) == (0, 1, 0, 6)
    assert got["entities_recovered"] == 1 and got["clusters_mixed"] == 1  # the side changes no cluster or entity count


def test_cluster_truth_rows():
    from splink_amd.labels import AGREEMENT_FIELDS, CLUSTER_TRUTH_COLUMNS, cluster_truth_rows
    assert tuple(AGREEMENT_FIELDS) == tuple(FIELDS)
    counts = np.array([[9, 4, 5, 6, 8, 3, 1, 2, 2, 36],
                       [9, 9, 5, 0, 8, 0, 0, 5, 0, 36],
                       [0, 0, 0, 0, 0, 0, 0, 0, 0, 0]], dtype=np.int64)
    t = cluster_truth_rows(counts, [0.5, 0.99, 0.1])
    assert list(t.columns) == ["threshold", "tp", "fp", "fn", "tn", "precision", "recall", "f1", "predicted_pairs",
                               "true_pairs", "records_labelled", "clusters_labelled", "clusters_mixed", "entities",
                               "entities_split", "entities_recovered"] == list(CLUSTER_TRUTH_COLUMNS)
    assert t["threshold"].tolist() == [0.5, 0.99, 0.1]  # as given, not sorted
    assert t.iloc[0][["tp", "fp", "fn", "tn"]].tolist() == [3, 3, 5, 36 - 6 - 8 + 3]
    assert t.iloc[0]["precision"] == 3 / 6 and t.iloc[0]["recall"] == 3 / 8 and t.iloc[0]["f1"] == 6 / 14
    assert t.iloc[1][["tp", "fp", "fn", "tn"]].tolist() == [0, 0, 8, 28]
    assert np.isnan(t.iloc[1]["precision"]) and t.iloc[1]["recall"] == 0.0 and t.iloc[1]["f1"] == 0.0
    assert np.isnan(t.iloc[2][["precision", "recall", "f1"]].to_numpy(dtype=np.float64)).all()
    for name in ("predicted_pairs", "true_pairs", "records_labelled", "clusters_labelled", "clusters_mixed", "entities",
                 "entities_split", "entities_recovered"):
        assert t[name].dtype == np.int64 and t[name].tolist() == counts[:, F[name]].tolist()
    assert (t["tp"] + t["fp"] + t["fn"] + t["tn"]).tolist() == counts[:, F["pairs_total"]].tolist()
    one = cluster_truth_rows(counts[0], [np.nan])
    assert len(one) == 1 and np.isnan(one["threshold"][0]) and one["tp"][0] == 3
    with pytest.raises(ValueError, match="2 thresholds for 3 rows"):
        cluster_truth_rows(counts, [0.5, 0.9])
