"""ScoreLabelCounts.truth_table (host side of spk_label_scores_*) against a brute-force loop over random
(state, score) arrays: the binning a device pass would do is restated with np.searchsorted, the table is recomputed
pair by pair.  No device."""
import numpy as np
import pandas as pd
import pytest

from splink_amd.labels import MATCH, NON_MATCH, UNKNOWN, LabelCounts, ScoreLabelCounts


def binned(state, score, t):
    """counts [3, T + 2]: bin = thresholds below the score (`>`), NaN in bin T + 1."""
    T = len(t)
    b = np.searchsorted(t, score, side="left")
    b[np.isnan(score)] = T + 1
    return np.bincount(state * (T + 2) + b, minlength=3 * (T + 2)).reshape(3, T + 2)


def ratio(a, b):
    return a / b if b else np.nan


def brute(state, score, t, totals, all_true):
    rows = []
    for x in t:
        tp = fp = unl = 0
        for s, v in zip(state.tolist(), score.tolist()):
            if v > x:  # NaN: never
                tp += s == MATCH
                fp += s == NON_MATCH
                unl += s == UNKNOWN
        fn, tn = totals[MATCH] - tp, totals[NON_MATCH] - fp
        rows.append((x, tp, fp, tn, fn, unl, ratio(tp, tp + fp), ratio(tp, tp + fn), ratio(fp, fp + tn),
                     ratio(2 * tp, 2 * tp + fp + fn), ratio(tp, all_true)))
    return rows


def check(state, score, t, extra=(0, 0), all_true=0):
    """extra: labelled (NON_MATCH, MATCH) pairs of the job beyond the counted ones (what a filter dropped)."""
    t = np.asarray(t, dtype=np.float64)
    counts = binned(state, score, t)
    totals = (int((state == NON_MATCH).sum()) + extra[0], int((state == MATCH).sum()) + extra[1])
    got = ScoreLabelCounts(counts, t, totals, "dedupe_only", all_true).truth_table()
    want = brute(state, score, t, totals, all_true)
    assert len(got) == len(t)
    for g, w in zip(got.itertuples(index=False), want):
        for a, b in zip(g, w):
            assert a == b or (np.isnan(a) and np.isnan(b)), (g, w)
    return got


def random_pairs(seed, n=400, nan=0.1, states=(0, 1, 2)):
    rng = np.random.Generator(np.random.PCG64(seed))
    state = rng.choice(states, n)
    score = np.round(rng.random(n), 2)  # ties, and values a threshold can equal
    score[rng.random(n) < nan] = np.nan
    return rng, state, score


def test_columns_order_and_dtypes_are_label_counts():
    _, state, score = random_pairs(1)
    got = check(state, score, [0.25, 0.5])
    lc = LabelCounts(["gamma_a"], [2], np.ones((3, 3), dtype=np.int64), np.array([0.1, 0.5, 0.9]))
    ref = lc.truth_table([0.25, 0.5])
    assert list(got.columns) == list(ref.columns)
    assert list(got.dtypes) == list(ref.dtypes)
    empty = ScoreLabelCounts(np.zeros((3, 2), dtype=np.int64), [], (0, 0)).truth_table()
    assert list(empty.columns) == list(ref.columns) and len(empty) == 0
    assert list(empty.dtypes) == list(lc.truth_table([]).dtypes)


@pytest.mark.parametrize("T", [0, 1, 1024])
def test_threshold_counts(T):
    rng, state, score = random_pairs(10 + T)
    t = np.sort(rng.random(T))
    check(state, score, t, extra=(7, 3), all_true=500)


def test_duplicates_infinities_and_occurring_values():
    _, state, score = random_pairs(2)
    occurring = np.unique(score[~np.isnan(score)])
    t = np.sort(np.concatenate([[-np.inf, -np.inf, np.inf], occurring[::7], occurring[::7], [0.5, 0.5],
                                np.nextafter(occurring[::11], 1), np.nextafter(occurring[::11], -1)]))
    got = check(state, score, t, all_true=40)
    assert got.iloc[0]["tp"] + got.iloc[0]["fp"] + got.iloc[0]["n_unlabelled_above"] == int((~np.isnan(score)).sum())
    assert got.iloc[-1]["tp"] == got.iloc[-1]["fp"] == 0  # nothing is above +inf
    # infinite scores: above every finite threshold, not above +inf
    score[:5] = np.inf
    score[5:9] = -np.inf
    check(state, score, t)


def test_nan_scores_are_never_predicted_and_all_unlabelled():
    _, state, score = random_pairs(3, nan=1.0)
    got = check(state, score, [-np.inf, 0.5])
    assert (got[["tp", "fp", "n_unlabelled_above"]].to_numpy() == 0).all()
    _, state, score = random_pairs(4, states=(UNKNOWN,))
    got = check(state, score, [0.1, 0.9])
    assert (got[["tp", "fp", "tn", "fn"]].to_numpy() == 0).all() and got["n_unlabelled_above"].iloc[0] > 0
    assert got[["precision", "recall", "fpr", "f1", "recall_of_all_true_pairs"]].isna().all().all()


def test_kept_row_predicts_every_counted_pair():
    _, state, score = random_pairs(5)
    counts = binned(state, score, np.zeros(0))
    assert counts.shape == (3, 2) and counts[:, 1].sum() == int(np.isnan(score).sum()) > 0
    nm, m = int((state == NON_MATCH).sum()), int((state == MATCH).sum())
    row = ScoreLabelCounts(counts, [], (nm + 11, m + 5), "dedupe_only", m + 9).kept_row()
    assert len(row) == 1 and row["threshold"].iloc[0] == -np.inf
    r = row.iloc[0]
    assert (r["tp"], r["fp"], r["tn"], r["fn"], r["n_unlabelled_above"]) == (m, nm, 11, 5, int((state == UNKNOWN).sum()))
    assert r["precision"] == m / (m + nm) and r["recall"] == m / (m + 5) and r["recall_of_all_true_pairs"] == m / (m + 9)
    ref = LabelCounts(["gamma_a"], [2], np.ones((3, 3), dtype=np.int64), np.array([0.1, 0.5, 0.9])).truth_table([0.0])
    assert list(row.columns) == list(ref.columns) and list(row.dtypes) == list(ref.dtypes)


def test_constructor_refusals():
    with pytest.raises(ValueError, match="counts must be"):
        ScoreLabelCounts(np.zeros((3, 3), dtype=np.int64), [0.5, 0.6], (0, 0))
    with pytest.raises(ValueError, match="ascending"):
        ScoreLabelCounts(np.zeros((3, 4), dtype=np.int64), [0.6, 0.5], (0, 0))
    with pytest.raises(ValueError, match="ascending"):
        ScoreLabelCounts(np.zeros((3, 3), dtype=np.int64), [np.nan], (0, 0))
    import splink_amd
    assert splink_amd.ScoreLabelCounts is ScoreLabelCounts and "ScoreLabelCounts" in splink_amd.__all__
    assert isinstance(ScoreLabelCounts(np.zeros((3, 3), dtype=np.int64), [0.5], (0, 0)).truth_table(), pd.DataFrame)
