"""labels.PairScoreLabelCounts from hand-made arrays (no device): the truth-table arithmetic against a brute-force
count over per-pair scores, labelled_pairs() and prediction_errors(), and what the constructor refuses."""
import numpy as np
import pandas as pd
import pytest

from splink_amd.labels import MATCH, NON_MATCH, SCORE_TRUTH_COLUMNS, UNKNOWN, PairScoreLabelCounts

TF = "tf_adjusted_match_prob"


def counts_of(state, score, t):
    T = len(t)
    b = np.searchsorted(np.asarray(t, dtype=np.float64), score, side="left")  # thresholds strictly below the score
    b[np.isnan(score)] = T + 1
    return np.bincount(np.asarray(state) * (T + 2) + b, minlength=3 * (T + 2)).reshape(3, T + 2)


class Case:
    """A frame of P pairs with random scores (some NULL); the first n_found labels name pairs of it, the rest do not."""

    def __init__(self, seed=0, P=500, n_found=40, n_missing=15):
        rng = np.random.Generator(np.random.PCG64(seed))
        self.score = np.round(rng.random(P), 2)  # ties, and values that thresholds can equal
        self.score[rng.random(P) < 0.1] = np.nan
        self.pair = np.concatenate([rng.permutation(P)[:n_found], np.full(n_missing, -1)]).astype(np.int64)
        n = n_found + n_missing
        order = rng.permutation(n)
        self.pair = self.pair[order]
        self.is_match = rng.random(n) < 0.5
        self.state = np.full(P, UNKNOWN)
        self.state[self.pair[self.pair >= 0]] = self.is_match[self.pair >= 0].astype(np.int64)
        self.label_score = np.where(self.pair >= 0, self.score[np.maximum(self.pair, 0)], np.nan)
        self.labels = pd.DataFrame({"unique_id_l": np.arange(n), "unique_id_r": np.arange(n) + 1000,
                                    "clerical_match_score": self.is_match.astype(float)}, index=np.arange(n) * 3)

    def make(self, t, **kw):
        counts = counts_of(self.state, self.score, t)
        totals = kw.pop("totals", counts.sum(axis=1))
        return PairScoreLabelCounts(counts, t, totals, "dedupe_only", self.labels, self.is_match, self.label_score, TF,
                                    label_pair=self.pair, **kw)


def test_truth_table_against_brute_force():
    case = Case()
    t = np.array([-np.inf, 0.0, 0.25, 0.25, 0.5, 0.77, 1.0, np.inf])
    c = case.make(t)
    assert c.true_pairs_total == int(case.is_match.sum())
    table = c.truth_table()
    assert list(table.columns) == list(SCORE_TRUTH_COLUMNS) and len(table) == len(t)
    n_match, n_non = int((case.state == MATCH).sum()), int((case.state == NON_MATCH).sum())
    for k, row in table.iterrows():
        above = case.score > t[k]  # NaN: never
        tp = int((above & (case.state == MATCH)).sum())
        fp = int((above & (case.state == NON_MATCH)).sum())
        assert (row["tp"], row["fp"], row["fn"], row["tn"]) == (tp, fp, n_match - tp, n_non - fp), k
        assert row["n_unlabelled_above"] == int((above & (case.state == UNKNOWN)).sum())
        assert row["recall_of_all_true_pairs"] == tp / case.is_match.sum()
    assert table["tp"].iloc[1] > table["tp"].iloc[5] > 0 and table["tp"].iloc[-1] == 0
    kept = c.kept_row().iloc[0]  # every counted pair, NULL scores included
    assert (kept["threshold"], kept["tp"], kept["fp"]) == (-np.inf, n_match, n_non) and kept["fn"] == kept["tn"] == 0
    # totals of a selection frame: fn and tn against the labelled candidates, kept or not
    found_by_blocking = np.ones(len(case.pair), dtype=bool)
    wide = case.make(t, totals=(n_non + 7, n_match + 5, 0), found_by_blocking=found_by_blocking)
    kept = wide.kept_row().iloc[0]
    assert (kept["fn"], kept["tn"]) == (5, 7)


def test_labelled_pairs_columns_and_nulls():
    case = Case(1)
    c = case.make([0.5])
    pairs = c.labelled_pairs()
    assert list(pairs.columns) == list(case.labels.columns) + ["found_by_blocking", TF]
    assert pairs.index.equals(case.labels.index) and len(pairs) == len(case.labels)  # its own row order
    assert np.array_equal(pairs["found_by_blocking"].to_numpy(), case.pair >= 0)
    assert np.array_equal(pairs[TF].to_numpy(), case.label_score, equal_nan=True)
    assert pairs[TF][case.pair < 0].isna().all() and (case.pair < 0).any()
    assert np.isnan(case.label_score[case.pair >= 0]).any()  # a pair that is found and has a NULL score
    # a selection frame: found_by_blocking is wider than kept
    by_blocking = (case.pair >= 0) | (np.arange(len(case.pair)) % 2 == 0)
    sel = case.make([0.5], totals=(400, 400, 0), found_by_blocking=by_blocking)
    pairs = sel.labelled_pairs()
    assert list(pairs.columns) == list(case.labels.columns) + ["found_by_blocking", "kept", TF]
    assert np.array_equal(pairs["kept"].to_numpy(), case.pair >= 0)
    assert np.array_equal(pairs["found_by_blocking"].to_numpy(), by_blocking)
    assert (pairs["found_by_blocking"] & ~pairs["kept"]).any()
    # a sharded job: found instead of label_pair
    counts = counts_of(case.state, case.score, [0.5])
    sharded = PairScoreLabelCounts(counts, [0.5], counts.sum(axis=1), "dedupe_only", case.labels, case.is_match,
                                   case.label_score, TF, found=case.pair >= 0)
    assert sharded.label_pair is None and sharded.labelled_pairs().equals(c.labelled_pairs())


def test_prediction_errors_on_above_and_below_a_score():
    labels = pd.DataFrame({"unique_id_l": [1, 2, 3, 4, 5, 6], "unique_id_r": [11, 12, 13, 14, 15, 16],
                           "clerical_match_score": [1.0, 0.0, 1.0, 0.0, 1.0, 1.0]})
    is_match = np.array([1, 0, 1, 0, 1, 1], dtype=np.uint8)
    #        match 0.8, non-match 0.8, match not found, non-match not found, match with a NULL score, match 0.3
    pair = np.array([0, 1, -1, -1, 2, 3])
    score = np.array([0.8, 0.8, np.nan, np.nan, np.nan, 0.3])
    counts = np.zeros((3, 2), dtype=np.int64)  # T = 0: bin 0 and the NULL bin
    counts[MATCH] = (2, 1)
    counts[NON_MATCH] = (1, 0)
    counts[UNKNOWN] = (6, 0)
    c = PairScoreLabelCounts(counts, [], counts.sum(axis=1), "link_only", labels, is_match, score, TF, label_pair=pair)

    def errors(t):
        e = c.prediction_errors(t)
        assert list(e.columns) == list(labels.columns) + ["found_by_blocking", TF, "error"]
        return dict(zip(e.index.tolist(), e["error"].tolist()))
    # strictly above: a score equal to the threshold is not predicted
    assert errors(0.8) == {0: "fn", 2: "fn", 4: "fn", 5: "fn"}
    assert errors(np.nextafter(0.8, 0)) == {1: "fp", 2: "fn", 4: "fn", 5: "fn"}
    assert errors(0.3) == {1: "fp", 2: "fn", 4: "fn", 5: "fn"}
    assert errors(0.1) == {1: "fp", 2: "fn", 4: "fn"}  # the unfound match and the NULL score stay fn at any threshold
    assert errors(-np.inf) == {1: "fp", 2: "fn", 4: "fn"}
    assert errors(0.9) == {0: "fn", 2: "fn", 4: "fn", 5: "fn"}
    assert c.prediction_errors(0.5)["unique_id_l"].tolist() == [2, 3, 5, 6]  # in the labels' own order


def test_constructor_refusals():
    case = Case(2)
    t = np.array([0.2, 0.6])
    counts = counts_of(case.state, case.score, t)
    totals = counts.sum(axis=1)
    args = (counts, t, totals, "dedupe_only", case.labels, case.is_match, case.label_score, TF)
    with pytest.raises(ValueError, match="label_pair, or found"):
        PairScoreLabelCounts(*args)
    with pytest.raises(ValueError, match="label_pair, or found"):
        PairScoreLabelCounts(*args, label_pair=case.pair, found=case.pair >= 0)
    with pytest.raises(ValueError, match="differ in length"):
        PairScoreLabelCounts(*args, label_pair=case.pair[:-1])
    with pytest.raises(ValueError, match="differ in length"):
        PairScoreLabelCounts(counts, t, totals, "dedupe_only", case.labels, case.is_match[:-1], case.label_score, TF,
                             label_pair=case.pair)
    with pytest.raises(ValueError, match="blocking did not produce"):
        PairScoreLabelCounts(*args, label_pair=case.pair, found_by_blocking=np.zeros(len(case.pair), dtype=bool))
    stray = case.label_score.copy()
    stray[np.flatnonzero(case.pair < 0)[0]] = 0.5
    with pytest.raises(ValueError, match="names no pair"):
        PairScoreLabelCounts(counts, t, totals, "dedupe_only", case.labels, case.is_match, stray, TF,
                             label_pair=case.pair)
    fewer = counts.copy()
    fewer[MATCH] = 0
    with pytest.raises(ValueError, match="fewer labelled pairs"):
        PairScoreLabelCounts(fewer, t, totals, "dedupe_only", case.labels, case.is_match, case.label_score, TF,
                             label_pair=case.pair)
    with pytest.raises(ValueError, match="ascending"):
        PairScoreLabelCounts(counts, t[::-1], totals, "dedupe_only", case.labels, case.is_match, case.label_score, TF,
                             label_pair=case.pair)
    with pytest.raises(ValueError, match=r"\[3, 5\]"):
        PairScoreLabelCounts(counts, [0.1, 0.2, 0.3], totals, "dedupe_only", case.labels, case.is_match,
                             case.label_score, TF, label_pair=case.pair)
