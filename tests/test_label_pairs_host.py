"""Host side of labels given as a table of pairs (splink_amd/labels.py: pair_label_rows, PairLabelCounts), without a
device.  Expected rows and tables are written out by hand."""
import numpy as np
import pandas as pd
import pytest

from splink_amd.labels import (MATCH, NON_MATCH, UNKNOWN, LabelCounts, PairLabelCounts, PairLabelSides,
                               pair_label_rows)

SCORE = "clerical_match_score"


def labels_table(pairs, scores, uid="unique_id", **more):
    return pd.DataFrame({f"{uid}_l": [p[0] for p in pairs], f"{uid}_r": [p[1] for p in pairs], SCORE: scores, **more})


# ---- pair_label_rows ---------------------------------------------------------------------------------------------
# device row i holds input row PERM[i]: ids in device row order
DEDUPE = PairLabelSides("dedupe_only", "unique_id", [np.array([40, 10, 30, 20, 50])])
LINK = PairLabelSides("link_only", "rec", [np.array(["b", "a", "c"], dtype=object),
                                           np.array(["c", "a", "x", "b"], dtype=object)])
# the concatenated table of link_and_dedupe, clustered: ids 1, 2 occur in both inputs, 7 only left, 9 only right
BOTH = PairLabelSides("link_and_dedupe", "unique_id", [np.array([2, 1, 9, 7, 1, 2])],
                      np.array(["right", "left", "right", "left", "right", "left"], dtype=object))


def test_dedupe_rows_orders_and_scores():
    lab = labels_table([(10, 20), (50, 40), (30, 10)], [0.9, 0.1, 0.5])
    l, r, y = pair_label_rows(DEDUPE, lab)
    assert (l.dtype, r.dtype, y.dtype) == (np.int32, np.int32, np.uint8)
    assert l.tolist() == [1, 4, 2] and r.tolist() == [3, 0, 1]  # a permuted device row order; pairs as given
    assert y.tolist() == [1, 0, 1]  # a score exactly at the threshold is a match
    assert pair_label_rows(DEDUPE, lab, match_threshold=0.51)[2].tolist() == [1, 0, 0]
    assert pair_label_rows(DEDUPE, lab, match_threshold=0.1)[2].tolist() == [1, 1, 1]
    # bool scores, and an empty table
    assert pair_label_rows(DEDUPE, labels_table([(10, 20), (20, 30)], [True, False]))[2].tolist() == [1, 0]
    l, r, y = pair_label_rows(DEDUPE, labels_table([], []))
    assert len(l) == len(r) == len(y) == 0 and y.dtype == np.uint8


def test_link_only_sides():
    lab = labels_table([("a", "b"), ("b", "a"), ("c", "x")], [1.0, 0.0, 0.7], uid="rec")
    l, r, y = pair_label_rows(LINK, lab)
    # _l names a record of the left input, _r one of the right: (a, b) and (b, a) are two pairs
    assert l.tolist() == [1, 0, 2] and r.tolist() == [3, 1, 2] and y.tolist() == [1, 0, 1]
    with pytest.raises(ValueError, match="not in the input table in row 1$"):  # x is a record of the right input
        pair_label_rows(LINK, labels_table([("a", "b"), ("x", "a")], [1, 1], uid="rec"))


def test_link_and_dedupe_source_tables():
    lab = labels_table([(1, 1), (2, 7), (9, 2), (7, 9)], [0.9, 0.2, True, 0.5],
                       _source_table_l=["left", "right", "right", "left"],
                       _source_table_r=["right", "left", "left", "right"])
    l, r, y = pair_label_rows(BOTH, lab)
    assert l.tolist() == [1, 0, 2, 3] and r.tolist() == [4, 3, 5, 2] and y.tolist() == [1, 0, 1, 1]
    # without the source columns only ids that one record carries resolve
    l, r, y = pair_label_rows(BOTH, labels_table([(7, 9)], [0.3]))
    assert (l.tolist(), r.tolist(), y.tolist()) == ([3], [2], [0])
    with pytest.raises(ValueError, match="more than one input record carries in rows 0, 2: give _source_table_l"):
        pair_label_rows(BOTH, labels_table([(1, 7), (7, 9), (9, 2)], [1, 1, 1]))
    with pytest.raises(ValueError, match="come together"):
        pair_label_rows(BOTH, labels_table([(7, 9)], [1], _source_table_l=["left"]))
    with pytest.raises(ValueError, match="neither 'left' nor 'right' in row 0"):
        pair_label_rows(BOTH, labels_table([(7, 9)], [1], _source_table_l=["l"], _source_table_r=["right"]))
    with pytest.raises(ValueError, match="not in the input table in row 0"):  # 7 is no record of the right input
        pair_label_rows(BOTH, labels_table([(7, 9)], [1], _source_table_l=["right"], _source_table_r=["right"]))
    # the same id on both sides is a pair of two records here, and of one record when the sources agree
    with pytest.raises(ValueError, match="with itself in row 0"):
        pair_label_rows(BOTH, labels_table([(1, 1)], [1], _source_table_l=["left"], _source_table_r=["left"]))


def test_value_errors_name_the_rows():
    ok = [(10, 20), (30, 40), (50, 10)]
    with pytest.raises(ValueError, match="no column 'unique_id_r', 'clerical_match_score'"):
        pair_label_rows(DEDUPE, pd.DataFrame({"unique_id_l": [10]}))
    with pytest.raises(ValueError, match="NULL id or score in rows 1, 2"):
        pair_label_rows(DEDUPE, labels_table([(10, 20), (30, None), (50, 10)], [1.0, 0.0, None]))
    with pytest.raises(ValueError, match="NULL id or score in row 0"):
        pair_label_rows(DEDUPE, labels_table([(np.nan, 20.0)], [1.0]))
    with pytest.raises(ValueError, match="not in the input table in rows 0, 2"):
        pair_label_rows(DEDUPE, labels_table([(10, 21), (30, 40), (60, 10)], [1, 0, 1]))
    with pytest.raises(ValueError, match="with itself in row 1"):
        pair_label_rows(DEDUPE, labels_table([(10, 20), (30, 30)], [1, 0]))
    with pytest.raises(ValueError, match="more than once in rows 0, 3"):  # the same order, the same score
        pair_label_rows(DEDUPE, labels_table(ok + [(10, 20)], [1, 0, 1, 1]))
    with pytest.raises(ValueError, match="more than once in rows 1, 3"):  # the other order, another score
        pair_label_rows(DEDUPE, labels_table(ok + [(40, 30)], [1, 0, 1, 1]))
    with pytest.raises(ValueError, match="more than once in rows 0, 1"):
        pair_label_rows(LINK, labels_table([("a", "b"), ("a", "b")], [1, 0], uid="rec"))
    # an id that two records of the input carry cannot be resolved
    twice = PairLabelSides("dedupe_only", "unique_id", [np.array([10, 20, 10, 30])])
    with pytest.raises(ValueError, match="more than one input record carries in row 0$"):
        pair_label_rows(twice, labels_table([(10, 20), (20, 30)], [1, 0]))
    assert pair_label_rows(twice, labels_table([(30, 20)], [1]))[0].tolist() == [3]


# ---- PairLabelCounts -----------------------------------------------------------------------------------------------
NAMES, LEVELS = ["gamma_a", "gamma_b"], [2, 3]  # 12 patterns; code = (a + 1) + 3 (b + 1)


def hand_counts():
    """Eight labels.  Found among the candidates: 0 (match, code 11), 1 (non-match, 11), 2 (match, 4), 3 (non-match,
    0), 6 (match, 3: a NULL score); not found: 4 (match), 5 (non-match), 7 (match)."""
    labels = labels_table([(1, 2), (3, 4), (5, 6), (7, 8), (9, 10), (11, 12), (13, 14), (15, 16)],
                          [0.9, 0.1, 1.0, 0.0, 0.8, 0.3, 0.6, 0.7])
    labels.index = [10, 11, 12, 13, 14, 15, 16, 17]  # its own index comes back
    is_match = np.array([1, 0, 1, 0, 1, 0, 1, 1], dtype=np.uint8)
    code = np.array([11, 11, 4, 0, -1, -1, 3, -1], dtype=np.int32)
    counts = np.zeros((3, 12), dtype=np.int64)
    counts[MATCH, [11, 4, 3]] = 1
    counts[NON_MATCH, [11, 0]] = 1
    counts[UNKNOWN] = [30, 2, 0, 1, 5, 0, 0, 0, 0, 0, 0, 4]
    mp = np.array([0.01, 0.02, 0.03, np.nan, 0.6, 0.5, 0.5, 0.7, 0.8, 0.85, 0.9, 0.95])
    return labels, is_match, code, counts, mp


def test_counts_and_inherited_truth_table():
    labels, is_match, code, counts, mp = hand_counts()
    pc = PairLabelCounts(NAMES, LEVELS, counts, mp, "dedupe_only", labels, is_match, code)
    assert isinstance(pc, LabelCounts) and pc.true_pairs_total == 5
    assert pc.missed_by_blocking == 2 and pc.non_matches_missed_by_blocking == 1
    tt = pc.truth_table([0.0, 0.55, 0.9])
    assert tt["tp"].tolist() == [2, 2, 1] and tt["fp"].tolist() == [2, 1, 1]
    assert tt["fn"].tolist() == [1, 1, 2] and tt["tn"].tolist() == [0, 1, 1]  # the NULL score is never predicted
    assert tt["n_unlabelled_above"].tolist() == [41, 9, 4]
    assert tt["recall_of_all_true_pairs"].tolist() == [2 / 5, 2 / 5, 1 / 5]  # over all labelled matches
    assert pc.truth_table().equals(LabelCounts(NAMES, LEVELS, counts, mp, "dedupe_only", 5).truth_table())
    assert pc.patterns()["n_match"].sum() == 3
    with pytest.raises(ValueError, match="differ in length"):
        PairLabelCounts(NAMES, LEVELS, counts, mp, "dedupe_only", labels, is_match[:-1], code)
    with pytest.raises(ValueError, match="outside the pattern space"):
        PairLabelCounts(NAMES, LEVELS, counts, mp, "dedupe_only", labels, is_match, np.where(code == 4, 12, code))


def test_labelled_pairs_and_prediction_errors():
    labels, is_match, code, counts, mp = hand_counts()
    pc = PairLabelCounts(NAMES, LEVELS, counts, mp, "dedupe_only", labels, is_match, code)
    lp = pc.labelled_pairs()
    assert list(lp.columns) == list(labels.columns) + ["found_by_blocking"] + NAMES + ["match_probability"]
    assert lp.index.tolist() == labels.index.tolist() and lp[list(labels.columns)].equals(labels)
    assert lp["found_by_blocking"].tolist() == [True, True, True, True, False, False, True, False]
    na = pd.NA
    assert lp["gamma_a"].tolist() == [1, 1, 0, -1, na, na, -1, na]
    assert lp["gamma_b"].tolist() == [2, 2, 0, -1, na, na, 0, na]
    assert np.array_equal(lp["match_probability"].to_numpy(),
                          [0.95, 0.95, 0.6, 0.01, np.nan, np.nan, np.nan, np.nan], equal_nan=True)
    # match_probability > 0.55: label 1 is a false positive; the unfound matches 4 and 7 and the NULL-scored match 6
    # are false negatives; the unfound non-match 5 is no error
    err = pc.prediction_errors(0.55)
    assert err.index.tolist() == [11, 14, 16, 17] and err["error"].tolist() == ["fp", "fn", "fn", "fn"]
    assert err.drop(columns="error").equals(lp.loc[[11, 14, 16, 17]])
    assert pc.prediction_errors(0.6)["error"].tolist() == ["fp", "fn", "fn", "fn", "fn"]  # 0.6 > 0.6 is false
    assert pc.prediction_errors(0.99)["error"].tolist() == ["fn"] * 5
    # an unscored frame's counts: the levels still, no scores, no errors
    plain = PairLabelCounts(NAMES, LEVELS, counts, None, "dedupe_only", labels, is_match, code)
    assert "match_probability" not in plain.labelled_pairs().columns
    assert plain.labelled_pairs()["gamma_a"].tolist() == lp["gamma_a"].tolist()
    with pytest.raises(ValueError, match="no match_probability"):
        plain.prediction_errors(0.5)
    lam, rows = plain.m_step()
    assert lam == np.float32(3 / 5)
