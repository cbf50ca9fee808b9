"""Scoring a linkage against labels (no counterpart in the reference release; later releases:
truth_space_table_from_labels_column, roc_chart_from_labels_column, estimate_m_from_label_column).

match_probability is a function of a pair's comparison pattern alone, so one device pass that counts the pairs per
(truth state, pattern) (spk_label_histogram) leaves the host with everything it needs, over n_patterns rows only:
the exact confusion matrix at every threshold, the true pairs blocking never produced, and the supervised estimate
of m / u / λ -- one M-step with match_probability replaced by the label.  Scores that are decided per pair
(tf_adjusted_match_prob, the pairs a filter or a best-match step kept) are counted per (truth state, threshold bin)
instead (spk_label_scores_*, ScoreLabelCounts).  Labels may also come as a table of pairs that a person marked match
or non-match (a clerical-review sample; later releases: truth_space_table_from_labels_table,
prediction_errors_from_labels_table, estimate_m_from_pairwise_labels): pair_label_rows turns it into device rows,
spk_label_pairs_histogram counts the candidate pairs against it, PairLabelCounts is what follows.  This module is the
host side: pure numpy / pandas, importable without a device.
"""
from __future__ import annotations

from typing import NamedTuple, Optional, Sequence

import numpy as np
import pandas as pd

from .engine import N_HEAD, m_step_rows

NON_MATCH, MATCH, UNKNOWN = 0, 1, 2  # SPK_LABEL_NON_MATCH / _MATCH / _UNKNOWN: the rows of LabelCounts.counts


def _group_sizes(ids):
    """{label id: records} over the non-NULL (non-negative) ids, as (sorted ids, counts)."""
    ids = np.asarray(ids, dtype=np.int64)
    return np.unique(ids[ids >= 0], return_counts=True)


def true_pairs_total(link_type, ids0, ids1=None) -> int:
    """The record pairs with equal non-NULL labels that the link type compares at all, whether or not blocking
    produced them: Σ C(n_g, 2) over the one table of dedupe_only and link_and_dedupe (for the latter the vertical
    concatenation: a pair within the left, within the right or across), Σ n_g(left) · n_g(right) for link_only."""
    v0, c0 = _group_sizes(ids0)
    if link_type != "link_only":
        return int(sum(int(c) * (int(c) - 1) // 2 for c in c0.tolist()))
    if ids1 is None:
        raise ValueError("true_pairs_total: link_only needs the right table's label ids")
    v1, c1 = _group_sizes(ids1)
    _, i0, i1 = np.intersect1d(v0, v1, assume_unique=True, return_indices=True)
    return int(sum(int(a) * int(b) for a, b in zip(c0[i0].tolist(), c1[i1].tolist())))


def _ratio(num, den):
    """num / den elementwise on integer arrays, NaN for 0 / 0."""
    num, den = np.asarray(num, dtype=np.int64), np.asarray(den, dtype=np.int64)
    out = np.full(len(num), np.nan, dtype=np.float64)
    ok = den != 0
    out[ok] = num[ok] / den[ok]
    return out


# The columns of spk_cluster_agreement's rows (SPK_AGREE_FIELDS), in its order.
AGREEMENT_FIELDS = ("records_labelled", "clusters_labelled", "entities", "predicted_pairs", "true_pairs", "tp",
                    "clusters_mixed", "entities_split", "entities_recovered", "pairs_total")
CLUSTER_TRUTH_COLUMNS = ("threshold", "tp", "fp", "fn", "tn", "precision", "recall", "f1", "predicted_pairs",
                         "true_pairs", "records_labelled", "clusters_labelled", "clusters_mixed", "entities",
                         "entities_split", "entities_recovered")


def cluster_truth_rows(counts, thresholds) -> pd.DataFrame:
    """The truth table of clusters: one row per row of `counts` (int64 [n, len(AGREEMENT_FIELDS)], what
    spk_cluster_agreement counts at one level each) and threshold, in the order given.  A pair is predicted iff its
    two records share a cluster, so with P predicted, T true and tp both: fp = P - tp, fn = T - tp, tn = pairs_total -
    P - T + tp, over the pairs of labelled records that the link type compares, whether or not blocking produced them.
    precision, recall and f1 are NaN for 0 / 0."""
    counts = np.asarray(counts, dtype=np.int64).reshape(-1, len(AGREEMENT_FIELDS))
    t = np.asarray(list(thresholds), dtype=np.float64)
    if len(t) != len(counts):
        raise ValueError(f"cluster_truth_rows: {len(t)} thresholds for {len(counts)} rows of counts")
    f = {name: counts[:, i] for i, name in enumerate(AGREEMENT_FIELDS)}
    tp, P, T = f["tp"], f["predicted_pairs"], f["true_pairs"]
    fp, fn = P - tp, T - tp
    data = {"threshold": t, "tp": tp, "fp": fp, "fn": fn, "tn": f["pairs_total"] - P - T + tp,
            "precision": _ratio(tp, P), "recall": _ratio(tp, T), "f1": _ratio(2 * tp, 2 * tp + fp + fn)}
    for name in CLUSTER_TRUTH_COLUMNS[8:]:
        data[name] = f[name]
    return pd.DataFrame(data, columns=list(CLUSTER_TRUTH_COLUMNS))


class LabelCounts:
    """Pairs per (truth state, comparison pattern) of one pair set, and what follows from them.

    names / n_levels: the gamma columns (`gamma_*`) and their level counts, which define the packed code
    (code = Σ_k (γ_k + 1) · Π_{j<k} (L_j + 1)); counts int64 [3, n_patterns] by NON_MATCH / MATCH / UNKNOWN (either
    label NULL); mp: match_probability per pattern (NaN = NULL) or None for an unscored frame; true_pairs_total as
    the function of that name gives it."""

    def __init__(self, names, n_levels, counts, mp=None, link_type="dedupe_only", true_pairs_total=0):
        self.names = list(names)
        self.n_levels = [int(L) for L in n_levels]
        n_pat = 1
        for L in self.n_levels:
            n_pat *= L + 1
        self.counts = np.ascontiguousarray(counts, dtype=np.int64)
        if self.counts.shape != (3, n_pat):
            raise ValueError(f"LabelCounts: counts must be [3, {n_pat}] for levels {self.n_levels}")
        self.mp = None if mp is None else np.ascontiguousarray(mp, dtype=np.float64)
        if self.mp is not None and self.mp.shape != (n_pat,):
            raise ValueError(f"LabelCounts: mp must be [{n_pat}]")
        self.link_type = link_type
        self.true_pairs_total = int(true_pairs_total)
        self.missed_by_blocking = self.true_pairs_total - int(self.counts[MATCH].sum())

    @property
    def n_patterns(self) -> int:
        return self.counts.shape[1]

    def levels(self, codes) -> np.ndarray:
        """int32 [len(codes), K]: the gamma levels of packed codes, decoded as the pattern space packs them."""
        codes = np.asarray(codes, dtype=np.int64)
        out = np.empty((len(codes), len(self.n_levels)), dtype=np.int32)
        stride = 1
        for k, L in enumerate(self.n_levels):
            out[:, k] = (codes // stride) % (L + 1) - 1
            stride *= L + 1
        return out

    def patterns(self) -> pd.DataFrame:
        """One row per pattern that occurs, ascending code: the gamma_* levels, match_probability if scored, then
        n_match, n_non_match, n_unlabelled."""
        codes = np.flatnonzero(self.counts.sum(axis=0) > 0)
        lev = self.levels(codes)
        data = {name: lev[:, k] for k, name in enumerate(self.names)}
        if self.mp is not None:
            data["match_probability"] = self.mp[codes]
        data["n_match"] = self.counts[MATCH, codes]
        data["n_non_match"] = self.counts[NON_MATCH, codes]
        data["n_unlabelled"] = self.counts[UNKNOWN, codes]
        return pd.DataFrame(data)

    def truth_table(self, thresholds=None) -> pd.DataFrame:
        """The confusion matrix of `match_probability > threshold` against the labels, one row per threshold,
        ascending -- filter()'s and clusters(threshold)'s `>`; a NULL (NaN) score is never predicted a match.
        thresholds=None: every distinct non-NULL score of a pattern that occurs, preceded by one threshold below
        them all, i.e. every point of the exact ROC.  tp, fp, tn, fn count labelled pairs only; n_unlabelled_above
        the pairs above the threshold with a NULL label; precision, recall, fpr, f1 are NaN for 0 / 0;
        recall_of_all_true_pairs = tp / true_pairs_total also counts the true pairs blocking never produced."""
        if self.mp is None:
            raise ValueError("truth_table: these counts carry no match_probability (label_counts() of an unscored "
                             "frame): take them from the frame run_expectation_step returns")
        occurs = (self.counts.sum(axis=0) > 0) & ~np.isnan(self.mp)
        score = self.mp[occurs]
        order = np.argsort(score, kind="stable")
        score = score[order]
        # suffix[:, i] = pairs of each state at the i-th smallest score and above (suffix[:, n] = 0)
        by_state = self.counts[:, occurs][:, order]
        suffix = np.zeros((3, len(score) + 1), dtype=np.int64)
        suffix[:, :-1] = np.cumsum(by_state[:, ::-1], axis=1)[:, ::-1]
        if thresholds is None:
            distinct = np.unique(score)
            t = np.concatenate([[np.nextafter(distinct[0], -np.inf)], distinct]) if len(distinct) else distinct
        else:
            t = np.sort(np.asarray(list(thresholds), dtype=np.float64))
            if np.isnan(t).any():
                raise ValueError("truth_table: a threshold is NaN")
        first_above = np.searchsorted(score, t, side="right")  # score[i] > t  <=>  i >= first_above
        above = suffix[:, first_above]
        tp, fp, unl = above[MATCH], above[NON_MATCH], above[UNKNOWN]
        fn = int(self.counts[MATCH].sum()) - tp
        tn = int(self.counts[NON_MATCH].sum()) - fp
        return pd.DataFrame({
            "threshold": t, "tp": tp, "fp": fp, "tn": tn, "fn": fn, "n_unlabelled_above": unl,
            "precision": _ratio(tp, tp + fp), "recall": _ratio(tp, tp + fn), "fpr": _ratio(fp, fp + tn),
            "f1": _ratio(2 * tp, 2 * tp + fp + fn),
            "recall_of_all_true_pairs": _ratio(tp, np.full(len(t), self.true_pairs_total, dtype=np.int64)),
        })

    def m_step_stats(self) -> np.ndarray:
        """The M-step's statistics vector (engine.N_HEAD + 4 per (column, level incl. -1), as spk_em_finalize
        returns it) with match_probability replaced by the label: 1 for MATCH, 0 for NON_MATCH, unlabelled pairs
        left out.  (The log-likelihood slots stay 0: the M-step does not read them.)"""
        nm, nn = self.counts[MATCH], self.counts[NON_MATCH]
        lab = nm + nn
        stats = np.zeros(N_HEAD + 4 * sum(L + 1 for L in self.n_levels), dtype=np.float64)
        stats[0], stats[1], stats[2] = nm.sum(), lab.sum(), lab.sum()
        lev = self.levels(np.arange(self.n_patterns))
        off = N_HEAD
        for k, L in enumerate(self.n_levels):
            for v in range(-1, L):
                at = lev[:, k] == v
                rows = int(lab[at].sum())
                stats[off: off + 4] = (rows, rows, int(nm[at].sum()), int(nn[at].sum()))
                off += 4
        return stats

    def m_step(self):
        """(λ, π rows) in the shape engine.m_step_rows returns: the supervised estimate of the parameters."""
        return m_step_rows(self.m_step_stats(), self.names, self.n_levels)


SCORE_TRUTH_COLUMNS = ("threshold", "tp", "fp", "tn", "fn", "n_unlabelled_above", "precision", "recall", "fpr", "f1",
                       "recall_of_all_true_pairs")  # LabelCounts.truth_table's, in its order


class ScoreLabelCounts:
    """Pairs per (truth state, score bin) where the score is decided per pair (spk_label_scores_*): the counterpart
    of LabelCounts for tf_adjusted_match_prob and for the pairs a filter or a best-match step kept.

    thresholds: T ascending doubles; counts int64 [3, T + 2] by NON_MATCH / MATCH / UNKNOWN: bin b in 0..T holds the
    pairs whose score is above exactly b of the thresholds (`>`), bin T + 1 the pairs with a NULL score.  totals: the
    labelled (NON_MATCH, MATCH) pairs among all candidate pairs of the job, kept or not -- what fn and tn are taken
    against; true_pairs_total as the function of that name gives it."""

    def __init__(self, counts, thresholds, totals, link_type="dedupe_only", true_pairs_total=0):
        self.thresholds = np.ascontiguousarray(thresholds, dtype=np.float64).reshape(-1)
        T = len(self.thresholds)
        if np.isnan(self.thresholds).any() or (self.thresholds[1:] < self.thresholds[:-1]).any():
            raise ValueError("ScoreLabelCounts: the thresholds must be ascending and not NaN")
        self.counts = np.ascontiguousarray(counts, dtype=np.int64)
        if self.counts.shape != (3, T + 2):
            raise ValueError(f"ScoreLabelCounts: counts must be [3, {T + 2}] for {T} thresholds")
        self.totals = (int(totals[NON_MATCH]), int(totals[MATCH]))
        self.link_type = link_type
        self.true_pairs_total = int(true_pairs_total)

    def _rows(self, t, above) -> pd.DataFrame:
        tp, fp, unl = above[MATCH], above[NON_MATCH], above[UNKNOWN]
        fn = self.totals[MATCH] - tp
        tn = self.totals[NON_MATCH] - fp
        return pd.DataFrame({
            "threshold": t, "tp": tp, "fp": fp, "tn": tn, "fn": fn, "n_unlabelled_above": unl,
            "precision": _ratio(tp, tp + fp), "recall": _ratio(tp, tp + fn), "fpr": _ratio(fp, fp + tn),
            "f1": _ratio(2 * tp, 2 * tp + fp + fn),
            "recall_of_all_true_pairs": _ratio(tp, np.full(len(t), self.true_pairs_total, dtype=np.int64)),
        }, columns=list(SCORE_TRUTH_COLUMNS))

    def truth_table(self) -> pd.DataFrame:
        """LabelCounts.truth_table's columns, one row per threshold: row k predicts the pairs of the bins above k
        (score > thresholds[k]); a NULL score is never predicted a match."""
        T = len(self.thresholds)
        # suffix[:, k] = pairs of each state in bins k + 1 .. T
        suffix = np.cumsum(self.counts[:, T:0:-1], axis=1)[:, ::-1] if T else np.zeros((3, 0), dtype=np.int64)
        return self._rows(self.thresholds.copy(), suffix)

    def kept_row(self) -> pd.DataFrame:
        """One row with threshold = -inf that predicts every counted pair, NULL scores included: a filtered or
        best-match frame as it stands."""
        return self._rows(np.array([-np.inf]), self.counts.sum(axis=1).reshape(3, 1))


def estimate_from_labels(df_gammas: object, params, settings: dict, spark: object, label_column: str):
    """The supervised counterpart of iterate(): one M-step over the labelled pairs of `df_gammas` (the frame
    add_gammas returns) with match_probability replaced by `label_column_l == label_column_r`, through
    params._update_params, then the E-step under the new parameters.  Returns that scored frame."""
    from .expectation_step import run_expectation_step
    from .frames import ExpectationFrame, GammaFrame, reject_filtered
    reject_filtered(df_gammas, "estimate_from_labels")
    gf = df_gammas.gammas if isinstance(df_gammas, ExpectationFrame) else df_gammas
    if not isinstance(gf, GammaFrame):
        raise ValueError("estimate_from_labels needs the records' labels: pass the frame add_gammas returns (a gamma "
                         "table has pairs without rows)")
    counts = gf.label_counts(label_column)
    if int(counts.counts[:UNKNOWN].sum()) == 0:
        raise ValueError(f"estimate_from_labels: no pair has a label on both sides in column {label_column!r}")
    lam, rows = counts.m_step()
    params._update_params(lam, rows)
    return run_expectation_step(gf, params, settings, spark)


# ---- labels given as a table of pairs ------------------------------------------------------------------------------
class PairLabelSides(NamedTuple):
    """What pair_label_rows needs to know of a job (frames.pair_label_sides makes one from a Job)."""
    link_type: str
    uid: str                               # the settings' unique_id_column_name
    uids: Sequence[np.ndarray]             # the unique ids in device row order: [table 0], or [left, right] (link_only)
    source: Optional[np.ndarray] = None    # link_and_dedupe: 'left' / 'right' per device row of the concatenated table


def _rows_text(mask, limit=8) -> str:
    at = np.flatnonzero(mask)
    more = f" (and {len(at) - limit} more)" if len(at) > limit else ""
    return "row" + ("s " if len(at) != 1 else " ") + ", ".join(str(int(i)) for i in at[:limit]) + more


def _rows_of_ids(uids, values) -> np.ndarray:
    """The position in `uids` of every value: -1 = not among them, -2 = it occurs there more than once."""
    uids = np.asarray(uids)
    index = pd.Index(uids)
    if index.is_unique:
        return np.asarray(index.get_indexer(values), dtype=np.int64)
    dup = np.asarray(index.duplicated(keep=False))
    once = np.flatnonzero(~dup)
    at = np.asarray(pd.Index(uids[once]).get_indexer(values), dtype=np.int64)
    out = np.where(at >= 0, once[np.maximum(at, 0)], -1) if len(once) else np.full(len(values), -1, dtype=np.int64)
    out[np.asarray(pd.Index(values).isin(uids[dup]))] = -2
    return out


def pair_label_rows(job_like: PairLabelSides, labels: pd.DataFrame, match_threshold: float = 0.5):
    """(rows_l int32, rows_r int32, is_match uint8): the labelled pairs of `labels` as device rows, in its row order.

    labels: `<uid>_l`, `<uid>_r` and `clerical_match_score` (a number or a bool); a pair is a match iff its score >=
    match_threshold (the later releases' threshold_actual).  Under link_only `_l` names a record of df_l and `_r` one
    of df_r; under link_and_dedupe the optional `_source_table_l` / `_source_table_r` ('left' / 'right') say which
    input each id belongs to, and are required for an id that both inputs hold; otherwise the order of a pair does not
    matter.  ValueError, naming the rows of `labels` at fault (positions, from 0): a missing column, a NULL id or
    score, an id that is not in the table, a pair of a record with itself, a pair given twice (in either order where
    the order does not matter, whether or not the scores agree)."""
    uid = job_like.uid
    col_l, col_r, col_s = f"{uid}_l", f"{uid}_r", "clerical_match_score"
    missing = [c for c in (col_l, col_r, col_s) if c not in labels.columns]
    if missing:
        raise ValueError(f"pair labels: the labels table has no column {', '.join(map(repr, missing))}")
    a, b, score = labels[col_l], labels[col_r], labels[col_s]
    null = (a.isna() | b.isna() | score.isna()).to_numpy()
    if null.any():
        raise ValueError(f"pair labels: a NULL id or score in {_rows_text(null)}")
    is_match = (score.to_numpy(dtype=np.float64) >= float(match_threshold)).astype(np.uint8)
    a, b = a.to_numpy(), b.to_numpy()
    one_table = job_like.link_type != "link_only"
    src_cols = [c for c in ("_source_table_l", "_source_table_r") if c in labels.columns]
    if job_like.link_type == "link_and_dedupe" and src_cols:
        if len(src_cols) != 2:
            raise ValueError("pair labels: _source_table_l and _source_table_r come together")
        source = np.asarray(job_like.source)
        halves = {s: np.flatnonzero(source == s) for s in ("left", "right")}
        rows = []
        for values, col in ((a, "_source_table_l"), (b, "_source_table_r")):
            src = labels[col].to_numpy()
            other = ~np.isin(src, ("left", "right"))
            if other.any():
                raise ValueError(f"pair labels: {col} is neither 'left' nor 'right' in {_rows_text(other)}")
            out = np.full(len(values), -1, dtype=np.int64)
            for s, half in halves.items():
                pick = src == s
                at = _rows_of_ids(np.asarray(job_like.uids[0])[half], values[pick])
                out[pick] = np.where(at >= 0, half[np.maximum(at, 0)], at) if len(half) else -1
            rows.append(out)
        rows_l, rows_r = rows
    else:
        rows_l = _rows_of_ids(job_like.uids[0], a)
        rows_r = _rows_of_ids(job_like.uids[0 if one_table else 1], b)
    twice = (rows_l == -2) | (rows_r == -2)
    if twice.any():
        hint = (": give _source_table_l / _source_table_r ('left' / 'right')"
                if job_like.link_type == "link_and_dedupe" and not src_cols else "")
        raise ValueError(f"pair labels: an id that more than one input record carries in {_rows_text(twice)}{hint}")
    absent = (rows_l < 0) | (rows_r < 0)
    if absent.any():
        raise ValueError(f"pair labels: an id that is not in the input table in {_rows_text(absent)}")
    if one_table:
        same = rows_l == rows_r
        if same.any():
            raise ValueError(f"pair labels: a pair of a record with itself in {_rows_text(same)}")
        lo, hi = np.minimum(rows_l, rows_r), np.maximum(rows_l, rows_r)
    else:
        lo, hi = rows_l, rows_r
    _, inverse, n_given = np.unique((lo << 32) | hi, return_inverse=True, return_counts=True)
    again = n_given[inverse.reshape(-1)] > 1
    if again.any():
        raise ValueError(f"pair labels: the same pair more than once in {_rows_text(again)}")
    return rows_l.astype(np.int32), rows_r.astype(np.int32), is_match


class PairLabelCounts(LabelCounts):
    """LabelCounts of the candidate pairs against a table of labelled pairs (spk_label_pairs_histogram): MATCH and
    NON_MATCH hold the labelled candidate pairs, UNKNOWN the candidate pairs without a label.

    labels: the labels table; is_match [len(labels)]: its thresholded scores; label_code [len(labels)]: the packed
    code of the candidate pair each label names, -1 when blocking did not produce it.  true_pairs_total is the number
    of labelled matches, so missed_by_blocking counts the labelled matches that are not among the candidates and
    recall_of_all_true_pairs is taken over all labelled matches; truth_table(), patterns() and m_step() are
    LabelCounts' own."""

    def __init__(self, names, n_levels, counts, mp, link_type, labels, is_match, label_code):
        self.labels = labels
        self.is_match = np.ascontiguousarray(is_match).astype(bool)
        self.label_code = np.ascontiguousarray(label_code, dtype=np.int64)
        if not len(labels) == len(self.is_match) == len(self.label_code):
            raise ValueError("PairLabelCounts: labels, is_match and label_code differ in length")
        super().__init__(names, n_levels, counts, mp, link_type, true_pairs_total=int(self.is_match.sum()))
        if len(self.label_code) and int(self.label_code.max()) >= self.n_patterns:
            raise ValueError("PairLabelCounts: a label_code outside the pattern space")
        self.non_matches_missed_by_blocking = int((~self.is_match).sum()) - int(self.counts[NON_MATCH].sum())

    def labelled_pairs(self) -> pd.DataFrame:
        """The labels table in its own row order plus found_by_blocking, the gamma_* levels of the candidate pair and,
        if scored, its match_probability (both NULL when blocking did not produce the pair)."""
        found = self.label_code >= 0
        out = self.labels.copy()
        out["found_by_blocking"] = found
        lev = self.levels(np.where(found, self.label_code, 0))
        for k, name in enumerate(self.names):
            out[name] = pd.arrays.IntegerArray(lev[:, k].astype(np.int32), mask=~found)
        if self.mp is not None:
            mp = np.full(len(found), np.nan, dtype=np.float64)
            mp[found] = self.mp[self.label_code[found]]
            out["match_probability"] = mp
        return out

    def prediction_errors(self, threshold: float) -> pd.DataFrame:
        """The rows of labelled_pairs() that `match_probability > threshold` gets wrong, with a column `error`: "fp"
        for a labelled non-match above the threshold, "fn" for a labelled match that is not -- a NULL score is never
        predicted a match, so a labelled match that blocking did not produce is an "fn"."""
        if self.mp is None:
            raise ValueError("prediction_errors: these counts carry no match_probability: take them from the frame "
                             "run_expectation_step returns")
        pairs = self.labelled_pairs()
        predicted = pairs["match_probability"].to_numpy() > float(threshold)
        fp, fn = predicted & ~self.is_match, ~predicted & self.is_match
        out = pairs[fp | fn].copy()
        out["error"] = np.where(fp[fp | fn], "fp", "fn")
        return out


class PairScoreLabelCounts(ScoreLabelCounts):
    """ScoreLabelCounts of a frame's pairs against a table of labelled pairs (spk_label_pairs_scores_*): the
    counterpart of PairLabelCounts for tf_adjusted_match_prob and for the pairs a filter or a best-match step kept.

    labels: the labels table; is_match [len(labels)]: its thresholded scores; label_score [len(labels)]: the score
    (the column `score_name`) of the frame's pair each label names, NaN when the frame has no such pair or its score
    is NULL; label_pair [len(labels)]: that pair's index in the frame, -1 = none, or None on a sharded job (the index
    is local to a rank) -- then `found` [len(labels)] says which labels name a pair of the frame.  found_by_blocking
    [len(labels)] (selection frames; None: the frame holds every candidate pair, so it is `found`): the label names
    a candidate pair of the job, kept or not.  true_pairs_total is the number of labelled matches, as in
    PairLabelCounts; truth_table() and kept_row() are ScoreLabelCounts' own."""

    def __init__(self, counts, thresholds, totals, link_type, labels, is_match, label_score, score_name,
                 label_pair=None, found=None, found_by_blocking=None):
        self.labels = labels
        self.is_match = np.ascontiguousarray(is_match).astype(bool)
        self.label_score = np.ascontiguousarray(label_score, dtype=np.float64)
        self.score_name = str(score_name)
        n = len(labels)
        if (label_pair is None) == (found is None):
            raise ValueError("PairScoreLabelCounts: give label_pair, or found on a sharded job")
        self.label_pair = None if label_pair is None else np.ascontiguousarray(label_pair, dtype=np.int64)
        self.found = self.label_pair >= 0 if found is None else np.ascontiguousarray(found).astype(bool)
        self.selection = found_by_blocking is not None
        self.found_by_blocking = (np.ascontiguousarray(found_by_blocking).astype(bool) if self.selection
                                  else self.found.copy())
        if not n == len(self.is_match) == len(self.label_score) == len(self.found) == len(self.found_by_blocking):
            raise ValueError("PairScoreLabelCounts: labels, is_match, label_score, label_pair and found_by_blocking "
                             "differ in length")
        if (self.found & ~self.found_by_blocking).any():
            raise ValueError("PairScoreLabelCounts: a label names a pair of the frame that blocking did not produce")
        if (~self.found & ~np.isnan(self.label_score)).any():
            raise ValueError("PairScoreLabelCounts: a score for a label that names no pair of the frame")
        super().__init__(counts, thresholds, totals, link_type, true_pairs_total=int(self.is_match.sum()))
        # a pair set may repeat a pair, so more pairs than labels may be counted, never fewer
        if int(self.counts[MATCH].sum()) < int((self.found & self.is_match).sum()) or \
                int(self.counts[NON_MATCH].sum()) < int((self.found & ~self.is_match).sum()):
            raise ValueError("PairScoreLabelCounts: fewer labelled pairs counted than labels found")

    def labelled_pairs(self) -> pd.DataFrame:
        """The labels table in its own row order plus found_by_blocking, for a filtered or best-match frame `kept`
        (the frame holds the pair), and the score column (NaN where the frame has no such pair)."""
        out = self.labels.copy()
        out["found_by_blocking"] = self.found_by_blocking
        if self.selection:
            out["kept"] = self.found
        out[self.score_name] = self.label_score
        return out

    def prediction_errors(self, threshold: float) -> pd.DataFrame:
        """The rows of labelled_pairs() that `score > threshold` gets wrong, with a column `error`: "fp" for a
        labelled non-match above the threshold, "fn" for a labelled match that is not -- a NULL score is never
        predicted a match, so a labelled match that is not among the frame's pairs is an "fn"."""
        pairs = self.labelled_pairs()
        predicted = self.label_score > float(threshold)
        fp, fn = predicted & ~self.is_match, ~predicted & self.is_match
        out = pairs[fp | fn].copy()
        out["error"] = np.where(fp[fp | fn], "fp", "fn")
        return out


def estimate_from_pair_labels(df_gammas: object, params, settings: dict, spark: object, labels: pd.DataFrame,
                              match_threshold: float = 0.5):
    """estimate_from_labels with the truth taken from a table of labelled pairs (pair_label_rows' columns): one M-step
    over the labelled candidate pairs, then the E-step under the new parameters.  Returns that scored frame."""
    from .expectation_step import run_expectation_step
    from .frames import ExpectationFrame, GammaFrame, reject_filtered
    reject_filtered(df_gammas, "estimate_from_pair_labels")
    gf = df_gammas.gammas if isinstance(df_gammas, ExpectationFrame) else df_gammas
    if not isinstance(gf, GammaFrame):
        raise ValueError("estimate_from_pair_labels needs the records: pass the frame add_gammas returns (a gamma "
                         "table has pairs without rows)")
    counts = gf.label_counts_from_pairs(labels, match_threshold)
    if int(counts.counts[:UNKNOWN].sum()) == 0:
        raise ValueError("estimate_from_pair_labels: no labelled pair is among the candidate pairs")
    lam, rows = counts.m_step()
    params._update_params(lam, rows)
    return run_expectation_step(gf, params, settings, spark)
