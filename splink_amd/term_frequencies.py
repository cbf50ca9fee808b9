"""Term-frequency adjustment (reference: splink/term_frequencies.py:122-168).

Per tf column c: over pairs whose c_l and c_r are equal and non-NULL, the mean match
probability per value (adj_lambda, :49-65) is Bayes-combined with 1-λ; pairs without a
lookup value get 0.5 (:68-95); tf_adjusted_match_prob = bayes(mp, adj_c1, ...) (:98-117).
The per-value sums and the per-pair Bayes combination run on the GPU
(spk_tf_scales, spk_tf_accumulate_exact / spk_tf_apply): the sums are exact fixed-point accumulators
relative to each value's largest term, so ranks
holding shards of the pairs all-reduce them as integers and every run and rank count gives
bit-identical adjustments; the per-value lookup arithmetic is a handful of operations per value.
"""
import warnings
from collections import OrderedDict

import numpy as np
import pandas as pd

from . import _native as N
from . import distributed as D
from . import table as T
from .check_types import check_types
from .frames import (ExpectationFrame, FilteredFrame, SplinkDataFrame, _HostColumns, df_e_column_order,
                     reject_filtered)
from .params import Params
from .select import compile_condition


def _bayes_pair(a, b):
    """sql_gen_bayes_string([a, b]) (:21-46) for vectors a and a scalar b."""
    num = a * b
    den = num + (1.0 - a) * (1.0 - b)
    with np.errstate(invalid="ignore", divide="ignore"):
        out = num / den
    out[den == 0] = np.nan
    return out


class TermFrequencyFrame(SplinkDataFrame):
    """The tf stage's frame.  The per-value adjustment tables are computed when it is made; the per-pair part
    (spk_tf_apply*) runs on the first toPandas(), and filter() / clusters() / truth_table() never run it: they select
    (spk_select_tf*) or count (spk_label_scores_tf*) on the device and copy the survivors or the counts only."""

    def __init__(self, df_e: ExpectationFrame, settings, tf_cols, tables, one_minus, retain_adjustment_columns,
                 dev_cols=None, host_ids=None):
        self.df_e = df_e
        self.job = df_e.job
        self.settings = settings
        self.tf_cols = tf_cols
        self.tables = tables        # per tf column: the adjustment per value id
        self.one_minus = one_minus  # the 1 - λ the tables were combined with
        self.dev_cols = dev_cols    # the columns' device dictionary ids ...
        self.host_ids = host_ids    # ... or (ids of side 0, ids of side 1) per column, factorised on the host
        self.retain = retain_adjustment_columns
        self._pair = None           # (tf_adjusted_match_prob, adjustments [P, n_tf])

    def _apply(self):
        if self._pair is None:
            job = self.job
            self.df_e.gammas.ensure_codes()
            job.score(self.df_e.lam, self.df_e.level_probs, want_host=False)  # device mp for exactly this df_e
            if self.dev_cols is not None:
                self._pair = job.ctx.tf_apply_columns(self.dev_cols, self.tables, 0, job.n_pairs, want_adj=True)
            else:
                ids0, ids1 = self.host_ids
                self._pair = job.ctx.tf_apply(ids0, ids1, self.tables, 0, job.n_pairs, want_adj=True)
        return self._pair

    @property
    def tf_mp(self):
        return self._apply()[0]

    @property
    def adj(self):
        return self._apply()[1]

    def _column_order(self):
        cols = ["tf_adjusted_match_prob", "match_probability"] + df_e_column_order(self.settings, tf_adj_cols=True)
        if not self.retain:
            cols = [c for c in cols if not (c.endswith("_adj") and c[:-4] in self.tf_cols)]
        return cols

    def toPandas(self):
        base = self.df_e.toPandas()
        data = OrderedDict()
        for c in self._column_order():
            if c == "tf_adjusted_match_prob":
                data[c] = self.tf_mp
            elif c.endswith("_adj") and c[:-4] in self.tf_cols:
                data[c] = self.adj[:, self.tf_cols.index(c[:-4])]
            else:
                data[c] = base[c].to_numpy()
        return pd.DataFrame(data)

    def filter(self, condition):
        """tf.filter("tf_adjusted_match_prob > 0.99 and gamma_surname >= 1"): the pairs for which the condition is
        TRUE, selected on the device (spk_select_tf*); only the survivors come back, with every column of this
        frame."""
        return TfFilteredFrame(self, compile_condition(condition, self.df_e.gammas.meta[0], allow_mp=True,
                                                       allow_tf=True))

    where = filter

    def clusters(self, threshold):
        """Shorthand for filter(f"tf_adjusted_match_prob > {threshold!r}").clusters()."""
        return self.filter(f"tf_adjusted_match_prob > {threshold!r}").clusters()

    def clusters_at_thresholds(self, thresholds):
        """Shorthand for filter(f"tf_adjusted_match_prob > {min(thresholds)!r}").clusters_at_thresholds(thresholds)."""
        from .frames import sweep_thresholds
        given, _, _ = sweep_thresholds(thresholds)
        return self.filter(f"tf_adjusted_match_prob > {min(given)!r}").clusters_at_thresholds(given)

    def best_matches(self, threshold=None, per="l", ties="first"):
        """Shorthand for filter(f"tf_adjusted_match_prob > {threshold!r}").best_matches(per, ties); threshold=None:
        the best match among every pair."""
        from .select import Predicate
        f = (TfFilteredFrame(self, Predicate()) if threshold is None
             else self.filter(f"tf_adjusted_match_prob > {threshold!r}"))
        return f.best_matches(per=per, ties=ties)

    def orderBy(self, col, ascending=True):  # noqa: N802 (Spark name)
        """tf.orderBy("tf_adjusted_match_prob", ascending=False).limit(k): the first k pairs by tf_adjusted_match_prob
        (or match_probability), selected on the device.  Shorthand for the same call on the unfiltered frame."""
        from .select import Predicate
        return TfFilteredFrame(self, Predicate()).orderBy(col, ascending)

    sort = orderBy

    def limit(self, k):
        """The first k pairs of this frame, in its order: shorthand for the same call on the unfiltered frame."""
        from .select import Predicate
        return TfFilteredFrame(self, Predicate()).limit(k)

    def truth_table(self, label_column, thresholds=None):
        """The confusion matrix of `tf_adjusted_match_prob > threshold` against the labels in the input column
        `label_column`, with df_e.truth_table's columns: the score is decided per pair on the device
        (spk_label_scores_tf*), the per-pair part of this frame never runs and no pair leaves the device.
        thresholds=None: the thresholds of df_e.truth_table(label_column), so the two tables line up row for row."""
        from .frames import _label_ids, _score_label_counts, _score_thresholds
        job, df_e = self.job, self.df_e
        if getattr(job, "passthrough", None) is not None:
            raise ValueError("truth_table() needs the records: a job made from a gamma table has pairs without rows")
        lab0, lab1 = _label_ids(job, label_column)  # a missing column fails before the device is touched
        if thresholds is None:
            thresholds = df_e.truth_table(label_column)["threshold"].to_numpy()
        t = _score_thresholds(thresholds, "truth_table")
        df_e.gammas.ensure_codes()
        m, u = job.flat_tables(df_e.level_probs)
        lam = float(df_e.lam)
        if self.dev_cols is not None:
            counts = job.ctx.label_scores_tf_columns(lab0, lab1, lam, float(1 - df_e.lam), m, u, self.dev_cols,
                                                     self.tables, t)
        else:
            ids0, ids1 = self.host_ids
            counts = job.ctx.label_scores_tf(lab0, lab1, lam, float(1 - df_e.lam), m, u, ids0, ids1, self.tables, t)
        return _score_label_counts(job, counts, None, t, lab0, lab1).truth_table()

    def label_counts_from_pairs(self, labels, match_threshold=0.5, thresholds=None):
        """Every pair of this frame against a table of labelled pairs (a clerical-review sample:
        labels.pair_label_rows' columns), by tf_adjusted_match_prob, counted on the device
        (spk_label_pairs_scores_tf*): a `PairScoreLabelCounts`.  The per-pair part of this frame never runs and no
        pair leaves the device but the scores of the labelled ones.  thresholds=None: the thresholds of
        df_e.truth_table_from_pairs(labels, match_threshold=match_threshold), so the two tables line up row for row."""
        from .frames import _pair_label_input, _pair_score_label_counts, _score_thresholds
        job, df_e = self.job, self.df_e
        labels, rows_l, rows_r, is_match = _pair_label_input(job, labels, match_threshold, "label_counts_from_pairs")
        if thresholds is None:
            thresholds = df_e.truth_table_from_pairs(labels, None, match_threshold)["threshold"].to_numpy()
        t = _score_thresholds(thresholds, "label_counts_from_pairs")
        df_e.gammas.ensure_codes()
        m, u = job.flat_tables(df_e.level_probs)
        lam = float(df_e.lam)
        if self.dev_cols is not None:
            counts, pair, score = job.ctx.label_pair_scores_tf_columns(rows_l, rows_r, is_match, lam,
                                                                       float(1 - df_e.lam), m, u, self.dev_cols,
                                                                       self.tables, t)
        else:
            ids0, ids1 = self.host_ids
            counts, pair, score = job.ctx.label_pair_scores_tf(rows_l, rows_r, is_match, lam, float(1 - df_e.lam), m,
                                                               u, ids0, ids1, self.tables, t)
        return _pair_score_label_counts(job, labels, is_match, counts, pair, score, t, "tf_adjusted_match_prob")

    def truth_table_from_pairs(self, labels, thresholds=None, match_threshold=0.5):
        """The confusion matrix of `tf_adjusted_match_prob > threshold` against a table of labelled pairs, with
        df_e.truth_table_from_pairs' columns.  Shorthand for
        label_counts_from_pairs(labels, match_threshold, thresholds).truth_table()."""
        return self.label_counts_from_pairs(labels, match_threshold, thresholds).truth_table()


class TfFilteredFrame(FilteredFrame):
    """`tf.filter(condition)`: toPandas() equals tf.toPandas()[mask].reset_index(drop=True).  A predicate without a
    tf term is selected the same way, since the survivors carry the tf columns either way."""

    def __init__(self, parent: TermFrequencyFrame, predicate):
        super().__init__(parent, predicate)
        self.gammas = parent.df_e.gammas

    def filter(self, condition):
        more = compile_condition(condition, self.gammas.meta[0], allow_mp=True, allow_tf=True)
        return TfFilteredFrame(self.parent, self.predicate.and_(more))

    where = filter

    # best_matches() ranks by tf_adjusted_match_prob unless by="match_probability"
    _best_by = ("tf_adjusted_match_prob", "match_probability")

    def _scored_parent(self):
        return self.parent.df_e

    def sample_pairs(self, *args, **kwargs):
        raise ValueError("sample_pairs() on a term-frequency frame: tf_adjusted_match_prob is decided per pair, and "
                         "the strata are decided per comparison pattern (sample the frame "
                         "run_expectation_step returns, on match_probability)")

    def _select(self):
        job, tf = self.job, self.parent
        self.gammas.ensure_codes()
        if self._n is not None and job.selection_owner is self and self._seq == job.codes_seq:
            return self._n
        df_e = tf.df_e
        m, u = job.flat_tables(df_e.level_probs)
        lam, terms = float(df_e.lam), self.predicate.native_terms()
        if tf.dev_cols is not None:
            n = job.ctx.select_tf_columns(lam, float(1 - df_e.lam), m, u, tf.dev_cols, tf.tables, terms)
        else:
            ids0, ids1 = tf.host_ids
            n = job.ctx.select_tf(lam, float(1 - df_e.lam), m, u, ids0, ids1, tf.tables, terms)
        job.selection_owner = self
        self._seq = job.codes_seq
        self._n = int(n)
        return self._n

    def _extra_columns(self, n):
        tf = self.parent
        if n:
            tf_mp, adj = self.job.ctx.select_copy_tf(0, n, len(tf.tf_cols), adj=tf.retain)
        else:
            tf_mp, adj = np.empty(0, dtype=np.float64), np.empty((0, len(tf.tf_cols)), dtype=np.float64)
        out = {"tf_adjusted_match_prob": tf_mp}
        if tf.retain:
            for i, c in enumerate(tf.tf_cols):
                out[c + "_adj"] = adj[:, i]
        return out


@check_types
def make_adjustment_for_term_frequencies(df_e: object, params: Params, settings: dict, spark: object,
                                         retain_adjustment_columns: bool = False):
    reject_filtered(df_e, "make_adjustment_for_term_frequencies")
    tf_cols = [c["col_name"] for c in settings["comparison_columns"] if c["term_frequency_adjustments"] is True]
    if not tf_cols:
        warnings.warn("No term frequency adjustment columns are specified in your settings object.  "
                      "Returning original df")
        return df_e
    job = df_e.job
    df_e.gammas.ensure_codes()
    job.score(df_e.lam, df_e.level_probs, want_host=False)  # device mp for exactly this df_e
    one_minus = float(1 - params.params["λ"])
    # value ids: the device dictionary ids of the string column when the job decoded it on the device
    # (no host pass over the values), else a joint host factorisation
    dev_cols = [job._col_index.get((c, "str")) for c in tf_cols]
    on_device = all(i is not None for i in dev_cols)
    ids0_list, ids1_list, tables = [], [], []
    shared = job.reduces_across_ranks()  # the reference groups over ALL pairs (:49-65); ranks hold shards
    for c, col in zip(tf_cols, dev_cols):
        # two passes over the pairs: each value's scale (the exponent of its largest mp; MAX over ranks),
        # then the fixed-point sums relative to it (integer SUM over ranks): every rank ends with the
        # one-GPU result, and tiny match probabilities keep their relative precision
        if on_device:
            n_values = job.ctx.tf_column_values(col)
            scale = job.ctx.tf_scales_column(col, n_values)
        else:
            sides = (0, 1) if job.link_type == "link_only" else (0,)
            vals = [pd.Series([None if T.is_null_scalar(v) else v for v in job.host_values(s, c).tolist()],
                              dtype=object) for s in sides]
            codes, n_values = T.factorize_joint(vals)
            ids0 = codes[0]
            ids1 = codes[1] if len(codes) > 1 else codes[0]
            scale = job.ctx.tf_scales(n_values, ids0, ids1)
            ids0_list.append(ids0)
            ids1_list.append(ids1)
        if shared:
            D.allreduce_host_(scale, op="max")
        if on_device:
            limbs, counts = job.ctx.tf_accumulate_column_exact(col, n_values, scale)
        else:
            limbs, counts = job.ctx.tf_accumulate_exact(n_values, ids0, ids1, scale)
        if shared:
            # exact fixed-point sums and integer counts: the all-reduce gives every rank the one-GPU result
            D.allreduce_host_(limbs)
            D.allreduce_host_(counts)
        sums = N.tf_limbs_to_sum(limbs, scale)
        with np.errstate(invalid="ignore", divide="ignore"):
            adj_lambda = np.where(counts > 0, sums / np.maximum(counts, 1), np.nan)
        tables.append(_bayes_pair(adj_lambda, one_minus))
    # the per-pair part is left to the frame: toPandas() applies the tables to every pair, filter() / clusters()
    # select on the device and copy the survivors only
    return TermFrequencyFrame(df_e, settings, tf_cols, tables, one_minus, retain_adjustment_columns,
                              dev_cols=dev_cols if on_device else None,
                              host_ids=None if on_device else (ids0_list, ids1_list))
