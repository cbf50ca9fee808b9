"""Device-resident, lazily materialised frames returned by the stage functions.

They stand where the reference returns Spark DataFrames (blocking.py:162, gammas.py:93,
expectation_step.py:26, term_frequencies.py:123) and offer the slice of that surface the
pipeline and its users need: `toPandas()`, `count()`, `columns`, `persist()` / `cache()` /
`unpersist()`, `createOrReplaceTempView()`.  Pairs, comparison codes and scores stay on the
GPU; `toPandas()` copies them back and gathers the retained input columns with the
reference's column names and order.  `filter(condition)` / `where` (Spark's DataFrame.filter on the
scored frame, or on the term-frequency stage's frame: term_frequencies.py) select on the device instead: a
`FilteredFrame` copies back the survivors only, and its `clusters()` (GraphFrames' connectedComponents over the
kept pairs) leaves the device with one label per record.  Its `best_matches(per, ties)` (the users' window query
row_number() over (partition by unique_id_l order by match_probability desc) = 1) narrows the survivors to the best
pair per record on the device: a `BestMatchFrame`.
"""
from __future__ import annotations

from collections import OrderedDict

import numpy as np
import pandas as pd


class SplinkDataFrame:
    """Common surface of the lazily evaluated frames."""

    def toPandas(self) -> pd.DataFrame:  # noqa: N802 (Spark name)
        raise NotImplementedError

    def to_pandas(self) -> pd.DataFrame:
        return self.toPandas()

    def count(self) -> int:
        return int(self.job.n_pairs)

    def __len__(self):
        return self.count()

    @property
    def columns(self):
        return list(self._column_order())

    def persist(self, *args, **kwargs):
        return self

    cache = persist

    def unpersist(self, *args, **kwargs):
        return self

    def createOrReplaceTempView(self, name):  # noqa: N802 (Spark name)
        return None


def _add_lr(cols: "OrderedDict", name: str):
    cols[name + "_l"] = None
    cols[name + "_r"] = None


def comparison_column_order(settings, link_type):
    """blocking.py:18-36 + _get_columns_to_retain_blocking, with _source_table for link_and_dedupe."""
    from .engine import columns_to_retain_blocking
    cols = columns_to_retain_blocking(settings)
    if link_type == "link_and_dedupe":
        cols = cols + ["_source_table"]
    out = OrderedDict()
    for c in cols:
        _add_lr(out, c)
    return list(out)


def gamma_column_order(settings):
    """gammas.py:25-62."""
    out = OrderedDict()
    _add_lr(out, settings["unique_id_column_name"])
    for col in settings["comparison_columns"]:
        if "col_name" in col:
            name = col["col_name"]
            if settings["retain_matching_columns"] or col["term_frequency_adjustments"]:
                _add_lr(out, name)
            out["gamma_" + name] = None
        if "custom_name" in col:
            if settings["retain_matching_columns"]:
                for c2 in col["custom_columns_used"]:
                    _add_lr(out, c2)
            out["gamma_" + col["custom_name"]] = None
    if settings["link_type"] == "link_and_dedupe":
        _add_lr(out, "_source_table")
    for c in settings["additional_columns_to_retain"]:
        _add_lr(out, c)
    return list(out)


def df_e_column_order(settings, tf_adj_cols=False):
    """expectation_step.py:128-165."""
    out = OrderedDict()
    _add_lr(out, settings["unique_id_column_name"])
    for col in settings["comparison_columns"]:
        if "col_name" in col:
            name = col["col_name"]
            if settings["retain_matching_columns"] or col["term_frequency_adjustments"]:
                _add_lr(out, name)
            out["gamma_" + name] = None
        if "custom_name" in col:
            name = col["custom_name"]
            if settings["retain_matching_columns"]:
                for c2 in col["custom_columns_used"]:
                    _add_lr(out, c2)
            out["gamma_" + name] = None
        if settings["retain_intermediate_calculation_columns"]:
            out[f"prob_gamma_{name}_non_match"] = None
            out[f"prob_gamma_{name}_match"] = None
            if tf_adj_cols and col.get("term_frequency_adjustments"):
                out[name + "_adj"] = None
    if settings["link_type"] == "link_and_dedupe":
        _add_lr(out, "_source_table")
    for c in settings["additional_columns_to_retain"]:
        _add_lr(out, c)
    return list(out)


class _HostColumns:
    """Gathers `<col>_l` / `<col>_r` values for the job's pairs from the host input tables."""

    def __init__(self, job):
        self.job = job
        self._cache = {}

    def get(self, name):
        if name in self._cache:
            return self._cache[name]
        job = self.job
        if getattr(job, "passthrough", None) is not None:
            df = job.passthrough
            if name not in df.columns:
                raise KeyError(name)
            v = df[name].to_numpy()
        else:
            base, side = name[:-2], name[-2:]
            rows_l, rows_r = job.pair_rows()
            s = 0 if side == "_l" else job.r_side()
            if base not in job.inputs[s].columns:
                raise KeyError(name)
            v = job.host_values(s, base)[rows_l if side == "_l" else rows_r]
        self._cache[name] = v
        return v


def _label_ids(job, label_column):
    """(ids of side 0, ids of side 1 or None): one dense label id per record in device row order, -1 = NULL, one
    id space for both sides (link_only: side 1 is the right table; otherwise the right rows index table 0)."""
    from . import table as T
    sides = (0, 1) if job.link_type == "link_only" else (0,)
    for s in sides:
        if label_column not in job.inputs[s].columns:
            raise ValueError(f"label column {label_column!r} is missing from input table {s}")
    key = ("label_ids", label_column)  # kept with the host columns: a new row order (block) drops both
    if key not in job._host_cols:
        vals = []
        for s in sides:
            v = job.host_values(s, label_column)
            if v.dtype == object:
                v = pd.Series([None if T.is_null_scalar(x) else x for x in v.tolist()], dtype=object)
            vals.append(pd.Series(v))  # numeric dtypes: NaN / NaT are the NULLs, and factorize gives them -1
        codes, _ = T.factorize_joint(vals)
        job._host_cols[key] = (codes[0], codes[1] if len(codes) > 1 else None)
    return job._host_cols[key]


def _node_label_ids(job, label_column):
    """One dense label id per record in node order -- the input tables' own row order, left rows then right, as the
    cluster frames number their records -- with _label_ids' NULL rules (-1 = NULL, one id space).  Not
    job.host_values: that is in device row order."""
    from . import table as T
    for s, t in enumerate(job.inputs):
        if label_column not in t.columns:
            raise ValueError(f"label column {label_column!r} is missing from input table {s}")
    key = ("node_label_ids", label_column)
    if key not in job._host_cols:
        vals = []
        for t in job.inputs:
            col = t[label_column]
            if isinstance(col.dtype, pd.api.extensions.ExtensionDtype):  # Arrow / nullable: NULL as None
                v = col.to_numpy(dtype=object, na_value=None)
            else:
                v = col.to_numpy()
            if v.dtype == object:
                v = pd.Series([None if T.is_null_scalar(x) else x for x in v.tolist()], dtype=object)
            vals.append(pd.Series(v))
        codes, _ = T.factorize_joint(vals)
        job._host_cols[key] = np.concatenate([np.asarray(c, dtype=np.int64) for c in codes])
    return job._host_cols[key]


def _cluster_agreement(job, label_column):
    """int64 [levels, 10]: every level of the sweep the context holds against `label_column` (spk_cluster_agreement)."""
    ids = _node_label_ids(job, label_column)
    return job.ctx.cluster_agreement(ids, len(job.inputs[0]), job.link_type == "link_only")


def _label_counts(gamma_frame, label_column, lam=None, level_probs=None):
    """LabelCounts of a frame's pairs against `label_column` of the input tables (spk_label_histogram); with lam /
    level_probs also the match_probability of every pattern under them."""
    from . import distributed as D
    from .labels import LabelCounts, true_pairs_total
    job = gamma_frame.job
    if getattr(job, "passthrough", None) is not None:
        raise ValueError("label_counts() needs the records: a job made from a gamma table has pairs without rows")
    ids0, ids1 = _label_ids(job, label_column)
    gamma_frame.ensure_codes()
    if level_probs is None:
        counts, mp = job.ctx.label_histogram(ids0, ids1)
    else:
        m, u = job.flat_tables(level_probs)
        counts, mp = job.ctx.label_histogram(ids0, ids1, float(lam), float(1 - lam), m, u)
    if job.reduces_across_ranks() or job.force_reduce:
        # ranks hold shards of the pairs: exact integer sums, so every rank ends with the one-GPU counts.  Every
        # rank holds all the records, so the true pairs are counted locally.
        D.allreduce_host_(counts, force=job.force_reduce)
    names, levels = gamma_frame.meta
    return LabelCounts(names, levels, counts, mp, job.link_type, true_pairs_total(job.link_type, ids0, ids1))


def pair_label_sides(job):
    """labels.PairLabelSides of a job: its unique ids (and, link_and_dedupe, source tables) in device row order."""
    from .labels import PairLabelSides
    sides = (0, 1) if job.link_type == "link_only" else (0,)
    for s in sides:
        if job.uid not in job.inputs[s].columns:
            raise ValueError(f"unique_id_column_name {job.uid!r} is not a column of input table {s}")
    source = job.host_values(0, "_source_table") if job.link_type == "link_and_dedupe" else None
    return PairLabelSides(job.link_type, job.uid, [job.host_values(s, job.uid) for s in sides], source)


def _pair_label_counts(gamma_frame, labels, match_threshold, lam=None, level_probs=None):
    """PairLabelCounts of a frame's pairs against the labels table `labels` (labels.pair_label_rows' columns;
    spk_label_pairs_histogram); with lam / level_probs also the match_probability of every pattern under them."""
    from . import distributed as D
    from .labels import PairLabelCounts, pair_label_rows
    job = gamma_frame.job
    if getattr(job, "passthrough", None) is not None:
        raise ValueError("label_counts_from_pairs() needs the records: a job made from a gamma table has pairs "
                         "without rows")
    if not isinstance(labels, pd.DataFrame):
        from .blocking import as_pandas
        labels = as_pandas(labels)
    rows_l, rows_r, is_match = pair_label_rows(pair_label_sides(job), labels, match_threshold)
    gamma_frame.ensure_codes()
    if level_probs is None:
        counts, mp, code = job.ctx.label_pairs_histogram(rows_l, rows_r, is_match)
    else:
        m, u = job.flat_tables(level_probs)
        counts, mp, code = job.ctx.label_pairs_histogram(rows_l, rows_r, is_match, float(lam), float(1 - lam), m, u)
    if job.reduces_across_ranks() or job.force_reduce:
        # ranks hold shards of the pairs: the counts sum exactly, and a labelled pair is a candidate of one rank only
        # (-1 on the others), so the maximum is its code
        D.allreduce_host_(counts, force=job.force_reduce)
        D.allreduce_host_(code, force=job.force_reduce, op="max")
    names, levels = gamma_frame.meta
    return PairLabelCounts(names, levels, counts, mp, job.link_type, labels, is_match, code)


def _score_thresholds(thresholds, what):
    """Thresholds as the spk_label_scores_* calls take them: float64, ascending (sorted here, as
    LabelCounts.truth_table sorts them), no NaN, at most _native.LABEL_SCORE_MAX_THRESHOLDS."""
    from . import _native as N
    t = np.sort(np.asarray(list(thresholds), dtype=np.float64).reshape(-1))
    if np.isnan(t).any():
        raise ValueError(f"{what}: a threshold is NaN")
    if len(t) > N.LABEL_SCORE_MAX_THRESHOLDS:
        raise ValueError(f"{what}: {len(t)} thresholds, more than the {N.LABEL_SCORE_MAX_THRESHOLDS} one pass "
                         "takes: pass explicit thresholds, fewer of them")
    return t


def _score_label_counts(job, counts, totals, t, ids0, ids1):
    """ScoreLabelCounts of one rank's (or the one GPU's) counts [3, T + 2] and totals [3] (or None: the counts' own
    row sums): on a sharded job both are summed over the ranks -- exact integers, so every rank ends with the one-GPU
    table; every rank holds all the records, so the true pairs are counted locally."""
    from . import distributed as D
    from .labels import ScoreLabelCounts, true_pairs_total
    if job.reduces_across_ranks() or job.force_reduce:
        D.allreduce_host_(counts, force=job.force_reduce)
        if totals is not None:
            D.allreduce_host_(totals, force=job.force_reduce)
    if totals is None:
        totals = counts.sum(axis=1)
    return ScoreLabelCounts(counts, t, totals, job.link_type, true_pairs_total(job.link_type, ids0, ids1))


def _pair_label_input(job, labels, match_threshold, what):
    """(labels as pandas, rows_l, rows_r, is_match) of a labels table (labels.pair_label_rows' columns and
    validation), before the device is touched."""
    from .labels import pair_label_rows
    if getattr(job, "passthrough", None) is not None:
        raise ValueError(f"{what}() needs the records: a job made from a gamma table has pairs without rows")
    if not isinstance(labels, pd.DataFrame):
        from .blocking import as_pandas
        labels = as_pandas(labels)
    return (labels,) + tuple(pair_label_rows(pair_label_sides(job), labels, match_threshold))


def _pair_score_label_counts(job, labels, is_match, counts, pair, score, t, score_name, candidates=None):
    """PairScoreLabelCounts of one rank's (or the one GPU's) spk_label_pairs_scores_* results.  candidates: for a
    selection frame, (counts [3, n_patterns], label_code) of spk_label_pairs_histogram over the parent's pairs -- the
    totals fn and tn are taken against, and which labels blocking produced; None: the counts' own row sums.  On a
    sharded job the counts and totals are summed over the ranks (exact integers); a labelled pair is a candidate of
    one rank only, so found / kept are all-reduced with max, and so is the score, with "none / NULL" mapped to -inf
    for the reduction and restored afterwards; label_pair, an index local to a rank, is then dropped."""
    from . import distributed as D
    from .labels import PairScoreLabelCounts
    totals = None if candidates is None else candidates[0].sum(axis=1)
    by_blocking = None if candidates is None else (np.asarray(candidates[1]) >= 0)
    if not (job.reduces_across_ranks() or job.force_reduce):
        if totals is None:
            totals = counts.sum(axis=1)
        return PairScoreLabelCounts(counts, t, totals, job.link_type, labels, is_match, score, score_name,
                                    label_pair=pair, found_by_blocking=by_blocking)
    D.allreduce_host_(counts, force=job.force_reduce)
    if totals is None:
        totals = counts.sum(axis=1)
    else:
        D.allreduce_host_(totals, force=job.force_reduce)
    found = (np.asarray(pair) >= 0).astype(np.int32)
    D.allreduce_host_(found, force=job.force_reduce, op="max")
    if by_blocking is not None:
        by_blocking = by_blocking.astype(np.int32)
        D.allreduce_host_(by_blocking, force=job.force_reduce, op="max")
    score = np.where(np.isnan(score), -np.inf, score)
    D.allreduce_host_(score, force=job.force_reduce, op="max")
    score = np.where(np.isneginf(score), np.nan, score)
    return PairScoreLabelCounts(counts, t, totals, job.link_type, labels, is_match, score, score_name,
                                found=found, found_by_blocking=by_blocking)


class ComparisonFrame(SplinkDataFrame):
    """Candidate pairs (block_using_rules)."""

    def __init__(self, job, settings):
        self.job = job
        self.settings = settings

    def _column_order(self):
        return comparison_column_order(self.settings, self.job.link_type)

    def toPandas(self):
        host = _HostColumns(self.job)
        return pd.DataFrame({c: host.get(c) for c in self._column_order()})


class GammaFrame(SplinkDataFrame):
    """Comparison vectors (add_gammas): packed codes on the device."""

    def __init__(self, job, settings, program=None, gammas=None):
        self.job = job
        self.settings = settings
        self.program = program
        self._host_gammas = gammas
        self.token = object()
        if gammas is None:
            job.gammas(settings, token=self.token)
        else:
            names, levels = program
            job.load_gammas(names, levels, gammas, token=self.token)
        # this frame's own (gamma names, levels): job.code_meta describes whichever frame's codes are installed
        self.meta = (list(job.code_meta[0]), list(job.code_meta[1]))

    def ensure_codes(self):
        """Re-install this frame's codes if another frame of the same job replaced them."""
        if self.job.codes_token is not self.token:
            if self._host_gammas is None:
                self.job.gammas(self.settings, token=self.token)
            else:
                names, levels = self.program
                self.job.load_gammas(names, levels, self._host_gammas, token=self.token)

    @property
    def gamma_names(self):
        return self.job.code_meta[0]

    @property
    def n_levels(self):
        return self.job.code_meta[1]

    def gamma_matrix(self) -> np.ndarray:
        self.ensure_codes()
        return self.job.gammas_host()

    def _column_order(self):
        if getattr(self.job, "passthrough", None) is not None:
            return list(self.job.passthrough.columns)
        return gamma_column_order(self.settings)

    def _frame(self, order):
        host = _HostColumns(self.job)
        gam = self.gamma_matrix()
        gidx = {n: i for i, n in enumerate(self.gamma_names)}
        data = OrderedDict()
        for c in order:
            if c in gidx:
                data[c] = gam[:, gidx[c]].astype(np.int32)
            else:
                data[c] = host.get(c)
        return pd.DataFrame(data)

    def toPandas(self):
        return self._frame(self._column_order())

    def filter(self, condition):
        """The pairs for which `condition` (a conjunction over gamma_* columns) is TRUE, selected on the device."""
        from .select import compile_condition
        return FilteredFrame(self, compile_condition(condition, self.meta[0], allow_mp=False))

    where = filter

    def label_counts(self, label_column):
        """The pairs per (truth state, comparison pattern) against the input column `label_column` (equal labels =
        a true match, a NULL label on either side = unlabelled), counted on the device: a `LabelCounts` without
        scores (its patterns() and m_step() work, truth_table() needs the scored frame's)."""
        return _label_counts(self, label_column)

    def label_counts_from_pairs(self, labels, match_threshold=0.5):
        """label_counts against a table of labelled pairs instead of a column of the records (a clerical-review
        sample: `<unique id>_l`, `<unique id>_r`, `clerical_match_score`, labels.pair_label_rows): a
        `PairLabelCounts` without scores.  A pair is a match iff its score >= match_threshold; candidate pairs
        without a label are unlabelled."""
        return _pair_label_counts(self, labels, match_threshold)


class ExpectationFrame(SplinkDataFrame):
    """E-step output (run_expectation_step): lazily scored with the parameters it was created with."""

    def __init__(self, gamma_frame: GammaFrame, settings, lam, level_probs):
        self.gammas = gamma_frame
        self.job = gamma_frame.job
        self.settings = settings
        self.lam = lam
        self.level_probs = [(list(m), list(u)) for m, u in level_probs]
        self._mp = None

    def match_probability(self) -> np.ndarray:
        if self._mp is None:
            self.gammas.ensure_codes()
            self._mp = self.job.score(self.lam, self.level_probs)
        return self._mp

    def _column_order(self):
        return ["match_probability"] + df_e_column_order(self.settings)

    def _prob_columns(self, gam):
        out = {}
        from .engine import quantise
        for k, name in enumerate(self.gammas.gamma_names):
            g = name[len("gamma_"):]
            m, u = self.level_probs[k]
            mt = np.array([1.0] + [quantise(p) for p in m])
            ut = np.array([1.0] + [quantise(p) for p in u])
            idx = gam[:, k].astype(np.int64) + 1
            out[f"prob_gamma_{g}_match"] = mt[idx]
            out[f"prob_gamma_{g}_non_match"] = ut[idx]
        return out

    def toPandas(self):
        order = self._column_order()
        mp = self.match_probability()
        self.gammas.ensure_codes()
        gam = self.job.gammas_host()
        gidx = {n: i for i, n in enumerate(self.gammas.gamma_names)}
        probs = self._prob_columns(gam)
        host = _HostColumns(self.job)
        data = OrderedDict()
        for c in order:
            if c == "match_probability":
                data[c] = mp
            elif c in gidx:
                data[c] = gam[:, gidx[c]].astype(np.int32)
            elif c in probs:
                data[c] = probs[c]
            else:
                data[c] = host.get(c)
        return pd.DataFrame(data)

    def filter(self, condition):
        """df_e.filter("match_probability > 0.9 and gamma_surname >= 1"): the pairs for which the condition is
        TRUE, selected on the device (spk_select); only the survivors come back."""
        from .select import compile_condition
        return FilteredFrame(self, compile_condition(condition, self.gammas.meta[0], allow_mp=True))

    where = filter

    def clusters(self, threshold):
        """Shorthand for filter(f"match_probability > {threshold!r}").clusters()."""
        return self.filter(f"match_probability > {threshold!r}").clusters()

    def clusters_at_thresholds(self, thresholds):
        """Shorthand for filter(f"match_probability > {min(thresholds)!r}").clusters_at_thresholds(thresholds)."""
        given, _, _ = sweep_thresholds(thresholds)
        return self.filter(f"match_probability > {min(given)!r}").clusters_at_thresholds(given)

    def best_matches(self, threshold=None, per="l", ties="first"):
        """Shorthand for filter(f"match_probability > {threshold!r}").best_matches(per, ties); threshold=None: the
        best match among every pair."""
        from .select import Predicate
        f = FilteredFrame(self, Predicate()) if threshold is None else self.filter(f"match_probability > {threshold!r}")
        return f.best_matches(per=per, ties=ties)

    def sample_pairs(self, per_stratum=200, strata=10, seed=0):
        """A stratified random sample of this frame's pairs for clerical review, drawn on the device: shorthand for
        the same call on the unfiltered FilteredFrame."""
        from .select import Predicate
        return FilteredFrame(self, Predicate()).sample_pairs(per_stratum=per_stratum, strata=strata, seed=seed)

    def orderBy(self, col, ascending=True):  # noqa: N802 (Spark name)
        """df_e.orderBy("match_probability", ascending=False).limit(k): the first k pairs in score order, selected on
        the device.  Shorthand for the same call on the unfiltered FilteredFrame."""
        from .select import Predicate
        return FilteredFrame(self, Predicate()).orderBy(col, ascending)

    sort = orderBy

    def limit(self, k):
        """The first k pairs of this frame, in its order: shorthand for the same call on the unfiltered FilteredFrame."""
        from .select import Predicate
        return FilteredFrame(self, Predicate()).limit(k)

    def label_counts(self, label_column):
        """GammaFrame.label_counts with the match_probability of every pattern under this frame's parameters."""
        return _label_counts(self.gammas, label_column, self.lam, self.level_probs)

    def truth_table(self, label_column, thresholds=None):
        """The confusion matrix of `match_probability > threshold` against the labels in the input column
        `label_column`, at the given thresholds or (None) at every distinct score: the exact ROC and
        precision / recall curve.  Shorthand for label_counts(label_column).truth_table(thresholds)."""
        return self.label_counts(label_column).truth_table(thresholds)

    def label_counts_from_pairs(self, labels, match_threshold=0.5):
        """GammaFrame.label_counts_from_pairs with the match_probability of every pattern under this frame's
        parameters: its labelled_pairs() and prediction_errors(threshold) carry the scores."""
        return _pair_label_counts(self.gammas, labels, match_threshold, self.lam, self.level_probs)

    def truth_table_from_pairs(self, labels, thresholds=None, match_threshold=0.5):
        """truth_table against a table of labelled pairs: tp, fp, tn, fn over the labelled candidate pairs,
        recall_of_all_true_pairs over all labelled matches.  Shorthand for
        label_counts_from_pairs(labels, match_threshold).truth_table(thresholds)."""
        return self.label_counts_from_pairs(labels, match_threshold).truth_table(thresholds)


class FilteredFrame(SplinkDataFrame):
    """`parent.filter(condition)`: lazily selected on the device.  count() runs the selection and returns the
    scalar; toPandas() copies the survivors only and equals parent.toPandas()[mask].reset_index(drop=True)."""

    def __init__(self, parent, predicate):
        self.parent = parent
        self.predicate = predicate
        self.job = parent.job
        self.settings = parent.settings
        self.gammas = parent.gammas if isinstance(parent, ExpectationFrame) else parent
        self._n = None
        self._seq = None   # job.codes_seq at the last spk_select of this frame
        self._pdf = None

    def _column_order(self):
        return self.parent._column_order()

    def filter(self, condition):
        from .select import compile_condition
        more = compile_condition(condition, self.gammas.meta[0], allow_mp=isinstance(self.parent, ExpectationFrame))
        return FilteredFrame(self.parent, self.predicate.and_(more))

    where = filter

    def _select(self):
        """Make the context's selection this frame's: re-install the frame's codes if another frame replaced
        them, and select again unless the last spk_select of the job was this frame's on these codes."""
        job = self.job
        self.gammas.ensure_codes()
        if self._n is not None and job.selection_owner is self and self._seq == job.codes_seq:
            return self._n
        if isinstance(self.parent, ExpectationFrame):
            m, u = job.flat_tables(self.parent.level_probs)
            lam = float(self.parent.lam)
            n = job.ctx.select(lam, float(1 - self.parent.lam), m, u, self.predicate.native_terms())
        else:
            n = job.ctx.select(0.0, 0.0, None, None, self.predicate.native_terms())
        job.selection_owner = self
        self._seq = job.codes_seq
        self._n = int(n)
        return self._n

    def count(self) -> int:
        if self._n is None:
            self._select()
        return self._n

    def toPandas(self):
        if self._pdf is None:
            self._pdf = self._materialise()
        return self._pdf.copy()

    def _scored_parent(self):
        """The ExpectationFrame whose parameters the survivors' match_probability and prob_gamma_* come from, or None
        (an unscored parent)."""
        return self.parent if isinstance(self.parent, ExpectationFrame) else None

    def _extra_columns(self, n):
        """Columns of this frame beyond the scored frame's, for the n survivors of the context's selection."""
        return {}

    def _materialise(self):
        job, parent = self.job, self._scored_parent()
        scored = parent is not None
        names = self.gammas.meta[0]  # the frame's own columns: the selection is made on its codes (_select)
        n = self._select()
        if list(job.code_meta[0]) != list(names):  # select_copy writes K levels per survivor into a buffer sized here
            raise RuntimeError("filter: the installed comparison codes are not this frame's")
        has_rows = getattr(job, "passthrough", None) is None
        if n:
            ordinal, rows_l, rows_r, gam, mp = job.ctx.select_copy(0, n, len(names), rows=has_rows, mp=scored)
        else:
            ordinal = np.empty(0, dtype=np.int64)
            rows_l = rows_r = np.empty(0, dtype=np.int32)
            gam = np.empty((0, len(names)), dtype=np.int8)
            mp = np.empty(0, dtype=np.float64)
        gidx = {g: i for i, g in enumerate(names)}
        probs = parent._prob_columns(gam) if scored else {}
        extra = self._extra_columns(n)
        data = OrderedDict()
        for c in self._column_order():
            if c in extra:
                data[c] = extra[c]
            elif c == "match_probability" and scored:
                data[c] = mp
            elif c in gidx:
                data[c] = gam[:, gidx[c]].astype(np.int32)
            elif c in probs:
                data[c] = probs[c]
            elif not has_rows:  # a gamma table handed in: its other columns pass through, by ordinal
                if c not in job.passthrough.columns:
                    raise KeyError(c)
                data[c] = job.passthrough[c].to_numpy()[ordinal]
            else:
                base, side = c[:-2], c[-2:]
                s = 0 if side == "_l" else job.r_side()
                if base not in job.inputs[s].columns:
                    raise KeyError(c)
                data[c] = job.host_values(s, base)[rows_l if side == "_l" else rows_r]
        return pd.DataFrame(data)

    def clusters(self):
        """The connected components of the graph whose edges are this frame's pairs (GraphFrames'
        connectedComponents on the reference's filtered frame), computed on the device: a `ClusterFrame`."""
        return ClusterFrame(self)

    def clusters_at_thresholds(self, thresholds, by=None):
        """The clusters of this frame's pairs with score > t for each of 1 to 32 thresholds t (any order), from one
        selection and one nested pass on the device: a `ClusterSweepFrame` with a cluster_id_{t!r} column per
        threshold, a summary() per threshold and metrics(t).  by: the score, the frame's first by default."""
        return ClusterSweepFrame(self, thresholds, by)

    # the scores best_matches() can rank by, the default first
    _best_by = ("match_probability",)

    def best_matches(self, per="l", ties="first", by=None):
        """For each record its best pair among this frame's pairs (the reference's users' window query,
        row_number() over (partition by unique_id_l order by match_probability desc) = 1), narrowed on the device
        (spk_select_best): a `BestMatchFrame`.  per: "l" / "r" the best pair of every left / right record, "either"
        the pairs that are the best of one of their two records, "mutual" of both (a one-to-one link).  Equal scores:
        ties="first" keeps the pair that comes first in the frame, ties="all" every pair at the maximum."""
        return BestMatchFrame(self, per, ties, self._best_by[0] if by is None else by)

    def sample_pairs(self, per_stratum=200, strata=10, seed=0):
        """A stratified random sample of this frame's pairs for clerical review, drawn on the device
        (spk_select_sample): a `SampleFrame`.  strata: that many equal-width bands of match_probability over [0, 1],
        or the bands' edges (left-closed, the last one closed on both sides; a pair with a NULL score or one outside
        the edges is never drawn).  per_stratum: the pairs to draw from every band, or one number per band; a band
        with fewer pairs is taken whole.  The draw is without replacement and a function of `seed` and the pairs'
        positions in the frame alone: the same seed with a larger per_stratum gives a superset."""
        return SampleFrame(self, per_stratum, strata, seed)

    def orderBy(self, col, ascending=True):  # noqa: N802 (Spark name)
        """This frame's pairs ordered by one of its score columns (a name, or asc(name) / desc(name)), as Spark orders
        them: NULLs first ascending and last descending; equal scores in the frame's own order.  A lazy `TopFrame`:
        .limit(k) keeps the first k, and only those leave the device (spk_select_top / spk_select_top_of)."""
        return TopFrame(self, col, ascending, None)

    sort = orderBy

    def limit(self, k):
        """The first k pairs of this frame, in its order: a lazy `TopFrame`."""
        return TopFrame(self, None, True, k)

    def _score_names(self):
        """The scores this frame's pairs carry, the default first."""
        return self._best_by

    def truth_table(self, label_column, thresholds=None, by=None):
        """This frame's pairs against the labels in the input column `label_column`, counted on the device
        (spk_label_scores_selection), with LabelCounts.truth_table's columns.  thresholds=None: one row with
        threshold = -inf that describes the frame as it stands -- every kept pair is a predicted match.  Given
        thresholds: one row per threshold, ascending, the kept pairs with score > threshold predicted (a NULL score
        never); by: the score, the frame's first by default.  fn and tn are taken against the labelled pairs among
        all candidate pairs of the job, so what the filter or the best-match step dropped counts as missed."""
        job = self.job
        if getattr(job, "passthrough", None) is not None:
            raise ValueError("truth_table() needs the records: a job made from a gamma table has pairs without rows")
        by, field = self._score_field(by, "truth_table")
        ids0, ids1 = _label_ids(job, label_column)  # a missing column fails before the device is touched
        t = _score_thresholds([] if thresholds is None else thresholds, "truth_table")
        self._select()
        counts = job.ctx.label_scores_selection(ids0, ids1, field, t)
        totals = job.ctx.label_histogram(ids0, ids1)[0].sum(axis=1)  # the parent's pairs: one pass, no scores
        slc = _score_label_counts(job, counts, totals, t, ids0, ids1)
        return slc.kept_row() if thresholds is None else slc.truth_table()

    def _score_field(self, by, what):
        """(the score's column name, its SEL_* field) for `by`, the frame's first score by default."""
        from . import _native as N
        names = self._score_names()
        by = names[0] if by is None else by
        if self._scored_parent() is None or by not in names:
            raise ValueError(f"{what}: this frame has no score {by!r}" +
                             (" (it was filtered from an unscored frame)" if self._scored_parent() is None
                              else f": by is one of {list(names)}"))
        return by, (N.SEL_TF_MP if by == "tf_adjusted_match_prob" else N.SEL_MP)

    def label_counts_from_pairs(self, labels, match_threshold=0.5, thresholds=None, by=None):
        """This frame's pairs against a table of labelled pairs (a clerical-review sample: labels.pair_label_rows'
        columns), counted on the device (spk_label_pairs_scores_selection): a `PairScoreLabelCounts`, whose
        labelled_pairs() says of every label whether blocking found the pair, whether this frame kept it and with
        which score, and whose prediction_errors(threshold) lists the labels the frame gets wrong.  thresholds: as
        for truth_table (None: none, kept_row() describes the frame as it stands); by: the score, the frame's first
        by default.  fn and tn are taken against the labelled pairs among all candidate pairs of the job."""
        job = self.job
        labels, rows_l, rows_r, is_match = _pair_label_input(job, labels, match_threshold, "label_counts_from_pairs")
        by, field = self._score_field(by, "label_counts_from_pairs")
        t = _score_thresholds([] if thresholds is None else thresholds, "label_counts_from_pairs")
        self._select()
        counts, pair, score = job.ctx.label_pair_scores_selection(rows_l, rows_r, is_match, field, t)
        hist, _, code = job.ctx.label_pairs_histogram(rows_l, rows_r, is_match)  # the parent's pairs: no scores
        return _pair_score_label_counts(job, labels, is_match, counts, pair, score, t, by, candidates=(hist, code))

    def truth_table_from_pairs(self, labels, thresholds=None, match_threshold=0.5, by=None):
        """truth_table against a table of labelled pairs: thresholds=None gives the one row that describes the frame
        as it stands, given thresholds one row each; tp, fp, tn, fn over the labelled candidate pairs,
        recall_of_all_true_pairs over all labelled matches."""
        slc = self.label_counts_from_pairs(labels, match_threshold, thresholds, by)
        return slc.kept_row() if thresholds is None else slc.truth_table()


class BestMatchFrame(FilteredFrame):
    """`filtered.best_matches(per, ties)`: lazily narrowed on the device.  The frame has the filtered frame's columns
    and a subset of its rows, in its order; clusters() gives the components of the kept pairs (per="mutual": a
    matching)."""

    def __init__(self, inner: FilteredFrame, per, ties, by):
        from .select import best_match_args
        if inner._scored_parent() is None:
            raise ValueError("best_matches: this frame has no score to rank the pairs by (it was filtered from an "
                             "unscored frame): filter the frame run_expectation_step returns")
        self._args = best_match_args(per, ties, by, allowed_by=inner._best_by)
        job = inner.job
        if getattr(job, "passthrough", None) is not None:
            raise ValueError("best_matches() needs the records: a job made from a gamma table has pairs without rows")
        if job.n_shards > 1:
            raise ValueError("best_matches() on a sharded job: a record's pairs span the shards (take the best of the "
                             "shards' best matches on the host)")
        super().__init__(inner.parent, inner.predicate)
        self.inner = inner
        self.gammas = inner.gammas
        self.per, self.ties, self.by = per, ties, by

    def _column_order(self):
        return self.inner._column_order()

    def _scored_parent(self):
        return self.inner._scored_parent()

    def _extra_columns(self, n):
        return self.inner._extra_columns(n)

    def _score_names(self):
        return self.inner._score_names()

    def _refuse(self, *args, **kwargs):
        raise ValueError("a best-match frame takes no further filter() or best_matches(): filter first, then take the "
                         "best matches (a filter after the narrowing asks a different question)")

    filter = where = best_matches = _refuse

    def sample_pairs(self, *args, **kwargs):
        raise ValueError("sample_pairs() on a best-match frame: the strata are those of the pairs' own "
                         "match_probability, decided per comparison pattern before any narrowing (sample the filtered "
                         "frame instead)")

    def _select(self):
        """Make the context's selection this frame's: the inner frame's selection (its own re-select rules: it
        selects again unless the context still holds its survivors), narrowed to the best pair per record."""
        job = self.job
        self.gammas.ensure_codes()
        if self._n is not None and job.selection_owner is self and self._seq == job.codes_seq:
            return self._n
        self.inner._select()
        job.selection_owner = None  # the narrowing replaces the inner frame's survivors, or leaves none if it fails
        field, mode, keep_ties = self._args
        n = job.ctx.select_best(field, mode, keep_ties)
        job.selection_owner = self
        self._seq = job.codes_seq
        self._n = int(n)
        return self._n


class SampleFrame(FilteredFrame):
    """`filtered.sample_pairs(per_stratum, strata, seed)`: lazily drawn on the device.  The frame has the filtered
    frame's columns and a subset of its rows, in its order, plus `stratum` (int32) and `sampling_weight` (float64: the
    stratum's pairs / its sampled pairs, so a labelled sample weights back to the whole frame); strata() gives the
    bands with their populations."""

    def __init__(self, inner: FilteredFrame, per_stratum, strata, seed):
        from .select import sample_args
        self._edges, self._quota, self._seed = sample_args(per_stratum, strata, seed)
        if inner._scored_parent() is None:
            raise ValueError("sample_pairs: this frame has no match_probability to stratify the pairs by (it was "
                             "filtered from an unscored frame): sample the frame run_expectation_step returns")
        if inner.job.n_shards > 1:
            raise ValueError("sample_pairs() on a sharded job: a stratum's pairs span the shards (sample every shard "
                             "and merge the samples on the host)")
        super().__init__(inner.parent, inner.predicate)
        self.inner = inner
        self.gammas = inner.gammas
        self._pop = self._kept = None

    def _column_order(self):
        return self.inner._column_order() + ["stratum", "sampling_weight"]

    def _refuse(self, *args, **kwargs):
        raise ValueError("a sample frame takes no further filter(), best_matches(), clusters() or sample_pairs(): "
                         "filter first, then sample (its rows are a random subset, and anything derived from them "
                         "would describe the draw, not the linkage)")

    filter = where = best_matches = clusters = clusters_at_thresholds = sample_pairs = _refuse

    def _refuse_order(self, *args, **kwargs):
        raise ValueError("a sample frame takes no orderBy() or limit(): its rows are a random subset, and the first k "
                         "of them would describe the draw, not the linkage (order the filtered frame instead)")

    orderBy = sort = limit = _refuse_order

    def _refuse_pair_labels(self, *args, **kwargs):
        raise ValueError("a sample frame takes no label_counts_from_pairs() or truth_table_from_pairs(): its rows are "
                         "a random subset, and a table against them would describe the draw, not the linkage (score "
                         "the filtered frame instead)")

    label_counts_from_pairs = truth_table_from_pairs = _refuse_pair_labels

    def _select(self):
        """Make the context's selection this frame's, under the ownership rules of FilteredFrame._select."""
        job, parent = self.job, self.parent
        self.gammas.ensure_codes()
        if self._n is not None and job.selection_owner is self and self._seq == job.codes_seq:
            return self._n
        m, u = job.flat_tables(parent.level_probs)
        job.selection_owner = None  # the call drops the context's selection first, and leaves none if it fails
        n = job.ctx.select_sample(float(parent.lam), float(1 - parent.lam), m, u, self.predicate.native_terms(),
                                  self._edges, self._quota, self._seed)
        _, self._pop, self._kept, _ = job.ctx.select_sample_info()
        job.selection_owner = self
        self._seq = job.codes_seq
        self._n = int(n)
        return self._n

    def strata(self):
        """One row per stratum: stratum, low, high (its edges), pairs (the frame's pairs in it), sampled."""
        self.count()
        n = len(self._quota)
        return pd.DataFrame({"stratum": np.arange(n, dtype=np.int32), "low": np.array(self._edges[:-1]),
                             "high": np.array(self._edges[1:]), "pairs": self._pop.astype(np.int64),
                             "sampled": self._kept.astype(np.int64)})

    def _extra_columns(self, n):
        """stratum from the survivors' own match_probability and the call's edges (the doubles the device compared),
        sampling_weight from the strata's counts."""
        from .select import sample_strata
        if n:
            mp = self.job.ctx.select_copy(0, n, len(self.gammas.meta[0]), rows=False, gammas=False, mp=True)[4]
        else:
            mp = np.empty(0, dtype=np.float64)
        b = sample_strata(mp, self._edges)
        weight = self._pop[b].astype(np.float64) / self._kept[b].astype(np.float64)
        return {"stratum": b.astype(np.int32), "sampling_weight": weight}


class TopFrame(FilteredFrame):
    """`frame.orderBy(col, ascending).limit(k)` / `frame.limit(k)`: lazily selected on the device.  The frame has the
    inner frame's columns; its rows are the first k of the inner frame's under the order (NULL scores lowest, equal
    scores in the inner frame's order; without a column: the inner frame's order), in that order.  Without limit()
    every pair of the inner frame is kept, sorted.  count() is the kept count, cut() describes the cut, and
    truth_table(label) scores the first k against labels."""

    def __init__(self, inner: FilteredFrame, column, ascending, k):
        from .select import top_args
        scored = inner._scored_parent() is not None
        self._field, self._order, self._k = top_args(column, ascending, k, inner._score_names() if scored else ())
        if inner.job.n_shards > 1:
            raise ValueError("orderBy() / limit() on a sharded job: the first k pairs span the shards (take the first "
                             "k of every shard and merge them on the host)")
        super().__init__(inner.parent, inner.predicate)
        self.inner = inner
        self.gammas = inner.gammas
        self._column, self._ascending = column, ascending
        self._cut = None

    def _column_order(self):
        return self.inner._column_order()

    def _scored_parent(self):
        return self.inner._scored_parent()

    def _extra_columns(self, n):
        return self.inner._extra_columns(n)

    def _score_names(self):
        return self.inner._score_names()

    def limit(self, k):
        """The first k rows of this order (a second limit() replaces the first)."""
        return TopFrame(self.inner, self._column, self._ascending, k)

    def _refuse(self, *args, **kwargs):
        raise ValueError("an ordered frame takes no further filter(), best_matches(), clusters(), sample_pairs() or "
                         "orderBy(): filter and narrow first, then order and limit (anything derived from the first k "
                         "rows would describe the cut, not the linkage)")

    filter = where = best_matches = clusters = clusters_at_thresholds = sample_pairs = orderBy = sort = _refuse

    def _select(self):
        """Make the context's selection this frame's.  A plain filtered frame goes down as one call with its terms
        (spk_select_top: no full selection is made); any other inner frame makes its own selection, which is then
        narrowed (spk_select_top_of)."""
        from . import _native as N
        job, inner = self.job, self.inner
        self.gammas.ensure_codes()
        if self._n is not None and job.selection_owner is self and self._seq == job.codes_seq:
            return self._n
        if type(inner) is FilteredFrame:
            job.selection_owner = None  # the call drops the context's selection first, and leaves none if it fails
            terms = self.predicate.native_terms()
            if isinstance(self.parent, ExpectationFrame):
                m, u = job.flat_tables(self.parent.level_probs)
                lam = float(self.parent.lam)
                n = job.ctx.select_top(lam, float(1 - self.parent.lam), m, u, terms, self._order, self._k)
            else:
                n = job.ctx.select_top(0.0, 0.0, None, None, terms, self._order, self._k)
        else:
            inner._select()
            job.selection_owner = None  # the narrowing replaces the inner frame's survivors, or leaves none if it fails
            n = job.ctx.select_top_of(N.SEL_MP if self._field is None else self._field, self._order, self._k)
        eligible, kept, score, tied, tied_kept, _ = job.ctx.select_top_info()
        self._cut = {"eligible": int(eligible), "kept": int(kept),
                     "score": None if tied == 0 or score != score else float(score),
                     "tied": int(tied), "tied_kept": int(tied_kept)}
        job.selection_owner = self
        self._seq = job.codes_seq
        self._n = int(n)
        return self._n

    def cut(self):
        """{"eligible": the inner frame's pairs, "kept": this frame's, "score": the k-th pair's score (None: no cut,
        that is k = 0 or k >= eligible or no order, or a NULL score), "tied": the inner frame's pairs with that score,
        "tied_kept": how many of them are kept (the first ones in the inner frame's order)}."""
        if self._cut is None:
            self._select()
        return dict(self._cut)

    def _materialise(self):
        from . import _native as N
        from .select import TOP_FIRST, top_order
        pdf = super()._materialise()  # the kept pairs in ascending ordinal
        if self._order == TOP_FIRST:
            return pdf
        by = "tf_adjusted_match_prob" if self._field == N.SEL_TF_MP else "match_probability"
        return pdf.iloc[top_order(pdf[by].to_numpy(), self._order)].reset_index(drop=True)


COPY_NODES = 1 << 26  # labels per spk_components_copy


def _merges_across_ranks(job):
    """The job's pairs are one rank's shard of a pair set split over the process group (or a test forces that path at
    one rank): its clusters are the merge of every rank's."""
    return job.reduces_across_ranks() or job.force_reduce


def _refuse_unreachable_shards(job, what):
    """A job with an explicit shard and no process group over the shards cannot reach the other shards' pairs."""
    if job.n_shards > 1 and not job.reduces_across_ranks():
        raise ValueError(f"{what} on one of a job's shards without a process group over all of them: a record's "
                         "cluster spans the shards' pairs, and the other shards are out of reach (run one rank per "
                         "shard, or merge the shards' labels yourself with Context.components_merge, DESIGN.md)")


def _merge_ranks_labels(job, n_nodes, copy_device, copy_host, merge):
    """Gather every rank's labels of one result (a collective) and merge them into this rank's: copy_device(tensor) /
    copy_host() read this rank's labels, merge(peers) is components_merge or one level's components_sweep_merge.
    Under nccl the labels never leave the devices; under gloo they are staged through the host.  Returns merge's
    (n_clusters, rounds).  Ranks are gathered COMPONENTS_MAX_PEERS at a time."""
    import torch
    from . import distributed as D
    from ._native import COMPONENTS_MAX_PEERS
    if D.stream_ordered_reduce(job.device):
        mine = torch.empty(n_nodes, dtype=torch.int32, device=f"cuda:{job.device}")
        copy_device(mine)
    else:
        mine = torch.from_numpy(copy_host().view(np.int32))
    peers = D.allgather_labels(mine, force=job.force_reduce)
    out = None
    for g in range(0, peers.shape[0], COMPONENTS_MAX_PEERS):
        part = peers[g:g + COMPONENTS_MAX_PEERS]
        n_clusters, rounds = merge(part if part.is_cuda else part.numpy())
        out = (n_clusters, rounds + (out[1] if out else 0))
    return out


def _merge_sweep_level(job, n_nodes, level):
    """_merge_ranks_labels for one level of the sweep the context holds."""
    ctx = job.ctx
    return _merge_ranks_labels(
        job, n_nodes, lambda out: ctx.components_sweep_copy_device(level, out),
        lambda: _copy_in_ranges(lambda s, c: ctx.components_sweep_copy(level, s, c), n_nodes, np.uint32),
        lambda peers: ctx.components_sweep_merge(level, peers))


def _refuse_sharded_metrics(job, what):
    if _merges_across_ranks(job):
        raise ValueError(f"{what} on a sharded job: node degrees and cluster edge counts need every shard's pairs, and "
                         "a rank holds the edges of its own shard only (the merged labels, n_clusters and "
                         "truth_table() are available)")


class ClusterFrame(SplinkDataFrame):
    """`filtered.clusters()`: one row per input record, in input order (two input tables: left rows, then right).

    cluster_id (int64) is the smallest input position among the records of the cluster, so
    `inputs.iloc[cluster_id]` is its representative; then the unique id, and for the two-table link types
    _source_table ('left' / 'right').  A record no kept pair touches is a cluster of its own.

    On a job sharded over a process group every rank labels its shard's pairs, the ranks all-gather their labels and
    each merges them on its device (spk_components_merge): every rank ends with the one-GPU cluster_ids, bit for bit.
    Materialising the frame (toPandas, n_clusters, rounds, truth_table) is then a collective: every rank makes the same
    calls in the same order.  metrics() needs degrees over all shards' pairs and is refused there, and so is bridges()."""

    def __init__(self, filtered: FilteredFrame):
        job = filtered.job
        if getattr(job, "passthrough", None) is not None:
            raise ValueError("clusters() needs the records: a job made from a gamma table has pairs without rows")
        _refuse_unreachable_shards(job, "clusters()")
        self.filtered = filtered
        self.job = job
        self.settings = filtered.settings
        self._labels = None
        self._info = None  # (n_nodes, n_clusters, rounds)

    def _column_order(self):
        cols = ["cluster_id", self.settings["unique_id_column_name"]]
        if self.job.link_type in ("link_only", "link_and_dedupe"):
            cols.append("_source_table")
        return cols

    def _run(self):
        """Select (the frame's re-select rules), then label: the labels are copied at once, so a later selection or
        components call of the job does not reach this frame."""
        if self._labels is None:
            job, ctx = self.job, self.job.ctx
            self.filtered._select()
            n_nodes, n_clusters, rounds = ctx.components()
            if _merges_across_ranks(job):  # a collective: this rank's rounds plus the merge's
                n_clusters, more = _merge_ranks_labels(
                    job, n_nodes, ctx.components_copy_device,
                    lambda: _copy_in_ranges(ctx.components_copy, n_nodes, np.uint32), ctx.components_merge)
                rounds += more
            self._labels = _copy_in_ranges(ctx.components_copy, n_nodes, np.uint32)
            self._info = (int(n_nodes), int(n_clusters), int(rounds))
        return self._labels

    def count(self) -> int:
        return int(sum(len(t) for t in self.job.inputs))

    @property
    def n_clusters(self) -> int:
        self._run()
        return self._info[1]

    @property
    def rounds(self) -> int:
        self._run()
        return self._info[2]

    def metrics(self):
        """Cluster and node metrics of these clusters (a `ClusterMetrics`): a one-level sweep over every pair of the
        frame's own selection, whatever its score, so clusters of pairs with NULL scores are covered too.  The sweep's
        labels are this frame's (the same definition over the same pairs): a frame that has none yet takes them, and
        one that has them does not copy them again."""
        _refuse_sharded_metrics(self.job, "metrics()")
        self._sweep_all()
        return ClusterMetrics(self, self._labels, self.job.ctx, 0)

    def bridges(self):
        """The bridges and 2-edge-connected cores of these clusters (a `ClusterBridges`): which link joined them?  Over
        the same one-level sweep of every pair of the frame's selection that metrics() takes."""
        _refuse_sharded_metrics(self.job, "bridges()")
        self._sweep_all()
        return ClusterBridges(self, self._labels, self.job.ctx, 0)

    def _sweep_all(self):
        """Make the context's sweep the one level of every pair of this frame's selection (on a job sharded over the
        process group: of every rank's, merged -- a collective)."""
        from ._native import SEL_ALL
        job = self.job
        job.sweep_owner = None
        self.filtered._select()
        n_nodes, _, n_clusters, rounds = job.ctx.components_sweep(SEL_ALL, [])
        if _merges_across_ranks(job):
            n_clusters[0], more = _merge_sweep_level(job, int(n_nodes), 0)
            rounds[0] += more
        if self._labels is None:
            self._labels = _copy_in_ranges(lambda s, c: job.ctx.components_sweep_copy(0, s, c), int(n_nodes), np.uint32)
            self._info = (int(n_nodes), int(n_clusters[0]), int(rounds[0]))

    def truth_table(self, label_column):
        """These clusters against `label_column` of the input tables, one row (labels.cluster_truth_rows) with
        threshold NaN: a pair of labelled records is predicted iff both lie in one cluster, so the closure's merges
        count in full (spk_cluster_agreement over the one-level sweep that metrics() takes)."""
        from .labels import cluster_truth_rows
        _node_label_ids(self.job, label_column)  # a missing column fails before the device is touched
        self._sweep_all()
        return cluster_truth_rows(_cluster_agreement(self.job, label_column), [np.nan])

    def toPandas(self, singletons=True):
        job = self.job
        uid = self.settings["unique_id_column_name"]
        data = OrderedDict()
        data["cluster_id"] = self._run().astype(np.int64)
        data[uid] = pd.concat([t[uid] for t in job.inputs], ignore_index=True)
        if job.link_type == "link_only":
            data["_source_table"] = np.repeat(np.array(["left", "right"], dtype=object), [len(t) for t in job.inputs])
        elif job.link_type == "link_and_dedupe":
            data["_source_table"] = job.inputs[0]["_source_table"].to_numpy()
        out = pd.DataFrame(data)
        if not singletons:
            size = np.bincount(data["cluster_id"], minlength=len(out))
            out = out[size[data["cluster_id"]] > 1].reset_index(drop=True)
        return out


def sweep_thresholds(thresholds):
    """clusters_at_thresholds' argument: 1 to 32 distinct floats, none NaN, in any order.  Returns (the thresholds as
    given, as floats; the same in descending order, as the device takes them; the level of each given one)."""
    from ._native import SWEEP_MAX_LEVELS
    try:
        given = [float(t) for t in thresholds]
    except TypeError:
        raise ValueError("clusters_at_thresholds: thresholds is a sequence of numbers") from None
    if not 1 <= len(given) <= SWEEP_MAX_LEVELS:
        raise ValueError(f"clusters_at_thresholds: 1 to {SWEEP_MAX_LEVELS} thresholds, not {len(given)}")
    if any(t != t for t in given):
        raise ValueError("clusters_at_thresholds: a threshold is NaN")
    if len(set(given)) != len(given):
        raise ValueError("clusters_at_thresholds: a threshold is repeated")
    desc = sorted(given, reverse=True)
    return given, np.array(desc, dtype=np.float64), [desc.index(t) for t in given]


def sweep_column_names(given):
    """One label column per threshold, in the order given: cluster_id_0.9 for 0.9 (the threshold's repr)."""
    return [f"cluster_id_{t!r}" for t in given]


def cluster_metric_columns(n_nodes, degree_sum, max_degree):
    """(n_edges, density, cluster_centralisation) per cluster from its node count, the sum of its degrees and its
    largest degree.  density = 2E / (n (n - 1)), NaN for n = 1; cluster_centralisation = (n max_degree - degree_sum) /
    ((n - 1)(n - 2)), NaN for n <= 2 (1 for a star, 0 for a clique or a cycle)."""
    n = np.asarray(n_nodes, dtype=np.float64)
    ds = np.asarray(degree_sum, dtype=np.float64)
    mx = np.asarray(max_degree, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        density = np.where(n > 1, ds / (n * (n - 1)), np.nan)
        central = np.where(n > 2, (n * mx - ds) / ((n - 1) * (n - 2)), np.nan)
    return np.asarray(degree_sum, dtype=np.int64) // 2, density, central


def _copy_in_ranges(copy, n_nodes, dtype):
    parts = [copy(s, min(COPY_NODES, n_nodes - s)) for s in range(0, n_nodes, COPY_NODES)]
    return np.concatenate(parts) if parts else np.empty(0, dtype=dtype)


class ClusterMetrics:
    """Cluster and node metrics of one set of clusters, counted on the device (spk_cluster_metrics) and held on the
    host: clusters() has one row per cluster, nodes() one per input record, in input order."""

    def __init__(self, frame, labels, ctx, level):
        self._frame = frame  # a ClusterFrame-shaped frame: the records' ids
        self._labels = labels
        n = len(labels)
        self.n_clusters_multi, self.records_clustered, self.largest_cluster = ctx.cluster_metrics(level)
        cols = [[], [], [], []]
        for s in range(0, n, COPY_NODES):
            for c, part in zip(cols, ctx.cluster_metrics_copy(s, min(COPY_NODES, n - s))):
                c.append(part)
        kinds = (np.uint32, np.uint32, np.uint64, np.uint32)
        self.degree, self.size, self.degree_sum, self.max_degree = [
            np.concatenate(c) if c else np.empty(0, dtype=k) for c, k in zip(cols, kinds)]

    def clusters(self, singletons=True):
        """cluster_id, n_nodes, n_edges, density, cluster_centralisation: one row per cluster, by cluster_id."""
        roots = np.flatnonzero(self._labels == np.arange(len(self._labels), dtype=np.int64))
        if not singletons:
            roots = roots[self.size[roots] > 1]
        n = self.size[roots].astype(np.int64)
        edges, density, central = cluster_metric_columns(n, self.degree_sum[roots], self.max_degree[roots])
        return pd.DataFrame(OrderedDict([("cluster_id", roots.astype(np.int64)), ("n_nodes", n), ("n_edges", edges),
                                         ("density", density), ("cluster_centralisation", central)]))

    def nodes(self):
        """The cluster frame's columns, then node_degree and node_centrality = degree / (nodes of its cluster - 1),
        NaN for a record that is a cluster of its own."""
        out = ClusterFrame.toPandas(self._frame)
        n = self.size[self._labels].astype(np.float64)
        out["node_degree"] = self.degree.astype(np.int64)
        with np.errstate(divide="ignore", invalid="ignore"):
            out["node_centrality"] = np.where(n > 1, self.degree / (n - 1), np.nan)
        return out


def bridge_edge_columns(settings, link_type):
    """The columns of ClusterBridges.edges(): cluster_id, the pair's unique ids as df_e names them, _source_table_l / _r
    where df_e has them (link_and_dedupe), the records on each side of the bridge, and the cluster's size."""
    uid = settings["unique_id_column_name"]
    cols = ["cluster_id", uid + "_l", uid + "_r"]
    if link_type == "link_and_dedupe":
        cols += ["_source_table_l", "_source_table_r"]
    return cols + ["nodes_l", "nodes_r", "n_nodes"]


def bridge_rows(side_u, side_v, min_side=1):
    """The positions of the bridges with min(nodes_l, nodes_r) >= min_side, in device order: min_side=2 drops the
    bridges by which a single record hangs."""
    try:
        ok = int(min_side) == min_side and min_side >= 1
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f"edges: min_side is a whole number >= 1, not {min_side!r}")
    return np.flatnonzero(np.minimum(side_u, side_v) >= int(min_side))


class ClusterBridges:
    """The bridges and cores of one set of clusters, found on the device (spk_cluster_bridges) and held on the host.  A
    bridge is a kept pair whose removal splits its cluster; a core is what stays connected when every bridge is cut.
    n_bridges, n_cores, largest_core (its records) and depth (of the deepest breadth-first tree, from each cluster's
    first record) are the call's scalars."""

    def __init__(self, frame, labels, ctx, level):
        self._frame = frame  # a ClusterFrame-shaped frame: the records' ids
        self._labels = labels
        n = len(labels)
        self.n_bridges, self.n_cores, self.largest_core, self.depth = ctx.cluster_bridges(level)
        self.rounds = ctx.cluster_bridges_info()[1]
        cols = [[], [], [], []]
        for s in range(0, self.n_bridges, COPY_NODES):
            for c, part in zip(cols, ctx.cluster_bridges_copy(s, min(COPY_NODES, self.n_bridges - s))):
                c.append(part)
        self.u, self.v, self.side_u, self.side_v = [
            np.concatenate(c) if c else np.empty(0, dtype=np.uint32) for c in cols]
        self.core = _copy_in_ranges(ctx.cluster_bridges_cores_copy, n, np.uint32)

    def edges(self, min_side=1):
        """One row per bridge, ascending by the pair's input positions (bridge_edge_columns): nodes_l / nodes_r are the
        records left on the left / right record's side when the pair is cut, n_nodes their sum, the cluster's size.
        Every record that hangs by one pair gives a (1, n - 1) row; min_side=2 keeps the bridges between groups."""
        job, frame = self._frame.job, self._frame
        keep = bridge_rows(self.side_u, self.side_v, min_side)
        u, v = self.u[keep].astype(np.int64), self.v[keep].astype(np.int64)
        records = ClusterFrame.toPandas(frame)
        uid = frame.settings["unique_id_column_name"]
        data = OrderedDict()
        data["cluster_id"] = self._labels[u].astype(np.int64)
        data[uid + "_l"] = records[uid].to_numpy()[u]
        data[uid + "_r"] = records[uid].to_numpy()[v]
        if job.link_type == "link_and_dedupe":
            data["_source_table_l"] = records["_source_table"].to_numpy()[u]
            data["_source_table_r"] = records["_source_table"].to_numpy()[v]
        data["nodes_l"] = self.side_u[keep].astype(np.int64)
        data["nodes_r"] = self.side_v[keep].astype(np.int64)
        data["n_nodes"] = data["nodes_l"] + data["nodes_r"]
        return pd.DataFrame(data, columns=bridge_edge_columns(frame.settings, job.link_type))

    def cores(self):
        """The cluster frame's columns plus core_id: the smallest input position among the records that stay connected
        to this one when every bridge is cut ("the clusters if every bridge were cut")."""
        out = ClusterFrame.toPandas(self._frame)
        out["core_id"] = self.core.astype(np.int64)
        return out


class _SweepLevelFrame(ClusterFrame):
    """ClusterSweepFrame.at(t): its `filtered` is the sweep's wide frame, so the metrics are the sweep's at t."""

    def metrics(self):
        sweep, t = self._of
        return sweep.metrics(t)

    def bridges(self):
        sweep, t = self._of
        return sweep.bridges(t)

    def truth_table(self, label_column):
        """The sweep's truth-table row at this frame's threshold."""
        sweep, t = self._of
        table = sweep.truth_table(label_column)
        return table.iloc[[sweep.thresholds.index(float(t))]].reset_index(drop=True)


class ClusterSweepFrame(SplinkDataFrame):
    """`filtered.clusters_at_thresholds(thresholds)`: the clusters of the frame's pairs with score > t, for every t, from
    one selection and one nested sweep on the device (spk_components_sweep).  One row per input record, in input
    order, and one column cluster_id_{t!r} per threshold, each equal to clusters(t)'s cluster_id.

    On a job sharded over a process group every rank sweeps its shard's pairs and the ranks merge level by level
    (spk_components_sweep_merge), so toPandas(), at(t) and truth_table() are collectives: every rank makes the same
    calls in the same order and ends with the one-GPU frames.  metrics(), summary() and bridges() are refused there."""

    def __init__(self, filtered: FilteredFrame, thresholds, by=None):
        from .select import BEST_BY
        self.thresholds, self._desc, self._level = sweep_thresholds(thresholds)
        scores = getattr(filtered, "inner", filtered)._best_by  # a best-match frame carries its inner frame's scores
        by = scores[0] if by is None else by
        if not isinstance(by, str) or by not in scores:
            raise ValueError(f"clusters_at_thresholds: by={by!r}; legal values: " + ", ".join(repr(b) for b in scores))
        if filtered._scored_parent() is None:
            raise ValueError("clusters_at_thresholds: this frame has no score to put thresholds on (it was filtered "
                             "from an unscored frame): filter the frame run_expectation_step returns")
        job = filtered.job
        if getattr(job, "passthrough", None) is not None:
            raise ValueError("clusters_at_thresholds() needs the records: a job made from a gamma table has pairs "
                             "without rows")
        _refuse_unreachable_shards(job, "clusters_at_thresholds()")
        self.filtered = filtered
        self.job = job
        self.settings = filtered.settings
        self.by = by
        self._field = BEST_BY[by]
        self._labels = None  # [level][node]
        self._info = None    # (n_nodes, n_edges [L], n_clusters [L], rounds [L]), levels in descending threshold

    def _sweep(self):
        """Make the context's sweep this frame's (the frame's re-select rules, then the sweep).  On a job sharded over
        the process group the ranks then gather and merge level by level (a collective per level, n_nodes labels per
        rank in flight), n_edges is summed over the ranks and n_clusters are the merged counts."""
        from . import distributed as D
        job = self.job
        job.sweep_owner = None
        self.filtered._select()
        info = job.ctx.components_sweep(self._field, self._desc)
        if _merges_across_ranks(job):
            n_nodes, n_edges, n_clusters, rounds = info
            for k in range(len(self._desc)):
                n_clusters[k], more = _merge_sweep_level(job, int(n_nodes), k)
                rounds[k] += more
                n_edges[k] = D.sum_over_ranks(int(n_edges[k]))
        job.sweep_owner = self
        return info

    def _run(self):
        """Select, sweep and copy every level's labels at once, in ranges: a later selection, components or sweep call
        of the job does not reach them."""
        if self._labels is None:
            ctx = self.job.ctx
            info = self._sweep()
            n_nodes = int(info[0])
            self._labels = [_copy_in_ranges(lambda s, c, k=k: ctx.components_sweep_copy(k, s, c), n_nodes, np.uint32)
                            for k in range(len(self._desc))]
            self._info = (n_nodes, info[1].copy(), info[2].copy(), info[3].copy())
        return self._labels

    def _held(self):
        """The context holds this frame's sweep (metrics and summary count on the device): sweep again if not."""
        self._run()
        if self.job.sweep_owner is not self:
            self._sweep()

    def _level_of(self, t):
        t = float(t)
        if t not in self.thresholds:
            raise ValueError(f"{t!r} is not one of this frame's thresholds: " + ", ".join(repr(x) for x in self.thresholds))
        return self._level[self.thresholds.index(t)]

    def _column_order(self):
        cols = [self.settings["unique_id_column_name"]]
        if self.job.link_type in ("link_only", "link_and_dedupe"):
            cols.append("_source_table")
        return cols + sweep_column_names(self.thresholds)

    def count(self) -> int:
        return int(sum(len(t) for t in self.job.inputs))

    def at(self, t):
        """The clusters at threshold t as a ClusterFrame: the same toPandas(singletons=...), n_clusters and rounds."""
        k = self._level_of(t)
        labels = self._run()[k]
        out = _SweepLevelFrame(self.filtered)
        out._of = (self, t)
        out._labels = labels
        out._info = (self._info[0], int(self._info[2][k]), int(self._info[3][k]))
        return out

    def toPandas(self):
        labels = self._run()
        base = ClusterFrame.toPandas(self.at(self.thresholds[0])).drop(columns="cluster_id")
        for t, name in zip(self.thresholds, sweep_column_names(self.thresholds)):
            base[name] = labels[self._level_of(t)].astype(np.int64)
        return base

    def metrics(self, t):
        """Cluster and node metrics at threshold t: a `ClusterMetrics`."""
        k = self._level_of(t)
        _refuse_sharded_metrics(self.job, "metrics()")
        self._held()
        return ClusterMetrics(self.at(t), self._labels[k], self.job.ctx, k)

    def bridges(self, t):
        """The bridges and cores of the clusters at threshold t: a `ClusterBridges`."""
        k = self._level_of(t)
        _refuse_sharded_metrics(self.job, "bridges()")
        self._held()
        return ClusterBridges(self.at(t), self._labels[k], self.job.ctx, k)

    def truth_table(self, label_column):
        """The clusters at every threshold against `label_column` of the input tables, one row per threshold in the
        order given (labels.cluster_truth_rows): a pair of labelled records is predicted at t iff both lie in one
        cluster at t.  One spk_cluster_agreement call over all levels of this frame's sweep; about ten integers per
        threshold leave the device."""
        from .labels import cluster_truth_rows
        _node_label_ids(self.job, label_column)  # a missing column fails before the device is touched
        self._held()
        counts = _cluster_agreement(self.job, label_column)
        return cluster_truth_rows(counts[[self._level_of(t) for t in self.thresholds]], self.thresholds)

    def summary(self):
        """One row per threshold, in the order given: threshold, n_edges (pairs with score > threshold), n_clusters,
        n_clusters_multi (clusters of two or more records), records_clustered (records in those), largest_cluster,
        rounds."""
        _refuse_sharded_metrics(self.job, "summary()")
        self._held()
        rows = []
        for t in self.thresholds:
            k = self._level_of(t)
            multi, nodes, largest = self.job.ctx.cluster_metrics(k)
            rows.append((t, int(self._info[1][k]), int(self._info[2][k]), multi, nodes, largest, int(self._info[3][k])))
        return pd.DataFrame(rows, columns=["threshold", "n_edges", "n_clusters", "n_clusters_multi",
                                           "records_clustered", "largest_cluster", "rounds"])


def reject_filtered(frame, what):
    """The stage functions run over every pair of a job: a filtered frame must not slip into them."""
    if isinstance(frame, BestMatchFrame):
        raise ValueError(f"{what} does not take a best-match frame (it would run over all of the job's pairs, not the "
                         "kept ones): pass the frame filter() was called on")
    if isinstance(frame, FilteredFrame):
        raise ValueError(f"{what} does not take a filtered frame (it would run over all of the job's pairs, not the "
                         "survivors): pass the frame filter() was called on")
    if isinstance(frame, (ClusterFrame, ClusterSweepFrame, ClusterMetrics, ClusterBridges)):
        raise ValueError(f"{what} does not take a cluster frame (it holds records, not pairs): pass the frame "
                         "filter() was called on")
