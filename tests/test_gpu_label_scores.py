"""Scores against labels, per pair, on the device (spk_label_scores_*) and the frames above them.

Hand-made contexts compare the counts with np.bincount over np.searchsorted(thresholds, score, side="left") of the
values spk_tf_apply / spk_select_copy* return (a NaN score in bin T + 1); the pipelines compare truth_table() of the
term-frequency, filtered and best-match frames with the table computed in pandas from the frames' own toPandas() with
the label column retained, the only route there was before.  Every comparison is exact."""
import ctypes
import socket
import warnings

import numpy as np
import pandas as pd
import pytest

from test_gpu_labels import labelled_records, m_u, make_ctx, random_case
from test_gpu_tf_select import random_tables

pytestmark = pytest.mark.gpu
warnings.filterwarnings("ignore")

MP = "match_probability"
TF = "tf_adjusted_match_prob"
LAM = 0.3
INTS = ["tp", "fp", "tn", "fn", "n_unlabelled_above"]
# column 0, level 1: m = u = 0, a NULL match_probability; column 1, level 2: u = 0, match_probability exactly 1, which
# a table entry of 0.0 turns into 0 / 0: a NULL tf score of a pair whose match_probability is not NULL
# (test_gpu_tf_select.py::test_null_tf_with_and_without_a_null_match_probability)
LEVELS = [2, 3]
M_NULL = np.array([0.3, 0.0, 0.2, 0.3, 0.5])
U_NULL = np.array([0.6, 0.0, 0.5, 0.4, 0.0])


@pytest.fixture(scope="module")
def amd():
    from splink_amd import AmdSession, _native
    if _native.device_count() == 0:
        pytest.fail("no HIP device visible: the -m gpu tests need an MI355X")
    return AmdSession(0)


def states(rows_l, rows_r, lab0, lab1=None):
    a = np.asarray(lab0)[rows_l]
    b = np.asarray(lab0 if lab1 is None else lab1)[rows_r]
    return np.where((a < 0) | (b < 0), 2, (a == b).astype(np.int64))


def expected(state, score, t):
    """[3, T + 2]: bin = thresholds below the score (`>`), a NaN score in bin T + 1."""
    T = len(t)
    b = np.searchsorted(np.asarray(t, dtype=np.float64), score, side="left")
    b[np.isnan(score)] = T + 1
    return np.bincount(np.asarray(state) * (T + 2) + b, minlength=3 * (T + 2)).reshape(3, T + 2)


class TfCase:
    """A context with loaded pairs and levels, label ids, host tf value ids and tables, and the parent values:
    ctx.score and ctx.tf_apply over every pair (computed once, never changed)."""

    def __init__(self, seed, P, levels=LEVELS, n0=97, n1=None, n_tf=1, m=M_NULL, u=U_NULL):
        rng = np.random.Generator(np.random.PCG64(seed))
        self.rng, self.P, self.levels = rng, P, levels
        self.rows_l, self.rows_r, self.g, self.lab0, self.lab1 = random_case(rng, P, levels, n0, n1)  # 15 % NULL labels
        self.c = make_ctx(self.rows_l, self.rows_r, self.g, levels, n0, n1)
        if m is None:
            m, u = m_u(levels, rng)
        self.m, self.u = m, u
        sizes = (6, 5)[:n_tf]  # the second table is shorter than the id range: an id past it reads no entry
        nr = n0 if n1 is None else n1
        self.ids0 = [rng.integers(-1, 6, n0).astype(np.int64) for _ in sizes]
        self.ids1 = [rng.integers(-1, 6, nr).astype(np.int64) for _ in sizes] if n1 is not None else \
            [x.copy() for x in self.ids0]
        self.tables = random_tables(rng, sizes)
        self.state = states(self.rows_l, self.rows_r, self.lab0, self.lab1)
        if P:
            self.mp = self.c.score(LAM, 1 - LAM, m, u, 0, P)
            self.tf, _ = self.c.tf_apply(self.ids0, self.ids1, self.tables, 0, P)
        else:
            self.mp = self.tf = np.zeros(0)

    def counts(self, t):
        return self.c.label_scores_tf(self.lab0, self.lab1, LAM, 1 - LAM, self.m, self.u, self.ids0, self.ids1,
                                      self.tables, t)

    def check(self, t):
        got = self.counts(t)
        assert got.dtype == np.int64 and got.shape == (3, len(t) + 2)
        assert np.array_equal(got, expected(self.state, self.tf, t)), len(t)
        assert got.sum() == self.P and self.c.label_scores_info() == (self.P, -1.0)
        return got


def thresholds_for(case, T):
    """T ascending thresholds over the range the scores take, with duplicates."""
    if T == 0:
        return np.zeros(0)
    if T == 1:
        return np.array([np.nanmedian(case.tf) if case.P and not np.isnan(case.tf).all() else 0.5])
    t = case.rng.random(T)
    t[::9] = t[1::9][:len(t[::9])]
    return np.sort(t)


# ---- 1. the all-pairs kernel: tail, vector path, partial wave, several workgroups, the grid-stride loop -----------
def _grid_step():
    import torch
    from splink_amd import _native as N
    return N.LABEL_SCORE_WG_PER_CU * torch.cuda.get_device_properties(0).multi_processor_count * N.LABEL_SCORE_STEP


@pytest.mark.parametrize("P", [0, 1, 63, 64, 65, 8 * 64 + 5, "grid_step"])
def test_pair_counts_against_tf_apply(P, amd):
    big = P == "grid_step"
    P = _grid_step() + 5 if big else P  # every workgroup of the capped grid takes a second step, and a tail
    case = TfCase(1000 + (7 if big else P), P)
    assert case.c.label_scores_info() == (-1, -1.0)
    for T in (0, 1, 1024):
        case.check(thresholds_for(case, T))
    if big:
        null_tf, null_mp = np.isnan(case.tf), np.isnan(case.mp)
        assert (null_tf & null_mp).any() and (null_tf & ~null_mp).any() and (~null_tf).any()
        assert len(np.unique(case.state)) == 3
    case.c.close()


@pytest.mark.parametrize("n_tf", [1, 2])
@pytest.mark.parametrize("two", [False, True], ids=["one_table", "link_only"])
@pytest.mark.parametrize("wide", [False, True], ids=["codes16", "codes32"])
def test_code_widths_tables_and_columns(wide, two, n_tf, amd):
    levels = [4] * 9 if wide else LEVELS  # 5^9 patterns: uint32 codes
    case = TfCase(50 + 4 * wide + 2 * two + n_tf, 8 * 700 + 3, levels, 211, 157 if two else None, n_tf,
                  *((None, None) if wide else (M_NULL, U_NULL)))
    assert (case.c.n_patterns() > 1 << 16) == wide
    case.c.enable_timing(True)
    t = thresholds_for(case, 72)
    got = case.counts(t)
    pairs, ms = case.c.label_scores_info()
    assert pairs == case.P and ms > 0.0
    case.c.enable_timing(False)
    assert np.array_equal(got, expected(case.state, case.tf, t))
    for T in (0, 1, 1024):
        case.check(thresholds_for(case, T))
    if two:
        with pytest.raises(ValueError, match="link_only"):  # NULL ids_side1 under link_only
            case.c.label_scores_tf(case.lab0, None, LAM, 1 - LAM, case.m, case.u, case.ids0, case.ids1, case.tables, [])
    else:  # an explicit second label array is honoured
        other = case.rng.integers(-1, 5, 211).astype(np.int64)
        got = case.c.label_scores_tf(case.lab0, other, LAM, 1 - LAM, case.m, case.u, case.ids0, case.ids1,
                                     case.tables, [0.5])
        assert np.array_equal(got, expected(states(case.rows_l, case.rows_r, case.lab0, other), case.tf, [0.5]))
    case.c.close()


# ---- 2. thresholds on occurring values: one ulp or a `>=` changes a count ------------------------------------------
def test_thresholds_equal_to_occurring_scores(amd):
    case = TfCase(5, 4099)
    values, n = np.unique(case.tf[~np.isnan(case.tf)], return_counts=True)
    tied = values[n >= 2]
    assert len(tied) >= 8 and n.max() > 10
    t = np.sort(np.concatenate([tied, np.nextafter(tied, -np.inf), np.nextafter(tied, np.inf)]))[:1024]
    got = case.check(t)
    # a `>=`, or a score one ulp off spk_tf_apply's, would move the pairs tied at a threshold one bin up or down
    k = int(np.searchsorted(t, tied[0], side="left"))
    assert t[k] == tied[0] and got[:, k].sum() == n[values == tied[0]][0]
    case.check(np.array([-np.inf, -np.inf, tied[3], tied[3], np.inf]))
    case.c.close()


# ---- 3. hot counters -------------------------------------------------------------------------------------------
def test_one_bin_and_every_bin(amd):
    from splink_amd import _native as N
    P, n0 = 8 * 600 + 7, 50
    m, u = np.full(5, 0.5), np.full(5, 0.25)
    # every pair with one pattern, one label and no tf lookup: one score, one state -- 64 equal LDS addresses per wave
    g = np.tile(np.array([1, 2]), (P, 1))
    rows = np.arange(P) % n0
    c = make_ctx(rows, rows[::-1].copy(), g, LEVELS, n0)
    lab = np.full(n0, 3, dtype=np.int64)
    none = [np.full(n0, -1, dtype=np.int64)]
    tables = [np.full(4, 0.5)]
    c.score(LAM, 1 - LAM, m, u, 0, P)
    tf, _ = c.tf_apply(none, none, tables, 0, P)
    s = float(tf[0])
    assert len(np.unique(tf)) == 1 and 0.0 < s < 1.0
    t = np.sort(np.concatenate([np.linspace(0.0, s, 500, endpoint=False), np.linspace(s, 1.0, 524)]))  # 500 below s
    got = c.label_scores_tf(lab, None, LAM, 1 - LAM, m, u, none, none, tables, t)
    want = np.zeros((3, 1026), dtype=np.int64)
    want[1, 500] = P
    assert np.array_equal(got, want)
    c.close()
    # every pair in a bin of its own, as far as the bins go: link_only, left row v carries value id v, the right
    # table one row per (state, value) with the value's id, so the tf score of pair p is bayes(1/2, table[p mod 1025])
    # = table[p mod 1025] up to rounding and its state p // 1025 mod 3
    T = N.LABEL_SCORE_MAX_THRESHOLDS
    p = np.arange(P)
    v = p % (T + 1)
    state = (p // (T + 1)) % 3
    n1 = 3 * (T + 1)
    rows_l = v.copy()
    rows_r = state * (T + 1) + v
    lab0 = np.full(T + 1, 5, dtype=np.int64)
    lab1 = np.concatenate([np.full(T + 1, 6), np.full(T + 1, 5), np.full(T + 1, -1)]).astype(np.int64)
    ids0 = [np.arange(T + 1, dtype=np.int64)]
    ids1 = [np.tile(np.arange(T + 1, dtype=np.int64), 3)]
    table = (np.arange(T + 1) + 0.5) / (T + 1)
    c = make_ctx(rows_l, rows_r, np.zeros((P, 2), dtype=np.int64), LEVELS, T + 1, n1)
    m = u = np.full(5, 0.5)
    lam = 0.5
    c.score(lam, 1 - lam, m, u, 0, P)
    tf, _ = c.tf_apply(ids0, ids1, [table], 0, P)
    distinct = np.unique(tf)
    assert len(distinct) == T + 1
    t = (distinct[:-1] + distinct[1:]) / 2  # T thresholds between the T + 1 values
    got = c.label_scores_tf(lab0, lab1, lam, 1 - lam, m, u, ids0, ids1, [table], t)
    want = expected(state, tf, t)
    assert np.array_equal(got, want) and (want[:, :T + 1] > 0).all() and want[:, T + 1].sum() == 0
    c.close()


# ---- 4. the selection kernel -------------------------------------------------------------------------------------
def selection_expected(case, field_tf, t, n_tf):
    c = case.c
    k = c.select_info()[0]
    if k == 0:
        return np.zeros((3, len(t) + 2), dtype=np.int64)
    _, l, r, _, mp = c.select_copy(0, k, len(case.levels))
    score = c.select_copy_tf(0, k, n_tf, adj=False)[0] if field_tf else mp
    return expected(states(l, r, case.lab0, case.lab1), score, t)


def test_selection_fields_and_best_matches(amd):
    from splink_amd import _native as N
    case = TfCase(21, 8 * 900 + 3, n_tf=2)
    c = case.c
    t_all = [np.zeros(0), thresholds_for(case, 1), thresholds_for(case, 1024)]
    # a plain selection: match_probability
    k = c.select(LAM, 1 - LAM, case.m, case.u, [(N.SEL_GAMMA, 1, N.SEL_OP[">="], 0.0)])
    assert 0 < k < case.P
    for t in t_all:
        got = c.label_scores_selection(case.lab0, case.lab1, N.SEL_MP, t)
        assert np.array_equal(got, selection_expected(case, False, t, 2)) and got.sum() == k
        assert c.label_scores_info() == (k, -1.0)
    assert got[:, -1].sum() > 0  # NULL match_probability among the survivors
    with pytest.raises(RuntimeError, match="without tf tables"):
        c.label_scores_selection(case.lab0, case.lab1, N.SEL_TF_MP, [])
    assert c.label_scores_info() == (-1, -1.0) and c.select_info()[0] == k  # the selection survives a refusal
    # a tf selection: both fields
    term = (N.SEL_TF_MP, 0, N.SEL_OP[">"], float(np.nanquantile(case.tf, 0.3)))
    k = c.select_tf(LAM, 1 - LAM, case.m, case.u, case.ids0, case.ids1, case.tables,
                    [term, (N.SEL_GAMMA, 0, N.SEL_OP[">="], -1.0)])
    assert 0 < k < case.P
    for field_tf in (False, True):
        for t in t_all:
            got = c.label_scores_selection(case.lab0, case.lab1, N.SEL_TF_MP if field_tf else N.SEL_MP, t)
            assert np.array_equal(got, selection_expected(case, field_tf, t, 2)) and got.sum() == k
    # narrowed to a one-to-one link
    kept = c.select_best(N.SEL_TF_MP, N.BEST_MUTUAL, 0)
    assert 0 < kept < k
    for field_tf in (False, True):
        for t in t_all:
            got = c.label_scores_selection(case.lab0, case.lab1, N.SEL_TF_MP if field_tf else N.SEL_MP, t)
            assert np.array_equal(got, selection_expected(case, field_tf, t, 2)) and got.sum() == kept
    # an empty selection counts nothing
    assert c.select(LAM, 1 - LAM, case.m, case.u, [(N.SEL_MP, 0, N.SEL_OP[">"], 2.0)]) == 0
    got = c.label_scores_selection(case.lab0, case.lab1, N.SEL_MP, t_all[1])
    assert got.shape == (3, 3) and got.sum() == 0 and c.label_scores_info() == (0, -1.0)
    c.close()


def test_selection_states(amd):
    from splink_amd import _native as N
    case = TfCase(22, 8 * 100 + 1)
    c = case.c
    with pytest.raises(RuntimeError, match="no selection"):
        c.label_scores_selection(case.lab0, None, N.SEL_MP, [])
    # a selection made without m / u has no match_probability
    k = c.select(0.0, 0.0, None, None, [(N.SEL_GAMMA, 0, N.SEL_OP[">="], 0.0)])
    assert k > 0
    with pytest.raises(RuntimeError, match="no m / u"):
        c.label_scores_selection(case.lab0, None, N.SEL_MP, [])
    with pytest.raises(ValueError, match="unknown field"):
        c.label_scores_selection(case.lab0, None, N.SEL_GAMMA, [])
    with pytest.raises(ValueError, match="unknown field"):
        c.label_scores_selection(case.lab0, None, N.SEL_ALL, [])
    # a stale selection: new codes
    c.select(LAM, 1 - LAM, case.m, case.u, [])
    assert c.label_scores_selection(case.lab0, None, N.SEL_MP, []).sum() == case.P
    c.gammas_load(case.levels, case.g.astype(np.int8))
    with pytest.raises(RuntimeError, match="changed since spk_select"):
        c.label_scores_selection(case.lab0, None, N.SEL_MP, [])
    c.close()


# ---- 5. errors and bystanders ----------------------------------------------------------------------------------
def test_argument_and_state_errors(amd):
    from splink_amd import _native as N
    case = TfCase(31, 8 * 50 + 3, n0=40)
    c = case.c
    args = (LAM, 1 - LAM, case.m, case.u, case.ids0, case.ids1, case.tables)
    c.select(LAM, 1 - LAM, case.m, case.u, [])
    for bad, what in (([0.1, np.nan], "NaN"), ([0.5, 0.4], "descend"), (np.linspace(0, 1, 1025), "1024")):
        with pytest.raises(ValueError, match=what):
            c.label_scores_tf(case.lab0, None, *args, bad)
        with pytest.raises(ValueError, match=what):
            c.label_scores_selection(case.lab0, None, N.SEL_MP, bad)
        assert c.label_scores_info() == (-1, -1.0)
    assert c.label_scores_tf(case.lab0, None, *args, np.linspace(0, 1, 1024)).sum() == case.P
    big = case.lab0.copy()
    big[5] = 1 << 31
    with pytest.raises(ValueError, match="2\\^31"):
        c.label_scores_tf(big, None, *args, [0.5])
    with pytest.raises(ValueError, match="2\\^31"):
        c.label_scores_selection(big, None, N.SEL_MP, [0.5])
    big[5] = (1 << 31) - 1
    assert c.label_scores_tf(big, None, *args, [0.5]).sum() == case.P
    t = np.array([0.5])
    with pytest.raises(ValueError, match="out_counts"):  # NULL out_counts (straight at the ABI)
        N.check(c._lib.spk_label_scores_selection(c._h, N._ptr(case.lab0), N._ptr(None), ctypes.c_int(N.SEL_MP),
                                                  ctypes.c_int(1), N._ptr(t), N._ptr(None)),
                "spk_label_scores_selection")
    with pytest.raises(ValueError, match="1..8 columns"):
        c.label_scores_tf(case.lab0, None, LAM, 1 - LAM, case.m, case.u, [], [], [], [])
    with pytest.raises(ValueError, match="1..8 columns"):
        c.label_scores_tf_columns(case.lab0, None, LAM, 1 - LAM, case.m, case.u, [], [], [])
    with pytest.raises(RuntimeError, match="dictionary ids"):  # columns made without device ids
        c.label_scores_tf_columns(case.lab0, None, LAM, 1 - LAM, case.m, case.u, [0], case.tables, [])
    c.close()
    gt = N.Context(0)  # a loaded gamma table: codes without pair rows
    gt.table_create(0, 40, 1)
    gt.gammas_load(LEVELS, case.g.astype(np.int8))
    with pytest.raises(RuntimeError, match="no pair rows"):
        gt.label_scores_tf(case.lab0, None, *args, [0.5])
    gt.select(LAM, 1 - LAM, case.m, case.u, [])
    with pytest.raises(RuntimeError, match="no pair rows"):
        gt.label_scores_selection(case.lab0, None, N.SEL_MP, [0.5])
    assert gt.label_scores_info() == (-1, -1.0)
    gt.close()
    nc = N.Context(0)
    nc.table_create(0, 40, 1)
    with pytest.raises(RuntimeError, match="no gammas"):
        nc.label_scores_tf(case.lab0, None, *args, [0.5])
    nc.close()


def test_bystanders_untouched(amd):
    """test_gpu_labels.py::test_bystanders_untouched for the new calls: the selection, the scores a later tf_apply
    reads (ctx->mp), the tf sums, the components and spk_ctx_memory are the same before and after."""
    from splink_amd import _native as N
    case = TfCase(41, 8 * 200 + 3, n0=120)
    c, P = case.c, case.P
    m, u = m_u(LEVELS, case.rng)
    cut = float(np.nanmedian(c.score(LAM, 1 - LAM, m, u, 0, P)))
    c.score(LAM, 1 - LAM, m, u, 0, P, want_host=False)
    k = c.select_tf(LAM, 1 - LAM, m, u, case.ids0, case.ids1, case.tables, [(N.SEL_MP, 0, N.SEL_OP[">"], cut)])
    assert 0 < k < P
    nodes, _, _ = c.components()

    def snapshot():
        return (c.select_copy(0, k, 2), c.select_copy_tf(0, k, 1), c.components_copy(0, nodes),
                c.tf_accumulate(6, case.ids0[0], case.ids1[0]), c.tf_apply(case.ids0, case.ids1, case.tables, 0, P),
                c.select_info()[0], c.components_info()[:2])

    before = snapshot()
    mem = c.memory()
    # other parameters (case.m / case.u) than the selection's and the scores'
    got = c.label_scores_tf(case.lab0, None, LAM, 1 - LAM, case.m, case.u, case.ids0, case.ids1, case.tables,
                            [0.2, 0.7])
    assert np.array_equal(got, expected(case.state, case.tf, [0.2, 0.7]))
    sel = c.label_scores_selection(case.lab0, None, N.SEL_TF_MP, [0.2, 0.7])
    assert sel.sum() == k
    assert c.memory() == mem  # the calls' buffers are gone
    after = snapshot()
    for x, y in zip(before[:5], after[:5]):
        for a, b in zip(x, y) if isinstance(x, tuple) else ((x, y),):
            assert (a is None and b is None) or np.array_equal(a, b, equal_nan=True)
    assert before[5:] == after[5:]
    c.close()


# ---- 6. pipelines ------------------------------------------------------------------------------------------------
def tf_job(amd, link_type, tables, shard=(0, 1)):
    """test_gpu_labels.py::scored_job with tf on surname, and the term-frequency frame."""
    from splink_amd.engine import Job
    from splink_amd.frames import ExpectationFrame, GammaFrame
    from splink_amd.params import Params
    from splink_amd.synthetic import cfg_settings
    from splink_amd.term_frequencies import make_adjustment_for_term_frequencies
    s = cfg_settings(2)
    s["link_type"] = link_type
    s["additional_columns_to_retain"] = ["cluster"]
    for col in s["comparison_columns"]:
        if col["col_name"] == "surname":
            col["term_frequency_adjustments"] = True
    params = Params(s, amd)
    st = params.settings
    job = Job(link_type, tables, "unique_id", 0, shard=shard)
    job.block(st["blocking_rules"])
    df_e = ExpectationFrame(GammaFrame(job, st), st, params.params["λ"], params._level_probabilities())
    make_tf = lambda: make_adjustment_for_term_frequencies(df_e, params, st, amd)  # noqa: E731
    return df_e, make_tf


def truth_states(pdf):
    a, b = pdf["cluster_l"], pdf["cluster_r"]
    known = (a.notna() & b.notna()).to_numpy()
    same = (a == b).to_numpy()
    return known & same, known & ~same, ~known


def pandas_table(pdf, score, ts, totals, all_true):
    """LabelCounts.truth_table's columns from a frame with the labels retained: the rows `pdf[score] > t` predicted
    (ts = None: every row of pdf, threshold -inf); totals: labelled (matches, non-matches) among all candidates."""
    match, non, unknown = truth_states(pdf)
    rows = []
    for t in ([-np.inf] if ts is None else ts):
        above = np.ones(len(pdf), dtype=bool) if ts is None else (pdf[score] > t).to_numpy()
        tp, fp, unl = int((above & match).sum()), int((above & non).sum()), int((above & unknown).sum())
        fn, tn = totals[0] - tp, totals[1] - fp
        div = lambda a, b: a / b if b else np.nan  # noqa: E731
        rows.append((t, tp, fp, tn, fn, unl, div(tp, tp + fp), div(tp, tp + fn), div(fp, fp + tn),
                     div(2 * tp, 2 * tp + fp + fn), div(tp, all_true)))
    return pd.DataFrame(rows, columns=["threshold"] + INTS + ["precision", "recall", "fpr", "f1",
                                                                "recall_of_all_true_pairs"])


def same_table(got, exp):
    assert list(got.columns) == list(exp.columns) and len(got) == len(exp)
    for col in got.columns:
        assert np.array_equal(got[col].to_numpy(), exp[col].to_numpy(), equal_nan=True), col


class Pipeline:
    def __init__(self, amd, link_type):
        df = labelled_records(3000, seed=3)
        self.tables = [df] if link_type == "dedupe_only" else \
            [df.iloc[::2].reset_index(drop=True), df.iloc[1::2].reset_index(drop=True)]
        self.df_e, self.make_tf = tf_job(amd, link_type, self.tables)
        self.pdf = self.make_tf().toPandas()  # the reference frame: made once, shared, never changed
        match, non, _ = truth_states(self.pdf)
        self.totals = (int(match.sum()), int(non.sum()))
        self.all_true = self.df_e.label_counts("cluster").true_pairs_total
        assert self.totals[0] > 0 and self.totals[1] > 0 and self.pdf[TF].nunique() > 100


@pytest.fixture(scope="module", params=["dedupe_only", "link_only"])
def pipe(request, amd):
    return Pipeline(amd, request.param)


def test_tf_truth_table_matches_pandas(pipe):
    tf = pipe.make_tf()

    def boom():
        raise AssertionError("the per-pair part of the tf frame ran")
    tf._apply = boom
    ref = pipe.df_e.truth_table("cluster")
    got = tf.truth_table("cluster")
    assert np.array_equal(got["threshold"].to_numpy(), ref["threshold"].to_numpy()) and len(got) > 10
    same_table(got, pandas_table(pipe.pdf, TF, ref["threshold"].to_numpy(), pipe.totals, pipe.all_true))
    assert list(got.dtypes) == list(ref.dtypes)
    # thresholds on occurring tf scores, given in any order
    occurring = np.sort(pipe.pdf[TF].dropna().unique())
    ts = np.concatenate([occurring[::max(len(occurring) // 40, 1)], [0.5, 0.99, -1.0, 2.0]])
    same_table(tf.truth_table("cluster", ts[::-1]), pandas_table(pipe.pdf, TF, np.sort(ts), pipe.totals, pipe.all_true))
    assert tf._pair is None
    with pytest.raises(ValueError, match="more than"):
        tf.truth_table("cluster", np.linspace(0, 1, 1025))
    with pytest.raises(ValueError, match="missing from input table 0"):
        tf.truth_table("truth")


def test_filter_identity_for_a_pattern_score(pipe):
    df_e = pipe.df_e
    mids = np.sort(pipe.pdf[MP].dropna().unique())
    t0 = float((mids[len(mids) // 3] + mids[len(mids) // 3 + 1]) / 2)
    ts = [t0] + [float(x) for x in mids[mids > t0][::5]] + [1.0]
    got = df_e.filter(f"{MP} > {t0!r}").truth_table("cluster", ts)
    ref = df_e.truth_table("cluster", ts)
    same_table(got, ref)
    assert got["tp"].iloc[0] > 0 and len(got) > 3


def test_gamma_filter_and_best_matches_rows(pipe):
    df_e, tf = pipe.df_e, pipe.make_tf()
    # a filter with a gamma term: its row against the labelled pairs of the unfiltered frame
    f = df_e.filter(f"gamma_surname >= 1 and {MP} > 0.05")
    kept = f.toPandas()
    assert 0 < len(kept) < len(pipe.pdf)
    same_table(f.truth_table("cluster"), pandas_table(kept, MP, None, pipe.totals, pipe.all_true))
    ts = [0.2, 0.9]
    same_table(f.truth_table("cluster", ts), pandas_table(kept, MP, ts, pipe.totals, pipe.all_true))
    # the same on the tf frame, by either score
    g = tf.filter(f"gamma_first_name >= 1 and {TF} > 0.05")
    kept = g.toPandas()
    assert 0 < len(kept) < len(pipe.pdf)
    same_table(g.truth_table("cluster"), pandas_table(kept, TF, None, pipe.totals, pipe.all_true))
    same_table(g.truth_table("cluster", ts), pandas_table(kept, TF, ts, pipe.totals, pipe.all_true))
    same_table(g.truth_table("cluster", ts, by=MP), pandas_table(kept, MP, ts, pipe.totals, pipe.all_true))
    with pytest.raises(ValueError, match="no score"):
        f.truth_table("cluster", ts, by=TF)
    with pytest.raises(ValueError, match="no score"):
        df_e.gammas.filter("gamma_surname >= 1").truth_table("cluster")
    # one-to-one links
    for frame in (df_e.best_matches(per="mutual"), tf.best_matches(per="mutual"), tf.best_matches(0.5, per="l")):
        kept = frame.toPandas()
        row = frame.truth_table("cluster")
        same_table(row, pandas_table(kept, MP, None, pipe.totals, pipe.all_true))
        unknown = int(truth_states(kept)[2].sum())  # 5 % NULL labels: kept pairs that are neither tp nor fp
        r = row.iloc[0]
        assert r["tp"] + r["fp"] + r["n_unlabelled_above"] == frame.count() == len(kept)
        assert r["tp"] + r["fp"] == frame.count() - unknown and r["tp"] > 0
        score = TF if "tf_adjusted_match_prob" in kept.columns else MP
        same_table(frame.truth_table("cluster", ts), pandas_table(kept, score, ts, pipe.totals, pipe.all_true))


def test_frames_leave_scores_tf_and_em_alone(pipe):
    """test_gpu_tf_select.py::test_select_tf_leaves_scores_tf_and_em_alone for truth_table(): a device-resident
    tf_mp, the tf sums and the EM statistics are the same before and after."""
    df_e, job = pipe.df_e, pipe.df_e.job
    tf = pipe.make_tf()
    df_e.gammas.ensure_codes()
    stats0 = job.em_stats(df_e.lam, df_e.level_probs)
    job.score(df_e.lam, df_e.level_probs, want_host=False)
    job.ctx.tf_apply_columns(tf.dev_cols, tf.tables, 0, job.n_pairs, want_adj=False, want_host=False)
    before = job.ctx.tf_copy(10, 200)
    assert before.tobytes() == pipe.pdf[TF].to_numpy()[10:210].tobytes()
    col = tf.dev_cols[0]
    nv = job.ctx.tf_column_values(col)

    def tf_state():
        scale = job.ctx.tf_scales_column(col, nv)
        limbs, counts = job.ctx.tf_accumulate_column_exact(col, nv, scale)
        return scale.copy(), limbs.copy(), counts.copy()
    state0 = tf_state()
    assert len(tf.truth_table("cluster", [0.5])) == 1
    assert len(tf.filter(f"{TF} > 0.5").truth_table("cluster")) == 1
    assert job.ctx.tf_copy(10, 200).tobytes() == before.tobytes()
    for a, b in zip(state0, tf_state()):
        assert np.array_equal(a, b)
    assert np.array_equal(stats0, job.em_stats(df_e.lam, df_e.level_probs), equal_nan=True)


def test_refusals_before_the_device(amd):
    from test_gpu_select import gamma_table_frame
    df = labelled_records(600, seed=9)
    df_e, _ = tf_job(amd, "dedupe_only", [df], shard=(0, 2))
    with pytest.raises(ValueError, match="shards"):  # best matches on a sharded job
        df_e.best_matches(per="mutual")
    f = df_e.filter(f"{MP} > 0.5")
    with pytest.raises(ValueError, match="missing from input table 0"):
        f.truth_table("truth")
    assert df_e.job.selection_owner is None  # nothing was selected
    # a gamma-table job has pairs without rows
    with pytest.raises(ValueError, match="needs the records"):
        gamma_table_frame(amd, 100, [2, 3, 4], seed=1).filter(f"{MP} > 0.5").truth_table("cluster")


# ---- 7. sharded ----------------------------------------------------------------------------------------------------
def test_two_shards_sum_to_the_whole_job(amd):
    from splink_amd import _native as N
    from splink_amd.frames import _label_ids
    tables = [labelled_records(2000, seed=7)]
    whole, make_tf = tf_job(amd, "dedupe_only", tables)
    tf = make_tf()
    m, u = whole.job.flat_tables(whole.level_probs)
    lam = float(whole.lam)
    t = np.sort(np.random.Generator(np.random.PCG64(1)).random(72))
    t0 = float(np.nanmedian(whole.match_probability()))

    def raw(df_e):
        job = df_e.job
        lab0, lab1 = _label_ids(job, "cluster")
        df_e.gammas.ensure_codes()
        assert [job.ctx.tf_column_values(c) for c in tf.dev_cols] == [len(x) for x in tf.tables]
        all_pairs = job.ctx.label_scores_tf_columns(lab0, lab1, lam, 1 - lam, m, u, tf.dev_cols, tf.tables, t)
        assert df_e.filter(f"{MP} > {t0!r}")._select() >= 0
        kept = job.ctx.label_scores_selection(lab0, lab1, N.SEL_MP, t)
        return all_pairs, kept, job.n_pairs
    want = raw(whole)
    parts = [raw(tf_job(amd, "dedupe_only", tables, shard=(i, 2))[0]) for i in range(2)]
    assert parts[0][2] > 0 and parts[1][2] > 0 and parts[0][2] + parts[1][2] == want[2]
    assert np.array_equal(parts[0][0] + parts[1][0], want[0]) and want[0].sum() == want[2]
    assert np.array_equal(parts[0][1] + parts[1][1], want[1]) and 0 < want[1].sum() < want[2]


@pytest.fixture
def nccl_group():
    import torch
    import torch.distributed as dist
    torch.cuda.set_device(0)
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1,
                            device_id=torch.device("cuda:0"))
    yield dist
    dist.destroy_process_group()


def test_sharded_path_at_one_rank(amd, nccl_group):
    """force_reduce, as tests/test_gpu_labels.py::test_sharded_path_at_one_rank sets it: the counts and totals go
    through the host all-reduce and the tables come back the same."""
    df_e, make_tf = tf_job(amd, "dedupe_only", [labelled_records(1500, seed=5)])
    tf = make_tf()
    f = df_e.filter("gamma_surname >= 1")
    local = (tf.truth_table("cluster"), f.truth_table("cluster"), f.truth_table("cluster", [0.3, 0.8]))
    df_e.job.force_reduce = True
    reduced = (tf.truth_table("cluster"), f.truth_table("cluster"), f.truth_table("cluster", [0.3, 0.8]))
    df_e.job.force_reduce = False
    for a, b in zip(local, reduced):
        same_table(a, b)
    assert local[0]["tp"].iloc[0] > 0 and local[1]["tp"].iloc[0] > 0
