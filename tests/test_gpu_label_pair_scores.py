"""Scores against a table of labelled pairs, per pair, on the device (spk_label_pairs_scores_*) and the frames above.

No expected value comes from the code under test.  The scores are the parent's: spk_tf_apply over every pair, or
spk_select_copy* of the survivors.  The truth state of a pair and the label it names come from a Python dict of the
labelled pairs under label_pairs_common.canonical's orientation rule; the bins from np.searchsorted(thresholds, score,
side="left"), i.e. the thresholds strictly below the score, a NaN score in bin T + 1.  The pipelines compare the
frames' tables with a merge of their own toPandas() with the labels table.  Every comparison is exact."""
import ctypes
import warnings

import numpy as np
import pandas as pd
import pytest

from label_pairs_common import canonical, capacity_of, distinct_pairs, home_slot, m_u, make_ctx, mixed_labels, random_case
from test_gpu_label_pairs import make_labels, record_keys, records, sparse_pair_set
from test_gpu_label_scores import LAM, LEVELS, M_NULL, U_NULL, expected, nccl_group, same_table, states  # noqa: F401
from test_gpu_tf_select import random_tables

pytestmark = pytest.mark.gpu
warnings.filterwarnings("ignore")

MP = "match_probability"
TF = "tf_adjusted_match_prob"
NONE = (-1, -1.0, -1, -1)  # label_pair_scores_info() before a call and after a failing one
COLUMNS = ["threshold", "tp", "fp", "tn", "fn", "n_unlabelled_above", "precision", "recall", "fpr", "f1",
           "recall_of_all_true_pairs"]


@pytest.fixture(scope="module")
def amd():
    from splink_amd import AmdSession, _native
    if _native.device_count() == 0:
        pytest.fail("no HIP device visible: the -m gpu tests need an MI355X")
    return AmdSession(0)


def step():
    from splink_amd import _native as N
    return N.LABEL_PAIR_SCORE_STEP


def lookup(rows_l, rows_r, lab_l, lab_r, y, one_table):
    """(state [P]: 0 / 1 from the label a pair names, 2 without one; label_pair [n_labels]: the largest index of a
    pair that names the label, -1 = none), by dict lookup."""
    truth = {canonical(a, b, one_table): i for i, (a, b) in enumerate(zip(lab_l, lab_r))}
    assert len(truth) == len(lab_l), "the test's own labels repeat a pair"
    rows_l, rows_r = np.asarray(rows_l, dtype=np.int64), np.asarray(rows_r, dtype=np.int64)
    lo, hi = (np.minimum(rows_l, rows_r), np.maximum(rows_l, rows_r)) if one_table else (rows_l, rows_r)
    distinct, inverse = np.unique(lo * (1 << 32) + hi, return_inverse=True)  # the dict is asked once per distinct pair
    hit = np.array([truth.get((int(k) >> 32, int(k) & 0xFFFFFFFF), -1) for k in distinct], dtype=np.int64)
    label = hit[inverse.reshape(-1)] if len(rows_l) else np.zeros(0, dtype=np.int64)
    y = np.asarray(y, dtype=np.int64)
    state = np.where(label >= 0, y[np.maximum(label, 0)] if len(y) else 0, 2)
    label_pair = np.full(len(lab_l), -1, dtype=np.int64)
    np.maximum.at(label_pair, label[label >= 0], np.flatnonzero(label >= 0))
    return state, label_pair


def scores_of(label_pair, score):
    return np.where(label_pair >= 0, np.asarray(score)[np.maximum(label_pair, 0)] if len(score) else np.nan, np.nan)


class PairCase:
    """A context with loaded pairs and levels, host tf value ids (-1 = NULL, ids past the shorter tables) and tables,
    and the parent values: ctx.score and ctx.tf_apply over every pair (computed once, never changed)."""

    def __init__(self, seed, P, levels=LEVELS, n0=97, n1=None, n_tf=1, m=M_NULL, u=U_NULL, sparse=False,
                 no_self=False):
        rng = np.random.Generator(np.random.PCG64(seed))
        self.rng, self.levels, self.n0, self.n1, self.n_tf = rng, levels, n0, n1, n_tf
        self.one_table = n1 is None
        rows_l, rows_r, g, _, _ = random_case(rng, P, levels, n0, n1)
        if sparse:  # pairs that are no candidates remain, however large P is
            rows_l, rows_r = sparse_pair_set(rng, P, n0)
        if no_self and self.one_table:
            keep = rows_l != rows_r
            rows_l, rows_r, g = rows_l[keep], rows_r[keep], g[keep]
        self.rows_l, self.rows_r, self.g, self.P = rows_l, rows_r, g, len(rows_l)
        self.c = make_ctx(rows_l, rows_r, g, levels, n0, n1)
        if m is None:
            m, u = m_u(levels, rng)
        self.m, self.u = m, u
        sizes = (6, 5, 4)[:n_tf]  # ids run to 5: the shorter tables have ids past their end
        nr = n0 if n1 is None else n1
        self.ids0 = [rng.integers(-1, 6, n0).astype(np.int64) for _ in sizes]
        self.ids1 = [rng.integers(-1, 6, nr).astype(np.int64) for _ in sizes] if n1 is not None else \
            [x.copy() for x in self.ids0]
        self.tables = random_tables(rng, sizes)
        if self.P:
            self.mp = self.c.score(LAM, 1 - LAM, m, u, 0, self.P)
            self.tf, _ = self.c.tf_apply(self.ids0, self.ids1, self.tables, 0, self.P)
        else:
            self.mp = self.tf = np.zeros(0)

    def labels(self, n):
        lab_l, lab_r, y, n_cand = mixed_labels(self.rng, n, self.rows_l, self.rows_r, self.n0, self.n1)
        return lab_l, lab_r, y, n_cand

    def call(self, lab, t):
        return self.c.label_pair_scores_tf(lab[0], lab[1], lab[2], LAM, 1 - LAM, self.m, self.u, self.ids0, self.ids1,
                                           self.tables, t)

    def check(self, lab, t):
        """One call against the dict and the parent's scores."""
        counts, pair, score = self.call(lab, t)
        state, want_pair = lookup(self.rows_l, self.rows_r, lab[0], lab[1], lab[2], self.one_table)
        assert counts.dtype == np.int64 and counts.shape == (3, len(t) + 2)
        assert pair.dtype == np.int64 and score.dtype == np.float64 and len(pair) == len(score) == len(lab[0])
        assert np.array_equal(counts, expected(state, self.tf, t)), len(t)
        assert np.array_equal(pair, want_pair)
        assert score.tobytes() == scores_of(want_pair, self.tf).tobytes()  # bit for bit, NaN included
        info = self.c.label_pair_scores_info()
        assert info[0] == self.P == counts.sum() and info[1] == -1.0 and info[2] == capacity_of(len(lab[0]))
        return counts, pair, score


def thresholds(case, T):
    """T ascending thresholds over the range the scores take: duplicates, and both infinities from T = 2 on."""
    if T == 0:
        return np.zeros(0)
    if T == 1:
        return np.array([np.nanmedian(case.tf) if case.P and not np.isnan(case.tf).all() else 0.5])
    if T == 2:
        return np.array([-np.inf, 0.5])
    if T == 3:
        return np.array([0.3, 0.3, np.inf])
    t = case.rng.random(T)
    t[::9] = t[1::9][:len(t[::9])]
    t[:2], t[-2:] = -np.inf, np.inf
    return np.sort(t)


# ---- 1. counts, label_pair and label_score: tail, vector path, partial wave, several workgroups, the grid loop -----
def _grid_pairs():
    import torch
    from splink_amd import _native as N
    return N.LABEL_PAIR_SCORE_WG_PER_CU * torch.cuda.get_device_properties(0).multi_processor_count * step() + 5


SIZES = [0, 1, 7, 8, 9, 63, 64, 65, "step-1", "step+5", "3steps", "grid"]


@pytest.mark.parametrize("n_labels", [0, 1, 64, 1000])
@pytest.mark.parametrize("P", SIZES)
def test_counts_pairs_and_scores(P, n_labels, amd):
    size = {"step-1": step() - 1, "step+5": step() + 5, "3steps": 3 * step(), "grid": None}.get(P, P)
    if size is None:
        size = _grid_pairs()  # every workgroup of the capped grid takes a second step, and there is a tail
    case = PairCase([SIZES.index(P), n_labels], size, sparse=True)
    assert case.c.label_pair_scores_info() == NONE
    lab = case.labels(n_labels)
    assert len(lab[0]) == n_labels and (n_labels < 2 or size < 64 or 0 < lab[3] < n_labels)  # candidates and others
    for T in (0, 1, 2, 3, 1024):
        counts, pair, _ = case.check(lab, thresholds(case, T))
        assert (pair >= 0).sum() == lab[3]
    if P == "grid":  # one counter that every workgroup flushes into: all pairs above no threshold
        counts, _, _ = case.check(lab, np.array([2.0]))
        assert counts[:, 0].sum() + counts[:, 2].sum() == size and counts[:, 1].sum() == 0
        null_tf, null_mp = np.isnan(case.tf), np.isnan(case.mp)
        assert (null_tf & null_mp).any() and (null_tf & ~null_mp).any() and (~null_tf).any()
    case.c.close()


@pytest.mark.parametrize("n_tf", [1, 3])
@pytest.mark.parametrize("two", [False, True], ids=["one_table", "link_only"])
@pytest.mark.parametrize("levels", [[3] * 7, [4] * 9], ids=["codes16", "codes32"])
def test_code_widths_link_types_and_columns(levels, two, n_tf, amd):
    wide = len(levels) == 9
    case = PairCase([50, int(wide), int(two), n_tf], step() + 8 * 300 + 3, levels, 211, 157 if two else None, n_tf, None, None)
    assert (case.c.n_patterns() > 1 << 16) == wide
    assert any((i == -1).any() for i in case.ids0) and (n_tf == 1 or (case.ids0[1] >= len(case.tables[1])).any())
    lab = case.labels(1000)
    assert 0 < lab[3] < 1000
    case.c.enable_timing(True)
    t = thresholds(case, 72)
    counts, pair, score = case.call(lab, t)
    info = case.c.label_pair_scores_info()
    assert info[0] == case.P and info[1] > 0.0 and info[2] == 2048 and 1 <= info[3] <= 2048
    case.c.enable_timing(False)
    state, want_pair = lookup(case.rows_l, case.rows_r, lab[0], lab[1], lab[2], not two)
    assert np.array_equal(counts, expected(state, case.tf, t)) and np.array_equal(pair, want_pair)
    assert len(np.unique(state)) == 3
    for T in (0, 3, 1024):
        case.check(lab, thresholds(case, T))
    case.c.close()


# ---- 2. orientation --------------------------------------------------------------------------------------------
def test_orientation_one_table(amd):
    case = PairCase(31, 8 * 90 + 3, n0=60, no_self=True)
    assert (case.rows_l > case.rows_r).any() and (case.rows_l < case.rows_r).any()
    seen, lab = set(), []
    for a, b in zip(case.rows_l.tolist(), case.rows_r.tolist()):  # every distinct pair labelled once, given as (r, l)
        if canonical(a, b, True) not in seen:
            seen.add(canonical(a, b, True))
            lab.append((b, a))
    lab_l, lab_r = np.array([p[0] for p in lab]), np.array([p[1] for p in lab])
    y = case.rng.integers(0, 2, len(lab)).astype(np.uint8)
    t = thresholds(case, 3)
    counts, pair, score = case.check((lab_l, lab_r, y), t)
    assert counts[2].sum() == 0 and (pair >= 0).all()
    again = case.call((lab_r, lab_l, y), t)  # the same labels as (l, r): the same result
    assert np.array_equal(again[0], counts) and np.array_equal(again[1], pair)
    assert again[2].tobytes() == score.tobytes()
    case.c.close()


def test_orientation_link_only(amd):
    n0 = n1 = 40
    case = PairCase(32, 10, n0=n0, n1=n1)
    case.c.close()
    # candidates (a, b) with a < b only; (b, a) names valid rows of both tables and is another pair
    case.rows_l, case.rows_r = np.triu_indices(n0, k=1)
    case.P = len(case.rows_l)
    case.g = np.stack([case.rng.integers(-1, L, case.P) for L in LEVELS], axis=1)
    case.c = make_ctx(case.rows_l, case.rows_r, case.g, LEVELS, n0, n1)
    case.mp = case.c.score(LAM, 1 - LAM, case.m, case.u, 0, case.P)
    case.tf, _ = case.c.tf_apply(case.ids0, case.ids1, case.tables, 0, case.P)
    pick = case.rng.permutation(case.P)[:100]
    y = case.rng.integers(0, 2, 100).astype(np.uint8)
    t = thresholds(case, 2)
    counts, pair, _ = case.check((case.rows_l[pick], case.rows_r[pick], y), t)
    assert counts[:2].sum() == 100 and np.array_equal(pair, pick)
    counts, pair, score = case.check((case.rows_r[pick], case.rows_l[pick], y), t)
    assert counts[:2].sum() == 0 and (pair == -1).all() and np.isnan(score).all()
    both_l = np.concatenate([case.rows_l[pick], case.rows_r[pick]])  # both orders: two labels, not one given twice
    both_r = np.concatenate([case.rows_r[pick], case.rows_l[pick]])
    counts, pair, _ = case.check((both_l, both_r, np.concatenate([y, 1 - y])), t)
    assert counts[:2].sum() == 100 and (pair[:100] >= 0).all() and (pair[100:] == -1).all()
    case.c.close()


# ---- 3. the table ----------------------------------------------------------------------------------------------
def test_load_one_half(amd):
    """1024 labels: capacity 2048, the largest load the capacity rule allows."""
    case = PairCase(41, 8 * 500 + 1, n0=300)
    lab = case.labels(1024)
    assert lab[3] == 512
    case.check(lab, thresholds(case, 3))
    _, _, cap, probe = case.c.label_pair_scores_info()
    assert cap == 2048 and 1 <= probe <= 2048
    case.c.close()


def test_constructed_collisions_wrap_around(amd):
    """Keys whose home slot is the last one of a 64-slot table, found with the documented hash: the chain wraps."""
    n0, cap = 97, 64
    last = [(a, b) for a in range(n0) for b in range(a + 1, n0) if home_slot(a, b, cap) == cap - 1][:5]
    assert len(last) >= 4
    case = PairCase(42, 10, n0=n0)
    case.c.close()
    rng = case.rng
    others = distinct_pairs(rng, 20, n0, avoid=last)
    lab = last + others
    assert capacity_of(len(lab)) == cap
    lab = [lab[i] for i in rng.permutation(len(lab))]
    lab_l, lab_r = np.array([p[0] for p in lab]), np.array([p[1] for p in lab])
    y = rng.integers(0, 2, len(lab)).astype(np.uint8)
    # candidates: every colliding key (twice, in both orders), half of the others, and pairs without a label
    extra = distinct_pairs(rng, 300, n0, avoid=lab)
    cand = last + [(b, a) for a, b in last] + others[::2] + extra
    cand = [cand[i] for i in rng.permutation(len(cand))]
    case.rows_l, case.rows_r = np.array([p[0] for p in cand]), np.array([p[1] for p in cand])
    case.P = len(cand)
    case.g = np.stack([rng.integers(-1, L, case.P) for L in LEVELS], axis=1)
    case.c = make_ctx(case.rows_l, case.rows_r, case.g, LEVELS, n0)
    case.mp = case.c.score(LAM, 1 - LAM, case.m, case.u, 0, case.P)
    case.tf, _ = case.c.tf_apply(case.ids0, case.ids1, case.tables, 0, case.P)
    counts, pair, _ = case.check((lab_l, lab_r, y), thresholds(case, 3))
    assert counts[:2].sum() == 2 * len(last) + 10 and (pair >= 0).sum() == len(last) + 10
    assert case.c.label_pair_scores_info()[3] >= 4
    case.c.close()


@pytest.mark.parametrize("labelled", ["all", "none"])
def test_every_pair_labelled_and_none(labelled, amd):
    n0 = 80
    case = PairCase(43, 10, n0=n0)
    case.c.close()
    rng = case.rng
    cand = distinct_pairs(rng, 8 * 150 + 5, n0)
    case.rows_l, case.rows_r = np.array([p[0] for p in cand]), np.array([p[1] for p in cand])
    case.P = len(cand)
    case.g = np.stack([rng.integers(-1, L, case.P) for L in LEVELS], axis=1)
    case.c = make_ctx(case.rows_l, case.rows_r, case.g, LEVELS, n0)
    case.mp = case.c.score(LAM, 1 - LAM, case.m, case.u, 0, case.P)
    case.tf, _ = case.c.tf_apply(case.ids0, case.ids1, case.tables, 0, case.P)
    lab = cand if labelled == "all" else distinct_pairs(rng, 700, n0, avoid=cand)
    lab = [lab[i] for i in rng.permutation(len(lab))]
    lab_l, lab_r = np.array([p[1] for p in lab]), np.array([p[0] for p in lab])
    y = rng.integers(0, 2, len(lab)).astype(np.uint8)
    counts, pair, score = case.check((lab_l, lab_r, y), thresholds(case, 3))
    if labelled == "all":
        assert counts[2].sum() == 0 and (pair >= 0).all() and len(set(pair.tolist())) == case.P
    else:
        assert counts[:2].sum() == 0 and (pair == -1).all() and np.isnan(score).all()
    case.c.close()


# ---- 4. a hand-loaded pair set that repeats a labelled pair ------------------------------------------------------
def test_duplicated_candidate_pair(amd):
    rows_l = np.array([3, 5, 9, 5, 1, 9, 9])
    rows_r = np.array([4, 9, 5, 9, 2, 5, 8])  # (5, 9) four times, in both orders: pairs 1, 2, 3 and 5
    g = np.array([[0, 0], [1, 2], [-1, 0], [0, 1], [1, 1], [1, -1], [0, 0]])
    c = make_ctx(rows_l, rows_r, g, LEVELS, 12)
    m, u = m_u(LEVELS, np.random.Generator(np.random.PCG64(4)))
    ids = [np.array([0, 1, 2, 3, 1, 2, 0, 1, 2, 2, 0, 1], dtype=np.int64)]
    tables = [np.array([0.2, 0.7, 0.9, 0.4])]
    c.score(LAM, 1 - LAM, m, u, 0, 7)
    tf, _ = c.tf_apply(ids, ids, tables, 0, 7)
    assert len(set(tf[[1, 2, 3, 5]].tolist())) == 4  # four codes: four different scores
    lab_l, lab_r, y = np.array([9, 1, 7]), np.array([5, 2, 8]), np.array([1, 0, 1], dtype=np.uint8)
    t = np.sort(tf[[1, 2, 3, 5]])[1:3]
    counts, pair, score = c.label_pair_scores_tf(lab_l, lab_r, y, LAM, 1 - LAM, m, u, ids, ids, tables, t)
    state, want_pair = lookup(rows_l, rows_r, lab_l, lab_r, y, True)
    assert np.array_equal(counts, expected(state, tf, t))
    assert counts[1].sum() == 4 and counts[0].sum() == 1 and counts[2].sum() == 2  # both copies (all four) counted
    assert pair.tolist() == [5, 4, -1] == want_pair.tolist()  # the largest index
    assert score[:2].tobytes() == tf[[5, 4]].tobytes() and np.isnan(score[2])
    c.close()


# ---- 5. agreement with the column route ----------------------------------------------------------------------
@pytest.mark.parametrize("two", [False, True], ids=["one_table", "link_only"])
def test_agrees_with_label_column(two, amd):
    from splink_amd import _native as N
    case = PairCase(51 + two, 8 * 400 + 7, n0=90, n1=70 if two else None, n_tf=3, no_self=True)
    rng, c = case.rng, case.c
    ids0 = rng.integers(0, 40, 90).astype(np.int64)
    ids0[rng.random(90) < 0.15] = -1
    ids1 = None
    if two:
        ids1 = rng.integers(0, 40, 70).astype(np.int64)
        ids1[rng.random(70) < 0.15] = -1
    a, b = ids0[case.rows_l], (ids0 if ids1 is None else ids1)[case.rows_r]
    seen, lab = set(), []
    for l, r, x, z in zip(case.rows_l.tolist(), case.rows_r.tolist(), a.tolist(), b.tolist()):
        if x >= 0 and z >= 0 and canonical(l, r, not two) not in seen:  # a repeated candidate pair: labelled once
            seen.add(canonical(l, r, not two))
            lab.append((l, r, int(x == z)))
    assert len(lab) < case.P
    lab = tuple(np.array([p[k] for p in lab]) for k in range(3))
    lab = (lab[0], lab[1], lab[2].astype(np.uint8))
    t = thresholds(case, 1024)
    by_column = c.label_scores_tf(ids0, ids1, LAM, 1 - LAM, case.m, case.u, case.ids0, case.ids1, case.tables, t)
    counts, _, _ = case.call(lab, t)
    assert np.array_equal(counts, by_column) and (counts.sum(axis=1) > 0).all()
    # and over a selection, by both fields
    k = c.select_tf(LAM, 1 - LAM, case.m, case.u, case.ids0, case.ids1, case.tables,
                    [(N.SEL_GAMMA, 0, N.SEL_OP[">="], 0.0)])
    assert 0 < k < case.P
    for field in (N.SEL_MP, N.SEL_TF_MP):
        by_column = c.label_scores_selection(ids0, ids1, field, t)
        counts, _, _ = c.label_pair_scores_selection(*lab, field, t)
        assert np.array_equal(counts, by_column) and counts[:2].sum() > 0
    c.close()


# ---- 6. the selection variant ------------------------------------------------------------------------------------
def check_selection(case, lab, field_tf, t):
    from splink_amd import _native as N
    c = case.c
    k = c.select_info()[0]
    counts, pair, score = c.label_pair_scores_selection(lab[0], lab[1], lab[2], N.SEL_TF_MP if field_tf else N.SEL_MP, t)
    assert counts.shape == (3, len(t) + 2) and counts.sum() == k and c.label_pair_scores_info()[0] == k
    if k == 0:
        assert (pair == -1).all() and np.isnan(score).all()
        return counts, pair
    _, l, r, _, mp = c.select_copy(0, k, len(case.levels))
    s = c.select_copy_tf(0, k, case.n_tf, adj=False)[0] if field_tf else mp
    state, want_pair = lookup(l, r, lab[0], lab[1], lab[2], case.one_table)
    assert np.array_equal(counts, expected(state, s, t))
    assert np.array_equal(pair, want_pair)  # the survivor's index
    assert score.tobytes() == scores_of(want_pair, s).tobytes()
    return counts, pair


def test_selection_fields_and_best_matches(amd):
    from splink_amd import _native as N
    case = PairCase(21, 8 * 900 + 3, n_tf=3, no_self=True)
    c = case.c
    lab = case.labels(1000)
    t_all = [np.zeros(0), thresholds(case, 1), thresholds(case, 3), thresholds(case, 1024)]
    # a plain selection: match_probability
    k = c.select(LAM, 1 - LAM, case.m, case.u, [(N.SEL_GAMMA, 1, N.SEL_OP[">="], 0.0)])
    assert 0 < k < case.P
    for t in t_all:
        counts, pair = check_selection(case, lab, False, t)
    assert counts[:, -1].sum() > 0 and 0 < (pair >= 0).sum() < lab[3]  # NULL scores; labels the selection dropped
    with pytest.raises(RuntimeError, match="without tf tables"):  # a selection of the wrong kind
        c.label_pair_scores_selection(*lab[:3], N.SEL_TF_MP, [])
    assert c.label_pair_scores_info() == NONE and c.select_info()[0] == k  # the selection survives a refusal
    # a tf selection: both fields
    term = (N.SEL_TF_MP, 0, N.SEL_OP[">"], float(np.nanquantile(case.tf, 0.3)))
    k = c.select_tf(LAM, 1 - LAM, case.m, case.u, case.ids0, case.ids1, case.tables,
                    [term, (N.SEL_GAMMA, 0, N.SEL_OP[">="], -1.0)])
    assert 0 < k < case.P
    for field_tf in (False, True):
        for t in t_all:
            check_selection(case, lab, field_tf, t)
    # narrowed to a one-to-one link
    kept = c.select_best(N.SEL_TF_MP, N.BEST_MUTUAL, 0)
    assert 0 < kept < k
    for field_tf in (False, True):
        for t in t_all:
            check_selection(case, lab, field_tf, t)
    # an empty selection counts nothing
    assert c.select(LAM, 1 - LAM, case.m, case.u, [(N.SEL_MP, 0, N.SEL_OP[">"], 2.0)]) == 0
    counts, _ = check_selection(case, lab, False, t_all[1])
    assert counts.shape == (3, 3) and counts.sum() == 0
    c.close()


def test_selection_states(amd):
    from splink_amd import _native as N
    case = PairCase(22, 8 * 100 + 1, no_self=True)
    c = case.c
    lab = case.labels(64)[:3]
    with pytest.raises(RuntimeError, match="no selection"):
        c.label_pair_scores_selection(*lab, N.SEL_MP, [])
    k = c.select(0.0, 0.0, None, None, [(N.SEL_GAMMA, 0, N.SEL_OP[">="], 0.0)])  # made without m / u
    assert k > 0
    with pytest.raises(RuntimeError, match="no m / u"):
        c.label_pair_scores_selection(*lab, N.SEL_MP, [])
    for field in (N.SEL_GAMMA, N.SEL_ALL):
        with pytest.raises(ValueError, match="unknown field"):
            c.label_pair_scores_selection(*lab, field, [])
    c.select(LAM, 1 - LAM, case.m, case.u, [])
    assert c.label_pair_scores_selection(*lab, N.SEL_MP, [])[0].sum() == case.P
    c.gammas_load(case.levels, case.g.astype(np.int8))  # a stale selection: new codes
    with pytest.raises(RuntimeError, match="changed since spk_select"):
        c.label_pair_scores_selection(*lab, N.SEL_MP, [])
    assert c.label_pair_scores_info() == NONE
    c.close()


# ---- 7. argument errors, state errors and limits -----------------------------------------------------------------
def test_argument_and_state_errors(amd):
    from splink_amd import _native as N
    case = PairCase(31, 8 * 50 + 3, n0=40, no_self=True)
    c = case.c
    good = case.labels(64)[:3]
    args = (LAM, 1 - LAM, case.m, case.u, case.ids0, case.ids1, case.tables)
    c.select(LAM, 1 - LAM, case.m, case.u, [])

    def both(lab, t, error, text):
        with pytest.raises(error, match=text):
            c.label_pair_scores_tf(*lab, *args, t)
        assert c.label_pair_scores_info() == NONE
        with pytest.raises(error, match=text):
            c.label_pair_scores_selection(*lab, N.SEL_MP, t)
        assert c.label_pair_scores_info() == NONE
        case.check(good, np.array([0.5]))  # a good call after the failing one
        check_selection(case, good, False, np.array([0.5]))

    for bad, what in (([0.1, np.nan], "NaN"), ([0.5, 0.4], "descend"), (np.linspace(0, 1, 1025), "1024")):
        both(good, bad, ValueError, what)
    i32, u8 = (lambda *x: np.array(x, dtype=np.int32)), (lambda *x: np.array(x, dtype=np.uint8))
    for text, lab in (("outside its table", (i32(1, 40), i32(2, 3), u8(0, 1))),
                      ("outside its table", (i32(1, 2), i32(2, -1), u8(0, 1))),
                      ("with itself", (i32(1, 4), i32(2, 4), u8(0, 1))),
                      ("given twice", (i32(1, 4, 1), i32(2, 5, 2), u8(0, 1, 0))),
                      ("given twice", (i32(1, 4, 2), i32(2, 5, 1), u8(0, 1, 1))),  # the other order, the other label
                      ("other than 0 or 1", (i32(1, 4), i32(2, 5), u8(0, 2)))):
        both(lab, [0.5], ValueError, text)
    assert case.call(good, np.linspace(0, 1, 1024))[0].sum() == case.P
    # straight at the ABI: NULL arrays with labels, NULL out_counts, more than 2^27 labels (before a label is read)
    t = np.array([0.5])
    out = np.zeros(3 * 3, dtype=np.uint64)

    def raw(n, lab_l, lab_r, y, counts):
        N.check(c._lib.spk_label_pairs_scores_selection(c._h, ctypes.c_int64(n), N._ptr(lab_l), N._ptr(lab_r), N._ptr(y),
                                                        ctypes.c_int(N.SEL_MP), ctypes.c_int(1), N._ptr(t),
                                                        N._ptr(counts), N._ptr(None), N._ptr(None)),
                "spk_label_pairs_scores_selection")
    ok = (i32(1, 4), i32(2, 5), u8(0, 1))
    with pytest.raises(ValueError, match="null rows_l"):
        raw(2, None, ok[1], ok[2], out)
    with pytest.raises(ValueError, match="null rows_l"):
        raw(2, ok[0], ok[1], None, out)
    with pytest.raises(ValueError, match="null out_counts"):
        raw(2, *ok, None)
    with pytest.raises(ValueError, match="2\\^27"):
        raw((1 << 27) + 1, *ok, out)
    assert c.label_pair_scores_info() == NONE
    raw(2, *ok, out)  # the per-label outputs are optional
    assert out.sum() == case.P
    with pytest.raises(ValueError, match="1..8 columns"):
        c.label_pair_scores_tf(*good, LAM, 1 - LAM, case.m, case.u, [], [], [], [])
    with pytest.raises(ValueError, match="1..8 columns"):
        c.label_pair_scores_tf_columns(*good, LAM, 1 - LAM, case.m, case.u, [], [], [])
    with pytest.raises(RuntimeError, match="dictionary ids"):  # columns made without device ids
        c.label_pair_scores_tf_columns(*good, LAM, 1 - LAM, case.m, case.u, [0], case.tables[:1], [])
    c.close()
    gt = N.Context(0)  # a loaded gamma table: codes without pair rows
    gt.table_create(0, 40, 1)
    gt.gammas_load(LEVELS, case.g.astype(np.int8))
    with pytest.raises(RuntimeError, match="no pair rows"):
        gt.label_pair_scores_tf(*good, *args, [0.5])
    gt.select(LAM, 1 - LAM, case.m, case.u, [])
    with pytest.raises(RuntimeError, match="no pair rows"):
        gt.label_pair_scores_selection(*good, N.SEL_MP, [0.5])
    assert gt.label_pair_scores_info() == NONE
    gt.close()
    nc = N.Context(0)
    nc.table_create(0, 40, 1)
    with pytest.raises(RuntimeError, match="no gammas"):
        nc.label_pair_scores_tf(*good, *args, [0.5])
    nc.close()


# ---- 8. bystanders -------------------------------------------------------------------------------------------------
def test_bystanders_untouched(amd):
    """The selection and its survivors, the scores a later tf_apply reads, the tf sums, the EM histogram, the
    components and spk_ctx_memory are the same before and after (a device-resident tf result: the frames' test)."""
    import torch
    from splink_amd import _native as N
    case = PairCase(41, 8 * 200 + 3, n0=120, no_self=True)
    c, P = case.c, case.P
    m, u = m_u(LEVELS, case.rng)
    cut = float(np.nanmedian(c.score(LAM, 1 - LAM, m, u, 0, P)))
    c.score(LAM, 1 - LAM, m, u, 0, P, want_host=False)
    k = c.select_tf(LAM, 1 - LAM, m, u, case.ids0, case.ids1, case.tables, [(N.SEL_MP, 0, N.SEL_OP[">"], cut)])
    assert 0 < k < P
    nodes, _, _ = c.components()

    def snapshot():
        hist = torch.zeros(c.n_patterns(), dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()
        c.em_histogram(hist.data_ptr())
        return (c.select_copy(0, k, 2), c.select_copy_tf(0, k, 1), c.components_copy(0, nodes), hist.cpu().numpy(), c.tf_accumulate(6, case.ids0[0], case.ids1[0]),
                c.tf_apply(case.ids0, case.ids1, case.tables, 0, P), c.select_info()[0], c.components_info()[:2])

    before = snapshot()
    mem = c.memory()
    lab = case.labels(300)[:3]
    # other parameters (case.m / case.u) than the selection's and the scores'
    counts, _, _ = case.check(lab, np.array([0.2, 0.7]))
    sel, pair, _ = c.label_pair_scores_selection(*lab, N.SEL_TF_MP, [0.2, 0.7])
    assert sel.sum() == k and (pair >= 0).any()
    assert c.memory() == mem  # the calls' buffers are gone
    with pytest.raises(ValueError):  # and after a failing call too
        c.label_pair_scores_selection(lab[0][:1], lab[0][:1], lab[2][:1], N.SEL_TF_MP, [])
    assert c.memory() == mem
    after = snapshot()
    for x, z in zip(before[:6], after[:6]):
        for a, b in zip(x, z) if isinstance(x, tuple) else ((x, z),):
            assert (a is None and b is None) or np.array_equal(a, b, equal_nan=True)
    assert before[6:] == after[6:]
    c.close()


# ---- 9. pipelines --------------------------------------------------------------------------------------------------
def tf_frames(amd, link_type, tables):
    """cfg2 with a term-frequency adjustment on surname, through the public calls: (df_e, tf)."""
    from splink_amd import Params, add_gammas, block_using_rules, run_expectation_step
    from splink_amd.synthetic import cfg_settings
    from splink_amd.term_frequencies import make_adjustment_for_term_frequencies
    s = cfg_settings(2)
    s["link_type"] = link_type
    s["additional_columns_to_retain"] = ["cluster"]
    next(c for c in s["comparison_columns"] if c["col_name"] == "surname")["term_frequency_adjustments"] = True
    params = Params(s, amd)
    st = params.settings
    kw = {"df": tables[0]} if link_type == "dedupe_only" else {"df_l": tables[0], "df_r": tables[1]}
    df_e = run_expectation_step(add_gammas(block_using_rules(st, amd, **kw), st, amd), params, st, amd)
    return df_e, make_adjustment_for_term_frequencies(df_e, params, st, amd)


def merged(link_type, labels, pdf):
    """The merge the device replaces: for every label the row of `pdf` it names (-1: none)."""
    at = {key: i for i, key in enumerate(record_keys(pdf, link_type))}
    assert len(at) == len(pdf)
    return np.array([at.get(key, -1) for key in record_keys(labels, link_type)], dtype=np.int64)


def merged_table(kept, score, row_kept, by_blocking, y, ts):
    """LabelCounts.truth_table's columns from the merge: `kept` the frame's own toPandas(), row_kept the row of it a
    label names, by_blocking which labels name a candidate pair of the job; ts = None: the one row of the frame as it
    stands."""
    state = np.full(len(kept), 2)
    state[row_kept[row_kept >= 0]] = y[row_kept >= 0]
    s = kept[score].to_numpy()
    totals = (int((by_blocking & y).sum()), int((by_blocking & ~y).sum()))
    rows = []
    for t in ([-np.inf] if ts is None else ts):
        above = np.ones(len(kept), dtype=bool) if ts is None else s > t
        tp, fp, unl = int((above & (state == 1)).sum()), int((above & (state == 0)).sum()), int((above & (state == 2)).sum())
        fn, tn = totals[0] - tp, totals[1] - fp
        div = lambda a, b: a / b if b else np.nan  # noqa: E731
        rows.append((t, tp, fp, tn, fn, unl, div(tp, tp + fp), div(tp, tp + fn), div(fp, fp + tn),
                     div(2 * tp, 2 * tp + fp + fn), div(tp, int(y.sum()))))
    return pd.DataFrame(rows, columns=COLUMNS)


def check_frame(frame, link_type, labels, y, by_blocking, score, selection, ts, cut):
    """One frame against the merge of its own toPandas() with the labels: the tables, labelled_pairs() and
    prediction_errors(cut)."""
    kept = frame.toPandas()
    row = merged(link_type, labels, kept)
    found = row >= 0
    lab_score = np.where(found, kept[score].to_numpy()[np.maximum(row, 0)], np.nan)
    by_blocking = by_blocking if selection else found
    if selection:
        same_table(frame.truth_table_from_pairs(labels), merged_table(kept, score, row, by_blocking, y, None))
    same_table(frame.truth_table_from_pairs(labels, ts[::-1]), merged_table(kept, score, row, by_blocking, y, np.sort(ts)))
    pc = frame.label_counts_from_pairs(labels, thresholds=ts)
    assert pc.true_pairs_total == y.sum() and pc.counts.sum() == len(kept) and np.array_equal(pc.label_pair, row)
    lp = pc.labelled_pairs()
    assert list(lp.columns) == list(labels.columns) + ["found_by_blocking"] + (["kept"] if selection else []) + [score]
    assert lp[list(labels.columns)].equals(labels)
    assert np.array_equal(lp["found_by_blocking"].to_numpy(), by_blocking)
    assert not selection or np.array_equal(lp["kept"].to_numpy(), found)
    assert lp[score].to_numpy().tobytes() == lab_score.tobytes()
    err = pc.prediction_errors(cut)
    above = lab_score > cut
    fp, fn = above & ~y, ~above & y
    assert np.array_equal(err.index.to_numpy(), np.flatnonzero(fp | fn))
    assert err["error"].tolist() == np.where(fp[fp | fn], "fp", "fn").tolist()
    assert err.drop(columns="error").equals(lp[fp | fn])
    return kept, found, lab_score


def check_pipeline(amd, link_type, tables):
    df_e, tf = tf_frames(amd, link_type, tables)

    def boom():
        raise AssertionError("the per-pair part of the tf frame ran")
    pdf = tf.toPandas()  # the CPU-side frame: made once, never changed
    rng = np.random.Generator(np.random.PCG64(len(pdf)))
    labels = make_labels(rng, link_type, tables, pdf, n_cand=min(1500, len(pdf) // 2), n_other=300)
    y = (labels["clerical_match_score"] >= 0.5).to_numpy()
    row = merged(link_type, labels, pdf)
    by_blocking = row >= 0
    cut = float(np.nanmedian(pdf[TF].to_numpy()[row[by_blocking]]))
    lab_tf = np.where(by_blocking, pdf[TF].to_numpy()[np.maximum(row, 0)], np.nan)
    kept_by_filter = lab_tf > cut
    # nothing passes vacuously: matches and non-matches that are kept, that were blocked but filtered out, that were
    # never blocked; pairs on both sides of the threshold
    for truth in (y, ~y):
        assert (truth & kept_by_filter).sum() > 5 and (truth & by_blocking & ~kept_by_filter).sum() > 5
        assert (truth & ~by_blocking).sum() > 5
    ts = np.array([cut, 0.05, 0.5, 0.99, -1.0, 2.0])
    # ---- the tf frame: every pair, the per-pair part never runs
    fresh = tf_frames(amd, link_type, tables)[1]
    fresh._apply = boom
    ref = df_e.truth_table_from_pairs(labels)
    got = fresh.truth_table_from_pairs(labels)
    assert np.array_equal(got["threshold"].to_numpy(), ref["threshold"].to_numpy()) and len(got) > 10
    assert list(got.columns) == list(ref.columns) and list(got.dtypes) == list(ref.dtypes)
    same_table(got, merged_table(pdf, TF, row, by_blocking, y, ref["threshold"].to_numpy()))
    assert fresh._pair is None
    check_frame(tf, link_type, labels, y, by_blocking, TF, False, ts, cut)
    # ---- a filter on the tf score, and by the other score
    f = tf.filter(f"{TF} > {cut!r}")
    kept, found, _ = check_frame(f, link_type, labels, y, by_blocking, TF, True, ts, cut)
    assert 0 < len(kept) < len(pdf) and np.array_equal(found, kept_by_filter)
    same_table(f.truth_table_from_pairs(labels, ts, by=MP),
               merged_table(kept, MP, merged(link_type, labels, kept), by_blocking, y, np.sort(ts)))
    # ---- a filter on the pattern score
    check_frame(df_e.filter(f"gamma_surname >= 1 and {MP} > 0.05"), link_type, labels, y, by_blocking, MP, True, ts, 0.5)
    # ---- one-to-one links
    for frame, score in ((tf.best_matches(per="mutual"), TF), (df_e.best_matches(per="mutual"), MP)):
        kept, found, _ = check_frame(frame, link_type, labels, y, by_blocking, score, True, ts, cut)
        assert 0 < found.sum() < by_blocking.sum() and (found & y).any()
    return df_e, tf, labels


def test_pipeline_dedupe_only(amd):
    check_pipeline(amd, "dedupe_only", [records(1500, seed=3)])


def test_pipeline_link_only(amd):
    df = records(1500, seed=4)
    check_pipeline(amd, "link_only", [df.iloc[::2].reset_index(drop=True), df.iloc[1::2].reset_index(drop=True)])


def test_pipeline_link_and_dedupe_colliding_ids(amd):
    df = records(1500, seed=5)
    left, right = df.iloc[::2].reset_index(drop=True), df.iloc[1::2].reset_index(drop=True)
    left["unique_id"] = np.arange(len(left))
    right["unique_id"] = np.arange(len(right))  # every id occurs in both inputs
    df_e, tf, labels = check_pipeline(amd, "link_and_dedupe", [left, right])
    with pytest.raises(ValueError, match="_source_table_l"):
        tf.truth_table_from_pairs(labels.drop(columns=["_source_table_l", "_source_table_r"]))


def test_refusals_before_the_device(amd):
    from test_gpu_select import gamma_table_frame
    df_e, tf = tf_frames(amd, "dedupe_only", [records(600, seed=9)])
    pdf = df_e.toPandas()
    labels = pdf[["unique_id_l", "unique_id_r"]].head(20).assign(clerical_match_score=1.0)
    df_e.job.selection_owner = None
    f = tf.filter(f"{TF} > 0.5")
    for frame in (tf, f, df_e.filter(f"{MP} > 0.5"), tf.best_matches(per="mutual")):
        with pytest.raises(ValueError, match="clerical_match_score"):
            frame.truth_table_from_pairs(labels.drop(columns="clerical_match_score"))
        with pytest.raises(ValueError, match="not in the input table"):
            frame.label_counts_from_pairs(labels.assign(unique_id_l=-5))
    assert df_e.job.selection_owner is None  # nothing was selected
    with pytest.raises(ValueError, match="no score"):
        df_e.filter(f"{MP} > 0.5").truth_table_from_pairs(labels, by=TF)
    with pytest.raises(ValueError, match="no score"):
        df_e.gammas.filter("gamma_surname >= 1").truth_table_from_pairs(labels)
    with pytest.raises(ValueError, match="sample frame"):
        df_e.sample_pairs(per_stratum=5).truth_table_from_pairs(labels)
    with pytest.raises(ValueError, match="more than"):
        tf.truth_table_from_pairs(labels, np.linspace(0, 1, 1025))
    with pytest.raises(ValueError, match="needs the records"):  # a gamma-table job has pairs without rows
        gamma_table_frame(amd, 100, [2, 3, 4], seed=1).filter(f"{MP} > 0.5").truth_table_from_pairs(labels)
    assert tf.label_counts_from_pairs(labels).counts[1].sum() == 20


def test_frames_leave_scores_tf_and_em_alone(amd):
    """test_gpu_label_scores.py's test of that name for the new frame calls: a device-resident tf result
    (spk_tf_copy), the tf sums and the EM statistics are the same before and after."""
    df_e, tf = tf_frames(amd, "dedupe_only", [records(600, seed=11)])
    job = df_e.job
    pdf = tf.toPandas()
    labels = pdf[["unique_id_l", "unique_id_r"]].head(50).assign(clerical_match_score=[1.0, 0.0] * 25)
    df_e.gammas.ensure_codes()
    stats0 = job.em_stats(df_e.lam, df_e.level_probs)
    job.score(df_e.lam, df_e.level_probs, want_host=False)
    job.ctx.tf_apply_columns(tf.dev_cols, tf.tables, 0, job.n_pairs, want_adj=False, want_host=False)
    before = job.ctx.tf_copy(10, 200)
    assert before.tobytes() == pdf[TF].to_numpy()[10:210].tobytes()
    col = tf.dev_cols[0]
    nv = job.ctx.tf_column_values(col)

    def tf_state():
        scale = job.ctx.tf_scales_column(col, nv)
        limbs, counts = job.ctx.tf_accumulate_column_exact(col, nv, scale)
        return scale.copy(), limbs.copy(), counts.copy()
    state0 = tf_state()
    assert len(tf.truth_table_from_pairs(labels, [0.5])) == 1
    assert len(tf.filter(f"{TF} > 0.5").truth_table_from_pairs(labels)) == 1
    assert job.ctx.tf_copy(10, 200).tobytes() == before.tobytes()
    for a, b in zip(state0, tf_state()):
        assert np.array_equal(a, b)
    assert np.array_equal(stats0, job.em_stats(df_e.lam, df_e.level_probs), equal_nan=True)


# ---- 10. the sharded path at one rank ----------------------------------------------------------------------------
def test_sharded_path_at_one_rank(amd, nccl_group):  # noqa: F811
    """force_reduce: the counts and totals (summed), found / kept and the scores (their maximum, NULL as -inf) go
    through the host all-reduce and come back as the local result; label_pair is not exposed."""
    tables = [records(1500, seed=5)]
    df_e, tf = tf_frames(amd, "dedupe_only", tables)
    pdf = df_e.toPandas()
    labels = make_labels(np.random.Generator(np.random.PCG64(9)), "dedupe_only", tables, pdf, n_cand=600, n_other=60)
    f = tf.filter("gamma_surname >= 1")

    def run():
        return (tf.label_counts_from_pairs(labels), f.label_counts_from_pairs(labels),
                f.label_counts_from_pairs(labels, thresholds=[0.3, 0.8], by=MP))
    local = run()
    df_e.job.force_reduce = True
    reduced = run()
    df_e.job.force_reduce = False
    for a, b in zip(local, reduced):
        assert np.array_equal(a.counts, b.counts) and a.totals == b.totals
        same_table(a.truth_table(), b.truth_table())
        same_table(a.kept_row(), b.kept_row())
        assert a.labelled_pairs().equals(b.labelled_pairs())
        assert a.prediction_errors(0.5).equals(b.prediction_errors(0.5))
        assert a.label_pair is not None and b.label_pair is None and np.array_equal(a.found, b.found)
    assert local[0].counts[1].sum() > 0 and 0 < local[1].found.sum() < 600 and np.isnan(local[1].label_score).any()
