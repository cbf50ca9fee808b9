"""Host side of scoring a linkage against labels (splink_amd/labels.py), without a device.

The oracle is brute force: the (state, pattern) counts expanded to one row per pair, counted with `>` per threshold
and accumulated pair by pair into the M-step's statistics.  Integer columns compare exactly, ratios with == on the
same integer quotients."""
import os
import re

import numpy as np
import pandas as pd
import pytest

from conftest import ROOT

from splink_amd import _native as N
from splink_amd.engine import N_HEAD, m_step_rows
from splink_amd.labels import MATCH, NON_MATCH, UNKNOWN, LabelCounts, estimate_from_labels, true_pairs_total

NAMES, LEVELS = ["gamma_a", "gamma_b"], [2, 3]
N_PAT = 12


def hand_counts():
    """Levels [2, 3]: 12 patterns; 4 and 5 share one score, 3 has a NULL score, 2 and 9 are empty, 7 holds
    unlabelled pairs only, 11 no matches."""
    counts = np.zeros((3, N_PAT), dtype=np.int64)
    counts[NON_MATCH] = [40, 9, 0, 3, 7, 2, 5, 0, 1, 0, 2, 1]
    counts[MATCH] = [1, 0, 0, 2, 3, 4, 6, 0, 9, 0, 11, 0]
    counts[UNKNOWN] = [5, 1, 0, 1, 0, 2, 0, 4, 1, 0, 0, 3]
    mp = np.array([0.0, 0.01, 0.02, np.nan, 0.3, 0.3, 0.55, 0.6, 0.8, 0.85, 0.97, 1.0])
    return counts, mp


def expand(counts, mp=None):
    """One row per pair: (state, code, score)."""
    state = np.concatenate([np.full(int(counts[s, c]), s) for s in range(3) for c in range(counts.shape[1])])
    code = np.concatenate([np.full(int(counts[s, c]), c) for s in range(3) for c in range(counts.shape[1])])
    return state.astype(np.int64), code.astype(np.int64), (None if mp is None else mp[code])


def div(a, b):
    return np.nan if b == 0 else a / b


def brute_row(state, score, t, total):
    with np.errstate(invalid="ignore"):
        pred = score > t  # NaN > t is False: a NULL score is never predicted a match
    tp, fp = int((pred & (state == MATCH)).sum()), int((pred & (state == NON_MATCH)).sum())
    fn, tn = int((~pred & (state == MATCH)).sum()), int((~pred & (state == NON_MATCH)).sum())
    return {"threshold": t, "tp": tp, "fp": fp, "tn": tn, "fn": fn,
            "n_unlabelled_above": int((pred & (state == UNKNOWN)).sum()),
            "precision": div(tp, tp + fp), "recall": div(tp, tp + fn), "fpr": div(fp, fp + tn),
            "f1": div(2 * tp, 2 * tp + fp + fn), "recall_of_all_true_pairs": div(tp, total)}


COLUMNS = ["threshold", "tp", "fp", "tn", "fn", "n_unlabelled_above", "precision", "recall", "fpr", "f1",
           "recall_of_all_true_pairs"]


def check_table(got, state, score, thresholds, total):
    assert list(got.columns) == COLUMNS
    assert len(got) == len(thresholds)
    for c in ("tp", "fp", "tn", "fn", "n_unlabelled_above"):
        assert got[c].dtype == np.int64
    for i, t in enumerate(thresholds):
        exp = brute_row(state, score, t, total)
        row = got.iloc[i]
        for c in COLUMNS:
            g, e = row[c], exp[c]
            assert (g == e) or (isinstance(e, float) and np.isnan(e) and np.isnan(g)), (t, c, g, e)


@pytest.mark.parametrize("thresholds", [[0.5], [-1.0, 0.0, 0.3, 0.29999999999999993, 0.97, 1.0, 2.0],
                                        [0.9, 0.1, 0.55, 0.1]])
def test_truth_table_explicit_thresholds(thresholds):
    counts, mp = hand_counts()
    state, _, score = expand(counts, mp)
    lc = LabelCounts(NAMES, LEVELS, counts, mp, "dedupe_only", 60)
    check_table(lc.truth_table(thresholds), state, score, sorted(thresholds), 60)


def test_truth_table_every_distinct_score():
    counts, mp = hand_counts()
    state, _, score = expand(counts, mp)
    lc = LabelCounts(NAMES, LEVELS, counts, mp, "dedupe_only", 60)
    got = lc.truth_table()
    # the scores of the patterns that occur (2 and 9 do not; 3 is NULL; 4 and 5 share one), below them all first
    distinct = [0.0, 0.01, 0.3, 0.55, 0.6, 0.8, 0.97, 1.0]
    t = got["threshold"].tolist()
    assert t[1:] == distinct and t[0] < distinct[0]
    check_table(got, state, score, t, 60)
    first, last = got.iloc[0], got.iloc[-1]
    # below every score: every pair with a score is predicted a match (pattern 3's NULL score never is)
    assert first["tp"] == counts[MATCH].sum() - 2 and first["fn"] == 2 and first["fp"] == counts[NON_MATCH].sum() - 3
    assert last["tp"] == last["fp"] == last["n_unlabelled_above"] == 0 and np.isnan(last["precision"])
    assert lc.missed_by_blocking == 60 - counts[MATCH].sum()


def test_truth_table_degenerate():
    counts = np.zeros((3, N_PAT), dtype=np.int64)
    mp = np.linspace(0.0, 1.0, N_PAT)
    lc = LabelCounts(NAMES, LEVELS, counts, mp, "dedupe_only", 0)
    assert len(lc.truth_table()) == 0 and len(lc.patterns()) == 0
    row = lc.truth_table([0.5]).iloc[0]
    assert row["tp"] == row["fp"] == row["tn"] == row["fn"] == 0
    assert all(np.isnan(row[c]) for c in ("precision", "recall", "fpr", "f1", "recall_of_all_true_pairs"))
    with pytest.raises(ValueError):
        LabelCounts(NAMES, LEVELS, counts, None).truth_table()  # unscored counts
    with pytest.raises(ValueError):
        lc.truth_table([0.1, np.nan])
    with pytest.raises(ValueError):
        LabelCounts(NAMES, LEVELS, np.zeros((3, 11), dtype=np.int64))


def test_patterns_frame():
    counts, mp = hand_counts()
    lc = LabelCounts(NAMES, LEVELS, counts, mp, "dedupe_only", 60)
    got = lc.patterns()
    codes = [c for c in range(N_PAT) if counts[:, c].sum() > 0]
    assert list(got.columns) == NAMES + ["match_probability", "n_match", "n_non_match", "n_unlabelled"]
    assert got["gamma_a"].tolist() == [c % 3 - 1 for c in codes]          # stride 1, L + 1 = 3
    assert got["gamma_b"].tolist() == [(c // 3) % 4 - 1 for c in codes]   # stride 3, L + 1 = 4
    assert np.array_equal(got["match_probability"].to_numpy(), mp[codes], equal_nan=True)
    assert got["n_match"].tolist() == counts[MATCH, codes].tolist()
    assert got["n_non_match"].tolist() == counts[NON_MATCH, codes].tolist()
    assert got["n_unlabelled"].tolist() == counts[UNKNOWN, codes].tolist()
    assert "match_probability" not in LabelCounts(NAMES, LEVELS, counts).patterns().columns


def stats_pair_by_pair(state, code, levels):
    """The M-step statistics accumulated one labelled pair at a time, match_probability := the label."""
    stats = np.zeros(N_HEAD + 4 * sum(L + 1 for L in levels))
    for s, c in zip(state.tolist(), code.tolist()):
        if s == UNKNOWN:
            continue
        y = 1.0 if s == MATCH else 0.0
        stats[0] += y
        stats[1] += 1
        stats[2] += 1
        off, stride = N_HEAD, 1
        for L in levels:
            g = (c // stride) % (L + 1) - 1
            slot = off + 4 * (g + 1)
            stats[slot] += 1
            stats[slot + 1] += 1
            stats[slot + 2] += y
            stats[slot + 3] += 1.0 - y
            off += 4 * (L + 1)
            stride *= L + 1
    return stats


def test_m_step_matches_pair_by_pair_statistics():
    counts, _ = hand_counts()  # holds -1 levels (codes 0, 1, 3, 6: gamma_a or gamma_b = -1)
    state, code, _ = expand(counts)
    lc = LabelCounts(NAMES, LEVELS, counts)
    exp_stats = stats_pair_by_pair(state, code, LEVELS)
    assert np.array_equal(lc.m_step_stats(), exp_stats)
    lam, rows = lc.m_step()
    exp_lam, exp_rows = m_step_rows(exp_stats, NAMES, LEVELS)
    assert lam == exp_lam and rows == exp_rows
    assert lam == float(np.float32(counts[MATCH].sum() / counts[:UNKNOWN].sum()))
    assert any(r["gamma_value"] == -1 for r in rows)


def test_m_step_column_never_observed_among_matches():
    """gamma_b's non-null levels occur among non-matches only (every match has gamma_b = -1): the M-step's
    denominator over the observed levels is 0 for m, so m is NULL there and u is estimated as usual."""
    counts = np.zeros((3, N_PAT), dtype=np.int64)
    counts[MATCH, [0, 1, 2]] = [3, 4, 5]         # gamma_b = -1
    counts[NON_MATCH, [3, 4, 8, 10]] = [6, 2, 7, 1]  # gamma_b = 0, 0, 1, 2
    counts[UNKNOWN, 5] = 50                      # left out
    state, code, _ = expand(counts)
    lc = LabelCounts(NAMES, LEVELS, counts)
    lam, rows = lc.m_step()
    assert (lam, rows) == m_step_rows(stats_pair_by_pair(state, code, LEVELS), NAMES, LEVELS)
    b = {r["gamma_value"]: r for r in rows if r["gamma_col"] == "gamma_b"}
    assert all(b[v]["new_probability_match"] is None for v in (0, 1, 2))
    assert [b[v]["new_probability_non_match"] for v in (0, 1, 2)] == [float(np.float32(x / 16)) for x in (8, 7, 1)]


def label_ids(rng, n, n_groups, nulls):
    ids = rng.integers(0, n_groups, n).astype(np.int64)
    ids[rng.random(n) < nulls] = -1
    return ids


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_true_pairs_total_against_quadratic_loop(seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    a, b = label_ids(rng, 40, 9, 0.2), label_ids(rng, 33, 9, 0.2)
    dedupe = sum(1 for i in range(len(a)) for j in range(i + 1, len(a)) if a[i] >= 0 and a[i] == a[j])
    link = sum(1 for x in a for y in b if x >= 0 and x == y)
    ab = np.concatenate([a, b])  # link_and_dedupe: one table, the vertical concatenation
    both = sum(1 for i in range(len(ab)) for j in range(i + 1, len(ab)) if ab[i] >= 0 and ab[i] == ab[j])
    assert true_pairs_total("dedupe_only", a) == dedupe
    assert true_pairs_total("link_only", a, b) == link
    assert true_pairs_total("link_and_dedupe", ab) == both
    assert both == dedupe + link + sum(1 for i in range(len(b)) for j in range(i + 1, len(b))
                                       if b[i] >= 0 and b[i] == b[j])
    assert true_pairs_total("dedupe_only", np.full(5, -1)) == 0
    with pytest.raises(ValueError):
        true_pairs_total("link_only", a)
    counts = np.zeros((3, N_PAT), dtype=np.int64)
    counts[MATCH, 4] = dedupe - 3
    assert LabelCounts(NAMES, LEVELS, counts, None, "dedupe_only", dedupe).missed_by_blocking == 3


# ---- ABI and frames ----------------------------------------------------------------------------------------
def test_abi_declares_the_label_calls():
    text = open(os.path.join(ROOT, "include", "splink_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("spk_label_histogram", "spk_label_info"):
        assert re.search(r"\bint\s+" + name + r"\s*\(\s*spk_ctx\s*\*\s*ctx\b", text), name
        assert name in N.EXPORTS
        assert hasattr(N.load_library(), name)
    for name, value in (("SPK_LABEL_NON_MATCH", N.LABEL_NON_MATCH), ("SPK_LABEL_MATCH", N.LABEL_MATCH),
                        ("SPK_LABEL_UNKNOWN", N.LABEL_UNKNOWN), ("SPK_LABEL_STATES", N.LABEL_STATES)):
        assert re.search(r"#define\s+" + name + r"\s+" + str(value) + r"\b", text), name
    assert (NON_MATCH, MATCH, UNKNOWN) == (N.LABEL_NON_MATCH, N.LABEL_MATCH, N.LABEL_UNKNOWN)


def test_label_histogram_needs_a_device():
    if N.device_count() > 0:
        return
    with pytest.raises(N.NativeUnavailable):
        N.Context(0).label_histogram(np.zeros(4, dtype=np.int64))


class _StubJob:
    """What label_counts reads of a job before it reaches the device."""

    def __init__(self, link_type, inputs, passthrough=None):
        self.link_type = link_type
        self.inputs = inputs
        self._host_cols = {}
        if passthrough is not None:
            self.passthrough = passthrough


def _gamma_frame(job):
    from splink_amd.frames import GammaFrame
    gf = object.__new__(GammaFrame)
    gf.job = job
    gf.meta = (NAMES, LEVELS)
    return gf


def test_frame_refusals():
    import splink_amd
    from splink_amd.frames import ExpectationFrame, FilteredFrame
    assert splink_amd.LabelCounts is LabelCounts and splink_amd.estimate_from_labels is estimate_from_labels
    assert {"LabelCounts", "estimate_from_labels"} <= set(splink_amd.__all__)
    records = pd.DataFrame({"unique_id": [1, 2], "cluster": [7, 7]})
    # a job made from a gamma table has pairs without rows
    gf = _gamma_frame(_StubJob("dedupe_only", [records], passthrough=pd.DataFrame({"gamma_a": [0]})))
    with pytest.raises(ValueError, match="gamma table"):
        gf.label_counts("cluster")
    df_e = object.__new__(ExpectationFrame)
    df_e.gammas, df_e.job, df_e.lam, df_e.level_probs = gf, gf.job, 0.5, [([0.5, 0.5], [0.5, 0.5])]
    with pytest.raises(ValueError, match="gamma table"):
        df_e.truth_table("cluster")
    # a label column missing from an input table (link_only: from the right one)
    with pytest.raises(ValueError, match="missing from input table 0"):
        _gamma_frame(_StubJob("dedupe_only", [records])).label_counts("truth")
    with pytest.raises(ValueError, match="missing from input table 1"):
        _gamma_frame(_StubJob("link_only", [records, records[["unique_id"]]])).label_counts("cluster")
    # the stage function runs over every pair of a job: no filtered frame, no gamma table
    filtered = object.__new__(FilteredFrame)
    with pytest.raises(ValueError, match="filtered frame"):
        estimate_from_labels(filtered, None, {}, None, "cluster")
    with pytest.raises(ValueError, match="add_gammas"):
        estimate_from_labels(pd.DataFrame({"gamma_a": [0]}), None, {}, None, "cluster")
