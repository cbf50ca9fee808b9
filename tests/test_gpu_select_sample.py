"""frame.sample_pairs() on the device (spk_select_sample): the sample equals the definition, exactly.

The expectation is the parent's toPandas() (already pinned to the reference) plus the key of
tools/emulate_select_sample.py: per stratum the quota rows with the smallest keys, in the parent's order."""
import warnings

import numpy as np
import pandas as pd
import pytest

from conftest import load_golden
from select_sample_common import emulator, expected_sample
from test_gpu_select import check, gamma_table_frame, scored

pytestmark = pytest.mark.gpu
warnings.filterwarnings("ignore")


@pytest.fixture(scope="module")
def amd():
    from splink_amd import AmdSession, _native
    if _native.device_count() == 0:
        pytest.fail("no HIP device visible: the -m gpu tests need an MI355X")
    return AmdSession(0)


def check_sample(sample, pdf, edges, quota, seed, eligible=None, parent=None):
    """sample.toPandas(), count() and strata() against the definition over the parent frame `pdf`; returns
    (the sample's frame, population, kept) per stratum."""
    exp, pop, cnt = expected_sample(pdf, edges, quota, seed, eligible)
    got = sample.toPandas()
    pd.testing.assert_frame_equal(got, exp, check_exact=True)
    assert list(got.dtypes) == list(exp.dtypes)
    assert got["stratum"].dtype == np.int32 and got["sampling_weight"].dtype == np.float64
    assert list(got.columns) == list(pdf.columns) + ["stratum", "sampling_weight"] == sample.columns
    assert sample.count() == len(exp) == len(sample) == int(cnt.sum())
    st = sample.strata()
    assert list(st.columns) == ["stratum", "low", "high", "pairs", "sampled"]
    assert np.array_equal(st["stratum"], np.arange(len(quota))) and st["stratum"].dtype == np.int32
    assert np.array_equal(st["low"], np.asarray(edges[:-1], dtype=np.float64))
    assert np.array_equal(st["high"], np.asarray(edges[1:], dtype=np.float64))
    assert np.array_equal(st["pairs"], pop) and np.array_equal(st["sampled"], cnt)
    assert st["pairs"].dtype == np.int64 and st["sampled"].dtype == np.int64
    if parent is not None:
        assert sample.columns[:-2] == parent.columns
    return got, pop, cnt


def quantile_edges(mp):
    """Edges at occurring probabilities: quartiles of the distinct scores, one stratum that holds a single value and an
    empty one after it (inside the widest gap between two adjacent distinct scores of the middle half, so the gap is
    more than one ulp); the first and last edges are the extreme scores."""
    d = np.sort(np.unique(mp[~np.isnan(mp)]))
    if len(d) < 8:
        return [float(d[0]), float(np.nextafter(d[0], 2.0)), 2.0]  # the smallest score alone; everything else
    i1, i3 = len(d) // 4, 3 * len(d) // 4
    i2 = i1 + 1 + int(np.argmax(np.diff(d[i1 + 1:i3])))  # i1 < i2 and i2 + 1 < i3
    assert np.nextafter(d[i2], 2.0) < d[i2 + 1]
    return [float(x) for x in (d[0], d[i1], d[i2], np.nextafter(d[i2], 2.0), d[i2 + 1], d[i3], d[-1])]


# ---- 1. chunk and wave edges --------------------------------------------------------------------------------
def _edge_sizes():
    from splink_amd import _native
    C = _native.SELECT_CHUNK
    return [1, 63, 64, 65, C - 1, C, C + 1, 3 * C + 17]


@pytest.mark.parametrize("n", _edge_sizes())
def test_chunk_and_wave_edges(n, amd):
    df_e = gamma_table_frame(amd, n, [2, 3, 4], seed=n)
    pdf = df_e.toPandas()
    assert len(pdf) == n and (pdf["unique_id_l"] == np.arange(n)).all()
    mp = pdf["match_probability"].to_numpy()
    edges = quantile_edges(mp)
    q = 2 if n < 200 else 5
    quota = [q, q + 1, q, q, q + 2, q][:len(edges) - 1]
    got, pop, cnt = check_sample(df_e.sample_pairs(per_stratum=quota, strata=edges, seed=n), pdf, edges, quota, n,
                                 parent=df_e)
    if n >= 64:
        assert len(edges) == 7 and pop[3] == 0  # the deliberately empty stratum
        assert sum(1 for b in range(6) if pop[b] > quota[b] > 0) >= 3
        assert pop.sum() == n  # the extreme scores are edges: left-closed at the first, right-closed at the last
        assert (mp == edges[1]).any() and (mp == edges[-1]).any()
        # a score equal to an inner edge is in the stratum to its right, one equal to the last edge in the last
        assert pop[1] == ((mp >= edges[1]) & (mp < edges[2])).sum() and pop[5] == (mp >= edges[5]).sum()
        assert pop[2] == (mp == edges[2]).sum() > 0
        assert (np.diff(got["unique_id_l"].to_numpy()) > 0).all()
        w = got["sampling_weight"].to_numpy()
        assert np.array_equal(w, pop[got["stratum"]] / cnt[got["stratum"]])
    else:
        assert len(got) == min(n, sum(min(a, b) for a, b in zip(quota, pop)))


# ---- 2. wide codes ------------------------------------------------------------------------------------------
def test_wide_codes_and_global_stratum_table(amd):
    """9 columns of 4 levels: 5^9 patterns, so uint32 codes and a stratum table read from global memory."""
    n = 5003
    df_e = gamma_table_frame(amd, n, [4] * 9, seed=9)
    assert df_e.job.ctx.n_patterns() == 5 ** 9
    pdf = df_e.toPandas()
    mp = pdf["match_probability"].to_numpy()
    edges = [float(x) for x in np.quantile(mp, [0.0, 0.2, 0.5, 0.8, 1.0])]
    quota = [7, 0, 10 ** 6, 13]
    got, pop, cnt = check_sample(df_e.sample_pairs(quota, edges, seed=99), pdf, edges, quota, 99, parent=df_e)
    assert pop.sum() == n and list(cnt) == [7, 0, pop[2], 13] and min(pop) > 13


# ---- 3. composition with terms ------------------------------------------------------------------------------
def test_sample_of_a_filtered_frame(amd):
    n = 5000
    df_e = gamma_table_frame(amd, n, [2, 3, 4], seed=3)
    pdf = df_e.toPandas()
    mp = pdf["match_probability"]
    t = float(mp.quantile(0.3))
    f = df_e.filter(f"match_probability > {t!r} and gamma_c1 >= 1")
    eligible = ((mp > t) & (pdf["gamma_c1"] >= 1)).to_numpy()
    edges = [i / 5 for i in range(6)]
    got, pop, cnt = check_sample(f.sample_pairs(per_stratum=4, strata=5, seed=12), pdf, edges, [4] * 5, 12, eligible, df_e)
    assert pop.sum() == eligible.sum() < n and 0 < len(got) < eligible.sum()
    assert (got["match_probability"] > t).all() and (got["gamma_c1"] >= 1).all()
    # the same through chained filters, and a condition that keeps nothing
    check_sample(df_e.filter(f"match_probability > {t!r}").filter("gamma_c1 >= 1").sample_pairs(4, 5, 12), pdf, edges,
                 [4] * 5, 12, eligible)
    none = df_e.filter("gamma_c0 is null").sample_pairs(4, 5, 12)
    assert none.count() == 0 and list(none.strata()["pairs"]) == [0] * 5


# ---- 4. NULL match_probability ------------------------------------------------------------------------------
def test_null_match_probability_is_never_sampled(amd):
    from splink_amd.frames import ExpectationFrame
    n = 2500
    base = gamma_table_frame(amd, n, [2, 3, 4], seed=6)
    probs = [(list(m), list(u)) for m, u in base.level_probs]
    probs[1][0][1] = 0.0  # m = u = 0 at level 1 of column c1: that pattern's denominator is 0, its probability NULL
    probs[1][1][1] = 0.0
    df_e = ExpectationFrame(base.gammas, base.settings, base.lam, probs)
    pdf = df_e.toPandas()
    null = pdf["match_probability"].isna().to_numpy()
    assert 0 < null.sum() < n
    edges = [0.0, 0.25, 0.5, 0.75, 1.0]
    got, pop, cnt = check_sample(df_e.sample_pairs(n, 4, seed=1), pdf, edges, [n] * 4, 1, parent=df_e)
    assert len(got) == pop.sum() == n - null.sum() and not got["match_probability"].isna().any()
    got, _, _ = check_sample(df_e.sample_pairs(5, 4, seed=1), pdf, edges, [5] * 4, 1)
    assert not got["match_probability"].isna().any()
    # the NULL rows alone: eligible under the term, in no stratum
    assert df_e.filter("match_probability is null").sample_pairs(n, 4, seed=1).count() == 0


# ---- 5. nesting and determinism -----------------------------------------------------------------------------
def test_nesting_determinism_and_64_strata(amd):
    n = 6000
    df_e = gamma_table_frame(amd, n, [2, 3, 4], seed=5)
    pdf = df_e.toPandas()
    edges = [i / 10 for i in range(11)]
    small, _, _ = check_sample(df_e.sample_pairs(5, 10, seed=7), pdf, edges, [5] * 10, 7)
    large, pop, cnt = check_sample(df_e.sample_pairs(50, 10, seed=7), pdf, edges, [50] * 10, 7)
    assert sum(1 for b in range(10) if pop[b] > 50) >= 3
    assert len(small) < len(large) and set(small["unique_id_l"]) < set(large["unique_id_l"])
    again = df_e.sample_pairs(5, 10, seed=7).toPandas()
    pd.testing.assert_frame_equal(again, small, check_exact=True)
    other = df_e.sample_pairs(5, 10, seed=8).toPandas()
    assert len(other) == len(small) and set(other["unique_id_l"]) != set(small["unique_id_l"])
    check_sample(df_e.sample_pairs(5, 10, seed=2 ** 64 - 1), pdf, edges, [5] * 10, 2 ** 64 - 1)
    # the largest histogram: 64 strata, and a single one
    e64 = [i / 64 for i in range(65)]
    got, pop, _ = check_sample(df_e.sample_pairs(3, 64, seed=7), pdf, e64, [3] * 64, 7)
    assert (pop > 3).sum() >= 3 and (pop == 0).any()
    check_sample(df_e.sample_pairs(11, 1, seed=7), pdf, [0.0, 1.0], [11], 7)


# ---- 6. extremes --------------------------------------------------------------------------------------------
def test_quota_at_or_above_every_population_and_quota_zero(amd):
    n = 4099
    df_e = gamma_table_frame(amd, n, [2, 3, 4], seed=8)
    pdf = df_e.toPandas()
    mp = pdf["match_probability"]
    lo, hi = float(mp.quantile(0.1)), float(mp.quantile(0.9))
    edges = [lo, (lo + hi) / 2, hi]
    inside = (mp >= lo) & (mp <= hi)
    assert 0 < inside.sum() < n
    pops = [int(((mp >= edges[0]) & (mp < edges[1])).sum()), int(((mp >= edges[1]) & (mp <= edges[2])).sum())]
    for quota in (pops, [p + 1 for p in pops], [n, n]):
        s = df_e.sample_pairs(quota, edges, seed=4)
        got, pop, cnt = check_sample(s, pdf, edges, quota, 4)
        assert list(pop) == pops == list(cnt)
        whole = df_e.filter(f"match_probability >= {lo!r} and match_probability <= {hi!r}")
        assert check(whole, pdf, inside, df_e) == len(got)
        pd.testing.assert_frame_equal(got[list(pdf.columns)], whole.toPandas(), check_exact=True)
        assert (got["sampling_weight"] == 1.0).all()
    got, pop, cnt = check_sample(df_e.sample_pairs([pops[0] - 1, pops[1] - 1], edges, seed=4), pdf, edges,
                                 [pops[0] - 1, pops[1] - 1], 4)
    assert len(got) == inside.sum() - 2
    empty = df_e.sample_pairs(0, edges, seed=4)
    got, pop, cnt = check_sample(empty, pdf, edges, [0, 0], 4)
    assert len(got) == 0 and list(pop) == pops and list(cnt) == [0, 0]
    # a parent with zero pairs
    none = gamma_table_frame(amd, 0, [2, 3, 4], seed=0)
    s = none.sample_pairs(5, 3, seed=0)
    assert s.count() == 0 and len(s.toPandas()) == 0 and list(s.strata()["pairs"]) == [0, 0, 0]


# ---- 7. a pipeline, and the labels' route back ---------------------------------------------------------------
def test_pipeline_sample_feeds_label_counts_from_pairs(amd):
    g = load_golden("synthetic_cfg1")
    _, df_e = scored(g, amd)
    pdf = df_e.toPandas()
    assert len(pdf) == len(g["df_e"]["match_probability"])
    edges = [0.0, 0.25, 0.5, 0.75, 1.0]
    sample = df_e.sample_pairs(per_stratum=3, strata=4, seed=11)
    got, pop, cnt = check_sample(sample, pdf, edges, [3] * 4, 11, parent=df_e)
    assert 0 < len(got) < len(pdf) and (pop > 3).any()
    # weighted back, the sample stands for every pair inside the edges
    assert got["sampling_weight"].sum() == pytest.approx(pop[cnt > 0].sum(), rel=1e-12)
    labels = got[["unique_id_l", "unique_id_r"]].copy()
    labels["clerical_match_score"] = (got["match_probability"] > 0.5).astype(float)
    lp = df_e.label_counts_from_pairs(labels).labelled_pairs()
    assert lp["found_by_blocking"].all() and len(lp) == len(got)
    assert np.array_equal(lp["match_probability"].to_numpy(), got["match_probability"].to_numpy())
    # the sample is still the context's selection afterwards, or is drawn again: the same rows
    pd.testing.assert_frame_equal(df_e.sample_pairs(3, 4, 11).toPandas(), got, check_exact=True)
    # a filtered pipeline frame
    t = float(pdf["match_probability"].median())
    check_sample(df_e.filter(f"match_probability > {t!r}").sample_pairs(2, 4, 5), pdf, edges, [2] * 4, 5,
                 (pdf["match_probability"] > t).to_numpy(), df_e)


# ---- 8. no interference, refusals ---------------------------------------------------------------------------
def test_sample_leaves_scores_tf_and_em_alone(amd):
    from splink_amd.frames import ExpectationFrame
    g = load_golden("link_tf")
    linker, df_e = scored(g, amd)
    job = df_e.job
    stats0 = job.em_stats(df_e.lam, df_e.level_probs)
    tf = linker.make_term_frequency_adjustments(df_e)
    tf0 = tf.toPandas()
    # a sample of the same codes under other parameters than the last score
    other = [([p for p in reversed(m)], [p for p in reversed(u)]) for m, u in df_e.level_probs]
    df_o = ExpectationFrame(df_e.gammas, df_e.settings, 0.123, other)
    opdf = df_o.toPandas()
    job.score(df_e.lam, df_e.level_probs, want_host=False)  # the last score is df_e's again
    t = float(opdf["match_probability"].median())
    f = df_o.filter(f"match_probability >= {t!r}")
    k = f.count()  # a filtered frame, selected before the sample
    assert 0 < k < len(opdf) and job.selection_owner is f
    tf_col = next(c["col_name"] for c in df_e.settings["comparison_columns"] if c["term_frequency_adjustments"])
    col = job._col_index[(tf_col, "str")]
    nv = job.ctx.tf_column_values(col)

    def tf_state():
        scale = job.ctx.tf_scales_column(col, nv)
        limbs, counts = job.ctx.tf_accumulate_column_exact(col, nv, scale)
        return scale.copy(), limbs.copy(), counts.copy()
    before = tf_state()
    edges = [0.0, 0.5, 1.0]
    sample = df_o.sample_pairs(4, 2, seed=21)
    got, pop, cnt = check_sample(sample, opdf, edges, [4, 4], 21, parent=df_o)
    assert 0 < len(got) < len(opdf)
    for a, b in zip(before, tf_state()):
        assert np.array_equal(a, b)
    # the filtered frame selects again before it copies: the sample took the context's selection over
    assert job.selection_owner is sample
    assert check(f, opdf, opdf["match_probability"] >= t, df_o) == k
    assert job.selection_owner is f
    pd.testing.assert_frame_equal(df_o.sample_pairs(4, 2, seed=21).toPandas(), got, check_exact=True)
    # the per-pair tf results and the EM statistics are as before, also right after a sample
    tf1 = linker.make_term_frequency_adjustments(df_e).toPandas()
    pd.testing.assert_frame_equal(tf0, tf1, check_exact=True)
    assert np.array_equal(stats0, job.em_stats(df_e.lam, df_e.level_probs), equal_nan=True)
    assert df_o.sample_pairs(3, 2, seed=22).count() == min(3, pop[0]) + min(3, pop[1])
    tf2 = linker.make_term_frequency_adjustments(df_e).toPandas()
    pd.testing.assert_frame_equal(tf0, tf2, check_exact=True)
    # refusals: the tf-filtered frame, a best-match frame, a frame filtered from the unscored one, a sample frame
    with pytest.raises(ValueError, match="term-frequency"):
        tf.filter("tf_adjusted_match_prob > 0.5").sample_pairs(3, 2)
    with pytest.raises(ValueError, match="best-match"):
        df_e.best_matches().sample_pairs(3, 2)
    gcol = df_e.gammas.meta[0][0]
    with pytest.raises(ValueError, match="unscored"):
        df_e.gammas.filter(f"{gcol} >= 0").sample_pairs(3, 2)
    for call in (lambda: sample.filter("match_probability > 0.5"), lambda: sample.best_matches(),
                 lambda: sample.clusters(), lambda: sample.sample_pairs(1, 2)):
        with pytest.raises(ValueError, match="sample frame"):
            call()
    with pytest.raises(ValueError, match="sample_pairs"):
        df_e.sample_pairs(3, [0.0, 0.5, 0.5])


# ---- 9. ABI states ------------------------------------------------------------------------------------------
def test_abi_states(amd):
    from splink_amd import _native as N
    emu = emulator()
    ctx = N.Context(0)
    rng = np.random.Generator(np.random.PCG64(11))
    n, levels = 5000, [2, 3]
    g = np.stack([rng.integers(-1, L, n) for L in levels], axis=1).astype(np.int8)
    m = np.array([0.2, 0.8, 0.1, 0.3, 0.6])
    u = np.array([0.7, 0.3, 0.5, 0.3, 0.2])
    edges, quota = [0.0, 0.3, 1.0], [10, 20]
    info = ctx.select_sample_info()
    assert info[0] == -1 and len(info[1]) == 0 and len(info[2]) == 0 and info[3] == -1.0
    with pytest.raises(RuntimeError):  # no codes yet
        ctx.select_sample(0.3, 0.7, m, u, [], edges, quota, 1)
    assert ctx.select_sample_info()[0] == -1
    ctx.gammas_load(levels, g)
    mp_all = ctx.score(0.3, 0.7, m, u, 0, n)
    k = ctx.select_sample(0.3, 0.7, m, u, [], edges, quota, 1)
    kept, stratum, pop, cnt = emu.sample(1, np.arange(n), mp_all, edges, quota)
    assert k == 30 == kept.sum() and ctx.select_info() == (k, -1.0)
    n_strata, got_pop, got_kept, ms = ctx.select_sample_info()
    assert n_strata == 2 and np.array_equal(got_pop, pop) and np.array_equal(got_kept, cnt) and ms == -1.0
    ordinal, _, _, gam, mp = ctx.select_copy(0, k, 2, rows=False)
    want = np.nonzero(kept)[0]
    assert np.array_equal(ordinal, want) and np.array_equal(gam, g[want]) and np.array_equal(mp, mp_all[want])
    with pytest.raises(RuntimeError, match="pair rows"):  # a loaded gamma table gives no rows
        ctx.select_copy(0, k, 2, rows=True)
    # with terms, and timing
    ctx.enable_timing(True)
    ne = (N.SEL_GAMMA, 0, N.SEL_OP["!="], -1.0)
    t = float(np.median(mp_all))
    k = ctx.select_sample(0.3, 0.7, m, u, [(N.SEL_MP, 0, N.SEL_OP["<="], t), ne], edges, quota, 2)
    kept = emu.sample(2, np.arange(n), mp_all, edges, quota, (mp_all <= t) & (g[:, 0] != -1))[0]
    assert np.array_equal(ctx.select_copy(0, k, 2, rows=False)[0], np.nonzero(kept)[0])
    assert ctx.select_sample_info()[3] >= 0.0 and ctx.select_info()[1] >= 0.0
    ctx.enable_timing(False)
    # new codes make the selection stale
    ctx.gammas_load(levels, g)
    with pytest.raises(RuntimeError, match="changed since spk_select"):
        ctx.select_copy(0, k, 2, rows=False, mp=False)
    # invalid arguments; a failing call leaves no selection and no figures
    bad = [dict(edges=[0.0, 0.3, 0.3]), dict(edges=[0.0, 0.5, 0.3]), dict(edges=[0.0, float("nan"), 1.0]),
           dict(edges=[0.0, 0.3, float("inf")]), dict(quota=[10, -1]), dict(edges=[0.5], quota=[]),
           dict(edges=list(np.linspace(0, 1, 66)), quota=[1] * 65),
           dict(terms=[(N.SEL_TF_MP, 0, N.SEL_OP[">"], 0.5)]), dict(terms=[(3, 0, N.SEL_OP[">"], 0.5)]),
           dict(terms=[(N.SEL_GAMMA, 0, 8, 1.0)]), dict(terms=[(N.SEL_GAMMA, 2, N.SEL_OP["="], 1.0)]), dict(terms=[ne] * 9)]
    for kw in bad:
        assert ctx.select_sample(0.3, 0.7, m, u, [], edges, quota, 1) == 30
        args = dict(terms=[], edges=edges, quota=quota)
        args.update(kw)
        with pytest.raises(ValueError):
            ctx.select_sample(0.3, 0.7, m, u, args["terms"], args["edges"], args["quota"], 1)
        assert ctx.select_info()[0] == -1 and ctx.select_sample_info()[0] == -1, kw
        with pytest.raises(RuntimeError):
            ctx.select_copy(0, 1, 2, rows=False, mp=False)
    # a plain selection afterwards replaces the sample; the sample's figures stay those of the last sample call
    assert ctx.select_sample(0.3, 0.7, m, u, [], edges, quota, 1) == 30
    assert ctx.select(0.0, 0.0, None, None, [ne]) == int((g[:, 0] != -1).sum())
    assert ctx.select_sample_info()[0] == 2
    # pairs loaded: rows come back; the narrowing and the components work on the sample
    ctx2 = N.Context(0)
    ctx2.table_create(0, 100, 1)
    rows_l = rng.integers(0, 100, n).astype(np.int32)
    rows_r = rng.integers(0, 100, n).astype(np.int32)
    ctx2.pairs_load(rows_l, rows_r)
    ctx2.gammas_load(levels, g)
    k = ctx2.select_sample(0.3, 0.7, m, u, [], edges, [40, 40], 5)
    kept = emu.sample(5, np.arange(n), mp_all, edges, [40, 40])[0]
    ordinal, l, r, _, _ = ctx2.select_copy(0, k, 2, rows=True, gammas=False, mp=False)
    assert k == 80 and np.array_equal(ordinal, np.nonzero(kept)[0])
    assert np.array_equal(l, rows_l[ordinal]) and np.array_equal(r, rows_r[ordinal])
    assert 0 < ctx2.select_best(N.SEL_MP, N.BEST_L, 0) <= k
    ctx2.pairs_load(rows_l, rows_r)
    with pytest.raises(RuntimeError):
        ctx2.select_copy(0, 1, 2, rows=False, gammas=False, mp=False)
