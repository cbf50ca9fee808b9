"""frame.orderBy(score).limit(k) and frame.limit(k) on the device (spk_select_top, spk_select_top_of): the rows equal
the inner frame's toPandas() sorted by the definition (NULL lowest, ties in frame order) and cut at k.

Every expected value comes from a path already pinned elsewhere, the inner frame's toPandas(), ordered by
select_top_common.definition_order (a stable Python sort); rows, order, dtypes and scores are compared exactly."""
import warnings

import numpy as np
import pandas as pd
import pytest

from select_top_common import assert_frames_identical, definition_order, expected_top
from test_gpu_select import gamma_table_frame, golden_case, scored
from test_gpu_tf_select import CtxCase, amd, link_tf, two_tf  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu
warnings.filterwarnings("ignore")
MP, TF = "match_probability", "tf_adjusted_match_prob"
ORDERS = [(None, True), (MP, True), (MP, False)]


def top_of(frame, by, ascending, k):
    if by is None:
        return frame.limit(k)
    f = frame.orderBy(by, ascending=ascending)
    return f if k is None else f.limit(k)


def check_top(frame, inner_pdf, by, ascending, k, mask=None):
    """top_of(frame, ...) equals the definition over inner_pdf[mask]: rows, order, dtypes, count() and cut()."""
    from splink_amd import TopFrame
    exp, cut = expected_top(inner_pdf, by, ascending, k, mask)
    top = top_of(frame, by, ascending, k)
    assert isinstance(top, TopFrame)
    assert top.count() == len(exp) == len(top)
    assert_frames_identical(top.toPandas(), exp)
    assert top.cut() == cut, (by, ascending, k, top.cut(), cut)
    return top


def k_inside_largest_tie(score, ascending):
    """A k whose cut falls inside the largest class of equal scores (NULLs are one class)."""
    score = np.asarray(score, dtype=np.float64)
    order = definition_order(score, ascending)
    s = score[order]
    start = np.concatenate([[0], np.nonzero(~((s[1:] == s[:-1]) | (np.isnan(s[1:]) & np.isnan(s[:-1]))))[0] + 1, [len(s)]])
    size = np.diff(start)
    i = int(np.argmax(size))
    return int(start[i] + max(size[i] // 2, 1))


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
    for by, ascending in ORDERS:
        inside = n // 2 if by is None else k_inside_largest_tie(pdf[MP], ascending)
        for k in (0, 1, inside, n, n + 5):
            top = check_top(df_e, pdf, by, ascending, k)
            if by is not None and k == inside and n >= 63:
                c = top.cut()
                assert 0 < c["tied_kept"] < c["tied"] and c["score"] is not None
    check_top(df_e, pdf, MP, False, None)  # an orderBy without limit keeps every pair, sorted


# ---- 2. one huge tie class across chunks --------------------------------------------------------------------
@pytest.mark.parametrize("ascending", [True, False])
def test_one_tie_class_across_chunks(ascending, amd):
    """One two-level column: 3 patterns, so the pairs at the cut span several chunks and the rank of a pair among
    them is carried across chunk boundaries."""
    from splink_amd import _native
    C = _native.SELECT_CHUNK
    n = 3 * C + 17
    df_e = gamma_table_frame(amd, n, [2], seed=2)
    assert df_e.job.ctx.n_patterns() == 3
    pdf = df_e.toPandas()
    k = k_inside_largest_tie(pdf[MP], ascending)
    top = check_top(df_e, pdf, MP, ascending, k)
    c = top.cut()
    assert c["tied"] > C
    assert c["tied_kept"] == int((top.toPandas()[MP] == c["score"]).sum())
    assert 0 < c["tied_kept"] < c["tied"]
    # the kept pairs at the cut are the class's first ones in frame order
    at = pdf[pdf[MP] == c["score"]]["unique_id_l"].to_numpy()[:c["tied_kept"]]
    got = top.toPandas()
    assert np.array_equal(got[got[MP] == c["score"]]["unique_id_l"].to_numpy(), at)
    for k2 in (k - c["tied_kept"], k - c["tied_kept"] + 1, k - c["tied_kept"] + c["tied"]):  # the class's edges
        check_top(df_e, pdf, MP, ascending, k2)


# ---- 3. wide codes ------------------------------------------------------------------------------------------
def test_wide_codes_and_global_tables(amd):
    """9 columns of 4 levels: 5^9 patterns, so uint32 codes, and the pattern counts and classes in global memory."""
    n = 5003
    df_e = gamma_table_frame(amd, n, [4] * 9, seed=9)
    assert df_e.job.ctx.n_patterns() == 5 ** 9 > 1 << 18
    pdf = df_e.toPandas()
    for by, ascending in ORDERS:
        for k in (0, 1, 100, 2500 if by is None else k_inside_largest_tie(pdf[MP], ascending), n, n + 5):
            check_top(df_e, pdf, by, ascending, k)
    t = float(pdf[MP].median())
    check_top(df_e.filter(f"{MP} > {t!r} and gamma_c8 >= 1"), pdf, MP, False, 77, (pdf[MP] > t) & (pdf["gamma_c8"] >= 1))


# ---- 4. with terms ------------------------------------------------------------------------------------------
def test_with_terms(amd):
    n = 4099
    df_e = gamma_table_frame(amd, n, [2, 3, 4], seed=5)
    pdf = df_e.toPandas()
    t = float(pdf[MP].quantile(0.3))
    mask = (pdf[MP] > t) & (pdf["gamma_c1"] >= 1)
    f = df_e.filter(f"{MP} > {t!r} and gamma_c1 >= 1")
    el = int(mask.sum())
    assert 0 < el < n
    for by, ascending in ORDERS:
        inside = el // 2 if by is None else k_inside_largest_tie(pdf[MP][mask], ascending)
        for k in (0, 1, inside, el, el + 5):
            check_top(f, pdf, by, ascending, k, mask)
    # the strongest pairs whose second column disagrees, asc() / desc(), sort, and the unscored frame's limit
    from splink_amd import asc, desc
    m0 = pdf["gamma_c1"] == 0
    exp, _ = expected_top(pdf, MP, False, 100, m0)
    assert_frames_identical(df_e.filter("gamma_c1 = 0").orderBy(desc(MP)).limit(100).toPandas(), exp)
    exp, _ = expected_top(pdf, MP, True, 100, m0)
    assert_frames_identical(df_e.filter("gamma_c1 = 0").sort(asc(MP)).limit(100).toPandas(), exp)
    gf = df_e.gammas
    gpdf = gf.toPandas()
    check_top(gf.filter("gamma_c2 < 2"), gpdf, None, True, 50, gpdf["gamma_c2"] < 2)
    with pytest.raises(ValueError, match="orderBy"):
        gf.filter("gamma_c2 < 2").orderBy(MP)
    with pytest.raises(ValueError, match="orderBy"):
        df_e.orderBy("gamma_c1")
    with pytest.raises(ValueError, match="orderBy"):
        df_e.orderBy(TF)
    with pytest.raises(ValueError, match="limit"):
        df_e.limit(-1)
    # a never-true predicate and an empty parent
    check_top(df_e.filter("gamma_c0 is null"), pdf, MP, False, 5, np.zeros(n, dtype=bool))
    empty = gamma_table_frame(amd, 0, [2, 3, 4], seed=0)
    check_top(empty, empty.toPandas(), MP, True, 5)
    check_top(empty, empty.toPandas(), None, True, 5)


# ---- 5. NULL scores -----------------------------------------------------------------------------------------
def test_null_scores_first_ascending_last_descending(amd):
    from splink_amd.frames import ExpectationFrame
    n = 2500
    base = gamma_table_frame(amd, n, [2, 3, 4], seed=6)
    probs = [(list(m), list(u)) for m, u in base.level_probs]
    probs[1][0][1] = 0.0  # m = u = 0 at level 1 of column c1: that pattern's denominator is 0, its probability NULL
    probs[1][1][1] = 0.0
    df_e = ExpectationFrame(base.gammas, base.settings, base.lam, probs)
    pdf = df_e.toPandas()
    null = pdf[MP].isna().to_numpy()
    nn = int(null.sum())
    assert 1 < nn < n - 1
    # ascending: the NULLs come first, in frame order
    top = check_top(df_e, pdf, MP, True, nn // 2)
    assert top.toPandas()[MP].isna().all()
    assert top.cut() == {"eligible": n, "kept": nn // 2, "score": None, "tied": nn, "tied_kept": nn // 2}
    check_top(df_e, pdf, MP, True, nn)
    top = check_top(df_e, pdf, MP, True, nn + 1)  # just past the class
    assert top.toPandas()[MP].isna().sum() == nn and top.cut()["score"] == float(pdf[MP].min())
    # descending: the NULLs come last
    top = check_top(df_e, pdf, MP, False, n - nn)
    assert not top.toPandas()[MP].isna().any()
    check_top(df_e, pdf, MP, False, n - nn - 1)
    top = check_top(df_e, pdf, MP, False, n - nn + nn // 2)  # inside the NULL class
    assert top.toPandas()[MP].isna().sum() == nn // 2 and top.cut()["tied"] == nn and top.cut()["score"] is None
    check_top(df_e.filter(f"{MP} is null"), pdf, MP, False, 3, null)
    check_top(df_e, pdf, MP, False, None)


# ---- 6. the tf path -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["link_tf", "two_tf"])
def test_tf_frames(which, request):
    case = request.getfixturevalue(which)
    tf, pdf = case.tf, case.pdf
    n = len(pdf)
    for by in (TF, MP):
        for ascending in (False, True):
            for k in (0, 1, 100, k_inside_largest_tie(pdf[by], ascending), n, n + 5):
                check_top(tf, pdf, by, ascending, k)
    check_top(tf, pdf, None, True, 100)
    t = float(pdf[TF].median())
    mask = (pdf[TF] > t) & (pdf[case.gcols[0]] >= 0)
    f = tf.filter(f"{TF} > {t!r} and {case.gcols[0]} >= 0")
    assert 0 < mask.sum() < n
    check_top(f, pdf, TF, False, 50, mask)
    check_top(f, pdf, MP, True, 50, mask)
    check_top(f, pdf, None, True, 50, mask)
    check_top(f, pdf, TF, True, None, mask)


def test_null_tf_scores(amd):
    """spk_select_top_of on the NULL construction of test_null_tf_with_and_without_a_null_match_probability: a NULL
    tf score with and without a NULL match_probability, ordered by either score."""
    m = [0.3, 0.0, 0.2, 0.3, 0.5]
    u = [0.6, 0.0, 0.5, 0.4, 0.0]
    c = CtxCase(5000, [2, 3], seed=6, m=m, u=u, id_hi=6, sizes=(6,))
    N, n = c.N, c.n
    null_tf, null_mp = np.isnan(c.tf), np.isnan(c.mp)
    assert (null_tf & null_mp).any() and (null_tf & ~null_mp).any() and 0 < null_tf.sum() < n
    for field, score in ((N.SEL_TF_MP, c.tf), (N.SEL_MP, c.mp)):
        nn = int(np.isnan(score).sum())
        for order, ascending in ((N.TOP_ASC, True), (N.TOP_DESC, False)):
            for k in (nn // 2, nn, nn + 1, n - nn, n - nn + nn // 2, k_inside_largest_tie(score, ascending)):
                assert c.select([]) == n
                kept = c.ctx.select_top_of(field, order, k)
                want = np.sort(definition_order(score, ascending)[:k])
                assert kept == k == c.ctx.select_info()[0]
                ordinal, l, r, gam, mp = c.ctx.select_copy(0, k, c.K)
                tf, adj = c.ctx.select_copy_tf(0, k, 1)
                assert np.array_equal(ordinal, want)
                assert np.array_equal(l, c.rows_l[want]) and np.array_equal(r, c.rows_r[want])
                assert np.array_equal(gam, c.g[want])
                for got, exp in ((mp, c.mp[want]), (tf, c.tf[want]), (adj, c.adj[want])):
                    assert got.tobytes() == exp.tobytes()  # bit for bit, NaN included
                eligible, n_kept, cut, tied, tied_kept, _ = c.ctx.select_top_info()
                s = score[definition_order(score, ascending)[k - 1]]
                assert (eligible, n_kept) == (n, k)
                assert tied == int((np.isnan(score) if s != s else score == s).sum()) and 0 < tied_kept <= tied
                assert (cut != cut) if s != s else (cut == s)


# ---- 7. best matches ----------------------------------------------------------------------------------------
def test_best_matches_ordered(amd):
    from splink_amd import desc
    _, df_e = scored(golden_case("synthetic_cfg1"), amd)
    pdf = df_e.toPandas()
    t = float(pdf[MP].quantile(0.2))
    bm = df_e.filter(f"{MP} > {t!r}").best_matches(per="mutual")
    inner = bm.toPandas()
    n = len(inner)
    assert n > 20
    for k in (0, 1, 10, k_inside_largest_tie(inner[MP], False), n, n + 5):
        exp, cut = expected_top(inner, MP, False, k)
        top = bm.orderBy(desc(MP)).limit(k)
        assert_frames_identical(top.toPandas(), exp)
        assert top.cut() == cut and top.count() == len(exp)
    check_top(bm, inner, MP, True, 7)
    check_top(bm, inner, None, True, 7)
    assert_frames_identical(bm.toPandas(), inner)  # the best-match frame selects again after the narrowing


# ---- 8. a pipeline ------------------------------------------------------------------------------------------
def test_pipeline_limit_and_truth_table(amd):
    g = golden_case("link_tf")
    _, df_e = scored(g, amd)
    pdf = df_e.toPandas()
    n = len(pdf)
    for k in (0, 1, 100, n, n + 5):
        top = df_e.limit(k)
        assert_frames_identical(top.toPandas(), pdf.head(k).reset_index(drop=True))
        assert top.count() == min(k, n)
    assert_frames_identical(df_e.limit(9).limit(4).toPandas(), pdf.head(4).reset_index(drop=True))
    for by, ascending in ORDERS[1:]:
        check_top(df_e, pdf, by, ascending, 100)
        check_top(df_e, pdf, by, ascending, k_inside_largest_tie(pdf[MP], ascending))
    # precision of the first k: one row, every kept pair a predicted match
    k = 200
    top = df_e.orderBy(MP, ascending=False).limit(k)
    row = top.truth_table("cluster")
    kept = top.toPandas()
    lab_l = pd.DataFrame(g["df_l"]).set_index("unique_id")["cluster"]
    lab_r = pd.DataFrame(g["df_r"]).set_index("unique_id")["cluster"]
    assert lab_l.notna().all() and lab_r.notna().all()  # every pair is labelled
    same = lab_l.loc[kept["unique_id_l"]].to_numpy() == lab_r.loc[kept["unique_id_r"]].to_numpy()
    assert len(row) == 1 and row["threshold"][0] == -np.inf
    assert int(row["tp"][0]) + int(row["fp"][0]) == k and int(row["n_unlabelled_above"][0]) == 0
    assert int(row["tp"][0]) == int(same.sum()) and row["precision"][0] == same.sum() / k


# ---- 9. state and ABI ---------------------------------------------------------------------------------------
def test_abi_states(amd):
    from splink_amd import _native as N
    ctx = N.Context(0)
    rng = np.random.Generator(np.random.PCG64(11))
    n, levels = 5000, [2, 3]
    g = np.stack([rng.integers(-1, L, n) for L in levels], axis=1).astype(np.int8)
    none = (-1, -1, -1, -1)

    def counts():
        e, k, cut, t, tk, ms = ctx.select_top_info()
        return (e, k, t, tk), cut, ms
    assert counts()[0] == none and np.isnan(counts()[1]) and counts()[2] == -1.0
    with pytest.raises(RuntimeError):  # no gammas
        ctx.select_top(0.0, 0.0, None, None, [], N.TOP_FIRST, 5)
    with pytest.raises(RuntimeError):  # no selection
        ctx.select_top_of(N.SEL_MP, N.TOP_FIRST, 5)
    ctx.gammas_load(levels, g)
    eq1 = (N.SEL_GAMMA, 1, N.SEL_OP["="], 1.0)
    want = np.nonzero(g[:, 1] == 1)[0]
    # frame order without m / u
    assert ctx.select_top(0.0, 0.0, None, None, [eq1], N.TOP_FIRST, 40) == 40
    assert counts()[0] == (len(want), 40, 0, 0) and np.isnan(counts()[1])
    assert ctx.select_info()[0] == 40
    ordinal, _, _, gam, _ = ctx.select_copy(0, 40, 2, rows=False, mp=False)
    assert np.array_equal(ordinal, want[:40]) and np.array_equal(gam, g[want[:40]])
    with pytest.raises(RuntimeError, match="m / u"):
        ctx.select_top_of(N.SEL_MP, N.TOP_DESC, 5)  # a selection made without m / u has no score
    assert ctx.select_info()[0] == -1 and counts()[0] == none  # a failing call leaves no selection and no figures
    # argument errors
    m = np.array([0.2, 0.8, 0.1, 0.3, 0.6])
    u = np.array([0.7, 0.3, 0.5, 0.3, 0.2])
    assert ctx.select_top(0.3, 0.7, m, u, [], N.TOP_DESC, 10) == 10 and counts()[0][:2] == (n, 10)
    for bad in (lambda: ctx.select_top(0.3, 0.7, m, u, [], N.TOP_DESC, -1),
                lambda: ctx.select_top(0.3, 0.7, m, u, [], 3, 5),
                lambda: ctx.select_top(0.3, 0.7, m, u, [], -1, 5),
                lambda: ctx.select_top(0.0, 0.0, None, None, [], N.TOP_ASC, 5),   # a score order without m / u
                lambda: ctx.select_top(0.0, 0.0, None, None, [(N.SEL_MP, 0, N.SEL_OP[">"], 0.5)], N.TOP_FIRST, 5),
                lambda: ctx.select_top(0.3, 0.7, m, u, [(N.SEL_TF_MP, 0, N.SEL_OP[">"], 0.5)], N.TOP_DESC, 5),
                lambda: ctx.select_top(0.3, 0.7, m, u, [eq1] * 9, N.TOP_DESC, 5)):
        assert ctx.select_top(0.3, 0.7, m, u, [], N.TOP_DESC, 10) == 10
        with pytest.raises(ValueError):
            bad()
        assert ctx.select_info()[0] == -1 and counts()[0] == none
    for bad in (lambda: ctx.select_top_of(N.SEL_MP, N.TOP_DESC, -1), lambda: ctx.select_top_of(N.SEL_MP, 7, 5),
                lambda: ctx.select_top_of(N.SEL_GAMMA, N.TOP_DESC, 5), lambda: ctx.select_top_of(9, N.TOP_ASC, 5)):
        assert ctx.select(0.3, 0.7, m, u, [eq1]) == len(want)
        with pytest.raises(ValueError):
            bad()
        assert ctx.select_info()[0] == -1 and counts()[0] == none
    # SPK_SEL_TF_MP on a plain selection; the field is ignored in frame order
    assert ctx.select(0.3, 0.7, m, u, [eq1]) == len(want)
    with pytest.raises(RuntimeError, match="tf"):
        ctx.select_top_of(N.SEL_TF_MP, N.TOP_DESC, 5)
    assert ctx.select(0.3, 0.7, m, u, [eq1]) == len(want)
    assert ctx.select_top_of(99, N.TOP_FIRST, 7) == 7
    assert np.array_equal(ctx.select_copy(0, 7, 2, rows=False)[0], want[:7])
    # an empty selection is legal
    assert ctx.select(0.3, 0.7, m, u, [(N.SEL_GAMMA, 0, N.SEL_OP["="], 5.0)]) == 0
    assert ctx.select_top_of(N.SEL_MP, N.TOP_DESC, 5) == 0 and counts()[0] == (0, 0, 0, 0)
    # the narrowing equals the selecting call, and the scores are the parent's bit for bit
    mp_all = ctx.score(0.3, 0.7, m, u, 0, n)
    k = 123
    assert ctx.select_top(0.3, 0.7, m, u, [eq1], N.TOP_DESC, k) == k
    a = ctx.select_copy(0, k, 2, rows=False)
    fig = counts()[0]
    assert ctx.select(0.3, 0.7, m, u, [eq1]) == len(want)
    assert ctx.select_top_of(N.SEL_MP, N.TOP_DESC, k) == k and counts()[0] == fig
    b = ctx.select_copy(0, k, 2, rows=False)
    exp = np.sort(want[definition_order(mp_all[want], False)[:k]])
    assert np.array_equal(a[0], exp) and np.array_equal(b[0], exp)
    assert a[4].tobytes() == b[4].tobytes() == mp_all[exp].tobytes()
    # timing
    ctx.enable_timing(True)
    assert ctx.select_top(0.3, 0.7, m, u, [eq1], N.TOP_ASC, k) == k and counts()[2] >= 0.0
    assert ctx.select_top_of(N.SEL_MP, N.TOP_DESC, 5) == 5 and counts()[2] >= 0.0
    ctx.enable_timing(False)
    assert ctx.select_top(0.3, 0.7, m, u, [eq1], N.TOP_ASC, k) == k and counts()[2] == -1.0
    # new codes make the selection stale
    ctx.gammas_load(levels, g)
    with pytest.raises(RuntimeError, match="changed since"):
        ctx.select_top_of(N.SEL_MP, N.TOP_DESC, 5)
    assert counts()[0] == none


def test_refusals(amd):
    from splink_amd.engine import Job
    from splink_amd.frames import ExpectationFrame, GammaFrame
    from splink_amd.params import Params
    from splink_amd.synthetic import cfg_settings, make_records
    df_e = gamma_table_frame(amd, 500, [2, 3, 4], seed=3)
    top = df_e.orderBy(MP).limit(10)
    for call in (lambda: top.filter("gamma_c0 = 1"), lambda: top.where("gamma_c0 = 1"), lambda: top.best_matches(),
                 lambda: top.clusters(), lambda: top.clusters_at_thresholds([0.5]), lambda: top.sample_pairs(),
                 lambda: top.orderBy(MP), lambda: top.sort(MP)):
        with pytest.raises(ValueError, match="ordered frame"):
            call()
    sample = df_e.sample_pairs(per_stratum=5, strata=4, seed=1)
    for call in (lambda: sample.orderBy(MP), lambda: sample.sort(MP), lambda: sample.limit(3)):
        with pytest.raises(ValueError, match="sample frame"):
            call()
    df = make_records(600, seed=10, surname_vocab=40, first_vocab=30, city_vocab=10)[
        ["unique_id", "first_name", "surname", "dob", "city", "email"]]
    params = Params(cfg_settings(2), amd)
    st = params.settings
    job = Job("dedupe_only", [df], "unique_id", 0, shard=(0, 3))
    job.block(st["blocking_rules"])
    shard = ExpectationFrame(GammaFrame(job, st), st, params.params["λ"], params._level_probabilities())
    for call in (lambda: shard.orderBy(MP), lambda: shard.limit(5), lambda: shard.filter(f"{MP} > 0.5").limit(5)):
        with pytest.raises(ValueError, match="sharded"):
            call()


def test_top_leaves_scores_tf_and_em_alone(link_tf):
    """test_gpu_select.py::test_filter_leaves_scores_tf_and_em_alone for the top calls, under other parameters than the
    last score's."""
    from splink_amd.frames import ExpectationFrame
    case = link_tf
    df_e, job, linker = case.df_e, case.job, case.linker
    stats0 = job.em_stats(df_e.lam, df_e.level_probs)
    other = [([p for p in reversed(m)], [p for p in reversed(u)]) for m, u in df_e.level_probs]
    df_o = ExpectationFrame(df_e.gammas, df_e.settings, 0.123, other)
    opdf = df_o.toPandas()
    job.score(df_e.lam, df_e.level_probs, want_host=False)  # the last score is df_e's again
    mp0 = job.ctx.score(float(df_e.lam), float(1 - df_e.lam), *job.flat_tables(df_e.level_probs), 0, len(opdf))
    job.score(df_e.lam, df_e.level_probs, want_host=False)
    tf_col = next(c["col_name"] for c in df_e.settings["comparison_columns"] if c["term_frequency_adjustments"])
    col = job._col_index[(tf_col, "str")]
    nv = job.ctx.tf_column_values(col)

    def tf_state():
        scale = job.ctx.tf_scales_column(col, nv)
        limbs, counts = job.ctx.tf_accumulate_column_exact(col, nv, scale)
        return scale.copy(), limbs.copy(), counts.copy()
    before = tf_state()
    check_top(df_o, opdf, MP, False, 50)
    check_top(df_o.filter(f"{MP} is not null").best_matches(per="l"),
              df_o.filter(f"{MP} is not null").best_matches(per="l").toPandas(), MP, True, 20)
    check_top(df_o, opdf, None, True, 20)
    for a, b in zip(before, tf_state()):
        assert np.array_equal(a, b)
    pd.testing.assert_frame_equal(case.pdf, linker.make_term_frequency_adjustments(df_e).toPandas(), check_exact=True)
    assert np.array_equal(stats0, job.em_stats(df_e.lam, df_e.level_probs), equal_nan=True)
    job.score(df_e.lam, df_e.level_probs, want_host=False)
    check_top(df_o, opdf, MP, True, 50)
    mp1 = job.ctx.score(float(df_e.lam), float(1 - df_e.lam), *job.flat_tables(df_e.level_probs), 0, len(opdf))
    assert mp0.tobytes() == mp1.tobytes()


def test_top_frame_reselects_after_losing_the_selection(amd):
    df_e = gamma_table_frame(amd, 3000, [2, 3, 4], seed=12)
    pdf = df_e.toPandas()
    top = df_e.orderBy(MP, ascending=False).limit(40)
    assert top.count() == 40 and df_e.job.selection_owner is top
    cut = top.cut()
    other = df_e.filter("gamma_c0 = 1")
    assert other.count() == int((pdf["gamma_c0"] == 1).sum()) and df_e.job.selection_owner is other
    exp, exp_cut = expected_top(pdf, MP, False, 40)
    assert_frames_identical(top.toPandas(), exp)  # selected again: the context held the other frame's survivors
    assert df_e.job.selection_owner is top and top.cut() == cut == exp_cut
