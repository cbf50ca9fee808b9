"""tf.filter(condition) / tf.clusters(t) on the device (spk_select_tf*): the survivors equal the term-frequency
frame masked by pandas.

Every expected value comes from the path already pinned to the reference: tf.toPandas(), or ctx.score +
ctx.tf_apply, masked in numpy / pandas under SQL NULL semantics and compared exactly (columns, order, dtypes,
values; tf_adjusted_match_prob and the adjustments bit for bit).  Thresholds are taken from the device's own
parent values, and every predicate must keep at least one pair and drop at least one."""
import copy
import warnings

import numpy as np
import pandas as pd
import pytest

from conftest import load_golden

pytestmark = pytest.mark.gpu
warnings.filterwarnings("ignore")

TF = "tf_adjusted_match_prob"
MP = "match_probability"


@pytest.fixture(scope="module")
def amd():
    from splink_amd import AmdSession, _native
    if _native.device_count() == 0:
        pytest.fail("no HIP device visible: the -m gpu tests need an MI355X")
    return AmdSession(0)


def frame(d):
    return pd.DataFrame(d) if d else None


def check(f, parent_pdf, mask, parent=None):
    """f.toPandas() == parent.toPandas()[mask].reset_index(drop=True), exactly; returns the survivor count."""
    exp = parent_pdf[np.asarray(mask, dtype=bool)].reset_index(drop=True)
    assert f.count() == len(exp) == len(f)
    got = f.toPandas()
    pd.testing.assert_frame_equal(got, exp, check_exact=True)
    assert list(got.dtypes) == list(exp.dtypes)
    if parent is not None:
        assert f.columns == parent.columns == list(got.columns)
    return len(exp)


def midpoints(values):
    """Midpoints between adjacent distinct non-NULL values: the device's rounding cannot move a pair across one."""
    d = np.sort(pd.Series(values).dropna().unique())
    assert len(d) >= 2
    return (d[:-1] + d[1:]) / 2


def union_find(n_nodes, u, v):
    """label[x] = the smallest id of x's component."""
    parent = list(range(n_nodes))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for a, b in zip(np.asarray(u).tolist(), np.asarray(v).tolist()):
        a, b = find(a), find(b)
        if a != b:
            parent[max(a, b)] = min(a, b)
    return np.array([find(x) for x in range(n_nodes)], dtype=np.int64)


class Case:
    """A scored pipeline with its tf frame; the reference frame is computed once and shared, never changed."""

    def __init__(self, linker, df_e):
        self.linker, self.df_e, self.job = linker, df_e, df_e.job
        self.tf = linker.make_term_frequency_adjustments(df_e)
        self._pdf = self.tf.toPandas()
        self.gcols = [c for c in self._pdf.columns if c.startswith("gamma_")]

    @property
    def pdf(self):
        return self._pdf.copy()


@pytest.fixture(scope="module")
def link_tf(amd):
    from splink_amd import Splink
    g = load_golden("link_tf")
    linker = Splink(copy.deepcopy(g["settings_in"]), amd, df_l=frame(g["df_l"]), df_r=frame(g["df_r"]))
    case = Case(linker, linker.get_scored_comparisons())
    assert len(case.pdf) == len(g["df_tf"][TF]) == 933
    assert case.tf.dev_cols is not None  # the device-id route
    return case


@pytest.fixture(scope="module")
def two_tf(amd):
    from splink_amd import Splink
    from splink_amd.synthetic import cfg_settings, make_records
    df = make_records(3000, seed=21, surname_vocab=120, first_vocab=80)[
        ["unique_id", "first_name", "surname", "dob", "city", "email"]]
    st = cfg_settings(2)
    st["retain_intermediate_calculation_columns"] = True  # the <col>_adj columns are intermediate columns
    for c in st["comparison_columns"]:
        if c["col_name"] in ("surname", "first_name"):
            c["term_frequency_adjustments"] = True
    linker = Splink(st, amd, df=df)
    case = Case(linker, linker.get_scored_comparisons())
    assert case.tf.tf_cols == ["first_name", "surname"]
    assert {"surname_adj", "first_name_adj"} <= set(case.pdf.columns)
    return case


def pick(case):
    """Thresholds from the device's own frame so that every predicate keeps some pairs and drops some."""
    pdf, n = case.pdf, len(case.pdf)
    tf, mp = pdf[TF], pdf[MP]
    mids = midpoints(tf)
    t_gt = float(mids[len(mids) // 2])
    assert 0 < (tf > t_gt).sum() < n
    mmids = midpoints(mp)
    conj = next((float(t), float(s), c) for t in mids[::7] for s in mmids[::5] for c in case.gcols
                if 0 < ((tf > t) & (mp >= s) & (pdf[c] >= 1)).sum() < n)
    chain = next((float(t), c) for t in mids[::-1] for c in case.gcols[::-1] if 0 < ((tf < t) & (pdf[c] != 0)).sum() < n)
    gonly = next((c, v) for v in (1, 0, 2, -1) for c in case.gcols if 0 < (pdf[c] == v).sum() < n)
    return t_gt, conj, chain, gonly


def pipeline_checks(case):
    tf_frame, pdf, n = case.tf, case.pdf, len(case.pdf)
    tf, mp = pdf[TF], pdf[MP]
    t_gt, (t_c, s_c, c_c), (t_ch, c_ch), (c_g, v_g) = pick(case)
    k = check(tf_frame.filter(f"{TF} > {t_gt!r}"), pdf, tf > t_gt, tf_frame)
    assert 0 < k < n
    k = check(tf_frame.where(f"{TF} > {t_c!r} and {MP} >= {s_c!r} and {c_c} >= 1"), pdf,
              (tf > t_c) & (mp >= s_c) & (pdf[c_c] >= 1), tf_frame)
    assert 0 < k < n
    chained = tf_frame.filter(f"{t_ch!r} > {TF}").where(f"{c_ch} <> 0")
    k = check(chained, pdf, (tf < t_ch) & (pdf[c_ch] != 0), tf_frame)
    assert 0 < k < n
    # a predicate without a tf term still returns the tf columns
    f = tf_frame.filter(f"{c_g} = {v_g}")
    assert not f.predicate.needs_tf
    k = check(f, pdf, pdf[c_g] == v_g, tf_frame)
    assert 0 < k < n
    return t_gt


# ---- 1. golden link_tf --------------------------------------------------------------------------------------
def test_link_tf_filters_match_pandas(link_tf):
    assert link_tf.pdf[TF].nunique() > 100  # distinct tf values, and ties among the 933 pairs
    pipeline_checks(link_tf)


@pytest.mark.parametrize("retain", [False, True])
def test_stage_function_with_and_without_adjustment_columns(link_tf, retain, amd):
    from splink_amd.term_frequencies import make_adjustment_for_term_frequencies
    linker = link_tf.linker
    tf_frame = make_adjustment_for_term_frequencies(link_tf.df_e, linker.params, linker.settings, amd,
                                                    retain_adjustment_columns=retain)
    pdf = tf_frame.toPandas()
    assert ("surname_adj" in pdf.columns) == retain
    t = float(midpoints(pdf[TF])[len(midpoints(pdf[TF])) // 3])
    k = check(tf_frame.filter(f"{TF} >= {t!r}"), pdf, pdf[TF] >= t, tf_frame)
    assert 0 < k < len(pdf)
    if retain:
        pd.testing.assert_frame_equal(pdf, link_tf.pdf, check_exact=True)


# ---- 2. two tf columns, dedupe_only -------------------------------------------------------------------------
def test_two_tf_columns_dedupe(two_tf):
    pipeline_checks(two_tf)
    # survivors with and without a surname lookup: pairs of the dob rule have unequal surnames (adjustment 0.5)
    pdf = two_tf.pdf
    tf, half = pdf[TF], pdf["surname_adj"] == 0.5
    t = next(float(x) for x in midpoints(tf)[::-1] if ((tf > x) & half).any() and ((tf > x) & ~half).any())
    f = two_tf.tf.filter(f"{TF} > {t!r}")
    k = check(f, pdf, tf > t, two_tf.tf)
    assert 0 < k < len(pdf)
    got = f.toPandas()
    assert (got["surname_adj"] == 0.5).any() and (got["surname_adj"] != 0.5).any()


# ---- 3. chunk and wave edges, host-id route at context level ------------------------------------------------
N_ROWS = 100


def random_tables(rng, sizes):
    out = []
    for size in sizes:
        t = rng.random(size)
        t[t == 0.0] = 0.5
        t[[1, 2, 3]] = [np.nan, 0.0, 1.0]
        out.append(t)
    return out


class CtxCase:
    """A context with loaded pairs and gamma levels, two host id arrays and their tables, and the parent values:
    ctx.score and ctx.tf_apply over every pair."""

    def __init__(self, n, levels, seed, m=None, u=None, id_hi=20, sizes=(20, 15)):
        from splink_amd import _native as N
        rng = np.random.Generator(np.random.PCG64(seed))
        self.N, self.n, self.K = N, n, len(levels)
        self.g = np.stack([rng.integers(-1, L, n) for L in levels], axis=1).astype(np.int8)
        self.rows_l = rng.integers(0, N_ROWS, n).astype(np.int32)
        self.rows_r = rng.integers(0, N_ROWS, n).astype(np.int32)
        ctx = N.Context(0)
        ctx.table_create(0, N_ROWS, 1)
        ctx.pairs_load(self.rows_l, self.rows_r)
        ctx.gammas_load(levels, self.g)
        self.ctx = ctx
        nm = sum(levels)
        self.m = rng.uniform(0.05, 0.95, nm) if m is None else np.asarray(m, dtype=np.float64)
        self.u = rng.uniform(0.05, 0.95, nm) if u is None else np.asarray(u, dtype=np.float64)
        self.lam = 0.3
        self.ids0 = [rng.integers(-1, id_hi, N_ROWS).astype(np.int64) for _ in sizes]
        self.ids1 = [rng.integers(-1, id_hi, N_ROWS).astype(np.int64) for _ in sizes]
        self.tables = random_tables(rng, sizes)  # the second table is shorter than the id range
        self.mp = ctx.score(self.lam, 1 - self.lam, self.m, self.u, 0, n)
        self.tf, self.adj = ctx.tf_apply(self.ids0, self.ids1, self.tables, 0, n)

    def select(self, terms):
        return self.ctx.select_tf(self.lam, 1 - self.lam, self.m, self.u, self.ids0, self.ids1, self.tables, terms)

    def check(self, terms, mask):
        """The survivors of `terms` are the pairs of `mask`, in ascending ordinal, with the parent's values."""
        want = np.nonzero(np.asarray(mask, dtype=bool))[0]
        k = self.select(terms)
        assert k == len(want) and self.ctx.select_info()[0] == k
        if k == 0:
            return 0
        ordinal, l, r, gam, mp = self.ctx.select_copy(0, k, self.K)
        tf, adj = self.ctx.select_copy_tf(0, k, len(self.tables))
        assert np.array_equal(ordinal, want)
        assert np.array_equal(l, self.rows_l[want]) and np.array_equal(r, self.rows_r[want])
        assert np.array_equal(gam, self.g[want])
        for got, exp in ((mp, self.mp[want]), (tf, self.tf[want]), (adj, self.adj[want])):
            assert got.tobytes() == exp.tobytes()  # bit for bit, NaN included
        return k


def tf_term(N, op, value=0.0):
    return (N.SEL_TF_MP, 0, N.SEL_OP[op], float(value))


def _edge_sizes():
    from splink_amd import _native
    C = _native.SELECT_CHUNK
    return [1, 63, 64, 65, C - 1, C, C + 1, 3 * C + 17]


@pytest.mark.parametrize("n", _edge_sizes())
def test_chunk_and_wave_edges(n, amd):
    """P = 1 has no predicate that keeps a pair and drops one; from 63 pairs on 0 < k < n is asserted."""
    c = CtxCase(n, [2, 3, 4], seed=100 + n)
    N, tf = c.N, c.tf
    t = float(np.nanmedian(tf))
    k = c.check([tf_term(N, ">=", t)], tf >= t)
    k2 = c.check([tf_term(N, "<", t), (N.SEL_GAMMA, 1, N.SEL_OP[">="], 1.0)], (tf < t) & (c.g[:, 1] >= 1))
    s = float(np.nanmedian(c.mp))
    k3 = c.check([(N.SEL_MP, 0, N.SEL_OP[">"], s), tf_term(N, "is not null")], (c.mp > s) & ~np.isnan(tf))
    c.check([(N.SEL_GAMMA, 0, N.SEL_OP["="], -1.0)], c.g[:, 0] == -1)  # no tf term: ranks from the pattern bitset
    if n >= 63:
        assert 0 < k < n and 0 < k2 < n and 0 < k3 < n
        assert (c.adj == 0.5).any() and (c.adj != 0.5).any()


def test_wide_codes_and_global_bitset(amd):
    """9 columns of 4 levels: 5^9 patterns, so uint32 codes and a keep bitset read from global memory."""
    n = 5003
    c = CtxCase(n, [4] * 9, seed=9)
    N, tf = c.N, c.tf
    assert c.ctx.n_patterns() == 5 ** 9 > 1 << 18
    t = float(np.nanmedian(tf))
    k = c.check([tf_term(N, ">", t), (N.SEL_GAMMA, 8, N.SEL_OP[">="], 1.0)], (tf > t) & (c.g[:, 8] >= 1))
    assert 0 < k < n
    k = c.check([tf_term(N, "<=", t)], tf <= t)
    assert 0 < k < n
    k = c.check([(N.SEL_GAMMA, 4, N.SEL_OP["<="], 2.0), (N.SEL_GAMMA, 0, N.SEL_OP["="], -1.0)],
                (c.g[:, 4] <= 2) & (c.g[:, 0] == -1))
    assert 0 < k < n


# ---- 4. boundaries ------------------------------------------------------------------------------------------
def test_threshold_equal_to_an_occurring_value_with_ties(amd):
    n = 4099
    c = CtxCase(n, [2, 3, 4], seed=5, id_hi=6, sizes=(6,))
    N, tf = c.N, c.tf
    values, counts = np.unique(tf[~np.isnan(tf)], return_counts=True)
    tied = [i for i in range(1, len(values) - 1) if counts[i] >= 2]
    t = float(values[tied[len(tied) // 2]])  # an occurring value with ties, and others on either side
    assert (tf == t).sum() >= 2 and (tf > t).any() and (tf < t).any()
    null = np.isnan(tf)
    for op, mask in ((">", tf > t), (">=", tf >= t), ("<", tf < t), ("<=", tf <= t), ("=", tf == t),
                     ("!=", (tf != t) & ~null)):
        k = c.check([tf_term(N, op, t)], mask)
        assert 0 < k < n, op


# ---- 5. NULLs -----------------------------------------------------------------------------------------------
def test_null_tf_with_and_without_a_null_match_probability(amd):
    n = 5000
    # column 0, level 1: m = u = 0, a NULL match_probability; column 1, level 2: u = 0, match_probability exactly 1,
    # which a table entry of 0.0 turns into 0 / 0: a NULL tf score of a pair whose match_probability is not NULL
    m = [0.3, 0.0, 0.2, 0.3, 0.5]
    u = [0.6, 0.0, 0.5, 0.4, 0.0]
    c = CtxCase(n, [2, 3], seed=6, m=m, u=u, id_hi=6, sizes=(6,))
    N, tf, mp = c.N, c.tf, c.mp
    null = np.isnan(tf)
    both = null & np.isnan(mp)
    tf_only = null & ~np.isnan(mp)
    assert both.any() and tf_only.any() and (mp[tf_only] == 1.0).all() and (c.adj[tf_only, 0] == 0.0).all()
    assert 0 < null.sum() < n
    t = float(np.sort(tf[~null])[(~null).sum() // 2])  # an occurring value
    for op, mask in ((">", tf > t), (">=", tf >= t), ("<", tf < t), ("<=", tf <= t), ("=", tf == t),
                     ("!=", (tf != t) & ~null)):
        k = c.check([tf_term(N, op, t)], mask & ~null)
        assert 0 < k < n, op
        assert not np.isnan(c.ctx.select_copy_tf(0, k, 1)[0]).any()
    assert c.check([tf_term(N, "is null")], null) == int(null.sum())
    assert c.check([tf_term(N, "is not null")], ~null) == int((~null).sum())
    k = c.check([tf_term(N, "is null"), (N.SEL_MP, 0, N.SEL_OP["is not null"], 0.0)], tf_only)
    assert k == int(tf_only.sum()) > 0


# ---- 6. no full copy, no interference -----------------------------------------------------------------------
def test_filter_copies_survivors_only(link_tf, monkeypatch):
    """The tf frame is made first (its per-value tables need the device scores); from then on nothing of P elements
    may reach the host: counting and materialising the filtered frame run with every full-copy call set to raise."""
    case = link_tf
    pdf, job = case.pdf, case.job
    tf_frame = case.linker.make_term_frequency_adjustments(case.df_e)
    t = float(midpoints(pdf[TF])[len(midpoints(pdf[TF])) // 2])
    saved = job._pairs_host
    job._pairs_host = None

    def boom(*a, **k):
        raise AssertionError("a full per-pair copy or a per-pair tf pass was requested")
    for name in ("pairs_copy", "gammas_copy", "score", "tf_apply", "tf_apply_columns", "tf_copy"):
        monkeypatch.setattr(job.ctx, name, boom)
    try:
        f = tf_frame.filter(f"{TF} > {t!r}")
        assert f.count() == int((pdf[TF] > t).sum())
        k = check(f, pdf, pdf[TF] > t, tf_frame)
        assert 0 < k < len(pdf)
        assert tf_frame._pair is None  # the frame's own per-pair part never ran
    finally:
        job._pairs_host = saved


def test_select_tf_leaves_scores_tf_and_em_alone(link_tf):
    case = link_tf
    job, df_e, tf_frame, pdf = case.job, case.df_e, case.tf, case.pdf
    df_e.gammas.ensure_codes()
    stats0 = job.em_stats(df_e.lam, df_e.level_probs)
    job.score(df_e.lam, df_e.level_probs, want_host=False)
    cols, tables = tf_frame.dev_cols, tf_frame.tables
    job.ctx.tf_apply_columns(cols, tables, 0, job.n_pairs, want_adj=False, want_host=False)
    before = job.ctx.tf_copy(10, 200)
    assert before.tobytes() == pdf[TF].to_numpy()[10:210].tobytes()
    col = cols[0]
    nv = job.ctx.tf_column_values(col)

    def tf_state():
        scale = job.ctx.tf_scales_column(col, nv)
        limbs, counts = job.ctx.tf_accumulate_column_exact(col, nv, scale)
        return scale.copy(), limbs.copy(), counts.copy()
    state0 = tf_state()
    # a selection under other parameters than the last score's
    other = [([p for p in reversed(m)], [p for p in reversed(u)]) for m, u in df_e.level_probs]
    m, u = job.flat_tables(other)
    from splink_amd import _native as N
    k = job.ctx.select_tf_columns(0.123, 1 - 0.123, m, u, cols, tables, [tf_term(N, ">", 0.5)])
    assert 0 <= k <= job.n_pairs
    job.selection_owner = None
    assert job.ctx.tf_copy(10, 200).tobytes() == before.tobytes()
    for a, b in zip(state0, tf_state()):
        assert np.array_equal(a, b)
    t = float(midpoints(pdf[TF])[3])
    assert 0 < tf_frame.filter(f"{TF} < {t!r}").count() < len(pdf)
    assert np.array_equal(stats0, job.em_stats(df_e.lam, df_e.level_probs), equal_nan=True)
    tf1 = case.linker.make_term_frequency_adjustments(df_e).toPandas()
    pd.testing.assert_frame_equal(tf1, pdf, check_exact=True)
    pd.testing.assert_frame_equal(tf_frame.toPandas(), pdf, check_exact=True)


# ---- 7. clusters --------------------------------------------------------------------------------------------
def expected_clusters(case, kept):
    job, uid = case.job, case.linker.settings["unique_id_column_name"]
    if job.link_type == "link_only":
        ids = [("left", x) for x in job.inputs[0][uid]] + [("right", x) for x in job.inputs[1][uid]]
        l = [("left", x) for x in kept[uid + "_l"]]
        r = [("right", x) for x in kept[uid + "_r"]]
    else:
        ids = [("", x) for x in job.inputs[0][uid]]
        l = [("", x) for x in kept[uid + "_l"]]
        r = [("", x) for x in kept[uid + "_r"]]
    pos = {key: i for i, key in enumerate(ids)}
    assert len(pos) == len(ids)
    data = {"cluster_id": union_find(len(ids), [pos[x] for x in l], [pos[x] for x in r]),
            uid: pd.concat([t[uid] for t in job.inputs], ignore_index=True)}
    if job.link_type != "dedupe_only":
        data["_source_table"] = np.array([key[0] for key in ids], dtype=object)
    return pd.DataFrame(data)


@pytest.mark.parametrize("which", ["link_tf", "two_tf"])
def test_clusters_match_union_find(which, request):
    case = request.getfixturevalue(which)
    pdf = case.pdf
    mids = midpoints(pdf[TF])
    t = float(mids[(2 * len(mids)) // 3])
    kept = pdf[pdf[TF] > t]
    assert 0 < len(kept) < len(pdf)
    exp = expected_clusters(case, kept)
    cf = case.tf.clusters(t)
    got = cf.toPandas()
    pd.testing.assert_frame_equal(got, exp, check_exact=True)
    assert cf.n_clusters == exp["cluster_id"].nunique() < len(exp)
    first = got.reset_index().groupby("cluster_id")["index"].min()
    assert (first.index.to_numpy() == first.to_numpy()).all()  # the label is the smallest input position
    same = case.tf.filter(f"{TF} > {t!r}").clusters().toPandas()
    pd.testing.assert_frame_equal(same, exp, check_exact=True)


# ---- 8. ownership -------------------------------------------------------------------------------------------
def test_tf_filtered_frame_reselects_after_losing_the_selection_and_the_codes(two_tf, amd):
    from splink_amd.frames import GammaFrame
    from splink_amd.params import Params
    from splink_amd.synthetic import cfg_settings
    case = two_tf
    pdf, job, df_e = case.pdf, case.job, case.df_e
    t = float(midpoints(pdf[TF])[len(midpoints(pdf[TF])) // 2])
    f = case.tf.filter(f"{TF} > {t!r} and gamma_dob >= 0")
    mask = (pdf[TF] > t) & (pdf["gamma_dob"] >= 0)
    n1 = f.count()
    assert n1 == int(mask.sum()) and job.selection_owner is f
    # another frame's filter takes the context's selection
    s = float(midpoints(pdf[MP])[2])
    other = df_e.filter(f"{MP} > {s!r}")
    assert other.count() == int((pdf[MP] > s).sum()) and job.selection_owner is other
    # and a second program's codes are installed over the frame's
    s2 = cfg_settings(2)
    s2["comparison_columns"] = [s2["comparison_columns"][i] for i in (4, 0, 3)]
    gf2 = GammaFrame(job, Params(s2, amd).settings)
    assert job.codes_token is gf2.token
    k = check(f, pdf, mask, case.tf)
    assert k == n1 and 0 < k < len(pdf)
    assert job.codes_token is df_e.gammas.token and job.selection_owner is f
    check(other, df_e.toPandas(), pdf[MP] > s, df_e)


# ---- 9. ABI states ------------------------------------------------------------------------------------------
def test_abi_states(amd):
    c = CtxCase(5000, [2, 3], seed=11)
    N, ctx, tf = c.N, c.ctx, c.tf
    t = float(np.nanmedian(tf))
    term = tf_term(N, ">", t)
    lam, om = c.lam, 1 - c.lam
    # plain select keeps rejecting the tf field
    with pytest.raises(ValueError, match="unknown field"):
        ctx.select(lam, om, c.m, c.u, [term])
    assert ctx.select_info()[0] == -1
    # a context made from a gamma table has no rows to look the value ids up with
    gt = N.Context(0)
    gt.gammas_load([2, 3], c.g)
    with pytest.raises(RuntimeError, match="pair rows"):
        gt.select_tf(lam, om, c.m, c.u, c.ids0, c.ids1, c.tables, [term])
    # 1..8 tf columns; m and u are required
    with pytest.raises(ValueError, match="1..8 columns"):
        ctx.select_tf(lam, om, c.m, c.u, [], [], [], [])
    with pytest.raises(ValueError, match="1..8 columns"):
        ctx.select_tf(lam, om, c.m, c.u, c.ids0[:1] * 9, c.ids1[:1] * 9, c.tables[:1] * 9, [term])
    with pytest.raises(ValueError, match="1..8 columns"):
        ctx.select_tf_columns(lam, om, c.m, c.u, [], [], [term])
    # select_copy_tf needs a selection made with tables
    k0 = ctx.select(lam, om, c.m, c.u, [(N.SEL_MP, 0, N.SEL_OP[">"], 0.5)])
    assert k0 == int((c.mp > 0.5).sum())
    with pytest.raises(RuntimeError, match="without tf tables"):
        ctx.select_copy_tf(0, 1, 2)
    # a failing call leaves no selection
    k = c.check([term], tf > t)
    assert 0 < k < c.n and ctx.select_info() == (k, -1.0)
    with pytest.raises(ValueError):
        c.select([term] * 9)
    assert ctx.select_info()[0] == -1
    with pytest.raises(RuntimeError):
        ctx.select_copy_tf(0, 1, 2)
    with pytest.raises(ValueError):
        c.select([(N.SEL_TF_MP, 0, 8, 0.5)])
    # eight terms of all three fields
    eight = [term, tf_term(N, "is not null"), (N.SEL_MP, 0, N.SEL_OP[">="], 0.0), (N.SEL_GAMMA, 0, N.SEL_OP[">="], -1.0)] * 2
    assert c.check(eight, tf > t) == k
    # ranges, and a stale selection
    part_tf, part_adj = ctx.select_copy_tf(7, 100, 2)
    want = np.nonzero(tf > t)[0][7:107]
    assert part_tf.tobytes() == tf[want].tobytes() and part_adj.tobytes() == c.adj[want].tobytes()
    assert ctx.select_copy_tf(7, 100, 2, adj=False)[1] is None
    with pytest.raises(ValueError):
        ctx.select_copy_tf(k - 1, 2, 2)
    # the survivors' tf buffers are counted with the EM / score / tf state, and the total stays the sum
    mem = ctx.memory()
    ctx.select_release()
    rel = ctx.memory()
    assert mem["em_score_tf"] - rel["em_score_tf"] >= (8 + 8 * 2) * k
    for x in (mem, rel):
        assert x["total"] == sum(v for key, v in x.items() if key != "total")
    with pytest.raises(RuntimeError):
        ctx.select_copy_tf(0, 1, 2)
    # timing covers the new kernels
    ctx.enable_timing(True)
    assert c.select([term]) == k
    assert ctx.select_info()[1] >= 0.0
    ctx.enable_timing(False)
    ctx.pairs_load(c.rows_l, c.rows_r)
    with pytest.raises(RuntimeError):
        ctx.select_copy_tf(0, 1, 2)
