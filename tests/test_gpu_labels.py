"""Pairs against labels on the device (spk_label_histogram) and the frames above it.

Hand-made contexts compare the counts with np.bincount(state * n_patterns + code); the pipelines compare
label_counts() / truth_table() / estimate_from_labels() with the group-by of df_e.toPandas() with the label column
retained, the only route there was before.  Every comparison is exact."""
import ctypes
import socket
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
warnings.filterwarnings("ignore")

MP = "match_probability"
LAM = 0.3
STEP = 512 * 8  # pairs one workgroup takes per step (LH_THREADS x LH_PAIRS in csrc/spk_labels.hip)


@pytest.fixture(scope="module")
def amd():
    from splink_amd import AmdSession, _native
    if _native.device_count() == 0:
        pytest.fail("no HIP device visible: the -m gpu tests need an MI355X")
    return AmdSession(0)


def make_ctx(rows_l, rows_r, g, levels, n0, n1=None):
    """A context with loaded pairs and levels, as test_gpu_best_matches.py::make_ctx makes one; n1: link_only."""
    from splink_amd import _native as N
    c = N.Context(0)
    if n1 is not None:
        c.set_link_type(N.LINK_TYPES["link_only"])
        c.table_create(1, n1, 1)
    c.table_create(0, n0, 1)
    c.pairs_load(np.asarray(rows_l, dtype=np.int32), np.asarray(rows_r, dtype=np.int32))
    c.gammas_load(levels, np.asarray(g, dtype=np.int8).reshape(len(rows_l), len(levels)))
    return c


def n_patterns(levels):
    return int(np.prod([L + 1 for L in levels]))


def codes_of(g, levels):
    stride = np.cumprod([1] + [L + 1 for L in levels[:-1]])
    return ((np.asarray(g, dtype=np.int64) + 1) * stride).sum(axis=1)


def expected(rows_l, rows_r, g, levels, ids0, ids1=None):
    a = np.asarray(ids0)[rows_l]
    b = np.asarray(ids0 if ids1 is None else ids1)[rows_r]
    state = np.where((a < 0) | (b < 0), 2, (a == b).astype(np.int64))
    n_pat = n_patterns(levels)
    return np.bincount(state * n_pat + codes_of(g, levels), minlength=3 * n_pat).reshape(3, n_pat)


def takes_lds(c, levels):
    """The variant the library takes for this pattern space: LDS counters iff 3 x n_patterns words fit the budget."""
    from splink_amd import _native as N
    return 3 * n_patterns(levels) * 4 <= min(N.LABEL_LDS_BYTES, c.lds_per_block())


def random_case(rng, P, levels, n0, n1=None, groups=40, nulls=0.15):
    rows_l = rng.integers(0, n0, P)
    rows_r = rng.integers(0, n0 if n1 is None else n1, P)
    g = np.stack([rng.integers(-1, L, P) for L in levels], axis=1) if P else np.zeros((0, len(levels)), np.int64)
    ids0 = rng.integers(0, groups, n0).astype(np.int64)
    ids0[rng.random(n0) < nulls] = -rng.integers(1, 1 << 40)  # any negative id is NULL
    ids1 = None
    if n1 is not None:
        ids1 = rng.integers(0, groups, n1).astype(np.int64)
        ids1[rng.random(n1) < nulls] = -1
    return rows_l, rows_r, g, ids0, ids1


def m_u(levels, rng):
    tot = sum(levels)
    return rng.random(tot) * 0.9 + 0.05, rng.random(tot) * 0.9 + 0.05


# ---- 1. pair counts: tail, vector path, partial wave, several workgroups, the grid-stride loop --------------
@pytest.mark.parametrize("P", [0, 1, 63, 64, 65, 8 * 64 + 5, 8 * 1500 + 5, 3 * STEP, 8 * (1024 * 512 + 37) + 5])
def test_pair_counts_against_bincount(P, amd):
    levels = [2, 3]
    rng = np.random.Generator(np.random.PCG64(P))
    rows_l, rows_r, g, ids0, _ = random_case(rng, P, levels, 97)
    c = make_ctx(rows_l, rows_r, g, levels, 97)
    assert takes_lds(c, levels) and c.label_info() == (-1, -1.0)
    counts, mp = c.label_histogram(ids0)
    assert mp is None and counts.dtype == np.int64 and counts.shape == (3, 12)
    assert np.array_equal(counts, expected(rows_l, rows_r, g, levels, ids0))
    assert counts.sum() == P and c.label_info() == (P, -1.0)
    c.close()


# ---- 2. pattern spaces: LDS counters, global counters, 32-bit codes; link_only and one table ---------------
@pytest.mark.parametrize("two", [False, True], ids=["one_table", "link_only"])
@pytest.mark.parametrize("levels,lds", [([2, 3], True), ([5] * 4, True), ([3] * 7, False), ([4] * 7, False)],
                         ids=["12", "1296", "16384", "78125"])
def test_pattern_spaces_and_identities(levels, lds, two, amd):
    rng = np.random.Generator(np.random.PCG64(len(levels) * 10 + two))
    P, n0, n1 = 8 * 700 + 3, 211, (157 if two else None)
    rows_l, rows_r, g, ids0, ids1 = random_case(rng, P, levels, n0, n1)
    c = make_ctx(rows_l, rows_r, g, levels, n0, n1)
    n_pat = n_patterns(levels)
    assert c.n_patterns() == n_pat and takes_lds(c, levels) == lds
    m, u = m_u(levels, rng)
    if len(levels) == 2:
        u[0] = 0.0
        m[0] = 0.0  # patterns whose only non-null level is this one: 0 / 0, a NULL score
    c.enable_timing(True)
    counts, mp = c.label_histogram(ids0, ids1, LAM, 1 - LAM, m, u)
    pairs, ms = c.label_info()
    assert pairs == P and ms > 0.0
    assert np.array_equal(counts, expected(rows_l, rows_r, g, levels, ids0, ids1))
    # the three states sum to the EM histogram, bin for bin
    import torch
    hist = torch.zeros(n_pat, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    c.em_histogram(hist.data_ptr())
    assert np.array_equal(counts.sum(axis=0), hist.cpu().numpy())
    # mp per pattern is spk_score's value of every pair, bit for bit (NaN with NaN)
    score = c.score(LAM, 1 - LAM, m, u, 0, P)
    assert np.array_equal(mp[codes_of(g, levels)], score, equal_nan=True)
    assert len(levels) != 2 or np.isnan(score).any()
    # without m / u: the same counts, no scores
    again, none = c.label_histogram(ids0, ids1)
    assert none is None and np.array_equal(again, counts)
    c.close()


# ---- 3. contention and labels --------------------------------------------------------------------------
@pytest.mark.parametrize("levels", [[2, 3], [3] * 7], ids=["lds", "global"])
def test_equal_keys_and_distinct_keys(levels, amd):
    n_pat = n_patterns(levels)
    P = 8 * 600 + 7
    # every pair with one code and one state: 64 equal keys per wave
    g = np.tile(np.array([L - 1 for L in levels]), (P, 1))
    rows = np.arange(P) % 50
    ids = np.full(50, 3, dtype=np.int64)
    c = make_ctx(rows, rows[::-1], g, levels, 50)
    counts, _ = c.label_histogram(ids)
    want = np.zeros((3, n_pat), dtype=np.int64)
    want[1, n_pat - 1] = P
    assert np.array_equal(counts, want)
    c.close()
    # every pair with a key of its own (as far as the space goes): code p mod n_pat, state p // n_pat mod 3
    p = np.arange(P)
    code = p % n_pat
    stride = np.cumprod([1] + [L + 1 for L in levels[:-1]])
    g = np.stack([(code // s) % (L + 1) - 1 for s, L in zip(stride, levels)], axis=1)
    state = (p // n_pat) % 3
    # rows: 0 and 1 carry label 5, 2 label 6, 3 is NULL
    rows_l = np.where(state == 2, 3, 0)
    rows_r = np.where(state == 1, 1, 2)
    ids = np.array([5, 5, 6, -1], dtype=np.int64)
    c = make_ctx(rows_l, rows_r, g, levels, 4)
    counts, _ = c.label_histogram(ids)
    assert np.array_equal(counts, np.bincount(state * n_pat + code, minlength=3 * n_pat).reshape(3, n_pat))
    assert np.array_equal(counts, expected(rows_l, rows_r, g, levels, ids))
    c.close()


def test_null_ids_and_second_id_array(amd):
    levels = [2, 3]
    rng = np.random.Generator(np.random.PCG64(11))
    P, n0, n1 = 8 * 300 + 1, 64, 23
    rows_l, rows_r, g, ids0, ids1 = random_case(rng, P, levels, n0, n1, groups=5, nulls=0.4)
    c = make_ctx(rows_l, rows_r, g, levels, n0, n1)
    a, b = ids0[rows_l], ids1[rows_r]
    assert ((a < 0) & (b < 0)).any() and ((a < 0) & (b >= 0)).any() and ((a >= 0) & (b < 0)).any()
    counts, _ = c.label_histogram(ids0, ids1)
    assert np.array_equal(counts, expected(rows_l, rows_r, g, levels, ids0, ids1))
    with pytest.raises(ValueError):  # link_only without the right table's ids
        c.label_histogram(ids0)
    c.close()
    # one table: ids_side1 = NULL reads the left array for both rows; an explicit second array is honoured
    rows_l, rows_r, g, ids0, _ = random_case(rng, P, levels, n0, groups=5, nulls=0.4)
    other = rng.integers(-1, 5, n0).astype(np.int64)
    c = make_ctx(rows_l, rows_r, g, levels, n0)
    assert np.array_equal(c.label_histogram(ids0)[0], expected(rows_l, rows_r, g, levels, ids0))
    assert np.array_equal(c.label_histogram(ids0, other)[0], expected(rows_l, rows_r, g, levels, ids0, other))
    c.close()


# ---- 4. states and bystanders ------------------------------------------------------------------------------
def test_states_and_errors(amd):
    from splink_amd import _native as N
    levels = [2, 3]
    ids = np.zeros(8, dtype=np.int64)
    c = N.Context(0)
    c.table_create(0, 8, 1)
    with pytest.raises(RuntimeError, match="no gammas"):  # SPK_E_STATE: no codes
        c.label_histogram(ids)
    c.pairs_load(np.arange(4, dtype=np.int32), np.arange(4, dtype=np.int32))
    with pytest.raises(RuntimeError, match="no gammas"):
        c.label_histogram(ids)
    c.close()
    c = N.Context(0)
    c.table_create(0, 8, 1)
    c.gammas_load(levels, np.zeros((4, 2), dtype=np.int8))  # a gamma table: codes without pair rows
    with pytest.raises(RuntimeError, match="no pair rows"):
        c.label_histogram(ids)
    assert c.label_info() == (-1, -1.0)
    c.close()
    rows = np.arange(8)
    c = make_ctx(rows, rows[::-1], np.zeros((8, 2)), levels, 8)
    big = ids.copy()
    big[5] = 1 << 31
    with pytest.raises(ValueError, match="2\\^31"):
        c.label_histogram(big)
    ok = ids.copy()
    ok[5] = (1 << 31) - 1
    assert c.label_histogram(ok)[0].sum() == 8
    out = np.zeros(3 * 12, dtype=np.uint64)
    mp = np.zeros(12)
    with pytest.raises(ValueError):  # scores asked for without m / u (straight at the ABI)
        N.check(c._lib.spk_label_histogram(c._h, N._ptr(ids), N._ptr(None), ctypes.c_double(0.5), ctypes.c_double(0.5),
                                           N._ptr(None), N._ptr(None), N._ptr(out), N._ptr(mp)), "spk_label_histogram")
    with pytest.raises(ValueError):  # NULL out_counts
        N.check(c._lib.spk_label_histogram(c._h, N._ptr(ids), N._ptr(None), ctypes.c_double(0.5), ctypes.c_double(0.5),
                                           N._ptr(None), N._ptr(None), N._ptr(None), N._ptr(None)), "spk_label_histogram")
    c.close()


def test_bystanders_untouched(amd):
    from splink_amd import _native as N
    levels = [2, 3]
    rng = np.random.Generator(np.random.PCG64(5))
    P, n0 = 8 * 200 + 3, 120
    rows_l, rows_r, g, ids0, _ = random_case(rng, P, levels, n0)
    c = make_ctx(rows_l, rows_r, g, levels, n0)
    m, u = m_u(levels, rng)
    c.score(LAM, 1 - LAM, m, u, 0, P, want_host=False)
    k = c.select(LAM, 1 - LAM, m, u, [(N.SEL_MP, 0, N.SEL_OP[">"], 0.4)])
    assert 0 < k < P
    nodes, clusters, _ = c.components()
    tf_ids = rng.integers(0, 7, n0).astype(np.int64)

    def snapshot():
        return (c.select_copy(0, k, 2), c.components_copy(0, nodes), c.tf_accumulate(7, tf_ids, tf_ids),
                c.select_info()[0], c.components_info()[:2])

    before = snapshot()
    mem = c.memory()
    m2, u2 = m_u(levels, rng)  # other parameters than the selection's and the scores'
    counts, mp = c.label_histogram(ids0, None, 0.6, 0.4, m2, u2)
    assert np.array_equal(counts, expected(rows_l, rows_r, g, levels, ids0))
    assert c.memory() == mem  # the call's buffers are gone
    after = snapshot()
    for x, y in zip(before[:3], after[:3]):
        for a, b in zip(x, y) if isinstance(x, tuple) else ((x, y),):
            assert np.array_equal(a, b, equal_nan=True)
    assert before[3:] == after[3:]
    c.close()


# ---- 5. end to end -------------------------------------------------------------------------------------------
def labelled_records(n, seed, nulls=0.05):
    from splink_amd.synthetic import make_records
    df = make_records(n, seed=seed, surname_vocab=120, first_vocab=80, city_vocab=20)[
        ["unique_id", "first_name", "surname", "dob", "city", "email", "cluster"]]
    rng = np.random.Generator(np.random.PCG64(seed))
    df["cluster"] = df["cluster"].astype(np.float64)
    df.loc[rng.random(n) < nulls, "cluster"] = np.nan
    return df


def scored_job(amd, link_type, tables):
    from splink_amd.engine import Job
    from splink_amd.frames import ExpectationFrame, GammaFrame
    from splink_amd.params import Params
    from splink_amd.synthetic import cfg_settings
    s = cfg_settings(2)
    s["link_type"] = link_type
    s["additional_columns_to_retain"] = ["cluster"]
    params = Params(s, amd)
    st = params.settings
    job = Job(link_type, tables, "unique_id", 0)
    job.block(st["blocking_rules"])
    gf = GammaFrame(job, st)
    return params, gf, ExpectationFrame(gf, st, params.params["λ"], params._level_probabilities())


def host_patterns(pdf, names, scored=True):
    """The group-by the device replaces: df_e.toPandas() with the label retained, by gamma columns and truth."""
    a, b = pdf["cluster_l"], pdf["cluster_r"]
    known = a.notna() & b.notna()
    d = pdf[names].copy()
    d["n_match"] = (known & (a == b)).astype(np.int64)
    d["n_non_match"] = (known & (a != b)).astype(np.int64)
    d["n_unlabelled"] = (~known).astype(np.int64)
    agg = {"n_match": "sum", "n_non_match": "sum", "n_unlabelled": "sum"}
    if scored:
        d[MP] = pdf[MP]
        assert (d.groupby(names)[MP].nunique(dropna=False) == 1).all()  # one score per pattern
        agg = {MP: "first", **agg}
    out = d.groupby(names, sort=False).agg(agg).reset_index()
    # ascending code: the first gamma column is the fastest digit
    out = out.sort_values(names[::-1], kind="stable").reset_index(drop=True)
    return out[names + list(agg)]


def restated_params(pdf, params, names):
    """estimate_from_labels in numpy: the M-step with match_probability := (cluster_l == cluster_r)."""
    f32 = lambda x: float(np.float32(x))  # noqa: E731
    a, b = pdf["cluster_l"], pdf["cluster_r"]
    known = (a.notna() & b.notna()).to_numpy()
    y = (a == b).to_numpy() & known
    n = ~y & known
    want = {"λ": f32(y.sum() / known.sum())}
    for name in names:
        g = pdf[name].to_numpy()
        L = params.params["π"][name]["num_levels"]
        den_m, den_u = (y & (g >= 0)).sum(), (n & (g >= 0)).sum()
        for v in range(L):
            at = g == v
            if not (known & at).any():
                pm = pu = 0  # a level never observed stays at 0
            else:
                pm = f32((y & at).sum() / den_m) if den_m else None
                pu = f32((n & at).sum() / den_u) if den_u else None
            want[(name, v)] = (pm, pu)
    return want


def check_pipeline(amd, link_type, tables):
    from splink_amd import LabelCounts, estimate_from_labels
    params, gf, df_e = scored_job(amd, link_type, tables)
    names = list(gf.meta[0])
    pdf = df_e.toPandas()
    lc = df_e.label_counts("cluster")
    assert isinstance(lc, LabelCounts) and lc.link_type == link_type and lc.counts.sum() == len(pdf) == df_e.count()
    got = lc.patterns()
    exp = host_patterns(pdf, names)
    assert list(got.columns) == list(exp.columns)
    for col in got.columns:
        assert np.array_equal(got[col].to_numpy(), exp[col].to_numpy(), equal_nan=True), col
    assert exp["n_match"].sum() > 0 and exp["n_non_match"].sum() > 0 and exp["n_unlabelled"].sum() > 0
    # the unscored frame: the same counts, no scores
    plain = gf.label_counts("cluster")
    assert plain.mp is None and np.array_equal(plain.counts, lc.counts)
    # true pairs: from the inputs' labels
    if link_type == "link_only":
        l, r = tables[0]["cluster"].value_counts(), tables[1]["cluster"].value_counts()
        total = int((l * r.reindex(l.index).fillna(0)).sum())
    else:
        vc = tables[0]["cluster"].value_counts()
        total = int((vc * (vc - 1) // 2).sum())
    assert lc.true_pairs_total == total and lc.missed_by_blocking == total - int(exp["n_match"].sum())
    assert total > 0 and lc.missed_by_blocking >= 0
    # every row of the truth table against the device's own filter
    tt = df_e.truth_table("cluster")
    assert len(tt) == exp[MP].nunique() + 1 and (np.diff(tt["threshold"]) > 0).all()
    for row in tt.itertuples():
        t = float(row.threshold)
        assert row.tp + row.fp + row.n_unlabelled_above == df_e.filter(f"{MP} > {t!r}").count(), t
        assert row.tp + row.fn == exp["n_match"].sum() and row.fp + row.tn == exp["n_non_match"].sum()
    assert tt.iloc[0]["tp"] + tt.iloc[0]["fp"] + tt.iloc[0]["n_unlabelled_above"] == int(pdf[MP].notna().sum())
    picked = df_e.truth_table("cluster", [0.5, 0.99])
    for row in picked.itertuples():
        above = pdf[pdf[MP] > row.threshold]
        known = above["cluster_l"].notna() & above["cluster_r"].notna()
        assert row.tp == int((known & (above["cluster_l"] == above["cluster_r"])).sum())
        assert row.fp == int((known & (above["cluster_l"] != above["cluster_r"])).sum())
    # the supervised estimate
    want = restated_params(pdf, params, names)
    df_e2 = estimate_from_labels(gf, params, params.settings, amd, "cluster")
    assert params.params["λ"] == want["λ"] and params.iteration == 2 and len(params.param_history) == 1
    for name in names:
        d = params.params["π"][name]
        for v in range(d["num_levels"]):
            got_mu = (d["prob_dist_match"][f"level_{v}"]["probability"],
                      d["prob_dist_non_match"][f"level_{v}"]["probability"])
            assert got_mu == want[(name, v)], (name, v)
    assert df_e2.lam == params.params["λ"] and df_e2.level_probs == [
        (list(m), list(u)) for m, u in params._level_probabilities()]
    m, u = gf.job.flat_tables(params._level_probabilities())
    lam = float(params.params["λ"])
    assert np.array_equal(df_e2.toPandas()[MP].to_numpy(), gf.job.ctx.score(lam, float(1 - lam), m, u, 0, len(pdf)),
                          equal_nan=True)
    return gf, lc


def test_pipeline_dedupe_only(amd):
    check_pipeline(amd, "dedupe_only", [labelled_records(3000, seed=3)])


def test_pipeline_link_only(amd):
    df = labelled_records(3000, seed=3)
    left = df.iloc[::2].reset_index(drop=True)
    right = df.iloc[1::2].reset_index(drop=True)
    check_pipeline(amd, "link_only", [left, right])


def test_label_column_forms_and_refusals(amd):
    """String labels with None, and the refusals a frame gives before it reaches the device."""
    from splink_amd import estimate_from_labels
    df = labelled_records(800, seed=9)
    as_text = df.copy()
    as_text["cluster"] = [None if np.isnan(x) else f"c{int(x)}" for x in df["cluster"]]
    _, gf_a, df_a = scored_job(amd, "dedupe_only", [df])
    _, gf_b, df_b = scored_job(amd, "dedupe_only", [as_text])
    a, b = df_a.label_counts("cluster"), df_b.label_counts("cluster")
    assert np.array_equal(a.counts, b.counts) and a.true_pairs_total == b.true_pairs_total
    assert a.counts[2].sum() > 0
    with pytest.raises(ValueError, match="missing from input table 0"):
        df_a.label_counts("truth")
    with pytest.raises(ValueError, match="filtered frame"):
        estimate_from_labels(df_a.filter(f"{MP} > 0.5"), None, {}, amd, "cluster")


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
    """force_reduce, as tests/test_gpu_dist.py sets it for the EM histogram: the counts go through the host
    all-reduce (RCCL, staged through the device) and come back the same."""
    _, gf, df_e = scored_job(amd, "dedupe_only", [labelled_records(1500, seed=5)])
    local = df_e.label_counts("cluster")
    gf.job.force_reduce = True
    reduced = df_e.label_counts("cluster")
    gf.job.force_reduce = False
    assert np.array_equal(local.counts, reduced.counts) and np.array_equal(local.mp, reduced.mp, equal_nan=True)
    assert local.true_pairs_total == reduced.true_pairs_total and local.counts[1].sum() > 0
