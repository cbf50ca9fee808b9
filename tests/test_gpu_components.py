"""frame.clusters() on the device (spk_components): label[v] is the smallest node id of v's component.

Expected values come from the union-find below (path halving, link to the smaller id); every comparison is exact.
The ABI cases hand spk_components_edges graphs no EM job would produce; the pipeline cases compare
df_e.filter(cond).clusters().toPandas() with the union-find over the unique ids of df_e.filter(cond).toPandas()."""
import copy
import importlib.util
import os
import warnings

import numpy as np
import pandas as pd
import pytest

from conftest import ROOT, load_golden

pytestmark = pytest.mark.gpu
warnings.filterwarnings("ignore")


@pytest.fixture(scope="module")
def amd():
    from splink_amd import AmdSession, _native
    if _native.device_count() == 0:
        pytest.fail("no HIP device visible: the -m gpu tests need an MI355X")
    return AmdSession(0)


@pytest.fixture(scope="module")
def ctx(amd):
    from splink_amd import _native as N
    return N.Context(0)


@pytest.fixture(scope="module")
def graphs():
    """The graphs of tools/emulate_components.py (the host emulation counts its rounds on these very graphs)."""
    spec = importlib.util.spec_from_file_location("emulate_components", os.path.join(ROOT, "tools", "emulate_components.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def union_find(n_nodes, u, v):
    """label[x] = the smallest id of x's component: find with path halving, link to the smaller id."""
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
    return np.array([find(x) for x in range(n_nodes)], dtype=np.uint32)


def run_edges(ctx, n, u, v):
    """components_edges, every label, and the bookkeeping: (labels, rounds)."""
    want = union_find(n, u, v)
    n_clusters, rounds = ctx.components_edges(n, u, v)
    got = ctx.components_copy(0, n)
    assert got.dtype == np.uint32 and np.array_equal(got, want)
    assert n_clusters == int(np.count_nonzero(want == np.arange(n)))
    assert ctx.components_info()[:3] == (n, len(u), rounds)
    return got, rounds


# ---- 1. degenerate shapes -----------------------------------------------------------------------------------
def test_degenerate_shapes(ctx):
    none = np.empty(0, dtype=np.uint32)
    assert ctx.components_edges(0, none, none) == (0, 0)
    assert len(ctx.components_copy(0, 0)) == 0 and ctx.components_info()[:3] == (0, 0, 0)
    got, rounds = run_edges(ctx, 5, none, none)
    assert np.array_equal(got, np.arange(5)) and rounds == 0
    got, _ = run_edges(ctx, 5, [3], [1])
    assert got.tolist() == [0, 1, 2, 1, 4]
    got, _ = run_edges(ctx, 5, [2], [2])  # a self-loop
    assert got.tolist() == [0, 1, 2, 3, 4]
    u = np.array([4, 2] * 500, dtype=np.uint32)  # one edge 1,000 times, both orientations
    got, _ = run_edges(ctx, 5, u, u[::-1].copy())
    assert got.tolist() == [0, 1, 2, 3, 2]


# ---- 2. lane, wave and workgroup edges ----------------------------------------------------------------------
def _edge_counts():
    from splink_amd import _native
    C = _native.COMPONENTS_CHUNK
    return [1, 63, 64, 65, 255, 256, 257, C - 1, C, C + 1, 3 * C + 17]


@pytest.mark.parametrize("m", _edge_counts())
def test_lane_wave_and_workgroup_edges(m, ctx):
    n = 4096
    rng = np.random.Generator(np.random.PCG64(m))
    u = rng.integers(0, n, m).astype(np.uint32)
    v = rng.integers(0, n, m).astype(np.uint32)
    got, _ = run_edges(ctx, n, u, v)
    for start, count in ((1, 63), (65, 257), (n - 33, 33), (1023, 2049)):  # odd offsets into the labels
        assert np.array_equal(ctx.components_copy(start, count), got[start:start + count])
    with pytest.raises(ValueError):
        ctx.components_copy(n - 1, 2)


# ---- 3. long path -------------------------------------------------------------------------------------------
def test_long_path_takes_logarithmic_rounds(ctx, graphs):
    n, u, v = graphs.path_graph()
    assert n == 65536 and len(u) == n - 1
    got, rounds = run_edges(ctx, n, u, v)
    assert (got == 0).all()
    print("long path: rounds", rounds)
    assert rounds <= 256  # 16 log2(n): label propagation needs ~6e4 rounds here, pointer jumping tens


# ---- 4. hub contention --------------------------------------------------------------------------------------
def test_hub_contention(ctx, graphs):
    n, u, v = graphs.hub_graph()
    hub = n - 1
    assert np.count_nonzero(u == hub) == 20000 and len(u) == 20000 + 32640
    got, rounds = run_edges(ctx, n, u, v)
    assert np.array_equal(got[:1000], np.arange(1000))          # the untouched nodes
    assert (got[1000:1256] == 1000).all()                        # the clique
    assert (got[1256:] == 1256).all() and got[hub] == 1256       # the star: its hub has the largest id
    print("hub: rounds", rounds)


# ---- 5. random forest of sizes ------------------------------------------------------------------------------
def test_random_graph_twice_bit_identical(ctx, graphs):
    n, u, v = graphs.random_graph()
    assert n == 200000 and len(u) == 150000
    first, r1 = run_edges(ctx, n, u, v)
    second, r2 = run_edges(ctx, n, u, v)
    assert first.tobytes() == second.tobytes()
    sizes = np.bincount(first)
    assert sizes.max() >= 3 and np.count_nonzero(sizes == 1) > 0
    print("random: rounds", r1, r2)


# ---- 6. ids past 2^31 ---------------------------------------------------------------------------------------
def test_ids_past_two_to_the_31(ctx):
    """The smallest shape that catches a signed 32-bit id or index; the label array takes about 8.6 GB."""
    B = 1 << 31
    n = B + 16
    u = np.array([B + 5, B + 5, 7], dtype=np.uint32)
    v = np.array([3, B + 9, 8], dtype=np.uint32)
    n_clusters, rounds = ctx.components_edges(n, u, v)  # an allocation failure raises: the test fails, it does not skip
    assert ctx.memory()["em_score_tf"] >= 4 * n
    low, high = ctx.components_copy(0, 16), ctx.components_copy(B, 16)
    want_low, want_high = np.arange(16, dtype=np.uint32), np.arange(B, B + 16, dtype=np.uint32)
    want_low[8] = 7
    want_high[5] = want_high[9] = 3
    assert np.array_equal(low, want_low) and np.array_equal(high, want_high)
    assert n_clusters == n - 3 and ctx.components_info()[:2] == (n, 3)
    ctx.components_release()
    assert ctx.memory()["em_score_tf"] < 4 * n


# ---- 7. invalid ids -----------------------------------------------------------------------------------------
def test_invalid_ids_leave_no_components(ctx):
    run_edges(ctx, 10, [1], [2])
    for u, v in (([1, 10], [2, 3]), ([1, 2], [2, 0xFFFFFFFF]), ([10] * 3000, [0] * 3000)):
        with pytest.raises(ValueError, match="n_nodes"):
            ctx.components_edges(10, np.array(u, dtype=np.uint32), np.array(v, dtype=np.uint32))
        assert ctx.components_info() == (-1, -1, -1, -1.0)
        with pytest.raises(RuntimeError):
            ctx.components_copy(0, 1)
    with pytest.raises(ValueError):
        ctx.components_edges((1 << 32), np.empty(0, dtype=np.uint32), np.empty(0, dtype=np.uint32))


# ---- 8. state -----------------------------------------------------------------------------------------------
def test_abi_states(amd):
    from splink_amd import _native as N
    c = N.Context(0)
    rng = np.random.Generator(np.random.PCG64(8))
    n_rows, n, levels = 300, 5000, [2, 3]
    g = np.stack([rng.integers(-1, L, n) for L in levels], axis=1).astype(np.int8)
    rows_l = rng.integers(0, n_rows, n).astype(np.int32)
    rows_r = rng.integers(0, n_rows, n).astype(np.int32)
    eq1 = (N.SEL_GAMMA, 1, N.SEL_OP["="], 1.0)
    with pytest.raises(RuntimeError, match="no selection"):
        c.components()
    c.gammas_load(levels, g)  # codes without pairs: a selection without rows
    c.select(0.0, 0.0, None, None, [eq1])
    with pytest.raises(RuntimeError, match="pair rows"):
        c.components()
    c.table_create(0, n_rows, 1)
    c.pairs_load(rows_l, rows_r)
    c.gammas_load(levels, g)
    k = c.select(0.0, 0.0, None, None, [eq1])
    keep = g[:, 1] == 1
    want = union_find(n_rows, rows_l[keep], rows_r[keep])
    n_nodes, n_clusters, rounds = c.components()
    assert (n_nodes, n_clusters) == (n_rows, int(np.count_nonzero(want == np.arange(n_rows)))) and rounds >= 1
    assert np.array_equal(c.components_copy(0, n_rows), want)
    assert c.components_info()[:3] == (n_rows, k, rounds) and c.components_info()[3] == -1.0
    # counted with the EM / score / tf state
    mem = c.memory()
    assert mem["total"] == sum(v for key, v in mem.items() if key != "total")
    # a new selection does not reach the labels
    c.select(0.0, 0.0, None, None, [(N.SEL_GAMMA, 0, N.SEL_OP["="], 0.0)])
    assert np.array_equal(c.components_copy(0, n_rows), want)
    c.select_release()
    assert np.array_equal(c.components_copy(3, 100), want[3:103])
    # new codes make the selection stale: no components from it, and the failing call leaves none
    c.select(0.0, 0.0, None, None, [eq1])
    c.gammas_load(levels, g)
    with pytest.raises(RuntimeError, match="changed since spk_select"):
        c.components()
    assert c.components_info()[0] == -1
    # timing, release
    c.enable_timing(True)
    c.select(0.0, 0.0, None, None, [eq1])
    assert c.components()[:2] == (n_nodes, n_clusters) and c.components_info()[3] >= 0.0
    c.enable_timing(False)
    released = c.memory()["em_score_tf"]
    c.components_release()
    assert released - c.memory()["em_score_tf"] >= 4 * n_rows
    with pytest.raises(RuntimeError, match="no components"):
        c.components_copy(0, 1)
    # new tables drop the labels
    c.components_edges(4, np.array([0], dtype=np.uint32), np.array([3], dtype=np.uint32))
    c.table_create(0, n_rows, 1)
    assert c.components_info()[0] == -1


def frame(d):
    return pd.DataFrame(d) if d else None


def scored(g, amd):
    from splink_amd import Splink
    linker = Splink(copy.deepcopy(g["settings_in"]), amd if g["jaro"] else "supress_warnings", df=frame(g.get("df")),
                    df_l=frame(g.get("df_l")), df_r=frame(g.get("df_r")))
    return linker, linker.get_scored_comparisons()


def test_components_leave_scores_tf_em_and_the_selection_alone(amd):
    g = load_golden("link_tf")
    linker, df_e = scored(g, amd)
    job = df_e.job
    pdf = df_e.toPandas()
    t = float(pdf["match_probability"].median())
    tf_col = next(c["col_name"] for c in df_e.settings["comparison_columns"] if c["term_frequency_adjustments"])

    def state(with_components):
        """Select, optionally label, then everything a components call must not have touched."""
        f = df_e.filter(f"match_probability >= {t!r}")
        k = f.count()
        assert 0 < k < len(pdf)
        if with_components:
            n_nodes, n_clusters, _ = job.ctx.components()
            assert 0 < n_clusters < n_nodes
        sel = job.ctx.select_copy(0, k, len(df_e.gammas.meta[0]))
        col = job._col_index[(tf_col, "str")]
        nv = job.ctx.tf_column_values(col)
        scale = job.ctx.tf_scales_column(col, nv)
        limbs, counts = job.ctx.tf_accumulate_column_exact(col, nv, scale)
        tf = linker.make_term_frequency_adjustments(df_e).toPandas()
        stats = job.em_stats(df_e.lam, df_e.level_probs)
        mp = job.score(df_e.lam, df_e.level_probs)
        return list(sel) + [scale.copy(), limbs.copy(), counts.copy(), stats.copy(), mp.copy()], tf
    job.score(df_e.lam, df_e.level_probs, want_host=False)
    plain, tf0 = state(False)
    job.score(df_e.lam, df_e.level_probs, want_host=False)
    job.selection_owner = None  # select again, as the first time
    labelled, tf1 = state(True)
    for a, b in zip(plain, labelled):
        assert np.array_equal(a, b, equal_nan=True)
    pd.testing.assert_frame_equal(tf0, tf1, check_exact=True)


# ---- 9. goldens ---------------------------------------------------------------------------------------------
def golden_case(name):
    return load_golden("link_options")[name[len("link_options/"):]] if name.startswith("link_options/") else load_golden(name)


def midpoints(g):
    """Midpoints between adjacent distinct golden probabilities (the device's rounding cannot move a pair across)."""
    mp = pd.DataFrame(g["df_e"])["match_probability"].astype(float)
    distinct = np.sort(mp.dropna().unique())
    assert len(distinct) >= 2
    return (distinct[:-1] + distinct[1:]) / 2


def expected_clusters(job, settings, kept):
    """The cluster frame from the kept pairs' unique ids: union-find over (source table, unique id)."""
    uid = settings["unique_id_column_name"]
    lt = job.link_type
    if lt == "link_only":
        ids = [("left", x) for x in job.inputs[0][uid]] + [("right", x) for x in job.inputs[1][uid]]
        l = [("left", x) for x in kept[uid + "_l"]]
        r = [("right", x) for x in kept[uid + "_r"]]
    elif lt == "link_and_dedupe":
        ids = list(zip(job.inputs[0]["_source_table"], job.inputs[0][uid]))
        l = list(zip(kept["_source_table_l"], kept[uid + "_l"]))
        r = list(zip(kept["_source_table_r"], kept[uid + "_r"]))
    else:
        ids = [("", x) for x in job.inputs[0][uid]]
        l = [("", x) for x in kept[uid + "_l"]]
        r = [("", x) for x in kept[uid + "_r"]]
    pos = {k: i for i, k in enumerate(ids)}
    assert len(pos) == len(ids)
    label = union_find(len(ids), [pos[k] for k in l], [pos[k] for k in r])
    data = {"cluster_id": label.astype(np.int64),
            uid: pd.concat([t[uid] for t in job.inputs], ignore_index=True)}
    if lt != "dedupe_only":
        data["_source_table"] = np.array([k[0] for k in ids], dtype=object)
    return pd.DataFrame(data)


def check_clusters(df_e, cond):
    """filter(cond).clusters() against the union-find over filter(cond).toPandas(); returns the cluster sizes."""
    from splink_amd import ClusterFrame
    f = df_e.filter(cond)
    kept = f.toPandas()
    job = df_e.job
    exp = expected_clusters(job, df_e.settings, kept)
    cf = f.clusters()
    assert isinstance(cf, ClusterFrame)
    got = cf.toPandas()
    uid = df_e.settings["unique_id_column_name"]
    assert list(got.columns) == ["cluster_id", uid] + (["_source_table"] if job.link_type != "dedupe_only" else [])
    assert got["cluster_id"].dtype == np.int64 and cf.columns == list(got.columns)
    pd.testing.assert_frame_equal(got, exp, check_exact=True)
    assert list(got.dtypes) == list(exp.dtypes)
    n = sum(len(t) for t in job.inputs)
    assert cf.count() == len(cf) == len(got) == n
    # cluster_id is the smallest input position of the cluster, and the partition is the union-find's
    first = got.reset_index().groupby("cluster_id")["index"].min()
    assert (first.index.to_numpy() == first.to_numpy()).all()
    sizes = np.bincount(got["cluster_id"].to_numpy(), minlength=n)
    assert cf.n_clusters == int(np.count_nonzero(sizes)) == exp["cluster_id"].nunique()
    assert cf.rounds >= (1 if len(kept) else 0)
    many = got[sizes[got["cluster_id"].to_numpy()] > 1].reset_index(drop=True)
    pd.testing.assert_frame_equal(cf.toPandas(singletons=False), many, check_exact=True)
    return sizes[sizes > 0]


@pytest.mark.parametrize("name", ["synthetic_cfg1", "link_options/link_only_plain_rules",
                                  "link_options/link_and_dedupe_repeat_rules"])
def test_pipeline_clusters_match_union_find(name, amd):
    g = golden_case(name)
    mids = midpoints(g)
    _, df_e = scored(g, amd)
    t = float(mids[len(mids) // 2])
    if name == "synthetic_cfg1":
        sizes = check_clusters(df_e, f"match_probability > {t!r}")
        n = len(g["df"]["unique_id"])
        assert df_e.filter(f"match_probability > {t!r}").count() == 462
        assert n == 1000 and sizes.sum() == n and sizes.max() == 10
        assert np.count_nonzero(sizes > 1) == 132 and np.count_nonzero(sizes >= 3) > 0 and np.count_nonzero(sizes == 1) > 0
    elif "link_and_dedupe" in name:
        t = float(mids[0])
        sizes = check_clusters(df_e, f"match_probability > {t!r}")
        assert sorted(sizes[sizes > 1].tolist()) == [3, 3]
    else:
        sizes = check_clusters(df_e, f"match_probability > {t!r}")
        assert sorted(sizes[sizes > 1].tolist()) == [2, 2]
        got = df_e.clusters(t).toPandas()
        n0 = len(df_e.job.inputs[0])
        assert (got["_source_table"][:n0] == "left").all() and (got["_source_table"][n0:] == "right").all()
        linked = got[got["_source_table"] == "right"]
        assert (linked["cluster_id"] < n0).sum() == 2  # the right rows' clusters are named by their left rows
    # the shorthand gives the same frame
    pd.testing.assert_frame_equal(df_e.clusters(t).toPandas(), df_e.filter(f"match_probability > {t!r}").clusters().toPandas(),
                                  check_exact=True)
    # every pair and no pair
    every = df_e.filter("match_probability >= 0").clusters()
    assert every.n_clusters <= every.count()
    none = df_e.filter("match_probability > 2").clusters()
    assert none.n_clusters == none.count() and none.rounds == 0 and len(none.toPandas(singletons=False)) == 0


# ---- 10. link_only at some size -----------------------------------------------------------------------------
def synthetic_tables(n, seed):
    from splink_amd.synthetic import make_records
    df = make_records(n, seed=seed, surname_vocab=120, first_vocab=80, city_vocab=20)[
        ["unique_id", "first_name", "surname", "dob", "city", "email"]]
    return df


def scored_job(amd, link_type, tables, cluster=True, shard=(0, 1)):
    from splink_amd.engine import Job
    from splink_amd.frames import ExpectationFrame, GammaFrame
    from splink_amd.params import Params
    from splink_amd.synthetic import cfg_settings
    s = cfg_settings(2)
    s["link_type"] = link_type
    params = Params(s, amd)
    st = params.settings
    job = Job(link_type, tables, "unique_id", 0, shard=shard, cluster=cluster)
    job.block(st["blocking_rules"])
    return ExpectationFrame(GammaFrame(job, st), st, params.params["λ"], params._level_probabilities())


def test_link_only_with_permuted_tables(amd):
    df = synthetic_tables(4000, seed=10)
    rng = np.random.Generator(np.random.PCG64(10))
    side = rng.random(len(df)) < 0.5  # copies of one entity fall on both sides
    left = df[side].sample(frac=1.0, random_state=1).reset_index(drop=True)
    right = df[~side].sample(frac=1.0, random_state=2).reset_index(drop=True)
    assert min(len(left), len(right)) > 1800
    df_e = scored_job(amd, "link_only", [left, right])
    job = df_e.job
    for p in job.perm:
        assert p is not None and not np.array_equal(p, np.arange(len(p)))
    pdf = df_e.toPandas()
    t = float(np.quantile(pdf["match_probability"], 0.9))
    sizes = check_clusters(df_e, f"match_probability > {t!r}")
    assert np.count_nonzero(sizes > 1) > 50 and np.count_nonzero(sizes == 1) > 0


# ---- 11. permutation independence ---------------------------------------------------------------------------
def test_clusters_do_not_depend_on_the_row_permutation(amd):
    df = synthetic_tables(3000, seed=11)
    a = scored_job(amd, "dedupe_only", [df], cluster=True)
    b = scored_job(amd, "dedupe_only", [df], cluster=False)
    assert a.job.perm[0] is not None and b.job.perm[0] is None
    t = float(np.quantile(a.toPandas()["match_probability"], 0.8))
    ca, cb = a.clusters(t), b.clusters(t)
    pd.testing.assert_frame_equal(ca.toPandas(), cb.toPandas(), check_exact=True)
    assert ca.n_clusters == cb.n_clusters < ca.count()
    sizes = check_clusters(a, f"match_probability > {t!r}")
    assert sizes.max() >= 3


# ---- 12. refusals -------------------------------------------------------------------------------------------
def test_refusals(amd):
    from splink_amd.expectation_step import run_expectation_step
    from splink_amd.maximisation_step import run_maximisation_step
    from splink_amd.params import Params
    data = {"unique_id_l": np.arange(50), "unique_id_r": np.arange(50) + 1,
            "gamma_c0": np.arange(50) % 3 - 1}
    settings = {"link_type": "dedupe_only", "blocking_rules": [], "comparison_columns": [{"col_name": "c0", "num_levels": 2}]}
    params = Params(settings, "supress_warnings")
    table_e = run_expectation_step(pd.DataFrame(data), params, params.settings, amd)
    with pytest.raises(ValueError, match="gamma table"):
        table_e.clusters(0.5)
    with pytest.raises(ValueError, match="gamma table"):
        table_e.filter("gamma_c0 = 1").clusters()
    df = synthetic_tables(1500, seed=12)
    sharded = scored_job(amd, "dedupe_only", [df], shard=(0, 2))
    with pytest.raises(ValueError, match="shards"):
        sharded.clusters(0.5)
    whole = scored_job(amd, "dedupe_only", [df])
    cf = whole.clusters(0.5)
    with pytest.raises(ValueError, match="cluster frame"):
        run_maximisation_step(cf, params, amd)
