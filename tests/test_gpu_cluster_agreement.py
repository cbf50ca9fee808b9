"""Clusters against labels on the device (spk_cluster_agreement) and truth_table() of the cluster frames.

The ABI cases go through components_sweep_edges + cluster_agreement: the expected rows are the pandas oracle of
agreement_common (group sizes, never sorted keys) over the labels the sweep itself returns, and on small cases also
the enumeration.  The pipeline cases compare clusters_at_thresholds(ts).truth_table() with the oracle over
sweep.toPandas(), the only route there was before.  Every comparison is exact."""
import ctypes
import warnings

import numpy as np
import pandas as pd
import pytest

from agreement_common import FIELDS, agreement_brute, agreement_oracle

pytestmark = pytest.mark.gpu
warnings.filterwarnings("ignore")
U32 = np.uint32
F = {name: i for i, name in enumerate(FIELDS)}
AG_THREADS = 1024      # places one workgroup takes per step of the k_ag_* kernels (csrc/spk_agreement.hip)
AG_WG_PER_CU = 2       # their grids are capped at this many workgroups per CU; past the cap the workgroups stride


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


def sweep(ctx, n, u, v, score=None, thr=()):
    """components_sweep_edges and every level's labels, int64 [L, n]."""
    ctx.components_sweep_edges(n, np.asarray(u, dtype=U32), np.asarray(v, dtype=U32), score, list(thr))
    L = max(len(thr), 1)
    return np.stack([ctx.components_sweep_copy(k, 0, n).astype(np.int64) for k in range(L)])


def check(ctx, labels, ids, forms, brute=False):
    """cluster_agreement under every (cross_only, n_left) of `forms` against the oracle on every level's labels."""
    ids = np.asarray(ids, dtype=np.int64)
    rows = []
    for cross, n_left in forms:
        got = ctx.cluster_agreement(ids, n_left, bool(cross))
        assert got.dtype == np.int64 and got.shape == (len(labels), len(FIELDS))
        for k, lab in enumerate(labels):
            want = agreement_oracle(lab, ids, n_left, cross)
            assert np.array_equal(got[k], want), (cross, n_left, k, dict(zip(FIELDS, zip(got[k].tolist(), want.tolist()))))
            if brute:
                assert np.array_equal(got[k], agreement_brute(lab, ids, n_left, cross)), (cross, n_left, k)
        rows.append(got)
    return rows


def forms_of(n):
    return [(0, 0), (1, n // 2), (1, 0), (1, n)]


def random_graph(rng, n, m):
    return rng.integers(0, n, m).astype(U32), rng.integers(0, n, m).astype(U32)


def random_ids(rng, n, groups, n_null):
    """n ids over `groups` values, exactly n_null of them NULL (any negative value)."""
    ids = rng.integers(0, groups, n).astype(np.int64)
    ids[rng.permutation(n)[:n_null]] = -rng.integers(1, 1 << 40, n_null)
    return ids


# ---- 1. degenerate shapes -----------------------------------------------------------------------------------
def test_degenerate_shapes(ctx):
    none = np.empty(0, dtype=U32)
    sweep(ctx, 0, none, none)
    for cross in (False, True):
        assert ctx.cluster_agreement(np.empty(0, np.int64), 0, cross).tolist() == [[0] * 10]
    labels = sweep(ctx, 1, none, none)
    got = check(ctx, labels, [5], [(0, 0), (1, 0), (1, 1)], brute=True)
    assert got[0].tolist() == [[1, 1, 1, 0, 0, 0, 0, 0, 1, 0]]
    check(ctx, labels, [-1], [(0, 0), (1, 1)], brute=True)
    labels = sweep(ctx, 5, none, none)  # no edges
    check(ctx, labels, [3, 3, -1, 4, 3], forms_of(5) + [(1, 1)], brute=True)
    labels = sweep(ctx, 5, [0, 1, 3], [1, 2, 4])
    got = check(ctx, labels, [-1, -7, -1, -(1 << 50), -2], forms_of(5), brute=True)  # every id NULL
    assert all(not g.any() for g in got)
    got = check(ctx, labels, [-1, -1, 2, -1, -1], forms_of(5), brute=True)  # exactly one labelled node
    assert got[0].tolist() == [[1, 1, 1, 0, 0, 0, 0, 0, 1, 0]]


@pytest.mark.parametrize("same_cluster", [False, True])
@pytest.mark.parametrize("same_id", [False, True])
def test_two_labelled_nodes(same_cluster, same_id, ctx):
    # nodes 0 and 3 are labelled; 1 and 2 are not (and lie in their clusters all the same)
    labels = sweep(ctx, 4, [0, 1, 2] if same_cluster else [0, 2], [1, 2, 3] if same_cluster else [1, 3])
    ids = [8, -1, -1, 8 if same_id else 6]
    got = check(ctx, labels, ids, [(0, 0), (1, 2), (1, 4), (1, 0), (1, 3), (1, 1)], brute=True)
    pair = [int(same_cluster), int(same_id), int(same_cluster and same_id)]
    assert got[0][0, [3, 4, 5, 9]].tolist() == pair + [1]          # every pair
    assert got[1][0, [3, 4, 5, 9]].tolist() == pair + [1]          # different sides
    assert got[2][0, [3, 4, 5, 9]].tolist() == [0, 0, 0, 0]        # both left
    assert got[3][0, [3, 4, 5, 9]].tolist() == [0, 0, 0, 0]        # both right
    assert got[0][0, [6, 7, 8]].tolist() == [int(same_cluster and not same_id), int(same_id and not same_cluster),
                                             2 * (not same_cluster and not same_id) + (same_cluster and same_id)]


# ---- 2. boundaries: M labelled nodes around a wave, a workgroup step and its double -------------------------------
@pytest.mark.parametrize("M", [63, 64, 65, 255, 256, 257, AG_THREADS - 1, AG_THREADS, AG_THREADS + 1,
                               2 * AG_THREADS - 1, 2 * AG_THREADS, 2 * AG_THREADS + 1, 5000])
def test_boundaries(M, ctx):
    rng = np.random.Generator(np.random.PCG64(M))
    n = M + M // 4  # a fifth of the nodes NULL
    labels = sweep(ctx, n, *random_graph(rng, n, n // 2))
    ids = random_ids(rng, n, max(2, M // 3), n - M)
    got = check(ctx, labels, ids, forms_of(n) + [(1, n // 3)], brute=M < 300)
    assert got[0][0, F["records_labelled"]] == M
    assert got[0][0, F["clusters_mixed"]] > 0 and got[0][0, F["entities_split"]] > 0


def test_past_the_grid_cap(ctx):
    """More labelled nodes than the capped grid covers in one trip: every workgroup strides."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    M = AG_WG_PER_CU * cus * AG_THREADS + AG_THREADS + 7
    rng = np.random.Generator(np.random.PCG64(2))
    n = M + 1000
    labels = sweep(ctx, n, *random_graph(rng, n, n // 3))
    got = check(ctx, labels, random_ids(rng, n, M // 4, 1000), [(0, 0), (1, n // 2)])
    assert got[0][0, F["records_labelled"]] == M


# ---- 3. extremes of the runs --------------------------------------------------------------------------------------
def test_run_extremes(ctx):
    n = 3 * AG_THREADS + 11
    chain = (np.arange(n - 1, dtype=U32), np.arange(1, n, dtype=U32))
    none = np.empty(0, dtype=U32)
    # one cluster of all nodes, all ids distinct: one cluster run from place 0 to M - 1, n (cluster, id) runs
    one = sweep(ctx, n, *chain)
    got = check(ctx, one, np.arange(n)[::-1].copy(), forms_of(n))
    assert got[0][0].tolist() == [n, 1, n, n * (n - 1) // 2, 0, 0, 1, 0, 0, n * (n - 1) // 2]
    # one cluster, one id: a single run from place 0 to M - 1, recovered
    got = check(ctx, one, np.zeros(n), forms_of(n))
    assert got[0][0, [5, 6, 7, 8]].tolist() == [n * (n - 1) // 2, 0, 0, 1]
    # (cluster, id) runs that straddle the workgroup steps: runs of 100 places (ids by place / 100)
    ids = np.arange(n) // 100
    check(ctx, one, ids, forms_of(n) + [(1, 250)])
    # left nodes that sort entirely before the right nodes of their cluster (left ids below right ids), and entirely after
    n_left = n // 2 + 3
    low_left = np.where(np.arange(n) < n_left, np.arange(n) % 7, 100 + np.arange(n) % 5)
    high_left = np.where(np.arange(n) < n_left, 100 + np.arange(n) % 7, np.arange(n) % 5)
    for ids3 in (low_left, high_left):
        got = check(ctx, one, ids3, [(1, n_left), (0, 0)])
        assert got[0][0, [3, 5]].tolist() == [n_left * (n - n_left), 0]
    # and with ids that both sides share
    check(ctx, one, np.arange(n) % 7, [(1, n_left), (1, 1), (1, n - 1)])
    # all nodes singletons with one id: n cluster runs, one entity
    alone = sweep(ctx, n, none, none)
    got = check(ctx, alone, np.full(n, (1 << 31) - 1), forms_of(n))
    assert got[0][0].tolist() == [n, n, 1, 0, n * (n - 1) // 2, 0, 0, 1, 0, n * (n - 1) // 2]
    # two clusters, cut inside a run of one id
    cut = AG_THREADS + 40
    keep = np.arange(n - 1) != cut - 1
    two = sweep(ctx, n, chain[0][keep], chain[1][keep])
    assert len(np.unique(two)) == 2
    got = check(ctx, two, ids, forms_of(n) + [(1, cut), (1, 250)])
    assert got[0][0, [6, 7]].tolist() == [2, 1]
    # the first and the last node NULL: the runs still start at place 0 and end at M - 1
    ids2 = ids.copy()
    ids2[[0, n - 1]] = -1
    check(ctx, two, ids2, forms_of(n))


# ---- 4. 64-bit sums -----------------------------------------------------------------------------------------------
def test_sums_past_32_bits(ctx):
    n = 200_000
    labels = sweep(ctx, n, np.zeros(n - 1, dtype=U32), np.arange(1, n, dtype=U32))  # one star
    ids = np.arange(n) % 2 + 40
    (all_pairs, across) = check(ctx, labels, ids, [(0, 0), (1, n // 2)])
    h = n // 2
    assert all_pairs[0, [3, 5]].tolist() == [n * (n - 1) // 2, 2 * (h * (h - 1) // 2)]
    assert all_pairs[0, 3] > 1 << 34 and all_pairs[0, 5] > 1 << 33
    assert across[0, [3, 5, 9]].tolist() == [h * h, 2 * (h // 2) ** 2, h * h]
    for cross, n_left in ((False, 0), (True, h)):
        a, b = ctx.cluster_agreement(ids, n_left, cross), ctx.cluster_agreement(ids, n_left, cross)
        assert a.tobytes() == b.tobytes()


# ---- 5. levels ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cross", [0, 1], ids=["all_pairs", "cross_only"])
def test_levels_of_a_random_graph(cross, ctx):
    n, m, h = 200_000, 150_000, 100_000
    rng = np.random.Generator(np.random.PCG64(77))
    # an entity is the nodes {2a, 2a + 1, 2a + h, 2a + 1 + h}, two on each side; a fifth of the ids NULL.  Half the
    # edges join two nodes of one entity, the other half are random.
    ids = (np.arange(n) % h // 2).astype(np.int64)
    ids[rng.permutation(n)[:n // 5]] = -1
    u, v = random_graph(rng, n, m)
    inside = np.arange(m) % 2 == 0
    v[inside] = (u[inside] % h // 2 * 2 + rng.integers(0, 2, m)[inside] + h * rng.integers(0, 2, m)[inside]).astype(U32)
    thr = [0.9, 0.8, 0.7, 0.6, 0.45, 0.3, 0.15, 0.0]
    labels = sweep(ctx, n, u, v, rng.random(m), thr)
    (got,) = check(ctx, labels, ids, [(cross, h + 17)])
    assert (np.diff(got[:, F["tp"]]) >= 0).all() and (np.diff(got[:, F["predicted_pairs"]]) >= 0).all()
    assert got[-1, F["tp"]] > got[0, F["tp"]] > 0
    for f in (0, 2, 4, 9):
        assert (got[:, f] == got[0, f]).all()
    assert (got[:, F["tp"]] <= got[:, F["true_pairs"]]).all()
    assert ctx.cluster_agreement_info()[0] == len(thr)


# ---- 6. arguments and state -----------------------------------------------------------------------------------------
def raw_call(c, ids, n_left, cross, out):
    from splink_amd._native import _ptr
    return c._lib.spk_cluster_agreement(c._h, _ptr(ids), ctypes.c_int64(n_left), ctypes.c_int(cross), _ptr(out))


def test_arguments_and_state(amd):
    from splink_amd import _native as N
    c = N.Context(0)
    assert c.cluster_agreement_info() == (-1, -1.0)
    ids = np.array([1, 1, 2, -1, 2, 0], dtype=np.int64)
    out = np.zeros((2, 10), dtype=np.int64)
    assert raw_call(c, ids, 0, 0, out) == N.SPK_E_STATE  # no sweep
    with pytest.raises(RuntimeError, match="no sweep"):
        c.cluster_agreement(ids)
    # bystanders: the labels of a components call, the sweep, one level's metrics, the memory
    c.components_edges(6, np.array([0, 4], dtype=U32), np.array([5, 5], dtype=U32))
    u, v = np.array([0, 2, 3], dtype=U32), np.array([1, 3, 4], dtype=U32)
    c.components_sweep_edges(6, u, v, np.array([0.9, 0.9, 0.2]), [0.5, 0.1])
    scalars = c.cluster_metrics(1)

    def bystanders():
        return ([c.components_sweep_copy(k, 0, 6).tobytes() for k in range(2)], c.components_copy(0, 6).tobytes(),
                [a.tobytes() for a in c.cluster_metrics_copy(0, 6)], c.cluster_metrics_info()[0],
                c.components_sweep_info()[:3], c.memory())

    before = bystanders()
    assert c.cluster_agreement_info() == (-1, -1.0)
    for bad in (lambda: raw_call(c, None, 0, 0, out), lambda: raw_call(c, ids, 0, 0, None),
                lambda: raw_call(c, ids, -1, 1, out), lambda: raw_call(c, ids, 7, 1, out),
                lambda: raw_call(c, np.array([1, 1, 1 << 31, -1, 2, 0], dtype=np.int64), 0, 0, out)):
        assert bad() == N.SPK_E_INVALID
        assert c.cluster_agreement_info() == (-1, -1.0) and not out.any()
    with pytest.raises(ValueError, match="2\\^31"):
        c.cluster_agreement([0, 0, 0, 0, 0, 1 << 40])
    with pytest.raises(ValueError, match="5 ids for the sweep's 6 nodes"):
        c.cluster_agreement(ids[:5])
    labels = np.stack([c.components_sweep_copy(k, 0, 6).astype(np.int64) for k in range(2)])
    top = ids.copy()
    top[ids == 2] = (1 << 31) - 1  # the largest id there is
    for these in (ids, top):
        got = check(c, labels, these, forms_of(6) + [(1, 6), (1, 2)], brute=True)
        assert c.cluster_agreement_info() == (2, -1.0)  # timing off
    assert got[0][:, F["tp"]].tolist() == [1, 2]
    assert bystanders() == before and c.cluster_metrics(1) == scalars
    # a failing call after a good one leaves the info as it was
    assert raw_call(c, ids, 9, 1, out) == N.SPK_E_INVALID and c.cluster_agreement_info() == (2, -1.0)
    plain = c.cluster_agreement(ids, 3, True)
    c.enable_timing(True)
    families = c.kernel_ms()
    timed = c.cluster_agreement(ids, 3, True)
    levels, ms = c.cluster_agreement_info()
    assert levels == 2 and ms >= 0.0 and np.array_equal(timed, plain)
    assert c.kernel_ms() == families  # the five kernel families are not this stage's
    c.enable_timing(False)
    c.cluster_agreement(ids)
    assert c.cluster_agreement_info() == (2, -1.0) and bystanders() == before
    # a one-level sweep without thresholds, and no sweep again after its release
    c.components_sweep_edges(6, u, v, None, [])
    assert c.cluster_agreement(ids).shape == (1, 10) and c.cluster_agreement_info() == (1, -1.0)
    c.components_sweep_release()
    assert raw_call(c, ids, 0, 0, out) == N.SPK_E_STATE and c.cluster_agreement_info() == (1, -1.0)
    c.close()


# ---- 7. the pipeline ------------------------------------------------------------------------------------------------
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
    params = Params(s, amd)
    st = params.settings
    job = Job(link_type, tables, "unique_id", 0)
    job.block(st["blocking_rules"])
    gf = GammaFrame(job, st)
    return job, ExpectationFrame(gf, st, params.params["λ"], params._level_probabilities())


def same_table(a, b, but=()):
    assert list(a.columns) == list(b.columns) and len(a) == len(b)
    for col in a.columns:
        if col not in but:
            assert a[col].dtype == b[col].dtype, col
            assert np.array_equal(a[col].to_numpy(), b[col].to_numpy(), equal_nan=True), col


def check_pipeline(amd, link_type, tables):
    from splink_amd.labels import cluster_truth_rows
    job, df_e = scored_job(amd, link_type, tables)
    ts = [0.99, 0.9, 0.5]
    frame = df_e.clusters_at_thresholds(ts)
    table = frame.truth_table("cluster")
    # the route there was: one row per record on the host, then group-bys per threshold
    pdf = frame.toPandas()
    truth = pd.concat([t["cluster"] for t in tables], ignore_index=True)
    ids = pd.factorize(truth)[0].astype(np.int64)  # NaN: -1
    assert (ids < 0).any() and len(ids) == len(pdf)
    cross, n_left = link_type == "link_only", len(tables[0])
    want = np.stack([agreement_oracle(pdf[f"cluster_id_{t!r}"].to_numpy(), ids, n_left, cross) for t in ts])
    same_table(table, cluster_truth_rows(want, ts))
    assert table["threshold"].tolist() == ts
    # against the pair table of the same labels
    lc = df_e.label_counts("cluster")
    assert (table["true_pairs"] == lc.true_pairs_total).all() and lc.true_pairs_total > 0
    pairs = df_e.truth_table("cluster", thresholds=ts).set_index("threshold")
    for row in table.itertuples():
        assert pairs.loc[row.threshold, "tp"] <= row.tp <= row.true_pairs and row.tn >= 0 and row.fp >= 0
    assert (np.diff(table["tp"]) >= 0).all()
    # the rows of one threshold
    for i, t in enumerate(ts[1:], start=1):
        row = table.iloc[[i]].reset_index(drop=True)
        same_table(frame.at(t).truth_table("cluster"), row)
        alone = df_e.clusters(t).truth_table("cluster")
        assert np.isnan(alone["threshold"][0])
        same_table(alone, row, but=("threshold",))
        assert job.sweep_owner is None  # clusters(t) swept for itself
    # a second sweep frame of the job in between: the first frame sweeps again and gives the same table
    other = df_e.clusters_at_thresholds([0.7])
    row = other.truth_table("cluster")
    assert job.sweep_owner is other and len(row) == 1 and row["threshold"][0] == 0.7
    assert table["tp"][1] <= row["tp"][0] <= table["tp"][2]
    same_table(frame.truth_table("cluster"), table)
    assert job.sweep_owner is frame
    same_table(other.truth_table("cluster"), row)
    # in the order given
    flipped = df_e.clusters_at_thresholds(ts[::-1]).truth_table("cluster")
    same_table(flipped, table.iloc[::-1].reset_index(drop=True))
    with pytest.raises(ValueError, match="label column 'truth' is missing from input table 0"):
        frame.truth_table("truth")
    with pytest.raises(ValueError, match="missing from input table"):
        df_e.clusters(0.9).truth_table("truth")


def test_pipeline_dedupe_only(amd):
    check_pipeline(amd, "dedupe_only", [labelled_records(2000, seed=3)])


def test_pipeline_link_only(amd):
    df = labelled_records(2000, seed=3)
    check_pipeline(amd, "link_only", [df.iloc[::2].reset_index(drop=True), df.iloc[1::2].reset_index(drop=True)])


def test_label_column_forms(amd):
    """String labels with None give the table of the float labels with NaN."""
    df = labelled_records(600, seed=9)
    as_text = df.copy()
    as_text["cluster"] = [None if np.isnan(x) else f"c{int(x)}" for x in df["cluster"]]
    _, a = scored_job(amd, "dedupe_only", [df])
    _, b = scored_job(amd, "dedupe_only", [as_text])
    ta, tb = (f.clusters_at_thresholds([0.5, 0.9]).truth_table("cluster") for f in (a, b))
    same_table(ta, tb)
    assert ta["records_labelled"][0] == int(df["cluster"].notna().sum()) < len(df)
