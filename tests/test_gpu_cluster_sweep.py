"""clusters_at_thresholds() and the cluster metrics on the device (spk_components_sweep, spk_cluster_metrics).

Expected labels come from a host union-find per level, expected metrics from np.add.at / np.bincount; every comparison
is exact.  The ABI cases go through components_sweep_edges; the pipeline cases compare every column of
clusters_at_thresholds(ts) with clusters(t) of the existing route."""
import copy
import warnings

import numpy as np
import pandas as pd
import pytest

from conftest import load_golden
from sweep_common import emulation, metrics_oracle, scores_for, thresholds_for

pytestmark = pytest.mark.gpu
warnings.filterwarnings("ignore")
U32 = np.uint32


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


def want_levels(n, u, v, score, thr):
    """Union-find per level: the edges with score > thr[k] (no threshold: every edge)."""
    emu = emulation()
    u, v = np.asarray(u, dtype=np.int64), np.asarray(v, dtype=np.int64)
    if len(thr) == 0:
        return np.stack([emu.union_find(n, u, v)]), [len(u)]
    with np.errstate(invalid="ignore"):
        keep = [np.asarray(score) > t for t in thr]
    return np.stack([emu.union_find(n, u[k], v[k]) for k in keep]), [int(k.sum()) for k in keep]


def run_sweep(ctx, n, u, v, score, thr, check_metrics=False, want=None):
    """components_sweep_edges, every label of every level, the bookkeeping and (check_metrics) every level's metrics:
    (labels [L, n], rounds).  want: want_levels' result, for a graph that is swept more than once."""
    u, v = np.asarray(u, dtype=U32), np.asarray(v, dtype=U32)
    thr = np.asarray(thr, dtype=np.float64)
    want, want_edges = want or want_levels(n, u, v, score, thr)
    L = len(want)
    n_edges, n_clusters, rounds = ctx.components_sweep_edges(n, u, v, score, thr)
    assert n_edges.tolist() == want_edges and len(rounds) == L and (rounds <= 256).all()
    got = np.stack([ctx.components_sweep_copy(k, 0, n) for k in range(L)])
    assert got.dtype == U32 and np.array_equal(got, want)
    assert n_clusters.tolist() == [int(np.count_nonzero(w == np.arange(n))) for w in want]
    assert (np.diff(n_clusters) <= 0).all() and (np.diff(got.astype(np.int64), axis=0) <= 0).all()
    assert ctx.components_sweep_info()[:3] == (L, n, want_edges[-1])
    if check_metrics:
        for k in range(L):
            with np.errstate(invalid="ignore"):
                keep = np.asarray(score) > thr[k] if len(thr) else np.ones(len(u), dtype=bool)
            exp = metrics_oracle(n, u[keep], v[keep], want[k])
            scalars = ctx.cluster_metrics(k)
            first = ctx.cluster_metrics_copy(0, n)
            assert scalars == exp[4] and ctx.cluster_metrics_info()[0] == k
            for a, b in zip(first, exp[:4]):
                assert np.array_equal(a.astype(np.int64), b)
            assert ctx.cluster_metrics(k) == scalars
            for a, b in zip(first, ctx.cluster_metrics_copy(0, n)):
                assert a.tobytes() == b.tobytes()
            if n > 70:
                for a, b in zip(first, ctx.cluster_metrics_copy(33, 37)):
                    assert np.array_equal(a[33:70], b)
    return got, rounds


# ---- 1. degenerate shapes -----------------------------------------------------------------------------------
def test_degenerate_shapes(ctx):
    none, nos = np.empty(0, dtype=U32), np.empty(0)
    run_sweep(ctx, 0, none, none, nos, [0.5], check_metrics=True)           # no nodes
    got, rounds = run_sweep(ctx, 5, none, none, nos, [0.5, 0.25], check_metrics=True)  # no edges
    assert (got == np.arange(5)).all() and rounds.tolist() == [0, 0]
    u, v, s = [3, 0, 4], [1, 4, 2], [0.9, 0.5, 0.1]
    got, _ = run_sweep(ctx, 5, u, v, s, [0.5], check_metrics=True)           # one threshold; 0.5 > 0.5 is false
    assert got.tolist() == [[0, 1, 2, 1, 4]]
    got, _ = run_sweep(ctx, 5, u, v, s, [0.9, 0.5, 0.1], check_metrics=True)  # a score equal to a threshold: next level
    assert got.tolist() == [[0, 1, 2, 3, 4], [0, 1, 2, 1, 4], [0, 1, 2, 1, 0]]
    got, rounds = run_sweep(ctx, 5, u, v, s, [3.0, 2.0, 1.0])                  # every score below the lowest
    assert (got == np.arange(5)).all() and rounds.tolist() == [0, 0, 0]
    got, _ = run_sweep(ctx, 5, u, v, s, [0.0, -1.0])                          # every score above the highest
    assert got.tolist() == [[0, 1, 0, 1, 0]] * 2
    nan = float("nan")
    got, _ = run_sweep(ctx, 5, u, v, [nan, 0.5, nan], [0.7, 0.2, -1.0], check_metrics=True)  # NaN is in no level
    assert got.tolist() == [[0, 1, 2, 3, 4], [0, 1, 2, 3, 0], [0, 1, 2, 3, 0]]
    inf = float("inf")
    got, _ = run_sweep(ctx, 5, u, v, [inf, -inf, 0.1], [inf, 0.0, -inf])      # thresholds +-inf
    assert got.tolist() == [[0, 1, 2, 3, 4], [0, 1, 2, 1, 2], [0, 1, 2, 1, 2]]
    got, _ = run_sweep(ctx, 5, u, v, None, [], check_metrics=True)            # SPK_SEL_ALL's shape: no thresholds
    assert got.tolist() == [[0, 1, 0, 1, 0]]
    got, _ = run_sweep(ctx, 5, u, v, [nan, nan, nan], [])                     # ... where a NaN score is an edge too
    assert got.tolist() == [[0, 1, 0, 1, 0]]
    got, _ = run_sweep(ctx, 5, [2, 3, 3], [2, 3, 1], [0.9, 0.1, 0.1], [0.5, 0.0], check_metrics=True)  # self-loops add 2
    assert got.tolist() == [[0, 1, 2, 3, 4], [0, 1, 2, 1, 4]]
    assert ctx.cluster_metrics_copy(0, 5)[0].tolist() == [0, 1, 2, 3, 0]
    u = np.array([4, 2] * 500, dtype=U32)  # one edge 1,000 times, both orientations, across two levels
    got, _ = run_sweep(ctx, 5, u, u[::-1].copy(), np.tile([0.9, 0.9, 0.1], 334)[:1000], [0.5, 0.0], check_metrics=True)
    assert got.tolist() == [[0, 1, 2, 3, 2]] * 2
    ctx.cluster_metrics(0)
    assert ctx.cluster_metrics_copy(2, 1)[0].tolist() == [667]


# ---- 2. level ranges: every level starts at a multiple of 4 edges -----------------------------------------------
def _edge_counts():
    from splink_amd import _native
    C = _native.COMPONENTS_CHUNK
    return [1, 3, 4, 5, 63, 64, 65, 255, 256, 257, C - 1, C, C + 1, 3 * C + 17]


def split_levels(m):
    """Six levels over m edges with counts = 1, 2, 3 mod 4 where m allows, levels 1 and 4 empty, the rest in level 5;
    plus three edges of no level."""
    counts = [0] * 6
    left = m
    for k, c in ((0, 5), (2, 2), (3, 7)):
        counts[k] = min(c if m >= 64 else c % 4, left)
        left -= counts[k]
    counts[5] = left
    return np.concatenate([np.repeat(np.arange(6), counts), [6, 6, 6]])


@pytest.mark.parametrize("m", _edge_counts())
def test_level_ranges_and_odd_offsets(m, ctx):
    n, L = 4096, 6
    rng = np.random.Generator(np.random.PCG64(m))
    level = split_levels(m)
    assert len(level) == m + 3
    k = rng.permutation(len(level))
    level = level[k]
    u = rng.integers(0, n, len(level)).astype(U32)
    v = rng.integers(0, n, len(level)).astype(U32)
    got, _ = run_sweep(ctx, n, u, v, scores_for(level, L), thresholds_for(L), check_metrics=m in (5, 257))
    for lv in (0, 3, 5):
        for start, count in ((1, 63), (65, 257), (n - 33, 33), (1023, 2049)):
            assert np.array_equal(ctx.components_sweep_copy(lv, start, count), got[lv, start:start + count])
    for lv, start, count in ((L, 0, 1), (-1, 0, 1), (0, n - 1, 2), (0, -1, 1)):
        with pytest.raises(ValueError):
            ctx.components_sweep_copy(lv, start, count)
    with pytest.raises(ValueError):
        ctx.cluster_metrics(L)


# ---- 3. the graphs of tools/emulate_components.py ---------------------------------------------------------------
@pytest.mark.parametrize("name,L", [("path", 8), ("hub", 4), ("random", 8), ("alternating", 2)])
def test_emulated_graphs_every_level_twice(name, L, ctx):
    emu = emulation()
    if name == "alternating":
        n, u, v, level = emu.alternating_path()
    else:
        n, u, v = emu.GRAPHS[name]()
        level = emu.random_levels(len(u), L, seed=L)
    score, thr = scores_for(level, L), thresholds_for(L)
    want = want_levels(n, u, v, score, thr)
    first, r1 = run_sweep(ctx, n, u, v, score, thr, want=want)
    second, r2 = run_sweep(ctx, n, u, v, score, thr, want=want)
    assert first.tobytes() == second.tobytes()
    print(name, "rounds per level", r1.tolist(), r2.tolist())
    ctx.components_sweep_set_mode(1)  # the other edge-set variant: the same labels
    try:
        other, r3 = run_sweep(ctx, n, u, v, score, thr, want=want)
    finally:
        ctx.components_sweep_set_mode(0)
    assert first.tobytes() == other.tobytes()
    print(name, "rounds per level, every edge up to the level", r3.tolist())


# ---- 4. metrics under contention --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["hub", "single_path", "random"])
def test_metrics_match_the_numpy_oracle(name, ctx):
    emu = emulation()
    if name == "hub":  # the 256-clique and the 20,000-leaf star share level 1; level 0 has a tenth of their edges
        n, u, v = emu.hub_graph()
        level = (np.random.default_rng(2).random(len(u)) >= 0.1).astype(np.int64)
        L = 2
    elif name == "single_path":  # 0 - 1 - ... - n-1: every wave of the node pass holds one label
        n = 50001
        u = np.arange(n - 1, dtype=U32)
        v, level, L = u + 1, np.zeros(n - 1, dtype=np.int64), 1
    else:  # repeated edges, both orientations
        n, u, v = emu.random_graph()
        L = 3
        level = emu.random_levels(len(u), L, seed=3)
    got, _ = run_sweep(ctx, n, u, v, scores_for(level, L), thresholds_for(L), check_metrics=True)
    if name == "hub":
        ctx.cluster_metrics(1)
        degree, size, degree_sum, max_degree = ctx.cluster_metrics_copy(0, n)
        assert degree[n - 1] == 20000 and size[1256] == 20001 and max_degree[1256] == 20000 and degree_sum[1256] == 40000
        assert size[1000] == 256 and max_degree[1000] == 255 and degree_sum[1000] == 256 * 255
    if name == "single_path":
        assert ctx.cluster_metrics(0) == (1, n, n)


# ---- 5. ids and offsets past 2^31 -------------------------------------------------------------------------------
def test_ids_and_level_offsets_past_two_to_the_31(ctx):
    """Two levels of 2^31 + 16 labels, about 17 GB: level 1 starts past 2^33 bytes.  Metrics are not run at this size
    (they would take about 52 GB more)."""
    B = 1 << 31
    n = B + 16
    u = np.array([B + 5, B + 5, 7, B + 1, 2], dtype=U32)
    v = np.array([3, B + 9, 8, B + 2, B + 15], dtype=U32)
    score = np.array([0.9, 0.9, 0.9, 0.4, 0.4])
    n_edges, n_clusters, rounds = ctx.components_sweep_edges(n, u, v, score, [0.5, 0.1])  # an allocation failure fails the test
    assert ctx.memory()["em_score_tf"] >= 8 * n
    want_low, want_high = np.arange(16, dtype=U32), np.arange(B, B + 16, dtype=U32)
    want_low[8] = 7
    want_high[5] = want_high[9] = 3
    assert np.array_equal(ctx.components_sweep_copy(0, 0, 16), want_low)
    assert np.array_equal(ctx.components_sweep_copy(0, B, 16), want_high)
    want_high[2] = B + 1
    want_high[15] = 2
    assert np.array_equal(ctx.components_sweep_copy(1, 0, 16), want_low)
    assert np.array_equal(ctx.components_sweep_copy(1, B, 16), want_high)
    assert n_edges.tolist() == [3, 5] and n_clusters.tolist() == [n - 3, n - 5]
    assert ctx.components_sweep_info()[:3] == (2, n, 5)
    ctx.components_sweep_release()
    assert ctx.memory()["em_score_tf"] < 4 * n


# ---- 6. invalid input leaves no sweep ---------------------------------------------------------------------------
def test_invalid_input_leaves_no_sweep(ctx):
    ok = ([1], [2], [0.9], [0.5])
    for u, v, s, t in (([1, 10], [2, 3], [0.9, 0.9], [0.5]), ([1, 2], [2, 0xFFFFFFFF], [0.9, 0.3], [0.5, 0.1]),
                       ([10] * 3000, [0] * 3000, [0.3] * 3000, [0.5, 0.4, 0.1])):
        run_sweep(ctx, 10, *ok)
        with pytest.raises(ValueError, match="n_nodes"):
            ctx.components_sweep_edges(10, np.array(u, dtype=U32), np.array(v, dtype=U32), s, t)
        assert ctx.components_sweep_info() == (-1, -1, -1, -1.0)
        with pytest.raises(RuntimeError):
            ctx.components_sweep_copy(0, 0, 1)
        with pytest.raises(RuntimeError):
            ctx.cluster_metrics(0)
    nan = float("nan")
    for t in ([0.1, 0.5], [0.5, 0.5], [0.5, nan], [nan], list(np.linspace(1, 0, 33))):
        run_sweep(ctx, 10, *ok)
        with pytest.raises(ValueError):
            ctx.components_sweep_edges(10, np.array([1], dtype=U32), np.array([2], dtype=U32), [0.9], t)
        assert ctx.components_sweep_info()[0] == -1
    with pytest.raises(ValueError):
        ctx.components_sweep_edges((1 << 32), np.empty(0, dtype=U32), np.empty(0, dtype=U32), np.empty(0), [0.5])


# ---- 7. state ---------------------------------------------------------------------------------------------------
def test_abi_states(amd):
    from splink_amd import _native as N
    emu = emulation()
    c = N.Context(0)
    rng = np.random.Generator(np.random.PCG64(8))
    n_rows, n, levels = 300, 5000, [2, 3]
    g = np.stack([rng.integers(-1, L, n) for L in levels], axis=1).astype(np.int8)
    rows_l = rng.integers(0, n_rows, n).astype(np.int32)
    rows_r = rng.integers(0, n_rows, n).astype(np.int32)
    eq1 = (N.SEL_GAMMA, 1, N.SEL_OP["="], 1.0)
    with pytest.raises(RuntimeError, match="no selection"):
        c.components_sweep(N.SEL_ALL, [])
    c.gammas_load(levels, g)  # codes without pairs: a selection without rows
    c.select(0.0, 0.0, None, None, [eq1])
    with pytest.raises(RuntimeError, match="pair rows"):
        c.components_sweep(N.SEL_ALL, [])
    c.table_create(0, n_rows, 1)
    c.pairs_load(rows_l, rows_r)
    c.gammas_load(levels, g)
    k = c.select(0.0, 0.0, None, None, [eq1])
    with pytest.raises(RuntimeError, match="m / u"):  # a selection made without m / u has no match_probability
        c.components_sweep(N.SEL_MP, [0.5])
    assert c.components_sweep_info()[0] == -1
    c.select(0.0, 0.0, None, None, [eq1])
    with pytest.raises(RuntimeError, match="tf tables"):  # nor, after a plain select, a tf_adjusted_match_prob
        c.components_sweep(N.SEL_TF_MP, [0.5])
    with pytest.raises(ValueError):
        c.components_sweep(N.SEL_ALL, [0.5])
    with pytest.raises(ValueError):
        c.components_sweep(N.SEL_GAMMA, [0.5])
    keep = g[:, 1] == 1
    want = emu.union_find(n_rows, rows_l[keep], rows_r[keep])
    n_nodes, n_edges, n_clusters, rounds = c.components_sweep(N.SEL_ALL, [])
    assert (n_nodes, n_edges.tolist()) == (n_rows, [k]) and n_clusters[0] == np.count_nonzero(want == np.arange(n_rows))
    assert np.array_equal(c.components_sweep_copy(0, 0, n_rows), want)
    assert c.components_sweep_info()[:3] == (1, n_rows, k) and c.components_sweep_info()[3] == -1.0
    exp = metrics_oracle(n_rows, rows_l[keep], rows_r[keep], want)
    assert c.cluster_metrics(0) == exp[4]
    for a, b in zip(c.cluster_metrics_copy(0, n_rows), exp[:4]):
        assert np.array_equal(a.astype(np.int64), b)
    mem = c.memory()
    assert mem["total"] == sum(v for key, v in mem.items() if key != "total")
    # the sweep and spk_components do not disturb each other; a new selection does not reach either
    assert c.components()[:2] == (n_rows, int(n_clusters[0]))
    assert np.array_equal(c.components_sweep_copy(0, 0, n_rows), want) and c.cluster_metrics(0) == exp[4]
    c.select(0.0, 0.0, None, None, [(N.SEL_GAMMA, 0, N.SEL_OP["="], 0.0)])
    c.components_sweep(N.SEL_ALL, [])
    assert np.array_equal(c.components_copy(0, n_rows), want)
    c.select_release()
    assert c.components_sweep_info()[0] == 1 and len(c.components_sweep_copy(0, 3, 100)) == 100
    # new codes make the selection stale: no sweep from it, and the failing call leaves none
    c.select(0.0, 0.0, None, None, [eq1])
    c.gammas_load(levels, g)
    with pytest.raises(RuntimeError, match="changed since spk_select"):
        c.components_sweep(N.SEL_ALL, [])
    assert c.components_sweep_info()[0] == -1
    # timing, release
    c.enable_timing(True)
    c.select(0.0, 0.0, None, None, [eq1])
    c.components_sweep(N.SEL_ALL, [])
    assert c.components_sweep_info()[3] >= 0.0
    c.cluster_metrics(0)
    assert c.cluster_metrics_info()[0] == 0 and c.cluster_metrics_info()[1] >= 0.0
    c.enable_timing(False)
    held = c.memory()["em_score_tf"]
    c.components_sweep_release()
    assert held - c.memory()["em_score_tf"] >= (4 + 20) * n_rows + 8 * k
    with pytest.raises(RuntimeError, match="no sweep"):
        c.components_sweep_copy(0, 0, 1)
    assert c.cluster_metrics_info() == (-1, -1.0)
    # new tables drop the sweep
    c.components_sweep_edges(4, np.array([0], dtype=U32), np.array([3], dtype=U32), None, [])
    c.table_create(0, n_rows, 1)
    assert c.components_sweep_info()[0] == -1


def test_spk_cluster_drops_the_sweep(amd):
    """spk_cluster permutes the tables' rows: a sweep made before it (host edges or a selection) is gone after it,
    as the labels of spk_components are."""
    from splink_amd import _native as N
    c = N.Context(0)
    rng = np.random.Generator(np.random.PCG64(9))
    n_rows, n, levels = 200, 3000, [2, 3]
    keys = rng.integers(0, 17, n_rows).astype(np.int64)
    rank = rng.permutation(n_rows).astype(np.int64)

    def tables():
        c.table_create(0, n_rows, 1)
        c.table_set_key(0, 0, 0, keys)
        c.table_set_rank(0, rank)

    def gone():
        assert c.components_sweep_info() == (-1, -1, -1, -1.0) and c.cluster_metrics_info() == (-1, -1.0)
        with pytest.raises(RuntimeError, match="no sweep"):
            c.components_sweep_copy(0, 0, 1)
        with pytest.raises(RuntimeError, match="no sweep"):
            c.cluster_metrics(0)
    # a sweep over host edges
    tables()
    c.components_sweep_edges(n_rows, np.array([0, 5], dtype=U32), np.array([3, 9], dtype=U32), [0.9, 0.2], [0.5, 0.1])
    c.cluster_metrics(1)
    assert c.components_sweep_info()[:3] == (2, n_rows, 2) and c.components_sweep_copy(1, 9, 1)[0] == 5
    perm, _ = c.cluster(n_rows)
    assert sorted(perm.tolist()) == list(range(n_rows)) and not np.array_equal(perm, np.arange(n_rows))
    gone()
    # a sweep over a selection
    tables()
    g = np.stack([rng.integers(-1, L, n) for L in levels], axis=1).astype(np.int8)
    c.pairs_load(rng.integers(0, n_rows, n).astype(np.int32), rng.integers(0, n_rows, n).astype(np.int32))
    c.gammas_load(levels, g)
    k = c.select(0.0, 0.0, None, None, [(N.SEL_GAMMA, 1, N.SEL_OP["="], 1.0)])
    assert c.components_sweep(N.SEL_ALL, [])[1].tolist() == [k] and c.components_sweep_info()[0] == 1
    c.cluster(n_rows)
    gone()


def test_edge_pass_forms_give_the_same_metrics(ctx):
    """spk_cluster_metrics_set_mode: the lanes sharing the wave's first end counted in the wave (the default), or one
    add per edge end -- the same bytes, on the hub graph (whole waves on the hub) and on a graph of repeated edges."""
    emu = emulation()
    for n, u, v in (emu.hub_graph(), (70, np.repeat([3, 3, 69, 4], 50), np.repeat([3, 8, 3, 4], 50))):
        ctx.components_sweep_edges(n, np.asarray(u, dtype=U32), np.asarray(v, dtype=U32), None, [])
        exp = metrics_oracle(n, u, v, ctx.components_sweep_copy(0, 0, n))
        out = []
        for mode in (1, 0, 1):
            ctx.cluster_metrics_set_mode(mode)
            try:
                scalars = ctx.cluster_metrics(0)
            finally:
                ctx.cluster_metrics_set_mode(1)
            out.append((scalars, [a.tobytes() for a in ctx.cluster_metrics_copy(0, n)]))
            assert scalars == exp[4] and np.array_equal(ctx.cluster_metrics_copy(0, n)[0].astype(np.int64), exp[0])
        assert out[0] == out[1] == out[2]
    with pytest.raises(ValueError):
        ctx.cluster_metrics_set_mode(2)


def frame(d):
    return pd.DataFrame(d) if d else None


def scored(g, amd):
    from splink_amd import Splink
    linker = Splink(copy.deepcopy(g["settings_in"]), amd if g["jaro"] else "supress_warnings", df=frame(g.get("df")),
                    df_l=frame(g.get("df_l")), df_r=frame(g.get("df_r")))
    return linker, linker.get_scored_comparisons()


def test_a_sweep_leaves_components_scores_tf_em_and_the_selection_alone(amd):
    from splink_amd import _native as N
    g = load_golden("link_tf")
    linker, df_e = scored(g, amd)
    job = df_e.job
    pdf = df_e.toPandas()
    t = float(pdf["match_probability"].median())
    hi = float(pdf["match_probability"].quantile(0.8))
    tf_col = next(c["col_name"] for c in df_e.settings["comparison_columns"] if c["term_frequency_adjustments"])

    def state(with_sweep):
        """Select and label, optionally sweep and count, then everything a sweep must not have touched."""
        f = df_e.filter(f"match_probability >= {t!r}")
        k = f.count()
        assert 0 < k < len(pdf)
        n_nodes = job.ctx.components()[0]
        if with_sweep:
            _, n_edges, n_clusters, _ = job.ctx.components_sweep(N.SEL_MP, [hi, t])
            assert 0 < n_edges[0] < n_edges[1] <= k and n_clusters[1] <= n_clusters[0] < n_nodes
            job.ctx.cluster_metrics(1)
        labels = job.ctx.components_copy(0, n_nodes)
        sel = job.ctx.select_copy(0, k, len(df_e.gammas.meta[0]))
        col = job._col_index[(tf_col, "str")]
        nv = job.ctx.tf_column_values(col)
        scale = job.ctx.tf_scales_column(col, nv)
        limbs, counts = job.ctx.tf_accumulate_column_exact(col, nv, scale)
        tf = linker.make_term_frequency_adjustments(df_e).toPandas()
        stats = job.em_stats(df_e.lam, df_e.level_probs)
        mp = job.score(df_e.lam, df_e.level_probs)
        return [labels] + list(sel) + [scale.copy(), limbs.copy(), counts.copy(), stats.copy(), mp.copy()], tf
    job.score(df_e.lam, df_e.level_probs, want_host=False)
    plain, tf0 = state(False)
    job.score(df_e.lam, df_e.level_probs, want_host=False)
    job.selection_owner = None  # select again, as the first time
    swept, tf1 = state(True)
    for a, b in zip(plain, swept):
        assert np.array_equal(a, b, equal_nan=True)
    pd.testing.assert_frame_equal(tf0, tf1, check_exact=True)


# ---- 8. pipeline parity -----------------------------------------------------------------------------------------
def golden_case(name):
    return load_golden("link_options")[name[len("link_options/"):]] if name.startswith("link_options/") else load_golden(name)


def thresholds_of(scores):
    """Up to 32 thresholds, shuffled: midpoints between distinct scores (subsampled) and actual scores."""
    distinct = np.sort(pd.Series(scores).dropna().unique())
    assert len(distinct) >= 2
    mids = (distinct[:-1] + distinct[1:]) / 2
    mids = mids[np.unique(np.linspace(0, len(mids) - 1, 24).astype(int))]
    actual = distinct[np.unique(np.linspace(0, len(distinct) - 1, 8).astype(int))]
    ts = np.unique(np.concatenate([mids, actual]))[:32]
    return [float(t) for t in np.random.default_rng(len(ts)).permutation(ts)]


def check_parity(frame_e, column, ts, wide=None):
    """clusters_at_thresholds(ts) of frame_e (or of the filtered / best-match frame `wide`) against the existing
    route, one clusters() per threshold."""
    from splink_amd import ClusterSweepFrame
    sweep = frame_e.clusters_at_thresholds(ts) if wide is None else wide.clusters_at_thresholds(ts)
    assert isinstance(sweep, ClusterSweepFrame) and sweep.thresholds == ts
    got = sweep.toPandas()
    uid = frame_e.settings["unique_id_column_name"]
    two = frame_e.job.link_type != "dedupe_only"
    assert list(got.columns) == [uid] + (["_source_table"] if two else []) + [f"cluster_id_{t!r}" for t in ts]
    assert sweep.columns == list(got.columns) and len(got) == sweep.count() == sum(len(t) for t in frame_e.job.inputs)
    summary = sweep.summary()
    assert list(summary.columns) == ["threshold", "n_edges", "n_clusters", "n_clusters_multi", "records_clustered",
                                     "largest_cluster", "rounds"]
    assert summary["threshold"].tolist() == ts
    for i, t in enumerate(ts):
        cf = n_edges = None  # a best-match frame takes no further filter: its caller checks the labels
        if wide is None:
            one = frame_e.filter(f"{column} > {t!r}")
            cf, n_edges = one.clusters(), one.count()
        col = got[f"cluster_id_{t!r}"]
        assert col.dtype == np.int64
        if cf is not None:
            exp = cf.toPandas()
            assert np.array_equal(col.to_numpy(), exp["cluster_id"].to_numpy())
            assert summary["n_clusters"][i] == cf.n_clusters and summary["n_edges"][i] == n_edges
            level = sweep.at(t)
            pd.testing.assert_frame_equal(level.toPandas(), exp, check_exact=True)
            pd.testing.assert_frame_equal(level.toPandas(singletons=False), cf.toPandas(singletons=False), check_exact=True)
            assert level.n_clusters == cf.n_clusters
        sizes = np.bincount(col.to_numpy(), minlength=len(got))
        multi = sizes[sizes >= 2]
        assert (summary["n_clusters_multi"][i], summary["records_clustered"][i], summary["largest_cluster"][i]) == \
            (len(multi), multi.sum(), sizes.max())
    return sweep, got, summary


def check_frame_metrics(filtered):
    """ClusterFrame.metrics() against pandas groupby over the filtered frame's pairs."""
    kept = filtered.toPandas()
    cf = filtered.clusters()
    clusters = cf.toPandas()
    uid = filtered.settings["unique_id_column_name"]
    lt = filtered.job.link_type
    if lt == "dedupe_only":
        key = {x: i for i, x in enumerate(clusters[uid])}
        l, r = kept[uid + "_l"].map(key), kept[uid + "_r"].map(key)
    else:
        src = (["left"] * len(kept), ["right"] * len(kept)) if lt == "link_only" else (kept["_source_table_l"], kept["_source_table_r"])
        key = {x: i for i, x in enumerate(zip(clusters["_source_table"], clusters[uid]))}
        l = pd.Series([key[x] for x in zip(src[0], kept[uid + "_l"])], dtype=np.int64)
        r = pd.Series([key[x] for x in zip(src[1], kept[uid + "_r"])], dtype=np.int64)
    m = cf.metrics()
    assert m._labels is cf._labels  # the frame's labels, not a second copy
    fresh = filtered.clusters()    # a frame that has not labelled yet takes the sweep's labels
    fm = fresh.metrics()
    assert fresh._labels is fm._labels and fresh.n_clusters == cf.n_clusters
    pd.testing.assert_frame_equal(fresh.toPandas(), clusters, check_exact=True)
    pd.testing.assert_frame_equal(fm.nodes(), m.nodes(), check_exact=True)
    nodes, per = m.nodes(), m.clusters()
    degree = pd.concat([l, r]).value_counts().reindex(range(len(clusters)), fill_value=0).sort_index()
    assert np.array_equal(nodes["node_degree"].to_numpy(), degree.to_numpy())
    assert list(nodes.columns) == list(clusters.columns) + ["node_degree", "node_centrality"]
    pd.testing.assert_frame_equal(nodes[list(clusters.columns)], clusters, check_exact=True)
    grouped = pd.DataFrame({"cluster_id": clusters["cluster_id"], "d": degree.to_numpy()}).groupby("cluster_id")["d"]
    exp = pd.DataFrame({"n_nodes": grouped.size(), "n_edges": grouped.sum() // 2, "mx": grouped.max()}).reset_index()
    assert list(per.columns) == ["cluster_id", "n_nodes", "n_edges", "density", "cluster_centralisation"]
    for c in ("cluster_id", "n_nodes", "n_edges"):
        assert np.array_equal(per[c].to_numpy(), exp[c].to_numpy())
    n, e, mx = exp["n_nodes"].to_numpy(float), exp["n_edges"].to_numpy(float), exp["mx"].to_numpy(float)
    with np.errstate(divide="ignore", invalid="ignore"):
        density = np.where(n > 1, 2 * e / (n * (n - 1)), np.nan)
        central = np.where(n > 2, (n * mx - 2 * e) / ((n - 1) * (n - 2)), np.nan)
        cent = np.where(n[np.searchsorted(exp["cluster_id"], clusters["cluster_id"])] > 1,
                        degree.to_numpy() / (n[np.searchsorted(exp["cluster_id"], clusters["cluster_id"])] - 1), np.nan)
    assert np.array_equal(per["density"], density, equal_nan=True)
    assert np.array_equal(per["cluster_centralisation"], central, equal_nan=True)
    assert np.array_equal(nodes["node_centrality"], cent, equal_nan=True)
    many = m.clusters(singletons=False)
    pd.testing.assert_frame_equal(many, per[per["n_nodes"] > 1].reset_index(drop=True), check_exact=True)
    assert e.sum() == len(kept)
    return m


@pytest.mark.parametrize("name", ["synthetic_cfg1", "link_options/link_only_plain_rules"])
def test_pipeline_sweep_matches_one_clusters_call_per_threshold(name, amd):
    g = golden_case(name)
    _, df_e = scored(g, amd)
    ts = thresholds_of(df_e.toPandas()["match_probability"])
    sweep, got, summary = check_parity(df_e, "match_probability", ts)
    t = sorted(ts)[len(ts) // 2]
    check_frame_metrics(df_e.filter(f"match_probability > {t!r}"))
    # metrics(t) of the sweep are those of the one-threshold route
    a, b = sweep.metrics(t), df_e.clusters(t).metrics()
    pd.testing.assert_frame_equal(a.clusters(), b.clusters(), check_exact=True)
    pd.testing.assert_frame_equal(a.nodes(), b.nodes(), check_exact=True)
    pd.testing.assert_frame_equal(sweep.at(t).metrics().nodes(), b.nodes(), check_exact=True)
    # another frame's selection and sweep in between: summary() and metrics() sweep again
    df_e.clusters(ts[0]).metrics()
    pd.testing.assert_frame_equal(sweep.summary(), summary, check_exact=True)
    pd.testing.assert_frame_equal(sweep.metrics(t).clusters(), b.clusters(), check_exact=True)
    with pytest.raises(ValueError, match="thresholds"):
        sweep.at(2.5)


def synthetic_tables(n, seed):
    from splink_amd.synthetic import make_records
    return make_records(n, seed=seed, surname_vocab=120, first_vocab=80, city_vocab=20)[
        ["unique_id", "first_name", "surname", "dob", "city", "email"]]


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


def test_link_only_with_permuted_tables_and_best_matches(amd):
    df = synthetic_tables(4000, seed=10)
    rng = np.random.Generator(np.random.PCG64(10))
    side = rng.random(len(df)) < 0.5
    left = df[side].sample(frac=1.0, random_state=1).reset_index(drop=True)
    right = df[~side].sample(frac=1.0, random_state=2).reset_index(drop=True)
    df_e = scored_job(amd, "link_only", [left, right])
    for p in df_e.job.perm:
        assert p is not None and not np.array_equal(p, np.arange(len(p)))
    scores = df_e.toPandas()["match_probability"]
    ts = thresholds_of(scores)
    sweep, got, summary = check_parity(df_e, "match_probability", ts)
    assert summary["largest_cluster"].max() >= 3
    t = float(np.quantile(scores, 0.9))
    check_frame_metrics(df_e.filter(f"match_probability > {t!r}"))
    # a one-to-one link: every cluster has at most two records and every degree is at most 1, at every threshold
    lo = float(np.quantile(scores, 0.5))
    best = df_e.filter(f"match_probability > {lo!r}").best_matches(per="mutual")
    bs = [t for t in ts if t >= lo][:8]
    sweep, got, summary = check_parity(df_e, "match_probability", bs, wide=best)
    kept = best.toPandas()
    assert (summary["largest_cluster"] <= 2).all() and summary["n_edges"].max() <= len(kept)
    pos_l = {x: i for i, x in enumerate(left["unique_id"])}
    pos_r = {x: len(left) + i for i, x in enumerate(right["unique_id"])}
    for i, t in enumerate(bs):
        at = kept[kept["match_probability"] > t]
        exp = emulation().union_find(len(got), [pos_l[x] for x in at["unique_id_l"]], [pos_r[x] for x in at["unique_id_r"]])
        assert np.array_equal(got[f"cluster_id_{t!r}"].to_numpy(), exp.astype(np.int64))
        assert summary["n_edges"][i] == int((kept["match_probability"] > t).sum())
        assert summary["n_clusters"][i] == len(got) - summary["n_edges"][i]
        m = sweep.metrics(t)
        assert m.nodes()["node_degree"].max() <= 1 and m.clusters()["n_nodes"].max() <= 2


def test_tf_frame_by_tf_adjusted_match_prob(amd):
    g = load_golden("link_tf")
    linker, df_e = scored(g, amd)
    tf = linker.make_term_frequency_adjustments(df_e)
    scores = tf.toPandas()["tf_adjusted_match_prob"]
    ts = thresholds_of(scores)
    sweep, _, _ = check_parity(tf, "tf_adjusted_match_prob", ts)
    assert sweep.by == "tf_adjusted_match_prob"
    # the same frame by its other score
    lo = min(ts)
    mp = tf.toPandas()["match_probability"]
    ms = thresholds_of(mp)[:6]
    other = tf.filter(f"tf_adjusted_match_prob > {lo!r}").clusters_at_thresholds(ms, by="match_probability")
    got = other.toPandas()
    for t in ms:
        exp = tf.filter(f"tf_adjusted_match_prob > {lo!r} and match_probability > {t!r}").clusters().toPandas()
        assert np.array_equal(got[f"cluster_id_{t!r}"].to_numpy(), exp["cluster_id"].to_numpy())


# ---- 9. refusals ------------------------------------------------------------------------------------------------
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
        table_e.clusters_at_thresholds([0.5, 0.9])
    df = synthetic_tables(1500, seed=12)
    sharded = scored_job(amd, "dedupe_only", [df], shard=(0, 2))
    with pytest.raises(ValueError, match="shards"):
        sharded.clusters_at_thresholds([0.5, 0.9])
    whole = scored_job(amd, "dedupe_only", [df])
    with pytest.raises(ValueError, match="no score"):
        whole.gammas.filter("gamma_surname >= 0").clusters_at_thresholds([0.5])
    for bad in ([], [0.5, 0.5], [float("nan")], list(np.linspace(0, 1, 33))):
        with pytest.raises(ValueError):
            whole.clusters_at_thresholds(bad)
    with pytest.raises(ValueError, match="by="):
        whole.filter("match_probability > 0.1").clusters_at_thresholds([0.5], by="tf_adjusted_match_prob")
    sweep = whole.clusters_at_thresholds([0.9, 0.5])
    for x in (sweep, sweep.metrics(0.5)):
        with pytest.raises(ValueError, match="cluster frame"):
            run_maximisation_step(x, params, amd)
