"""clusters(t).bridges() on the device (spk_cluster_bridges).

Expected bridges, side sizes, cores and scalars come from the host oracle of bridges_common.py (a low-link DFS by edge
index plus union-find); every comparison is exact.  The ABI cases go through components_sweep_edges; the pipeline cases
compare the frames with the oracle over filter(...).toPandas()."""
import copy
import warnings

import numpy as np
import pandas as pd
import pytest

import bridges_common as B
from conftest import load_golden
from sweep_common import metrics_oracle, scores_for, thresholds_for

pytestmark = pytest.mark.gpu
warnings.filterwarnings("ignore")
U32 = np.uint32
NO_RESULT = (-1, -1, -1.0)


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


def device_result(ctx, level, n):
    """spk_cluster_bridges of one level and everything it holds, as the oracle's dict (plus rounds)."""
    out4 = ctx.cluster_bridges(level)
    lv, rounds, _ = ctx.cluster_bridges_info()
    assert lv == level
    u, v, su, sv = ctx.cluster_bridges_copy(0, out4[0])
    core = ctx.cluster_bridges_cores_copy(0, n)
    if out4[0] > 2:  # a range inside, and outputs left out
        a = ctx.cluster_bridges_copy(1, out4[0] - 2)
        for whole, part in zip((u, v, su, sv), a):
            assert np.array_equal(whole[1:-1], part)
    if n > 70:
        assert np.array_equal(ctx.cluster_bridges_cores_copy(33, 37), core[33:70])
    return {"u": u, "v": v, "side_u": su, "side_v": sv, "core": core, "out4": out4, "rounds": rounds}


def check_level(ctx, level, n, u, v, want=None):
    """The level's result against the oracle over the edges (u, v) that the level holds."""
    want = want or B.oracle(n, u, v)
    got = device_result(ctx, level, n)
    B.same(got, want)
    assert got["rounds"] == (want["out4"][3] + 1 if len(u) else 0)  # rounds = depth + 1: the depths are the BFS depths
    if len(got["u"]):
        key = got["u"].astype(np.uint64) << np.uint64(32) | got["v"].astype(np.uint64)
        assert (np.diff(key.astype(np.int64)) > 0).all()  # ascending by (u, v), no bridge twice
    return got


def run(ctx, n, u, v, want=None):
    """One level of every edge through components_sweep_edges, checked; returns the device's result."""
    u, v = np.asarray(u, dtype=U32), np.asarray(v, dtype=U32)
    ctx.components_sweep_edges(n, u, v, None, [])
    return check_level(ctx, 0, n, u, v, want)


def run_levels(ctx, n, u, v, level, L, order=None):
    """L levels (edge i is new at level[i]) through components_sweep_edges; every level in `order` checked against
    the oracle over the edges up to it."""
    u, v, level = np.asarray(u, dtype=U32), np.asarray(v, dtype=U32), np.asarray(level)
    ctx.components_sweep_edges(n, u, v, scores_for(level, L), thresholds_for(L))
    out = []
    for k in order if order is not None else range(L):
        out.append(check_level(ctx, k, n, u[level <= k], v[level <= k]))
    return out


# ---- 1. degenerate shapes -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(B.degenerate_graphs()))
def test_degenerate_shapes(name, ctx):
    n, u, v = B.degenerate_graphs()[name]
    got = run(ctx, n, u, v)
    if len(u) >= 2:  # the same in two levels with an odd first count: level 1's range holds padding self-loops (0, 0)
        run_levels(ctx, n, u, v, [0] + [1] * (len(u) - 1), 2)
    if name == "idle_nodes":
        three = run_levels(ctx, n, u, v, [0, 0, 0, 1, 2], 3)  # ranges start at 0, 4, 8: four (0, 0) inside level 2's
        for res in [got] + three:
            assert res["core"][0] == 0 and 0 not in res["u"].tolist() + res["v"].tolist()
            assert res["core"].tolist()[4] == 4 and res["core"].tolist()[8:] == [8, 9]
        assert list(zip(got["u"], got["v"], got["side_u"], got["side_v"])) == [(5, 6, 1, 2), (6, 7, 2, 1)]


def test_no_nodes(ctx):
    none = np.empty(0, dtype=U32)
    got = run(ctx, 0, none, none)
    assert got["out4"] == (0, 0, 0, 0) and got["rounds"] == 0 and len(got["core"]) == 0


# ---- 2. boundaries -------------------------------------------------------------------------------------------------
def _edge_counts():
    from splink_amd import _native
    C = _native.COMPONENTS_CHUNK
    return [63, 64, 65, 255, 256, 257, C - 1, C, C + 1]


@pytest.mark.parametrize("m", _edge_counts())
def test_edge_counts_around_the_wave_the_workgroup_and_the_chunk(m, ctx):
    n, u, v = B.chain_of_edges(m)
    got = run(ctx, n, u, v)
    assert 0 < got["out4"][0] < n - 1


def test_two_levels_with_an_odd_first_count(ctx):
    n, u, v = B.chain_of_edges(257)
    level = np.ones(257, dtype=np.int64)
    level[:5] = 0  # level 1 starts at edge 8, behind three padding self-loops
    run_levels(ctx, n, u, v, level, 2)


# ---- 3. shapes -------------------------------------------------------------------------------------------------------
def test_hub_star_clique_and_idle_nodes(ctx):
    n, u, v = B.emulation()._CC.hub_graph()
    got = run(ctx, n, u, v)
    star = u == n - 1
    assert got["out4"][:3] == (20000, 1000 + 1 + 20001, 256)
    assert sorted(zip(got["u"].tolist(), got["v"].tolist())) == sorted(zip(u[star].tolist(), v[star].tolist()))
    assert (got["side_u"] == 20000).all() and (got["side_v"] == 1).all()  # the hub's side keeps n - 1 of the star's 20,001


def test_path_through_a_permutation(ctx):
    n, u, v, order = B.permuted_path(2000)
    got = run(ctx, n, u, v)
    at = int(np.flatnonzero(order == 0)[0])
    assert got["out4"] == (n - 1, n, 1, max(at, n - 1 - at)) and got["rounds"] == max(at, n - 1 - at) + 1
    assert (got["side_u"].astype(np.int64) + got["side_v"] == n).all()


def test_cycle_with_and_without_a_tail(ctx):
    n, u, v = B.permuted_cycle(4096)
    assert run(ctx, n, u, v)["out4"][:3] == (0, 1, 4096)
    n, u, v = B.permuted_cycle(4096, tail=10)
    got = run(ctx, n, u, v)
    assert got["out4"][:3] == (10, 11, 4096)
    assert sorted(np.minimum(got["side_u"], got["side_v"]).tolist()) == list(range(1, 11))


def test_barbell(ctx):
    n, u, v = B.barbell(64)
    got = run(ctx, n, u, v)
    assert got["out4"][:3] == (1, 2, 64)
    assert [got[k].tolist() for k in ("u", "v", "side_u", "side_v")] == [[63], [64], [64], [64]]


_RANDOM = {}


def random_graph():
    """The random multigraph (a fifth of the edges repeated, half of those reversed) and its oracle, computed once."""
    if not _RANDOM:
        n, u, v = B.emulation()._CC.random_graph()
        _RANDOM["g"] = (n, u, v, B.oracle(n, u, v))
    return _RANDOM["g"]


def test_random_graph_twice_gives_the_same_bytes(ctx):
    n, u, v, want = random_graph()
    assert (n, len(u)) == (200000, 150000) and want["out4"][0] > 10000 and want["out4"][2] > 1000
    runs = []
    for _ in range(2):  # a sweep of its own each time: the edges' order inside the range and the forest vary
        got = run(ctx, n, u, v, want)
        runs.append([got[k].tobytes() for k in ("u", "v", "side_u", "side_v", "core")] + [got["out4"], got["rounds"]])
    assert runs[0] == runs[1]


# ---- 4. levels ---------------------------------------------------------------------------------------------------------
def test_alternating_path_level_by_level(ctx):
    n, u, v, level = B.emulation()._CC.alternating_path(2000)
    first, zero, again = run_levels(ctx, n, u, v, level, 2, order=[1, 0, 1])
    assert zero["out4"] == (n // 2 - 1, n, 1, 1)  # every edge an isolated bridge
    assert (zero["side_u"] == 1).all() and (zero["side_v"] == 1).all()
    assert first["out4"] == (n - 1, n, 1, n - 1) and first["rounds"] == n
    for k in ("u", "v", "side_u", "side_v", "core"):
        assert first[k].tobytes() == again[k].tobytes()
    assert first["out4"] == again["out4"] and first["rounds"] == again["rounds"]


# ---- 5. the limit ------------------------------------------------------------------------------------------------------
def test_a_tree_deeper_than_the_cap_is_refused_and_leaves_no_result(ctx):
    from splink_amd import _native as N
    cap = N.BRIDGES_MAX_ROUNDS
    n, u, v = B.id_order_path(cap)  # depth cap - 1: the deepest tree the cap allows
    got = run(ctx, n, u, v)
    assert got["out4"] == (cap - 1, cap, 1, cap - 1) and got["rounds"] == cap
    n, u, v = B.id_order_path(cap + 10)
    ctx.components_sweep_edges(n, u, v, None, [])
    multi = ctx.cluster_metrics(0)
    assert multi == (1, n, n)
    with pytest.raises(ValueError, match="depth"):  # SPK_E_LIMIT
        ctx.cluster_bridges(0)
    assert ctx.cluster_bridges_info() == NO_RESULT
    for call in (lambda: ctx.cluster_bridges_copy(0, 0), lambda: ctx.cluster_bridges_cores_copy(0, 1)):
        with pytest.raises(RuntimeError, match="no bridges"):
            call()
    assert (ctx.components_sweep_copy(0, 0, n) == 0).all() and ctx.components_sweep_info()[:3] == (1, n, n - 1)
    assert ctx.cluster_metrics_info()[0] == 0 and ctx.cluster_metrics_copy(0, 1)[1].tolist() == [n]
    assert ctx.cluster_metrics(0) == multi
    n, u, v = B.degenerate_graphs()["triangle_pendant"]
    assert run(ctx, n, u, v)["out4"] == (1, 4, 3, 2)


# ---- 6. state ------------------------------------------------------------------------------------------------------------
def test_abi_states(amd):
    from splink_amd import _native as N
    c = N.Context(0)
    with pytest.raises(RuntimeError, match="no sweep"):
        c.cluster_bridges(0)
    assert c.cluster_bridges_info() == NO_RESULT
    with pytest.raises(RuntimeError, match="no bridges"):
        c.cluster_bridges_copy(0, 0)
    n, u, v = B.chain_of_edges(257)
    level = (np.arange(257) % 2).astype(np.int64)
    want = [B.oracle(n, u[level <= k], v[level <= k]) for k in range(2)]
    c.components_sweep_edges(n, u, v, scores_for(level, 2), thresholds_for(2))
    labels = [c.components_sweep_copy(k, 0, n) for k in range(2)]
    # a level or a range outside: SPK_E_INVALID
    for bad in (-1, 2):
        with pytest.raises(ValueError, match="level"):
            c.cluster_bridges(bad)
    before = c.memory()["em_score_tf"]
    B.same(device_result(c, 1, n), want[1])
    nb = want[1]["out4"][0]
    assert c.memory()["em_score_tf"] - before >= 16 * nb + 4 * n
    mem = c.memory()
    assert mem["total"] == sum(x for key, x in mem.items() if key != "total")
    for start, count in ((-1, 1), (0, nb + 1), (nb, 1), (nb + 1, 0), (0, -1)):
        with pytest.raises(ValueError, match="range"):
            c.cluster_bridges_copy(start, count)
    for start, count in ((-1, 1), (0, n + 1), (n, 1), (0, -1)):
        with pytest.raises(ValueError, match="range"):
            c.cluster_bridges_cores_copy(start, count)
    assert all(len(a) == 0 for a in c.cluster_bridges_copy(nb, 0)) and len(c.cluster_bridges_cores_copy(n, 0)) == 0
    with pytest.raises(ValueError, match="level"):
        c.cluster_bridges(5)
    assert c.cluster_bridges_info()[0] == 1  # a call that fails its argument checks touches nothing, as the metrics'
    # metrics, then bridges, then metrics: neither disturbs the other, and the labels stay
    keep = level <= 1
    exp = metrics_oracle(n, u[keep], v[keep], labels[1])
    assert c.cluster_metrics(1) == exp[4]
    m0 = [a.tobytes() for a in c.cluster_metrics_copy(0, n)]
    b0 = device_result(c, 0, n)
    B.same(b0, want[0])
    assert c.cluster_metrics_info()[0] == 1 and [a.tobytes() for a in c.cluster_metrics_copy(0, n)] == m0
    assert c.cluster_metrics(0) == metrics_oracle(n, u[level <= 0], v[level <= 0], labels[0])[4]
    assert c.cluster_bridges_info()[0] == 0
    for a, k in zip(c.cluster_bridges_copy(0, b0["out4"][0]), ("u", "v", "side_u", "side_v")):
        assert a.tobytes() == b0[k].tobytes()
    assert c.cluster_bridges_cores_copy(0, n).tobytes() == b0["core"].tobytes()
    for k in range(2):
        assert np.array_equal(c.components_sweep_copy(k, 0, n), labels[k])
    # timing
    c.enable_timing(True)
    c.cluster_bridges(1)
    assert c.cluster_bridges_info()[2] >= 0.0
    c.enable_timing(False)
    c.cluster_bridges(1)
    assert c.cluster_bridges_info()[2] == -1.0
    # a merged level: the stored edges are one shard's
    c.components_sweep_merge(1, np.arange(n, dtype=U32))
    assert c.cluster_bridges_info() == NO_RESULT
    with pytest.raises(RuntimeError, match="merged"):
        c.cluster_bridges(1)
    # the next sweep, the release and new tables drop the result
    c.components_sweep_edges(n, u, v, None, [])
    c.cluster_bridges(0)
    c.components_sweep_edges(n, u, v, None, [])
    assert c.cluster_bridges_info() == NO_RESULT
    c.cluster_bridges(0)
    held = c.memory()["em_score_tf"]
    c.components_sweep_release()
    assert held - c.memory()["em_score_tf"] >= 16 * nb + 4 * n + 4 * n + 8 * 257
    assert c.cluster_bridges_info() == NO_RESULT
    with pytest.raises(RuntimeError, match="no sweep"):
        c.cluster_bridges(0)
    c.components_sweep_edges(4, np.array([0], dtype=U32), np.array([3], dtype=U32), None, [])
    assert c.cluster_bridges(0) == (1, 4, 1, 1)
    c.table_create(0, 300, 1)
    assert c.cluster_bridges_info() == NO_RESULT


def test_spk_cluster_drops_the_result(amd):
    from splink_amd import _native as N
    c = N.Context(0)
    rng = np.random.Generator(np.random.PCG64(9))
    n_rows = 200
    c.table_create(0, n_rows, 1)
    c.table_set_key(0, 0, 0, rng.integers(0, 17, n_rows).astype(np.int64))
    c.table_set_rank(0, rng.permutation(n_rows).astype(np.int64))
    c.components_sweep_edges(n_rows, np.array([0, 5], dtype=U32), np.array([3, 9], dtype=U32), None, [])
    assert c.cluster_bridges(0) == (2, n_rows, 1, 1) and c.cluster_bridges_info()[:2] == (0, 2)
    c.cluster(n_rows)
    assert c.cluster_bridges_info() == NO_RESULT
    with pytest.raises(RuntimeError, match="no sweep"):
        c.cluster_bridges(0)
    with pytest.raises(RuntimeError, match="no bridges"):
        c.cluster_bridges_cores_copy(0, 1)


def frame(d):
    return pd.DataFrame(d) if d else None


def scored(g, amd):
    from splink_amd import Splink
    linker = Splink(copy.deepcopy(g["settings_in"]), amd if g["jaro"] else "supress_warnings", df=frame(g.get("df")),
                    df_l=frame(g.get("df_l")), df_r=frame(g.get("df_r")))
    return linker, linker.get_scored_comparisons()


def test_bridges_leave_components_scores_tf_em_the_selection_and_the_sweep_alone(amd):
    from splink_amd import _native as N
    g = load_golden("link_tf")
    linker, df_e = scored(g, amd)
    job = df_e.job
    pdf = df_e.toPandas()
    t = float(pdf["match_probability"].median())
    hi = float(pdf["match_probability"].quantile(0.8))
    tf_col = next(c["col_name"] for c in df_e.settings["comparison_columns"] if c["term_frequency_adjustments"])

    def state(with_bridges):
        """Select, label, sweep and count, optionally find the bridges, then everything they must not have touched."""
        f = df_e.filter(f"match_probability >= {t!r}")
        k = f.count()
        assert 0 < k < len(pdf)
        n_nodes = job.ctx.components()[0]
        job.ctx.components_sweep(N.SEL_MP, [hi, t])
        scalars = job.ctx.cluster_metrics(1)
        if with_bridges:
            assert job.ctx.cluster_bridges(1)[0] > 0 and job.ctx.cluster_bridges(0)[1] > 0
        assert job.ctx.cluster_metrics_info()[0] == 1
        sweep = [job.ctx.components_sweep_copy(lv, 0, n_nodes) for lv in range(2)]
        sweep += list(job.ctx.cluster_metrics_copy(0, n_nodes))
        labels = job.ctx.components_copy(0, n_nodes)
        sel = job.ctx.select_copy(0, k, len(df_e.gammas.meta[0]))
        col = job._col_index[(tf_col, "str")]
        nv = job.ctx.tf_column_values(col)
        scale = job.ctx.tf_scales_column(col, nv)
        limbs, counts = job.ctx.tf_accumulate_column_exact(col, nv, scale)
        tf = linker.make_term_frequency_adjustments(df_e).toPandas()
        stats = job.em_stats(df_e.lam, df_e.level_probs)
        mp = job.score(df_e.lam, df_e.level_probs)
        return [labels, np.array(scalars)] + sweep + list(sel) + [scale.copy(), limbs.copy(), counts.copy(), stats.copy(),
                                                                   mp.copy()], tf
    job.score(df_e.lam, df_e.level_probs, want_host=False)
    plain, tf0 = state(False)
    job.score(df_e.lam, df_e.level_probs, want_host=False)
    job.selection_owner = None  # select again, as the first time
    found, tf1 = state(True)
    for a, b in zip(plain, found):
        assert np.array_equal(a, b, equal_nan=True)
    pd.testing.assert_frame_equal(tf0, tf1, check_exact=True)


# ---- 7. pipeline -------------------------------------------------------------------------------------------------------
def golden_case(name):
    if name.startswith("link_options/"):
        return load_golden("link_options")[name[len("link_options/"):]]
    return load_golden(name)


def node_ids(filtered, kept):
    """The kept pairs of a filtered frame as node ids (input positions; two tables: left rows, then right), through
    the records' unique ids, as the cluster frame lists them."""
    records = filtered.clusters().toPandas()
    uid = filtered.settings["unique_id_column_name"]
    lt = filtered.job.link_type
    if lt == "dedupe_only":
        key = {x: i for i, x in enumerate(records[uid])}
        l, r = [key[x] for x in kept[uid + "_l"]], [key[x] for x in kept[uid + "_r"]]
    else:
        if lt == "link_only":
            src = (["left"] * len(kept), ["right"] * len(kept))
        else:
            src = (kept["_source_table_l"], kept["_source_table_r"])
        key = {x: i for i, x in enumerate(zip(records["_source_table"], records[uid]))}
        l = [key[x] for x in zip(src[0], kept[uid + "_l"])]
        r = [key[x] for x in zip(src[1], kept[uid + "_r"])]
    return records, np.array(l, dtype=U32), np.array(r, dtype=U32)


def check_frames(filtered, br, min_cluster=3):
    """A ClusterBridges of the filtered frame's pairs against the oracle over filter(...).toPandas()."""
    from splink_amd.frames import bridge_edge_columns
    kept = filtered.toPandas()
    records, l, r = node_ids(filtered, kept)
    n = len(records)
    want = B.oracle(n, l, r)
    assert np.bincount(records["cluster_id"]).max() >= min_cluster and want["out4"][0] > 0
    uid = filtered.settings["unique_id_column_name"]
    e = br.edges()
    assert list(e.columns) == bridge_edge_columns(filtered.settings, filtered.job.link_type)
    assert (br.n_bridges, br.n_cores, br.largest_core, br.depth) == want["out4"] and br.rounds == br.depth + 1
    ids = records[uid].to_numpy()
    for col, exp in ((uid + "_l", ids[want["u"]]), (uid + "_r", ids[want["v"]]), ("nodes_l", want["side_u"]),
                     ("nodes_r", want["side_v"])):
        assert np.array_equal(e[col].to_numpy(), exp), col
    assert np.array_equal(e["cluster_id"].to_numpy(), records["cluster_id"].to_numpy()[want["u"]])
    sizes = np.bincount(records["cluster_id"], minlength=n)
    assert np.array_equal(e["n_nodes"].to_numpy(), sizes[e["cluster_id"]]) and e["n_nodes"].dtype == np.int64
    # every bridge row is a row of the filtered frame, with the same left and right ids
    pair_cols = [c for c in e.columns if c.endswith("_l") and c != "nodes_l" or c.endswith("_r") and c != "nodes_r"]
    merged = e[pair_cols].merge(kept[pair_cols].drop_duplicates(), on=pair_cols, how="left", indicator=True)
    assert len(merged) == len(e) and (merged["_merge"] == "both").all()
    two = br.edges(min_side=2)
    between = e[np.minimum(e["nodes_l"], e["nodes_r"]) >= 2].reset_index(drop=True)
    pd.testing.assert_frame_equal(two, between, check_exact=True)
    cores = br.cores()
    assert list(cores.columns) == list(records.columns) + ["core_id"]
    pd.testing.assert_frame_equal(cores[list(records.columns)], records, check_exact=True)
    assert np.array_equal(cores["core_id"].to_numpy(), want["core"]) and cores["core_id"].dtype == np.int64
    return e, cores


@pytest.mark.parametrize("name", ["synthetic_cfg1", "link_options/link_only_plain_rules"])
def test_pipeline_bridges_match_the_oracle_over_the_filtered_pairs(name, amd):
    g = golden_case(name)
    _, df_e = scored(g, amd)
    scores = df_e.toPandas()["match_probability"]
    # synthetic_cfg1: the median (a cluster of 63 records, 104 bridges, 11 of them between groups); the link_only golden
    # has four pairs, which form one path of five records only below its lowest score
    t = float(scores.median()) if name == "synthetic_cfg1" else float(scores.min()) / 2
    filtered = df_e.filter(f"match_probability > {t!r}")
    br = df_e.clusters(t).bridges()
    e, cores = check_frames(filtered, br)
    other = float(scores.quantile(0.9))
    sweep = df_e.clusters_at_thresholds([other, t])
    for again in (sweep.bridges(t), sweep.at(t).bridges()):
        pd.testing.assert_frame_equal(again.edges(), e, check_exact=True)
        pd.testing.assert_frame_equal(again.cores(), cores, check_exact=True)
        assert (again.n_bridges, again.n_cores, again.largest_core, again.depth) == (br.n_bridges, br.n_cores,
                                                                                     br.largest_core, br.depth)
    # another frame's sweep in between: bridges(t) sweeps again
    df_e.clusters(other).metrics()
    pd.testing.assert_frame_equal(sweep.bridges(t).edges(), e, check_exact=True)
    with pytest.raises(ValueError, match="thresholds"):
        sweep.bridges(2.5)


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


def test_link_only_with_permuted_tables_maps_nodes_back_to_the_right_ids(amd):
    df = synthetic_tables(4000, seed=10)
    rng = np.random.Generator(np.random.PCG64(10))
    side = rng.random(len(df)) < 0.5
    left = df[side].sample(frac=1.0, random_state=1).reset_index(drop=True)
    right = df[~side].sample(frac=1.0, random_state=2).reset_index(drop=True)
    df_e = scored_job(amd, "link_only", [left, right])
    for p in df_e.job.perm:
        assert p is not None and not np.array_equal(p, np.arange(len(p)))
    scores = df_e.toPandas()["match_probability"]
    t = float(np.quantile(scores, 0.9))
    filtered = df_e.filter(f"match_probability > {t!r}")
    e, _ = check_frames(filtered, filtered.clusters().bridges())
    # a left id is a left table's id and a right id a right table's: the orientation is the selection's
    assert set(e["unique_id_l"]) <= set(left["unique_id"]) and set(e["unique_id_r"]) <= set(right["unique_id"])


# ---- 8. refusals -------------------------------------------------------------------------------------------------------
def test_refusals(amd):
    from splink_amd.expectation_step import run_expectation_step
    from splink_amd.maximisation_step import run_maximisation_step
    from splink_amd.params import Params
    data = {"unique_id_l": np.arange(50), "unique_id_r": np.arange(50) + 1, "gamma_c0": np.arange(50) % 3 - 1}
    settings = {"link_type": "dedupe_only", "blocking_rules": [],
                "comparison_columns": [{"col_name": "c0", "num_levels": 2}]}
    params = Params(settings, "supress_warnings")
    table_e = run_expectation_step(pd.DataFrame(data), params, params.settings, amd)
    for make in (lambda: table_e.clusters(0.5).bridges(), lambda: table_e.clusters_at_thresholds([0.5]).bridges(0.5)):
        with pytest.raises(ValueError, match="gamma table"):
            make()
    df = synthetic_tables(1500, seed=12)
    whole = scored_job(amd, "dedupe_only", [df])
    one, sweep = whole.clusters(0.5), whole.clusters_at_thresholds([0.9, 0.5])
    found = sweep.bridges(0.5)
    whole.job.force_reduce = True  # the sharded path at one rank, as the merge tests force it
    try:
        for call in (one.bridges, lambda: sweep.bridges(0.5), lambda: sweep.at(0.5).bridges()):
            with pytest.raises(ValueError, match="sharded job"):
                call()
    finally:
        whole.job.force_reduce = False
    for x in (found,):
        with pytest.raises(ValueError, match="cluster frame"):
            run_maximisation_step(x, params, amd)
