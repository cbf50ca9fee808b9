"""The stages that run after scoring share one HIP-event stopwatch (one lazily created event pair in the context) and
spk_components* / spk_components_sweep* share one round loop.

1. The stages back to back on one context, with timing off, on, and switched on halfway: every stage's results are the
   same in every run, and every *_info time says whether its own stage was timed.
2. components_edges and components_sweep_edges without thresholds give the same labels and cluster count."""
import numpy as np
import pytest

from sweep_common import emulation

pytestmark = pytest.mark.gpu
U32 = np.uint32

N_ROWS = 64
LEVELS = [2, 3]
M = np.array([0.2, 0.8, 0.1, 0.3, 0.6])  # per column and level: the higher the level, the likelier a match
U = np.array([0.8, 0.2, 0.6, 0.3, 0.1])
LAM = 0.3


@pytest.fixture(scope="module")
def native():
    from splink_amd import _native
    if _native.device_count() == 0:
        pytest.fail("no HIP device visible: the -m gpu tests need an MI355X")
    return _native


class Case:
    """About 5,000 pairs over 64 records: more than two select chunks with a partial last one.  The 63 edges of the
    path 0 - 1 - ... - 63 are spread over all the chunks and carry the top pattern, so every selection below keeps them
    and the kept graph has one component, which takes more than one round."""

    def __init__(self, N):
        self.n = n = 2 * N.SELECT_CHUNK + 904
        rng = np.random.Generator(np.random.PCG64(23))
        self.g = np.stack([rng.integers(-1, L, n) for L in LEVELS], axis=1).astype(np.int8)
        self.rows_l = rng.integers(0, N_ROWS, n).astype(np.int32)
        self.rows_r = rng.integers(0, N_ROWS, n).astype(np.int32)
        path = np.arange(N_ROWS - 1) * 79  # 62 * 79 = 4898 < n
        assert path[-1] < n and path[-1] // N.SELECT_CHUNK == 2
        self.rows_l[path] = np.arange(N_ROWS - 1)
        self.rows_r[path] = np.arange(1, N_ROWS)
        self.g[path] = [1, 2]
        self.path = path
        self.ids = [rng.integers(-1, 20, N_ROWS).astype(np.int64) for _ in range(2)]  # tf value ids of the two sides
        table = rng.random(20)
        table[[1, 2, 3]] = [np.nan, 0.0, 1.0]
        self.tables = [table]
        self.labels = (np.arange(N_ROWS) // 4).astype(np.int64)
        self.labels[::7] = -1


def run_stages(N, c, case, on_from):
    """select, select_tf, select_best, components, components_sweep, cluster_metrics x 2, label_histogram, pairs_sample
    on context c; timing is off for the stages before index `on_from` and on from there (0: on throughout, None:
    never).  Returns (results per stage, ms per stage, stages that ran with timing on)."""
    res, ms, timed = {}, {}, {}
    c.enable_timing(False)
    c.pairs_load(case.rows_l, case.rows_r)
    c.gammas_load(LEVELS, case.g)
    K = len(LEVELS)
    mp_term = (N.SEL_MP, 0, N.SEL_OP[">"], 0.5)

    def stage(index, name):
        if on_from is not None and index >= on_from:
            c.enable_timing(True)
        timed[name] = on_from is not None and index >= on_from

    stage(0, "select")
    k = c.select(LAM, 1 - LAM, M, U, [mp_term])
    assert c.select_info()[0] == k
    res["select"] = (k,) + c.select_copy(0, k, K)
    ms["select"] = c.select_info()[1]

    stage(1, "select_tf")
    k = c.select_tf(LAM, 1 - LAM, M, U, case.ids[:1], case.ids[1:], case.tables, [mp_term])
    res["select_tf"] = (k,) + c.select_copy(0, k, K) + c.select_copy_tf(0, k, 1)
    ms["select_tf"] = c.select_info()[1]

    stage(2, "select_best")
    kept = c.select_best(N.SEL_MP, N.BEST_L, 1)
    before, kept_info, ms["select_best"] = c.select_best_info()
    assert (before, kept_info) == (k, kept) and 0 < kept < k
    res["select_best"] = (kept,) + c.select_copy(0, kept, K) + c.select_copy_tf(0, kept, 1)
    # spk_select_info keeps its meaning: the time of the selecting call
    assert c.select_info() == (kept, ms["select_tf"])

    stage(3, "components")
    n_nodes, n_clusters, rounds = c.components()
    assert rounds >= 2
    res["components"] = (n_nodes, n_clusters, c.components_copy(0, n_nodes))
    ms["components"] = c.components_info()[3]

    stage(4, "components_sweep")
    top = float(res["select_best"][5].max())
    n_nodes, n_edges, n_clusters, rounds = c.components_sweep(N.SEL_MP, [np.nextafter(top, 0.0), 0.0])
    assert rounds[0] >= 2 and n_edges[1] == kept
    res["components_sweep"] = (n_nodes, n_edges, n_clusters, c.components_sweep_copy(0, 0, n_nodes),
                               c.components_sweep_copy(1, 0, n_nodes))
    ms["components_sweep"] = c.components_sweep_info()[3]

    for level in (0, 1):
        name = f"cluster_metrics_{level}"
        stage(5 + level, name)
        res[name] = (c.cluster_metrics(level),) + c.cluster_metrics_copy(0, n_nodes)
        assert c.cluster_metrics_info()[0] == level
        ms[name] = c.cluster_metrics_info()[1]

    stage(7, "label_histogram")
    res["label_histogram"] = c.label_histogram(case.labels, None, LAM, 1 - LAM, M, U)
    pairs, ms["label_histogram"] = c.label_info()
    assert pairs == case.n

    stage(8, "pairs_sample")
    n_out = c.pairs_sample(N.LINK_TYPES["dedupe_only"], 5, 3000, 0, 3000)
    draws, kept_draws, ms["pairs_sample"] = c.pairs_sample_info()
    assert (draws, kept_draws) == (3000, n_out) and 0 < n_out <= 3000
    res["pairs_sample"] = (n_out,) + c.pairs_copy(0, n_out)
    c.enable_timing(False)
    return res, ms, timed


def same(a, b):
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()  # bit for bit, NaN included
    return a == b


def check_times(ms, timed):
    for name, on in timed.items():
        print(f"{name}: timing {'on' if on else 'off'}, ms {ms[name]!r}")
    for name, on in timed.items():
        if on:
            assert ms[name] > 0.0, name  # every stage here launches at least one kernel
        else:
            assert ms[name] == -1.0, name


def test_stages_in_sequence_share_one_stopwatch(native):
    N = native
    case = Case(N)

    def context():
        c = N.Context(0)
        c.table_create(0, N_ROWS, 1)
        c.table_set_rank(0, np.arange(N_ROWS, dtype=np.int64))
        return c
    c = context()
    off, ms, timed = run_stages(N, c, case, None)
    assert not any(timed.values())
    check_times(ms, timed)
    # what the sequence is meant to exercise
    k, ordinal = off["select"][0], off["select"][1]
    chunks = np.bincount(ordinal // N.SELECT_CHUNK, minlength=3)
    assert len(chunks) == 3 and (chunks > 0).all() and np.isin(case.path, ordinal).all() and k < case.n
    assert np.isin(case.path, off["select_best"][1]).all()
    assert off["components"][1] == 1 and (off["components"][2] == 0).all()
    n_edges, n_clusters = off["components_sweep"][1], off["components_sweep"][2]
    assert 0 < n_edges[0] <= n_edges[1] and n_clusters.tolist() == [1, 1]
    assert off["cluster_metrics_1"][0] == (1, N_ROWS, N_ROWS)
    assert off["label_histogram"][0].sum() == case.n

    on, ms, timed = run_stages(N, c, case, 0)  # the event pair is created by the first stage
    assert all(timed.values())
    check_times(ms, timed)
    # the pair exists by now; the stages before the switch must still report no time
    half, ms, timed = run_stages(N, c, case, 3)
    assert [on_ for on_ in timed.values()] == [False] * 3 + [True] * 6
    check_times(ms, timed)
    # a context of its own: the pair is created in the middle of the sequence, by components
    fresh, ms, timed = run_stages(N, context(), case, 3)
    check_times(ms, timed)
    for name in off:
        for other in (on, half, fresh):
            assert same(off[name], other[name]), name


def _graphs():
    emu = emulation()
    rng = np.random.Generator(np.random.PCG64(31))
    none = np.empty(0, dtype=U32)
    return {
        "no_nodes": lambda: (0, none, none),
        "no_edges": lambda: (5, none, none),
        "path": emu.path_graph,
        "hub": emu.hub_graph,
        "random": lambda: (1000, rng.integers(0, 1000, 300).astype(U32), rng.integers(0, 1000, 300).astype(U32)),
    }


@pytest.mark.parametrize("name", ["no_nodes", "no_edges", "path", "hub", "random"])
def test_components_and_sweep_share_the_round_loop(name, native):
    n, u, v = _graphs()[name]()
    u, v = np.asarray(u, dtype=U32), np.asarray(v, dtype=U32)
    c = native.Context(0)
    n_clusters, _ = c.components_edges(n, u, v)
    labels = c.components_copy(0, n)
    n_edges, sweep_clusters, _ = c.components_sweep_edges(n, u, v, None, [])
    sweep_labels = c.components_sweep_copy(0, 0, n)
    assert n_edges.tolist() == [len(u)]
    assert sweep_clusters.tolist() == [n_clusters]
    assert labels.dtype == sweep_labels.dtype == U32 and np.array_equal(labels, sweep_labels)
    want = emulation().union_find(n, u.astype(np.int64), v.astype(np.int64))
    assert np.array_equal(labels, want) and n_clusters == int(np.count_nonzero(want == np.arange(n)))
