"""clusters_at_thresholds() and the cluster metrics: the entry points, the header, the host emulation of the nested
sweep's rounds, the thresholds' validation, the column names and the closed forms of the metrics (no GPU)."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from sweep_common import emulation, metrics_oracle

from splink_amd import _native as N

SYMBOLS = ["spk_components_sweep", "spk_components_sweep_edges", "spk_components_sweep_copy",
           "spk_components_sweep_info", "spk_components_sweep_release", "spk_cluster_metrics",
           "spk_cluster_metrics_copy", "spk_cluster_metrics_info"]
ROUNDS = 64  # a quarter of the device's cap per level, as test_components_host.py holds for one run


def test_native_and_frame_methods_exist():
    from splink_amd import BestMatchFrame, ClusterFrame, ClusterMetrics, ClusterSweepFrame, FilteredFrame
    from splink_amd.frames import ExpectationFrame
    from splink_amd.term_frequencies import TermFrequencyFrame, TfFilteredFrame
    for name in ("components_sweep", "components_sweep_edges", "components_sweep_copy", "components_sweep_info",
                 "components_sweep_release", "cluster_metrics", "cluster_metrics_copy"):
        assert callable(getattr(N.Context, name)), name
    for cls in (FilteredFrame, BestMatchFrame, TfFilteredFrame, ExpectationFrame, TermFrequencyFrame):
        assert callable(cls.clusters_at_thresholds), cls
    for name in ("toPandas", "at", "summary", "metrics"):
        assert callable(getattr(ClusterSweepFrame, name)), name
    assert callable(ClusterFrame.metrics) and callable(ClusterMetrics.clusters) and callable(ClusterMetrics.nodes)
    assert set(SYMBOLS) <= set(N.EXPORTS)
    assert N.SEL_ALL == -1 and N.SWEEP_MAX_LEVELS == 32


def test_header_declares_the_symbols_and_the_library_has_them():
    raw = open(os.path.join(ROOT, "include", "splink_hip.h")).read()
    assert re.search(r"#define SPK_SEL_ALL \(-1\)", raw) and re.search(r"#define SPK_SWEEP_MAX_LEVELS 32\b", raw)
    for later in ("cluster_pairwise_predictions_at_multiple_thresholds", "compute_graph_metrics"):
        assert later in raw
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for name in SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(\s*spk_ctx \*ctx" % name, text), name
    lib = N.load_library()
    for name in SYMBOLS:
        assert hasattr(lib, name), name


def check_emulated(n, u, v, level, n_levels, climb=None, prefix=False):
    emu = emulation()
    want = emu.union_find_levels(n, u, v, level, n_levels)
    got, rounds = emu.components_sweep(n, u, v, level, n_levels, climb=climb or emu.CLIMB, prefix=prefix)
    assert got.dtype == np.uint32 and got.shape == (n_levels, n) and np.array_equal(got, want)
    assert len(rounds) == n_levels and max(rounds) <= ROUNDS, rounds
    return want, rounds


@pytest.mark.parametrize("name,n_levels", [("path", 8), ("hub", 4), ("random", 8)])
def test_emulated_sweep_reaches_the_union_find_labels_of_every_level(name, n_levels):
    emu = emulation()
    n, u, v = emu.GRAPHS[name]()
    level = emu.random_levels(len(u), n_levels, seed=n_levels)
    assert set(np.unique(level)) == set(range(n_levels + 1))  # every level, and edges of none
    want, rounds = check_emulated(n, u, v, level, n_levels)
    assert (np.diff(want.astype(np.int64), axis=0) <= 0).all()  # a level's labels never rise
    print(name, "rounds per level", rounds)


def test_emulated_sweep_on_the_alternating_path():
    emu = emulation()
    n, u, v, level = emu.alternating_path()
    assert n == 65536 and np.count_nonzero(level == 0) == n // 2 - 1 and np.count_nonzero(level == 1) == n // 2
    want, rounds = check_emulated(n, u, v, level, 2)
    assert np.count_nonzero(want[0] == np.arange(n)) == n // 2 + 1 and (want[1] == 0).all()
    check_emulated(n, u, v, level, 2, prefix=True)


def test_emulated_sweep_on_tiny_random_graphs():
    rng = np.random.default_rng(17)
    for i in range(300):
        n = int(rng.integers(1, 13))
        m = int(rng.integers(0, 25))
        n_levels = int(rng.integers(1, 6))
        u, v = rng.integers(0, n, m), rng.integers(0, n, m)
        level = rng.integers(0, n_levels + 1, m)
        for climb in (2, 8):
            check_emulated(n, u, v, level, n_levels, climb=climb, prefix=i % 3 == 0)


def test_threshold_validation():
    from splink_amd.frames import sweep_thresholds
    given, desc, level = sweep_thresholds([0.5, 0.99, 0.9])
    assert given == [0.5, 0.99, 0.9] and desc.tolist() == [0.99, 0.9, 0.5] and level == [2, 0, 1]
    assert desc.dtype == np.float64
    given, desc, level = sweep_thresholds((float("-inf"), 1, float("inf")))
    assert desc.tolist() == [float("inf"), 1.0, float("-inf")] and level == [2, 1, 0]
    assert len(sweep_thresholds(np.linspace(0, 1, 32))[0]) == 32
    for bad in ([], [0.5, float("nan")], [0.5, 0.5], [0.1, 0.2, 0.1], np.linspace(0, 1, 33), 0.5, ["a"]):
        with pytest.raises(ValueError):
            sweep_thresholds(bad)


def test_column_names_and_order():
    from splink_amd.frames import sweep_column_names
    assert sweep_column_names([0.5, 0.99, 1.0, 1e-3]) == ["cluster_id_0.5", "cluster_id_0.99", "cluster_id_1.0",
                                                           "cluster_id_0.001"]


def closed_forms(n, u, v):
    """(density, centralisation) of the one cluster that holds node 0, through the oracle's integer arrays."""
    from splink_amd.frames import cluster_metric_columns
    emu = emulation()
    labels = emu.union_find(n, u, v)
    _, size, degree_sum, max_degree, _ = metrics_oracle(n, u, v, labels)
    edges, density, central = cluster_metric_columns(size[:1], degree_sum[:1], max_degree[:1])
    return int(size[0]), int(edges[0]), float(density[0]), float(central[0])


def test_density_and_centralisation_closed_forms():
    k = 7
    star = closed_forms(k, np.zeros(k - 1, dtype=int), np.arange(1, k))
    assert star == (k, k - 1, 2.0 / k, 1.0)
    i, j = np.triu_indices(k, 1)
    assert closed_forms(k, i, j) == (k, k * (k - 1) // 2, 1.0, 0.0)
    n, e, density, central = closed_forms(k, np.arange(k - 1), np.arange(1, k))  # a path: two ends of degree 1
    assert (n, e, density) == (k, k - 1, 2.0 / k) and central == (k * 2 - 2 * (k - 1)) / ((k - 1) * (k - 2))
    n, e, density, central = closed_forms(2, [0], [1])
    assert (n, e, density) == (2, 1, 1.0) and np.isnan(central)
    n, e, density, central = closed_forms(1, [], [])
    assert (n, e) == (1, 0) and np.isnan(density) and np.isnan(central)


def test_the_new_frames_are_refused_by_the_stage_functions():
    from splink_amd.frames import ClusterMetrics, ClusterSweepFrame, reject_filtered
    for cls in (ClusterSweepFrame, ClusterMetrics):
        with pytest.raises(ValueError, match="cluster frame"):
            reject_filtered(cls.__new__(cls), "run_maximisation_step")
