"""Shared by test_cluster_sweep_host.py and test_gpu_cluster_sweep.py: the host emulation module, levels as scores and
thresholds, and the numpy oracle of the cluster metrics.  Nothing here touches the device."""
import importlib.util
import os

import numpy as np

from conftest import ROOT

_EMU = None


def emulation():
    """tools/emulate_components.py as a module (its graphs, union-find and emulated sweep)."""
    global _EMU
    if _EMU is None:
        spec = importlib.util.spec_from_file_location("emulate_components",
                                                      os.path.join(ROOT, "tools", "emulate_components.py"))
        _EMU = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(_EMU)
    return _EMU


def thresholds_for(n_levels):
    """n_levels - 1, ..., 1, 0: strictly descending, one per level."""
    return np.arange(n_levels - 1, -1, -1, dtype=np.float64)


def scores_for(level, n_levels):
    """A score per edge that puts it in its level under thresholds_for(n_levels): threshold + 0.5 for an edge of a
    level; the edges of no level take, in turn, the lowest threshold itself (the test is strict), a lower score, NaN."""
    level = np.asarray(level, dtype=np.int64)
    score = (n_levels - 1 - level) + 0.5
    out = np.flatnonzero(level >= n_levels)
    score[out] = np.array([0.0, -3.25, np.nan])[np.arange(len(out)) % 3]
    return score


def metrics_oracle(n, u, v, labels):
    """(degree, size, degree_sum, max_degree, (clusters of >= 2 nodes, nodes in them, largest cluster)) of the graph
    (u, v) over n nodes whose components are `labels`; the per-cluster arrays sit at the roots, 0 elsewhere."""
    u = np.asarray(u, dtype=np.int64)
    v = np.asarray(v, dtype=np.int64)
    labels = np.asarray(labels, dtype=np.int64)
    degree = np.zeros(n, dtype=np.int64)
    np.add.at(degree, u, 1)
    np.add.at(degree, v, 1)
    size = np.bincount(labels, minlength=n).astype(np.int64)
    degree_sum = np.zeros(n, dtype=np.int64)
    np.add.at(degree_sum, labels, degree)
    max_degree = np.zeros(n, dtype=np.int64)
    np.maximum.at(max_degree, labels, degree)
    multi = size[size >= 2]
    scalars = (len(multi), int(multi.sum()), int(size.max()) if n else 0)
    return degree, size, degree_sum, max_degree, scalars
