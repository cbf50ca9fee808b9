"""Shared by tests/test_components_merge_host.py and tests/test_gpu_components_merge.py: the three test graphs of
tools/emulate_components.py, their edges dealt over P parts, and the union-find labels of the whole, computed once."""
import functools
import importlib.util
import os

import numpy as np

from conftest import ROOT

GRAPH_NAMES = ("path", "hub", "random")   # 65,536-node shuffled path; 20,000-leaf star + 256-clique + idle; 200,000 / 150,000
PARTS = (2, 3, 8)
DEALINGS = ("round_robin", "blocks")
ROUND_CAP = 256  # CC_MAX_ROUNDS


@functools.lru_cache(maxsize=None)
def emulation():
    spec = importlib.util.spec_from_file_location("emulate_components", os.path.join(ROOT, "tools", "emulate_components.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def union_find(n_nodes, u, v):
    """label[x] = the smallest id of x's component: find with path halving, link to the smaller id (independent of
    the emulation and of the device)."""
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


@functools.lru_cache(maxsize=None)
def graph(name):
    """(n_nodes, u, v, union-find labels of all edges); the arrays are shared between tests and read-only."""
    n, u, v = emulation().GRAPHS[name]()
    want = union_find(n, u, v)
    for a in (u, v, want):
        a.setflags(write=False)
    return n, u, v, want


def dealt(name, parts, how):
    """The graph's edges as `parts` edge lists [(u, v), ...]."""
    n, u, v, _ = graph(name)
    part = emulation().deal_edges(len(u), parts, how)
    return [(u[part == p], v[part == p]) for p in range(parts)]
