"""Shared by test_bridges_host.py and test_gpu_cluster_bridges.py: the oracle of bridges, side sizes and cores (an
iterative low-link DFS that tells parallel edges apart by index, plus union-find), the emulation module, and the test
graphs.  The test's own code, no graph library; nothing here touches the device."""
import importlib.util
import os

import numpy as np

from conftest import ROOT

_EMU = None


def emulation():
    """tools/emulate_bridges.py as a module."""
    global _EMU
    if _EMU is None:
        spec = importlib.util.spec_from_file_location("emulate_bridges", os.path.join(ROOT, "tools", "emulate_bridges.py"))
        _EMU = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(_EMU)
    return _EMU


# ---- the oracle -------------------------------------------------------------------------------------------------------
def _union_find(n, u, v):
    """Smallest id of every node's component (path halving, link to the smaller id), as a list."""
    p = list(range(n))

    def find(x):
        while p[x] != x:
            p[x] = p[p[x]]
            x = p[x]
        return x

    for a, b in zip(u, v):
        a, b = find(a), find(b)
        if a != b:
            p[max(a, b)] = min(a, b)
    return [find(x) for x in range(n)]


def _adjacency(n, u, v):
    """CSR of the edges without self-loops: per node its (neighbour, edge index) entries."""
    keep = [i for i in range(len(u)) if u[i] != v[i]]
    deg = [0] * (n + 1)
    for i in keep:
        deg[u[i] + 1] += 1
        deg[v[i] + 1] += 1
    for x in range(n):
        deg[x + 1] += deg[x]
    start = deg[:]
    fill = deg[:n]
    nbr, eid = [0] * start[n], [0] * start[n]
    for i in keep:
        a, b = u[i], v[i]
        nbr[fill[a]], eid[fill[a]] = b, i
        fill[a] += 1
        nbr[fill[b]], eid[fill[b]] = a, i
        fill[b] += 1
    return start, nbr, eid


def bridge_edges(n, u, v):
    """Indices of the bridges: low-link DFS, iterative; the edge a node was entered by is skipped by its index, so a
    second copy of it is a back edge and the pair is no bridge."""
    start, nbr, eid = _adjacency(n, u, v)
    disc, low = [-1] * n, [0] * n
    out = []
    clock = 0
    for s in range(n):
        if disc[s] >= 0:
            continue
        disc[s] = low[s] = clock
        clock += 1
        stack = [(s, -1, start[s])]
        while stack:
            x, via, pos = stack[-1]
            if pos < start[x + 1]:
                stack[-1] = (x, via, pos + 1)
                y, e = nbr[pos], eid[pos]
                if e == via:
                    continue
                if disc[y] >= 0:
                    if disc[y] < low[x]:
                        low[x] = disc[y]
                else:
                    disc[y] = low[y] = clock
                    clock += 1
                    stack.append((y, e, start[y]))
            else:
                stack.pop()
                if stack:
                    px = stack[-1][0]
                    if low[x] < low[px]:
                        low[px] = low[x]
                    if low[x] > disc[px]:
                        out.append(via)
    return sorted(out)


def _bfs_depth(n, u, v, label):
    """The largest breadth-first distance of a node from its component's smallest id."""
    start, nbr, _ = _adjacency(n, u, v)
    dist = [0 if label[x] == x else -1 for x in range(n)]
    frontier = [x for x in range(n) if label[x] == x]
    d = 0
    while frontier:
        nxt = []
        for x in frontier:
            for pos in range(start[x], start[x + 1]):
                y = nbr[pos]
                if dist[y] < 0:
                    dist[y] = d + 1
                    nxt.append(y)
        if nxt:
            d += 1
        frontier = nxt
    return d


def oracle(n, u, v):
    """What spk_cluster_bridges must give for the multigraph (u, v) over n nodes, as a dict: u, v, side_u, side_v
    (uint32, ascending by (u, v), stored orientation), core (uint32 [n]), out4 = (bridges, cores, largest core, depth).

    Sides: contract every core (a component of the graph minus all bridges, by union-find) to a point; the bridges
    then form a forest over the cores, and a bridge's two sides are the node counts of its deeper core's subtree and
    of the rest of the cluster."""
    u = [int(x) for x in np.asarray(u).tolist()]
    v = [int(x) for x in np.asarray(v).tolist()]
    label = _union_find(n, u, v)
    br = bridge_edges(n, u, v)
    is_bridge = set(br)
    rest = [i for i in range(len(u)) if i not in is_bridge]
    core = _union_find(n, [u[i] for i in rest], [v[i] for i in rest])
    core_size = [0] * n
    for x in range(n):
        core_size[core[x]] += 1
    cluster_size = [0] * n
    for x in range(n):
        cluster_size[label[x]] += 1
    # the bridge forest over the cores, rooted at each cluster's own core (label[x] is the smallest id: core[label] = label)
    adj = {}
    for i in br:
        a, b = core[u[i]], core[v[i]]
        adj.setdefault(a, []).append(b)
        adj.setdefault(b, []).append(a)
    depth, parent, order = {}, {}, []
    for root in sorted({label[c] for c in adj}):
        depth[root], parent[root] = 0, root
        stack = [root]
        while stack:
            x = stack.pop()
            order.append(x)
            for y in adj[x]:
                if y not in depth:
                    depth[y], parent[y] = depth[x] + 1, x
                    stack.append(y)
    subtree = {c: core_size[c] for c in depth}
    for x in reversed(order):
        if parent[x] != x:
            subtree[parent[x]] += subtree[x]
    rows = []
    for i in br:
        a, b = core[u[i]], core[v[i]]
        child_is_u = depth[a] > depth[b]
        low = subtree[a if child_is_u else b]
        other = cluster_size[label[u[i]]] - low
        rows.append((u[i], v[i], low if child_is_u else other, other if child_is_u else low))
    rows.sort()
    cols = [np.array([r[k] for r in rows], dtype=np.uint32) for k in range(4)]
    n_cores = sum(1 for x in range(n) if core[x] == x)
    return {"u": cols[0], "v": cols[1], "side_u": cols[2], "side_v": cols[3], "core": np.array(core, dtype=np.uint32),
            "out4": (len(br), n_cores, max(core_size) if n else 0, _bfs_depth(n, u, v, label))}


def brute_force(n, u, v):
    """The definition itself, for small graphs: delete each stored edge in turn and label what is left.  Returns the
    rows (u, v, side_u, side_v) sorted, to check the oracle with."""
    u = [int(x) for x in np.asarray(u).tolist()]
    v = [int(x) for x in np.asarray(v).tolist()]
    rows = []
    for i in range(len(u)):
        if u[i] == v[i]:
            continue
        lab = _union_find(n, u[:i] + u[i + 1:], v[:i] + v[i + 1:])
        if lab[u[i]] != lab[v[i]]:
            rows.append((u[i], v[i], lab.count(lab[u[i]]), lab.count(lab[v[i]])))
    return sorted(rows)


def same(got, want):
    """Every output of a result dict equals the oracle's, element for element."""
    for k in ("u", "v", "side_u", "side_v", "core"):
        assert got[k].dtype == np.uint32 and np.array_equal(got[k], want[k]), k
    assert tuple(got["out4"]) == tuple(want["out4"]), (got["out4"], want["out4"])


# ---- the graphs --------------------------------------------------------------------------------------------------------
def _arr(pairs):
    a = np.array(pairs, dtype=np.uint32).reshape(-1, 2)
    return a[:, 0].copy(), a[:, 1].copy()


TRIANGLE = [(1, 2), (2, 3), (3, 1)]
TRIANGLE_B = [(5, 6), (6, 7), (7, 5)]


def degenerate_graphs():
    """name -> (n_nodes, u, v): the shapes on which a bridge finder goes wrong first."""
    g = {
        "no_edges": (5, []),
        "self_loops": (4, [(1, 1), (3, 3), (0, 0)]),
        "one_edge": (4, [(2, 1)]),
        "edge_twice": (4, [(1, 2), (1, 2)]),
        "edge_twice_reversed": (4, [(1, 2), (2, 1)]),
        "triangle": (5, TRIANGLE),
        "triangle_pendant": (6, TRIANGLE + [(3, 4)]),
        "triangles_one_edge": (9, TRIANGLE + TRIANGLE_B + [(3, 5)]),
        "triangles_two_edges": (9, TRIANGLE + TRIANGLE_B + [(3, 5), (6, 2)]),
        "triangles_shared_node": (8, TRIANGLE + [(3, 5), (5, 6), (6, 3)]),
        # node 0 idle, with the padding self-loops (0, 0) of the odd edge count in range; 4, 8 and 9 idle too
        "idle_nodes": (10, [(1, 2), (2, 3), (3, 1), (5, 6), (6, 7)]),
    }
    return {k: (n,) + _arr(p) for k, (n, p) in g.items()}


def chain_of_edges(m, seed=1):
    """m edges over m // 2 + 3 nodes: a path with chords, so some edges are bridges and some are not."""
    rng = np.random.default_rng(seed + m)
    n = m // 2 + 3
    path = np.arange(n - 1, dtype=np.uint32)
    extra = m - (n - 1)
    a = rng.integers(0, n, extra).astype(np.uint32)
    b = np.minimum(a + rng.integers(0, 4, extra).astype(np.uint32), n - 1).astype(np.uint32)
    u, v = np.concatenate([path, a]), np.concatenate([path + 1, b])
    k = rng.permutation(m)
    return n, u[k], v[k]


def permuted_path(n=2000, seed=3):
    """One path through a seeded permutation of the ids, edges shuffled, orientations mixed; also returns the order."""
    rng = np.random.default_rng(seed)
    order = rng.permutation(n).astype(np.uint32)
    u, v = order[:-1].copy(), order[1:].copy()
    flip = rng.random(n - 1) < 0.5
    u[flip], v[flip] = order[1:][flip], order[:-1][flip]
    k = rng.permutation(n - 1)
    return n, u[k], v[k], order


def permuted_cycle(n=4096, tail=0, seed=6):
    """A cycle of n nodes in permuted ids, and a path of `tail` more nodes hanging off it."""
    rng = np.random.default_rng(seed)
    ids = rng.permutation(n + tail).astype(np.uint32)
    ring = ids[:n]
    u, v = ring.copy(), np.roll(ring, -1)
    if tail:
        chain = np.concatenate([ring[:1], ids[n:]])
        u, v = np.concatenate([u, chain[:-1]]), np.concatenate([v, chain[1:]])
    k = rng.permutation(len(u))
    return n + tail, u[k], v[k]


def barbell(clique=64, seed=7):
    """Two cliques and one edge between them."""
    rng = np.random.default_rng(seed)
    i, j = np.triu_indices(clique, 1)
    u = np.concatenate([i, j + clique, [clique - 1]]).astype(np.uint32)
    v = np.concatenate([j, i + clique, [clique]]).astype(np.uint32)
    k = rng.permutation(len(u))
    return 2 * clique, u[k], v[k]


def id_order_path(n):
    """0 - 1 - ... - n-1: rooted at node 0, depth n - 1."""
    a = np.arange(n - 1, dtype=np.uint32)
    return n, a, a + 1


def random_multigraph(rng, n_max=14, m_max=24):
    """A small seeded multigraph with self-loops, repeats and reversed repeats."""
    n = int(rng.integers(1, n_max + 1))
    m = int(rng.integers(0, m_max + 1))
    u = rng.integers(0, n, m)
    v = rng.integers(0, n, m)
    if m:
        d = rng.integers(0, m, m // 4)
        o = rng.integers(0, m, m // 4)
        u, v = np.concatenate([u, u[d], v[o]]), np.concatenate([v, v[d], u[o]])
    k = rng.permutation(len(u))
    return n, u[k].astype(np.uint32), v[k].astype(np.uint32)
