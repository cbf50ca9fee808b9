"""Host emulation of spk_bridges.hip's launches (numpy, no GPU): bridges, side sizes and cores of a multigraph from a
level-synchronous spanning forest and cycle marking.

The model is the least favourable one the device allows: inside one launch every plain load sees the arrays as they
stood when the launch began, and among the compare-and-swaps on one depth word the winner is arbitrary -- here drawn
from a seeded generator, so different seeds build different spanning forests over the same depths.

    init    depth[v] = 0 at the roots (label[v] == v), unvisited elsewhere
    forest  round d, per edge (u, v) with u != v: one end at depth d, the other unvisited in the snapshot -> that end
            is claimed at depth d + 1 by one of the edges that try; parent and pedge (the edge's index) are the winner's
    mark    per edge with u != v that is the tree edge of neither end: walk both ends up to their meeting point, the
            deeper first, and mark every node left (at most 2 * max depth steps)
    sub     d = max depth .. 1: sub[parent[x]] += sub[x] for the nodes at depth d
    bridges the nodes x with depth[x] > 0 and mark[x] == 0 own the bridge pedge[x]; side of x = sub[x], the other side
            = sub[label[x]] - sub[x]; sorted by (u, v) in the stored orientation
    cores   the components' rounds (tools/emulate_components.py) over the edges that are neither bridge nor self-loop

The loop ends after the first round that claims nothing, so rounds = max depth + 1 (0 without edges), whatever the
winners.

    python tools/emulate_bridges.py            # the test graphs: rounds, bridges, cores
"""
import importlib.util
import os

import numpy as np

MAX_ROUNDS = 4096  # spk_bridges.hip: BR_MAX_ROUNDS
UNVISITED = -1


def _components_module():
    spec = importlib.util.spec_from_file_location(
        "emulate_components", os.path.join(os.path.dirname(os.path.abspath(__file__)), "emulate_components.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


_CC = _components_module()


def forest(n_nodes, u, v, label, seed=0, max_rounds=MAX_ROUNDS):
    """(depth, parent, pedge, rounds) of the spanning forest rooted at the nodes with label[x] == x."""
    rng = np.random.default_rng(seed)
    u = np.asarray(u, dtype=np.int64)
    v = np.asarray(v, dtype=np.int64)
    nodes = np.arange(n_nodes, dtype=np.int64)
    depth = np.where(np.asarray(label, dtype=np.int64) == nodes, 0, UNVISITED).astype(np.int64)
    parent = nodes.copy()
    pedge = np.full(n_nodes, -1, dtype=np.int64)
    idx = np.arange(len(u), dtype=np.int64)
    loop = u == v
    rounds = 0
    quiet = len(u) == 0
    while not quiet:
        if rounds == max_rounds:
            raise RuntimeError("a spanning tree deeper than %d" % (max_rounds - 1))
        du, dv = depth[u], depth[v]  # the snapshot
        fwd = ~loop & (du == rounds) & (dv == UNVISITED)
        bwd = ~loop & (dv == rounds) & (du == UNVISITED)
        child = np.concatenate([v[fwd], u[bwd]])
        par = np.concatenate([u[fwd], v[bwd]])
        edge = np.concatenate([idx[fwd], idx[bwd]])
        if len(child):
            order = rng.permutation(len(child))  # the arrival order of the compare-and-swaps
            _, first = np.unique(child[order], return_index=True)
            win = order[first]
            depth[child[win]] = rounds + 1
            parent[child[win]] = par[win]
            pedge[child[win]] = edge[win]
        rounds += 1
        quiet = len(child) == 0
    return depth, parent, pedge, rounds


def marks(u, v, depth, parent, pedge):
    """mark[x] = 1 iff x's tree edge lies on the fundamental cycle of some non-tree edge."""
    u = np.asarray(u, dtype=np.int64)
    v = np.asarray(v, dtype=np.int64)
    idx = np.arange(len(u), dtype=np.int64)
    walk = (u != v) & (pedge[u] != idx) & (pedge[v] != idx)
    a, b = u[walk].copy(), v[walk].copy()
    da, db = depth[a].copy(), depth[b].copy()
    mark = np.zeros(len(depth), dtype=np.uint8)
    bound = 2 * int(depth.max()) if len(depth) else 0
    for _ in range(bound):
        live = a != b
        if not live.any():
            break
        up_a = live & (da >= db)
        up_b = live & ~up_a
        mark[a[up_a]] = 1
        mark[b[up_b]] = 1
        a[up_a] = parent[a[up_a]]
        da[up_a] -= 1
        b[up_b] = parent[b[up_b]]
        db[up_b] -= 1
    assert (a == b).all(), "a walk did not meet within 2 * max depth steps"
    return mark


def bridges(n_nodes, u, v, label=None, seed=0, max_rounds=MAX_ROUNDS):
    """The device's result under the model above, as a dict: u, v, side_u, side_v (uint32, sorted by (u, v)), core
    (uint32 [n_nodes]), out4 = (bridges, cores, largest core, max depth), rounds."""
    u = np.asarray(u, dtype=np.int64)
    v = np.asarray(v, dtype=np.int64)
    if label is None:
        label = _CC.union_find(n_nodes, u, v)
    label = np.asarray(label, dtype=np.int64)
    depth, parent, pedge, rounds = forest(n_nodes, u, v, label, seed, max_rounds)
    assert (depth != UNVISITED).all(), "a node stayed unvisited"
    max_depth = rounds - 1 if rounds else 0
    assert max_depth == (int(depth.max()) if n_nodes else 0)
    mark = marks(u, v, depth, parent, pedge)
    sub = np.ones(n_nodes, dtype=np.int64)
    for d in range(max_depth, 0, -1):
        at = np.flatnonzero(depth == d)
        np.add.at(sub, parent[at], sub[at])
    own = np.flatnonzero((depth > 0) & (mark == 0))
    e = pedge[own]
    bu, bv = u[e], v[e]
    mine, rest = sub[own], sub[label[own]] - sub[own]
    side_u = np.where(bu == own, mine, rest)
    side_v = np.where(bu == own, rest, mine)
    order = np.argsort((bu << 32) | bv, kind="stable")
    is_bridge = np.zeros(len(u), dtype=bool)
    is_bridge[e] = True
    keep = ~is_bridge & (u != v)
    core, _ = _CC.components(n_nodes, u[keep], v[keep])
    sizes = np.bincount(core, minlength=n_nodes) if n_nodes else np.zeros(0, dtype=np.int64)
    n_cores = int((core == np.arange(n_nodes)).sum())
    return {"u": bu[order].astype(np.uint32), "v": bv[order].astype(np.uint32),
            "side_u": side_u[order].astype(np.uint32), "side_v": side_v[order].astype(np.uint32),
            "core": core.astype(np.uint32),
            "out4": (len(own), n_cores, int(sizes.max()) if n_nodes else 0, max_depth), "rounds": rounds}


def main():
    for name, make in _CC.GRAPHS.items():
        n, u, v = make() if name != "path" else make(2000)
        got = bridges(n, u, v)
        print("%-7s nodes %7d edges %7d: rounds %5d  bridges %6d  cores %7d  largest core %6d" % (
            name, n, len(u), got["rounds"], got["out4"][0], got["out4"][1], got["out4"][2]))


if __name__ == "__main__":
    main()
