"""Host emulation of spk_components.hip's rounds (numpy, no GPU): how many rounds does min-label hooking with
pointer jumping need on a given graph?

The model is the least favourable one the device allows: inside one launch every plain load sees the label array
as it stood when the launch began (on the device a load may also see a newer, smaller label; the emulation never
does), and the atomic minima land at the end of the launch.  One round is the two launches of
spk_components.hip:

    hook  per edge (u, v):  a = climb(u), b = climb(v)  (label of label ... at most CLIMB loads, stops at a root);
                            a != b:  label[max(a, b)] = min(label[max(a, b)], min(a, b))      (atomic min)
    jump  per node v:       r = climb(v);  r < label[v]:  label[v] = min(label[v], r)          (atomic min)

and the loop ends after the first round in which no atomic lowered a word.  Labels only decrease, and only to ids
of the same component, so at that point every label is the smallest id of its component (see the kernel file).

    python tools/emulate_components.py            # round counts of the test graphs, against a union-find
"""
import numpy as np

CLIMB = 8          # spk_components.hip: CC_CLIMB
ROUND_CAP = 256    # spk_components.hip: CC_MAX_ROUNDS


def union_find(n_nodes, u, v):
    """Smallest id of every node's component: find with path halving, link to the smaller id."""
    p = list(range(n_nodes))

    def find(x):
        while p[x] != x:
            p[x] = p[p[x]]
            x = p[x]
        return x

    for a, b in zip(np.asarray(u).tolist(), np.asarray(v).tolist()):
        a, b = find(a), find(b)
        if a != b:
            p[max(a, b)] = min(a, b)
    return np.array([find(x) for x in range(n_nodes)], dtype=np.uint32)


def _climb(label, x, steps=CLIMB):
    """label[x], then up to steps - 1 more loads of the label's label, against one snapshot."""
    r = label[x]
    for _ in range(steps - 1):
        nxt = label[r]
        if np.array_equal(nxt, r):
            break
        r = nxt
    return r


def components(n_nodes, u, v, climb=CLIMB, round_cap=ROUND_CAP):
    """(labels uint32 [n_nodes], rounds): rounds counts every hook + jump pair run, the last (quiet) one included."""
    u = np.asarray(u, dtype=np.int64)
    v = np.asarray(v, dtype=np.int64)
    label = np.arange(n_nodes, dtype=np.int64)
    nodes = np.arange(n_nodes, dtype=np.int64)
    for rounds in range(1, round_cap + 1):
        before = label.copy()
        a, b = _climb(label, u, climb), _climb(label, v, climb)
        ne = a != b
        if ne.any():
            nxt = label.copy()
            np.minimum.at(nxt, np.maximum(a[ne], b[ne]), np.minimum(a[ne], b[ne]))
            label = nxt
        label = np.minimum(label, _climb(label, nodes, climb))
        if np.array_equal(label, before):
            return label.astype(np.uint32), rounds
    raise RuntimeError("no fixed point within %d rounds" % round_cap)


# ---- the graphs of tests/test_gpu_components.py (cases 3 to 5) ---------------------------------------------------
def path_graph(n=65536, seed=3):
    """One path through a seeded random permutation of the ids, edges shuffled, orientations mixed."""
    rng = np.random.default_rng(seed)
    order = rng.permutation(n).astype(np.uint32)
    u, v = order[:-1].copy(), order[1:].copy()
    flip = rng.random(n - 1) < 0.5
    u[flip], v[flip] = order[1:][flip], order[:-1][flip]
    k = rng.permutation(n - 1)
    return n, u[k], v[k]


def hub_graph(leaves=20000, clique=256, idle=1000, seed=4):
    """A star whose hub has the largest id, a clique, and `idle` nodes without edges."""
    rng = np.random.default_rng(seed)
    n = idle + clique + leaves + 1
    hub = n - 1
    su = np.full(leaves, hub, dtype=np.uint32)
    sv = np.arange(idle + clique, idle + clique + leaves, dtype=np.uint32)
    i, j = np.triu_indices(clique, 1)
    cu, cv = (idle + i).astype(np.uint32), (idle + j).astype(np.uint32)
    u, v = np.concatenate([su, cu]), np.concatenate([sv, cv])
    k = rng.permutation(len(u))
    return n, u[k], v[k]


def random_graph(n=200000, m=150000, seed=5):
    """Seeded random edges, a tenth of them repeated, a tenth repeated the other way round."""
    rng = np.random.default_rng(seed)
    base = m - 2 * (m // 10)
    u = rng.integers(0, n, base, dtype=np.int64).astype(np.uint32)
    v = rng.integers(0, n, base, dtype=np.int64).astype(np.uint32)
    d = rng.integers(0, base, m // 10)
    o = rng.integers(0, base, m // 10)
    uu, vv = np.concatenate([u, u[d], v[o]]), np.concatenate([v, v[d], u[o]])
    k = rng.permutation(m)
    return n, uu[k], vv[k]


GRAPHS = {"path": path_graph, "hub": hub_graph, "random": random_graph}


def main():
    for name, make in GRAPHS.items():
        n, u, v = make()
        want = union_find(n, u, v)
        for climb in (2, CLIMB):
            got, rounds = components(n, u, v, climb=climb, round_cap=ROUND_CAP)
            print("%-7s nodes %7d edges %7d climb %d: rounds %4d  labels %s" % (
                name, n, len(u), climb, rounds, "equal" if np.array_equal(got, want) else "DIFFER"))


if __name__ == "__main__":
    main()
