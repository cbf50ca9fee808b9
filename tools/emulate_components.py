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

components_sweep adds the levels of spk_components_sweep, components_merge the rounds of spk_components_merge (one
launch per round: the jump, then per node the star edges to the other ranks' labels), under the same model.

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


def components_sweep(n_nodes, u, v, level, n_levels, climb=CLIMB, round_cap=ROUND_CAP, prefix=False):
    """spk_components_sweep's levels under the same model: edge i is new at level[i] (>= n_levels: in no level) and
    belongs to every later level.  Level k starts from level k - 1's final labels (level 0: label[v] = v) and runs
    rounds whose hook launch takes the level's new edges and whose jump launch also hooks, for every node v, the star
    edge (v, label_{k-1}[v]) -- against the jump launch's own snapshot, landing at its end.  prefix=True is the other
    variant: the hook takes every edge up to the level and the jump is the plain one.  A level without new edges runs
    no round.  Returns (labels uint32 [n_levels, n_nodes], rounds per level)."""
    u = np.asarray(u, dtype=np.int64)
    v = np.asarray(v, dtype=np.int64)
    level = np.asarray(level, dtype=np.int64)
    nodes = np.arange(n_nodes, dtype=np.int64)
    label = nodes.copy()
    out, rounds_per_level = [], []
    for k in range(n_levels):
        prev = label.copy()
        mine = level <= k if prefix else level == k
        hu, hv = u[mine], v[mine]
        rounds = 0
        quiet = not (level == k).any()
        while not quiet:
            if rounds == round_cap:
                raise RuntimeError("level %d: no fixed point within %d rounds" % (k, round_cap))
            before = label.copy()
            a, b = _climb(label, hu, climb), _climb(label, hv, climb)
            ne = a != b
            if ne.any():
                nxt = label.copy()
                np.minimum.at(nxt, np.maximum(a[ne], b[ne]), np.minimum(a[ne], b[ne]))
                label = nxt
            up = _climb(label, nodes, climb)
            nxt = np.minimum(label, up)
            if k > 0 and not prefix:
                b = _climb(label, prev, climb)
                ne = up != b
                if ne.any():
                    np.minimum.at(nxt, np.maximum(up[ne], b[ne]), np.minimum(up[ne], b[ne]))
            label = nxt
            rounds += 1
            quiet = np.array_equal(label, before)
        out.append(label.astype(np.uint32))
        rounds_per_level.append(rounds)
    return np.stack(out) if out else np.empty((0, n_nodes), dtype=np.uint32), rounds_per_level


def components_merge(label, peers, climb=CLIMB, round_cap=ROUND_CAP):
    """spk_components_merge's rounds under the same model: `label` is one rank's final labels, peers [P, n] the other
    ranks' over the same node ids.  A round is one launch (there is no edge list, so no hook launch): per node v the
    jump, then for every peer p the star edge (v, peers[p][v]) -- an entry equal to v is skipped -- every climb against
    the launch's own snapshot, every write landing at its end.  A hook re-parents the larger end only if it is a root
    (the device's compare-and-swap against its own id: the rank's own components live in the labels alone, so no node
    may be cut off its parent).  At least one round runs; the loop ends after the first one in which every star edge
    had equal ends and no word was lowered.  Returns (labels uint32 [n], rounds)."""
    label = np.asarray(label, dtype=np.int64).copy()
    peers = np.asarray(peers, dtype=np.int64).reshape(-1, len(label))
    nodes = np.arange(len(label), dtype=np.int64)
    if ((peers > nodes) | (peers < 0)).any():
        raise ValueError("a peer label is greater than its own index")
    for rounds in range(1, round_cap + 1):
        before = label
        up = _climb(label, nodes, climb)
        nxt = np.minimum(label, up)
        hooked = False  # a star edge with different ends: the round is not quiet, whether or not its swap lands
        for q in peers:
            star = q != nodes
            a, b = up[star], _climb(label, q[star], climb)
            ne = a != b
            hooked |= bool(ne.any())
            hi, lo = np.maximum(a[ne], b[ne]), np.minimum(a[ne], b[ne])
            root = label[hi] == hi  # the device swaps the larger end only while it is its own label
            if root.any():
                np.minimum.at(nxt, hi[root], lo[root])
        label = nxt
        if np.array_equal(label, before) and not hooked:
            return label.astype(np.uint32), rounds
    raise RuntimeError("merge: no fixed point within %d rounds" % round_cap)


def deal_edges(n_edges, parts, how):
    """The part of every edge: "round_robin" (edge i to part i % parts, so a long path forms only in the union) or
    "blocks" (contiguous ranges of the edge list)."""
    i = np.arange(n_edges, dtype=np.int64)
    if how == "round_robin":
        return i % parts
    if how == "blocks":
        return i * parts // max(n_edges, 1)
    raise ValueError(how)


def alternating_path(n=65536):
    """The path 0 - 1 - ... - n-1 in two levels: the odd edges (2i+1, 2i+2) are level 0, the even ones (2i, 2i+1)
    level 1, so level 1 joins n / 2 pairs into one path."""
    a = np.arange(n - 1, dtype=np.uint32)
    return n, a, a + 1, ((a + 1) % 2).astype(np.int64)


def random_levels(n_edges, n_levels, seed, none=0.1):
    """A seeded level per edge in [0, n_levels), about a tenth of the edges in no level (n_levels)."""
    rng = np.random.default_rng(seed)
    level = rng.integers(0, n_levels, n_edges)
    level[rng.random(n_edges) < none] = n_levels
    return level


def union_find_levels(n_nodes, u, v, level, n_levels):
    """union_find of the edges with level <= k, for every k: uint32 [n_levels, n_nodes]."""
    level = np.asarray(level)
    u, v = np.asarray(u), np.asarray(v)
    return np.stack([union_find(n_nodes, u[level <= k], v[level <= k]) for k in range(n_levels)])


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
        n_levels = 4 if name == "hub" else 8
        level = random_levels(len(u), n_levels, seed=n_levels)
        want = union_find_levels(n, u, v, level, n_levels)
        for prefix in (False, True):
            got, rounds = components_sweep(n, u, v, level, n_levels, prefix=prefix)
            print("%-7s sweep of %d levels, %s: rounds %s  labels %s" % (
                name, n_levels, "every edge up to the level" if prefix else "new edges and star edges", rounds,
                "equal" if np.array_equal(got, want) else "DIFFER"))
        want = union_find(n, u, v)
        for parts in (2, 3, 8):
            for how in ("round_robin", "blocks"):
                part = deal_edges(len(u), parts, how)
                own = [components(n, u[part == p], v[part == p]) for p in range(parts)]
                got, rounds = components_merge(own[0][0], np.stack([lab for lab, _ in own[1:]]))
                print("%-7s merge of %d parts dealt %-11s: own rounds %s  merge rounds %3d  labels %s" % (
                    name, parts, how, [r for _, r in own], rounds, "equal" if np.array_equal(got, want) else "DIFFER"))


if __name__ == "__main__":
    main()
