"""Oracles of spk_cluster_agreement's ten fields, shared by the host and the GPU tests.

agreement_oracle counts from pandas group sizes (sums of C(n, 2) or nL * nR over groups, nunique per group);
agreement_brute enumerates the pairs and the sets.  Neither sorts keys or looks at runs, as the device route does."""
import numpy as np
import pandas as pd

FIELDS = ("records_labelled", "clusters_labelled", "entities", "predicted_pairs", "true_pairs", "tp", "clusters_mixed",
          "entities_split", "entities_recovered", "pairs_total")


def _frame(labels, ids, n_left, cross_only):
    labels = np.asarray(labels, dtype=np.int64)
    ids = np.asarray(ids, dtype=np.int64)
    assert labels.shape == ids.shape and labels.ndim == 1
    side = (np.arange(len(ids)) >= n_left).astype(np.int64) if cross_only else np.zeros(len(ids), dtype=np.int64)
    keep = ids >= 0
    return pd.DataFrame({"c": labels[keep], "g": ids[keep], "side": side[keep]})


def _pairs(df, by, cross_only):
    """Counted pairs whose two nodes agree on the columns `by` (none: all counted pairs)."""
    if not len(df):
        return 0
    sizes = df.groupby(by + ["side"]).size().unstack("side", fill_value=0) if by else \
        df.groupby("side").size().to_frame().T
    n_l = sizes[0].to_numpy().astype(object) if 0 in sizes.columns else np.zeros(len(sizes), dtype=object)
    n_r = sizes[1].to_numpy().astype(object) if 1 in sizes.columns else np.zeros(len(sizes), dtype=object)
    if cross_only:
        return int((n_l * n_r).sum())
    n = n_l + n_r
    return int((n * (n - 1) // 2).sum())


def agreement_oracle(labels, ids, n_left, cross_only):
    """int64 [10] in FIELDS' order for one level's labels."""
    df = _frame(labels, ids, n_left, cross_only)
    out = dict.fromkeys(FIELDS, 0)
    out["records_labelled"] = len(df)
    if len(df):
        ids_of_cluster = df.groupby("c")["g"].nunique()
        by_id = df.groupby("g")["c"].agg(["nunique", "first"])
        out["clusters_labelled"] = len(ids_of_cluster)
        out["entities"] = len(by_id)
        out["clusters_mixed"] = int((ids_of_cluster >= 2).sum())
        out["entities_split"] = int((by_id["nunique"] >= 2).sum())
        alone = ids_of_cluster.reindex(by_id["first"]).to_numpy() == 1
        out["entities_recovered"] = int(((by_id["nunique"].to_numpy() == 1) & alone).sum())
    out["predicted_pairs"] = _pairs(df, ["c"], cross_only)
    out["true_pairs"] = _pairs(df, ["g"], cross_only)
    out["tp"] = _pairs(df, ["c", "g"], cross_only)
    out["pairs_total"] = _pairs(df, [], cross_only)
    return np.array([out[f] for f in FIELDS], dtype=np.int64)


def agreement_brute(labels, ids, n_left, cross_only):
    """The same by enumeration, O(n^2): small cases only."""
    labels, ids = [int(x) for x in labels], [int(x) for x in ids]
    nodes = [v for v in range(len(ids)) if ids[v] >= 0]
    out = dict.fromkeys(FIELDS, 0)
    for a, u in enumerate(nodes):
        for v in nodes[a + 1:]:
            if cross_only and (u < n_left) == (v < n_left):
                continue
            same_c, same_g = labels[u] == labels[v], ids[u] == ids[v]
            out["pairs_total"] += 1
            out["predicted_pairs"] += same_c
            out["true_pairs"] += same_g
            out["tp"] += same_c and same_g
    ids_of_cluster, clusters_of_id = {}, {}
    for v in nodes:
        ids_of_cluster.setdefault(labels[v], set()).add(ids[v])
        clusters_of_id.setdefault(ids[v], set()).add(labels[v])
    out["records_labelled"] = len(nodes)
    out["clusters_labelled"] = len(ids_of_cluster)
    out["entities"] = len(clusters_of_id)
    out["clusters_mixed"] = sum(len(s) >= 2 for s in ids_of_cluster.values())
    out["entities_split"] = sum(len(s) >= 2 for s in clusters_of_id.values())
    out["entities_recovered"] = sum(len(s) == 1 and len(ids_of_cluster[next(iter(s))]) == 1
                                    for s in clusters_of_id.values())
    return np.array([out[f] for f in FIELDS], dtype=np.int64)


def labels_of_edges(n_nodes, u, v):
    """label[x] = the smallest node id of x's component (union-find on the host), as spk_components* define it."""
    parent = np.arange(n_nodes, dtype=np.int64)

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for a, b in zip(np.asarray(u).tolist(), np.asarray(v).tolist()):
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    return np.array([find(x) for x in range(n_nodes)], dtype=np.int64)
