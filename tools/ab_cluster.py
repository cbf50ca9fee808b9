"""Connected components of the kept pairs against the selection and against the host route, at cfg2 (1 M records,
~46 M pairs).

(a) device time and rounds of spk_components over the survivors of `match_probability > 0.9` (spk_components_info,
    HIP events around its launches) next to spk_select's time on the same pairs (spk_select_info);
(b) wall time of df_e.filter(cond).clusters().toPandas() against the route without clusters():
    df_e.filter(cond).toPandas(), then a union-find over the unique ids on the host
    (scipy.sparse.csgraph.connected_components when importable, else numpy min-label rounds).

Each figure is the median of `reps` runs after one warm-up, from fresh frames (no cached result).

    python tools/ab_cluster.py [threshold] [reps] [out.json]
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402,F401
from splink_amd.engine import Job  # noqa: E402
from splink_amd.frames import ExpectationFrame, GammaFrame  # noqa: E402
from splink_amd.params import Params  # noqa: E402
from splink_amd.session import AmdSession  # noqa: E402
from splink_amd.synthetic import cfg_settings, make_records  # noqa: E402

try:
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
except ImportError:
    connected_components = None

thr = float(sys.argv[1]) if len(sys.argv) > 1 else 0.9
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 10
out_path = sys.argv[3] if len(sys.argv) > 3 else None

cols = ["first_name", "surname", "dob", "city", "email"]
df = make_records(1_000_000, surname_vocab=15000, arrow=True)[["unique_id"] + cols]
params = Params(cfg_settings(2), AmdSession(0))
st = params.settings
job = Job("dedupe_only", [df], "unique_id", 0)
job.ctx.enable_timing(True)
job.block(st["blocking_rules"])
gf = GammaFrame(job, st)
lam, probs = params.params["λ"], params._level_probabilities()
cond = f"match_probability > {thr!r}"
res = {"config": 2, "records": len(df), "pairs": int(job.n_pairs), "condition": cond,
       "host_route": "scipy connected_components" if connected_components else "numpy min-label rounds"}


def fresh():
    return ExpectationFrame(gf, st, lam, probs)


def host_clusters(uid_all, uid_l, uid_r):
    """cluster_id per record from the kept pairs' unique ids: the smallest input position of the component."""
    n = len(uid_all)
    order = np.argsort(uid_all, kind="stable")
    u = order[np.searchsorted(uid_all, uid_l, sorter=order)]
    v = order[np.searchsorted(uid_all, uid_r, sorter=order)]
    if connected_components is not None:
        g = coo_matrix((np.ones(len(u), dtype=np.int8), (u, v)), shape=(n, n))
        _, comp = connected_components(g, directed=False)
        first = np.full(comp.max() + 1 if n else 0, n, dtype=np.int64)
        np.minimum.at(first, comp, np.arange(n))
        return first[comp]
    label = np.arange(n, dtype=np.int64)
    while True:  # hook to the smaller label, then jump until flat
        a, b = label[u], label[v]
        if np.array_equal(a, b):
            return label
        np.minimum.at(label, np.maximum(a, b), np.minimum(a, b))
        while True:
            up = label[label]
            if np.array_equal(up, label):
                break
            label = up


# (a) device time: spk_select, then spk_components over its survivors
select_ms, comp_ms = [], []
for i in range(reps + 1):
    f = fresh().filter(cond)
    res["survivors"] = int(f.count())
    _, s_ms = job.ctx.select_info()
    c = f.clusters()
    res["n_clusters"], res["rounds"] = int(c.n_clusters), int(c.rounds)
    _, _, _, c_ms = job.ctx.components_info()
    if i:
        select_ms.append(s_ms)
        comp_ms.append(c_ms)
res["spk_select_ms_median"] = float(np.median(select_ms))
res["spk_select_ms_min"] = float(min(select_ms))
res["spk_components_ms_median"] = float(np.median(comp_ms))
res["spk_components_ms_min"] = float(min(comp_ms))

# (b) wall time to one cluster_id per record
ts = []
for i in range(reps + 1):
    f = fresh().filter(cond)
    t0 = time.perf_counter()
    got = f.clusters().toPandas()
    if i:
        ts.append(time.perf_counter() - t0)
res["clusters_toPandas_s_median"] = float(np.median(ts))
res["clusters_toPandas_s_min"] = float(min(ts))
ts = []
uid_all = df["unique_id"].to_numpy()
for i in range(reps + 1):
    job._host_cols = {}  # the host route converts the retained input columns again in every run
    f = fresh().filter(cond)
    t0 = time.perf_counter()
    kept = f.toPandas()
    host = host_clusters(uid_all, kept["unique_id_l"].to_numpy(), kept["unique_id_r"].to_numpy())
    if i:
        ts.append(time.perf_counter() - t0)
res["filter_toPandas_then_host_s_median"] = float(np.median(ts))
res["filter_toPandas_then_host_s_min"] = float(min(ts))
res["identical"] = bool(np.array_equal(got["cluster_id"].to_numpy(), host))
sizes = np.bincount(got["cluster_id"].to_numpy())
res["largest_cluster"] = int(sizes.max())
res["records_in_clusters_of_2_or_more"] = int(sizes[sizes > 1].sum())
print(json.dumps(res))
if out_path:
    with open(out_path, "w") as fh:
        json.dump(res, fh, indent=1)
