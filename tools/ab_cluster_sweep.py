"""Clusters at several thresholds: the nested sweep against one select + components per threshold, at cfg2 (1 M
records, ~46 M pairs, initial parameters), thresholds 0.99 0.95 0.9 0.8 0.7 0.6 0.5 0.3.

(a) device ms of one wide spk_select + spk_components_sweep against the sum over the thresholds of spk_select +
    spk_components (the existing entry points), the two routes alternating in one process;
(b) wall time of clusters_at_thresholds(ts).toPandas() against the loop of clusters(t).toPandas();
(c) spk_cluster_metrics ms per level, next to a pandas groupby over the kept pairs of that level;
(d) rounds per level, next to the separate runs';
(e) the shipped edge-set variant (new edges and star edges) against the other (every edge up to the level).

Medians of `reps` runs after one warm-up, with the minimum and maximum of each (the run-to-run spread).

    python tools/ab_cluster_sweep.py [reps] [out.log]
"""
import json
import os
import sys
import time

import numpy as np
import pandas as pd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402,F401
from splink_amd.engine import Job  # noqa: E402
from splink_amd.frames import ExpectationFrame, GammaFrame  # noqa: E402
from splink_amd.params import Params  # noqa: E402
from splink_amd.session import AmdSession  # noqa: E402
from splink_amd.synthetic import cfg_settings, make_records  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
out_path = sys.argv[2] if len(sys.argv) > 2 else None
TS = [0.99, 0.95, 0.9, 0.8, 0.7, 0.6, 0.5, 0.3]

cols = ["first_name", "surname", "dob", "city", "email"]
df = make_records(1_000_000, surname_vocab=15000, arrow=True)[["unique_id"] + cols]
params = Params(cfg_settings(2), AmdSession(0))
st = params.settings
job = Job("dedupe_only", [df], "unique_id", 0)
job.ctx.enable_timing(True)
job.block(st["blocking_rules"])
gf = GammaFrame(job, st)
lam, probs = params.params["λ"], params._level_probabilities()
res = {"config": 2, "records": len(df), "pairs": int(job.n_pairs), "thresholds": TS, "reps": reps}


def fresh():
    return ExpectationFrame(gf, st, lam, probs)


def spread(xs):
    return {"median": float(np.median(xs)), "min": float(min(xs)), "max": float(max(xs))}


def sweep_route(mode):
    """One wide select and the sweep: (select ms, sweep ms, rounds per level)."""
    job.ctx.components_sweep_set_mode(mode)
    try:
        s = fresh().clusters_at_thresholds(TS)
        s._run()
    finally:
        job.ctx.components_sweep_set_mode(0)
    return job.ctx.select_info()[1], job.ctx.components_sweep_info()[3], [int(r) for r in s._info[3]]


def loop_route():
    """One select and one components per threshold: (sum of select ms, sum of components ms, rounds per threshold)."""
    sel = comp = 0.0
    rounds = []
    for t in TS:
        c = fresh().clusters(t)
        rounds.append(int(c.rounds))
        sel += job.ctx.select_info()[1]
        comp += job.ctx.components_info()[3]
    return sel, comp, rounds


# (a), (d), (e): device time, the three routes alternating
runs = {"sweep": [], "sweep_every_edge": [], "loop": []}
for i in range(reps + 1):
    for name, call in (("loop", loop_route), ("sweep", lambda: sweep_route(0)), ("sweep_every_edge", lambda: sweep_route(1))):
        out = call()
        if i:
            runs[name].append(out)
for name, rs in runs.items():
    res[name + "_select_ms"] = spread([r[0] for r in rs])
    res[name + "_components_ms"] = spread([r[1] for r in rs])
    res[name + "_device_ms"] = spread([r[0] + r[1] for r in rs])
    res[name + "_rounds"] = rs[-1][2]

# (b) wall time to the labels on the host, alternating
wall = {"sweep": [], "loop": []}
for i in range(reps + 1):
    t0 = time.perf_counter()
    parts = [fresh().clusters(t).toPandas()["cluster_id"].to_numpy() for t in TS]
    t1 = time.perf_counter()
    got = fresh().clusters_at_thresholds(TS).toPandas()
    t2 = time.perf_counter()
    if i:
        wall["loop"].append(t1 - t0)
        wall["sweep"].append(t2 - t1)
res["loop_toPandas_s"] = spread(wall["loop"])
res["sweep_toPandas_s"] = spread(wall["sweep"])
res["identical"] = all(np.array_equal(got[f"cluster_id_{t!r}"].to_numpy(), p) for t, p in zip(TS, parts))

# (c) metrics per level on the device, next to pandas over the kept pairs of that level
sweep = fresh().clusters_at_thresholds(TS)
res["summary"] = sweep.summary().to_dict(orient="list")
metrics_ms, pandas_s = [], []
wide = fresh().filter(f"match_probability > {min(TS)!r}").toPandas()[["unique_id_l", "unique_id_r", "match_probability"]]
for t in TS:
    k = sweep._level_of(t)
    ms = []
    for i in range(reps + 1):
        sweep._held()
        job.ctx.cluster_metrics(k)
        if i:
            ms.append(job.ctx.cluster_metrics_info()[1])
    metrics_ms.append(spread(ms))
    labels = pd.Series(sweep._labels[k].astype(np.int64), index=df["unique_id"].to_numpy())
    t0 = time.perf_counter()
    kept = wide[wide["match_probability"] > t]
    degree = pd.concat([kept["unique_id_l"], kept["unique_id_r"]]).value_counts()
    per = pd.DataFrame({"cluster_id": labels, "d": degree.reindex(labels.index, fill_value=0)}).groupby("cluster_id")["d"]
    host = pd.DataFrame({"n_nodes": per.size(), "degree_sum": per.sum(), "max_degree": per.max()})
    pandas_s.append(time.perf_counter() - t0)
    m = sweep.metrics(t).clusters()
    assert np.array_equal(m["n_nodes"].to_numpy(), host["n_nodes"].to_numpy())
    assert np.array_equal(2 * m["n_edges"].to_numpy(), host["degree_sum"].to_numpy())
res["cluster_metrics_ms"] = metrics_ms
res["pandas_groupby_s"] = pandas_s
print(json.dumps(res))
if out_path:
    with open(out_path, "w") as fh:
        json.dump(res, fh, indent=1)
