"""Bridges and cores of the clusters on the device (spk_cluster_bridges) at cfg2 (1 M records, ~46 M pairs, initial
parameters): the pairs with match_probability > 0.95, > 0.3, and every pair.

(a) device ms of spk_cluster_bridges over the one-level sweep that clusters(t).bridges() takes, its forest rounds, and
    bridges / cores / largest core / depth; wall time of clusters(t).bridges() with its copies;
(b) today's route on the same pairs, its wall time broken down: filter(...).toPandas(), the unique ids to node ids, and
    networkx.bridges over the kept pairs (the host oracle of tests/bridges_common.py where networkx is missing).  Its
    bridge count must equal the device's.  Not run over every pair: a host graph of 46 M edges is out of reach;
(c) the whole call on the hub graph of tools/emulate_components.py and on one clique of 2,048 nodes, for the A/B of
    the marking launch with and without the load before the store: run `marks` with the library as built and with
    SPLINK_AMD_LIB naming the variant (tools/build_ab.py OUT.so spk_bridges.hip -DBR_MARK_STORE_ALWAYS), the two
    alternating in one session.

Medians of `reps` runs after one warm-up, with the minimum and maximum of each (the run-to-run spread).

    python tools/ab_cluster_bridges.py [reps] [out.log] [marks]      (marks: (c) only)
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402,F401
import emulate_components as emu  # noqa: E402
from splink_amd import _native as N  # noqa: E402
from splink_amd.engine import Job  # noqa: E402
from splink_amd.frames import ExpectationFrame, FilteredFrame, GammaFrame  # noqa: E402
from splink_amd.params import Params  # noqa: E402
from splink_amd.select import Predicate  # noqa: E402
from splink_amd.session import AmdSession  # noqa: E402
from splink_amd.synthetic import cfg_settings, make_records  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
out_path = sys.argv[2] if len(sys.argv) > 2 else None
marks_only = "marks" in sys.argv[3:]
lib = os.path.basename(os.environ.get("SPLINK_AMD_LIB", "libsplink_hip.so"))


def spread(xs):
    return {"median": float(np.median(xs)), "min": float(min(xs)), "max": float(max(xs))}


def emit(row):
    print(json.dumps(row), flush=True)
    if out_path:
        with open(out_path, "a") as fh:
            fh.write(json.dumps(row) + "\n")


def host_bridges(n, u, v):
    """(number of bridges on the host, what found them)."""
    try:
        import networkx as nx
    except ImportError:
        import bridges_common as B
        return len(B.bridge_edges(n, u.tolist(), v.tolist())), "tests/bridges_common.py"
    g = nx.Graph()
    g.add_nodes_from(range(n))
    g.add_edges_from(zip(u.tolist(), v.tolist()))
    return sum(1 for _ in nx.bridges(g)), "networkx.bridges"


# ---- (c) graphs with hot mark words, on host edges -------------------------------------------------------------------
ctx = N.Context(0)
ctx.enable_timing(True)
i, j = np.triu_indices(2048, 1)
for name, (n, u, v) in (("hub", emu.hub_graph()), ("clique of 2048", (2048, i.astype(np.uint32), j.astype(np.uint32)))):
    ctx.components_sweep_edges(n, u, v, None, [])
    ms = []
    first = None
    for rep in range(reps + 1):
        out4 = ctx.cluster_bridges(0)
        got = (out4, ctx.cluster_bridges_copy(0, out4[0])[2].tobytes(), ctx.cluster_bridges_cores_copy(0, n).tobytes())
        first = first or got
        assert got == first
        if rep:
            ms.append(ctx.cluster_bridges_info()[2])
    emit({"lib": lib, "graph": name, "nodes": int(n), "edges": int(len(u)), "out4": list(first[0]),
          "rounds": ctx.cluster_bridges_info()[1], "spk_cluster_bridges_ms": spread(ms)})
ctx.close()
if marks_only:
    sys.exit(0)

# ---- (a), (b) cfg2 -------------------------------------------------------------------------------------------------
cols = ["first_name", "surname", "dob", "city", "email"]
df = make_records(1_000_000, surname_vocab=15000, arrow=True)[["unique_id"] + cols]
params = Params(cfg_settings(2), AmdSession(0))
st = params.settings
job = Job("dedupe_only", [df], "unique_id", 0)
job.ctx.enable_timing(True)
job.block(st["blocking_rules"])
gf = GammaFrame(job, st)
lam, probs = params.params["λ"], params._level_probabilities()
ids = np.asarray(df["unique_id"])
pos = {x: k for k, x in enumerate(ids.tolist())}

for t in (0.95, 0.3, None):
    scored = ExpectationFrame(gf, st, lam, probs)
    filtered = scored.filter(f"match_probability > {t!r}") if t is not None else FilteredFrame(scored, Predicate())
    cf = filtered.clusters()
    cf._sweep_all()
    ms, out4 = [], None
    for rep in range(reps + 1):
        out4 = job.ctx.cluster_bridges(0)
        if rep:
            ms.append(job.ctx.cluster_bridges_info()[2])
    t0 = time.perf_counter()
    br = filtered.clusters().bridges()
    edges = br.edges()
    wall = time.perf_counter() - t0
    row = {"config": 2, "records": len(df), "pairs": int(job.n_pairs), "threshold": t, "reps": reps,
           "edges": int(job.ctx.components_sweep_info()[2]), "bridges": out4[0], "cores": out4[1], "largest_core": out4[2],
           "depth": out4[3], "rounds": job.ctx.cluster_bridges_info()[1], "spk_cluster_bridges_ms": spread(ms),
           "sweep_ms": job.ctx.components_sweep_info()[3],
           "largest_cluster": int(edges["n_nodes"].max()) if len(edges) else 0,
           "bridges_between_groups": int(len(br.edges(min_side=2))), "frame_bridges_edges_wall_s": wall}
    if t is not None:
        t0 = time.perf_counter()
        kept = filtered.toPandas()
        t1 = time.perf_counter()
        u = np.array([pos[x] for x in kept["unique_id_l"].tolist()], dtype=np.uint32)
        v = np.array([pos[x] for x in kept["unique_id_r"].tolist()], dtype=np.uint32)
        t2 = time.perf_counter()
        found, how = host_bridges(len(df), u, v)
        t3 = time.perf_counter()
        assert found == out4[0], (found, out4)
        row["host_route"] = {"toPandas_s": t1 - t0, "node_ids_s": t2 - t1, "bridges_s": t3 - t2, "by": how,
                             "total_s": t3 - t0, "bridges": found}
    emit(row)
