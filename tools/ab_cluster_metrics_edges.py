"""spk_cluster_metrics' edge pass: one atomic add per edge end against counting, inside the wave, the lanes that share
the first lane's end (spk_cluster_metrics_set_mode 0 / 1), on the graphs of tools/emulate_components.py.

The hub graph (a 20,000-leaf star and a 256-clique) is run with its edges shuffled, as the tests hand them over, and
sorted by their first end, so that whole waves sit on the hub word -- the order a selection's pairs have, which come
in ascending pair ordinal with a block's left rows together.  Device ms of the whole spk_cluster_metrics call
(clears, edge pass, node pass, scalars), medians of `reps` after a warm-up with min and max, the two forms
alternating in one process.

    python tools/ab_cluster_metrics_edges.py [reps]
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import emulate_components as emu  # noqa: E402
from splink_amd import _native as N  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
ctx = N.Context(0)
ctx.enable_timing(True)


def cases():
    n, u, v = emu.hub_graph()
    yield "hub, shuffled", n, u, v
    k = np.argsort(u, kind="stable")
    yield "hub, sorted by first end", n, u[k], v[k]
    n, u, v = emu.random_graph()
    yield "random", n, u, v
    n = 1_000_000
    yield "one star of 10^6 leaves", n + 1, np.full(n, n, dtype=np.uint32), np.arange(n, dtype=np.uint32)


for name, n, u, v in cases():
    ctx.components_sweep_edges(n, u, v, None, [])
    ms = {0: [], 1: []}
    first = None
    for i in range(reps + 1):
        for mode in (0, 1):
            ctx.cluster_metrics_set_mode(mode)
            scalars = ctx.cluster_metrics(0)
            got = (scalars, ctx.cluster_metrics_copy(0, n)[0].tobytes())
            first = first or got
            assert got == first
            if i:
                ms[mode].append(ctx.cluster_metrics_info()[1])
    ctx.cluster_metrics_set_mode(1)
    print(json.dumps({"graph": name, "nodes": int(n), "edges": int(len(u)), **{
        ("one_add_per_end_ms" if m == 0 else "counted_in_the_wave_ms"): {
            "median": float(np.median(x)), "min": float(min(x)), "max": float(max(x))} for m, x in ms.items()}}))
