"""Random pairs for u: the device sampler against the host route, and the comparison pass over a sampled set
against the pass over the blocked set, at the 1 M-record synthetic table with as many draws as cfg2 has blocked
pairs (45,981,122).

(a) device time of spk_pairs_sample (spk_pairs_sample_info, HIP events around its launches: count kernel, scan and
    emit kernel for dedupe_only, the emit kernel alone for link_only -- two tables of the 1 M rows), and the 8 bytes
    per surviving pair it must write over that time;
(b) the route there was before: the same number of pairs drawn with numpy (two integer arrays, the link-type
    predicate by one comparison and a swap) and handed to spk_pairs_load, wall time to the synchronised call's end;
(c) device time of the comparison pass (spk_ctx_kernel_ms "gamma") over the sampled set and over the blocked set of
    the same settings, and the cells per column each pass left to its exact kernels (spk_gammas_exact_counts).  The
    sampling job keeps the input row order (no blocking rule to cluster by); the blocked job is clustered by its
    first rule as usual.

The runs alternate (sampler dedupe / sampler link_only / host route, then blocked pass / sampled pass) inside one
loop; each figure is the median of `reps` runs (`big_reps` for the host route) after one warm-up, with min and max.

    python tools/ab_sample.py [reps] [big_reps]
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402,F401
from splink_amd import _native as N  # noqa: E402
from splink_amd.engine import Job  # noqa: E402
from splink_amd.params import Params  # noqa: E402
from splink_amd.session import AmdSession  # noqa: E402
from splink_amd.synthetic import cfg_settings, make_records  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
big_reps = int(sys.argv[2]) if len(sys.argv) > 2 else 2
DRAWS = 45_981_122  # cfg2's blocked pairs
SEED = 1

cols = ["first_name", "surname", "dob", "city", "email"]
df = make_records(1_000_000, surname_vocab=15000, arrow=True)[["unique_id"] + cols]
n = len(df)
st = Params(cfg_settings(2), AmdSession(0)).settings
names = [c["col_name"] for c in st["comparison_columns"]]


def spread(xs):
    return {"median": float(np.median(xs)), "min": float(min(xs)), "max": float(max(xs)), "n": len(xs)}


blocked = Job("dedupe_only", [df], "unique_id", 0)
blocked.ctx.enable_timing(True)
blocked.block(st["blocking_rules"])
sampled = Job("dedupe_only", [df], "unique_id", 0, cluster=False)
sampled.ctx.enable_timing(True)
link = N.Context(0)  # link_only needs the tables' sizes alone
link.set_link_type(N.LINK_TYPES["link_only"])
link.table_create(0, n, 1)
link.table_create(1, n, 1)
link.enable_timing(True)

res = {"config": 2, "records": n, "total_draws": DRAWS, "blocked_pairs": int(blocked.n_pairs), "reps": reps,
       "big_reps": big_reps}


def host_route():
    """Draw on the host, upload through spk_pairs_load (which validates every index in a host loop)."""
    rng = np.random.Generator(np.random.PCG64(SEED))
    a = rng.integers(0, n, DRAWS, dtype=np.int32)
    b = rng.integers(0, n - 1, DRAWS, dtype=np.int32)
    b += b >= a
    uid = df["unique_id"].to_numpy()
    swap = uid[a] > uid[b]
    l, r = np.where(swap, b, a), np.where(swap, a, b)
    sampled.load_pairs(l, r)
    sampled.ctx.sync()


# ---- (a), (b): the pair set
ms_dedupe, ms_link, kept, host_s = [], [], None, []
for i in range(reps + 1):
    sampled.sample_pairs(DRAWS, 0, DRAWS, SEED)
    _, kept, ms_d = sampled.ctx.pairs_sample_info()
    link.pairs_sample(N.LINK_TYPES["link_only"], SEED, DRAWS, 0, DRAWS)
    _, kept_l, ms_l = link.pairs_sample_info()
    if i:
        ms_dedupe.append(ms_d)
        ms_link.append(ms_l)
    if i <= big_reps:
        t0 = time.perf_counter()
        host_route()
        if i:
            host_s.append(time.perf_counter() - t0)
res["sampler"] = {
    "dedupe_only_ms": spread(ms_dedupe), "dedupe_only_kept": int(kept),
    "dedupe_only_write_GBps_at_median": 8 * kept / (np.median(ms_dedupe) * 1e-3) / 1e9,
    "link_only_ms": spread(ms_link), "link_only_kept": int(kept_l),
    "link_only_write_GBps_at_median": 8 * kept_l / (np.median(ms_link) * 1e-3) / 1e9,
}
res["numpy_then_pairs_load_s"] = spread(host_s)
res["host_over_device_dedupe_median"] = np.median(host_s) / (np.median(ms_dedupe) * 1e-3)
link.close()

# ---- (c): the comparison pass
sampled.sample_pairs(DRAWS, 0, DRAWS, SEED)
g_blocked, g_sampled = [], []
for i in range(reps + 1):
    blocked.gammas(st)
    blocked.ctx.sync()
    b_ms = blocked.ctx.kernel_ms()["gamma"]
    sampled.gammas(st)
    sampled.ctx.sync()
    s_ms = sampled.ctx.kernel_ms()["gamma"]
    if i:
        g_blocked.append(b_ms)
        g_sampled.append(s_ms)
res["comparison_pass"] = {
    "blocked_ms": spread(g_blocked), "blocked_pairs": int(blocked.n_pairs),
    "blocked_pairs_per_s_at_median": blocked.n_pairs / (np.median(g_blocked) * 1e-3),
    "sampled_ms": spread(g_sampled), "sampled_pairs": int(sampled.n_pairs),
    "sampled_pairs_per_s_at_median": sampled.n_pairs / (np.median(g_sampled) * 1e-3),
    "blocked_exact_cells": dict(zip(names, blocked.ctx.gammas_exact_counts(len(names)))),
    "sampled_exact_cells": dict(zip(names, sampled.ctx.gammas_exact_counts(len(names)))),
}
print(json.dumps(res))
