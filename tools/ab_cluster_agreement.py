"""Clusters against labels: spk_cluster_agreement against the host route it replaces, at cfg2 (1 M records, ~46 M
pairs, initial parameters, label = the synthetic records' ground-truth `cluster`), thresholds 0.99 0.95 0.9 0.8 0.7
0.6 0.5 0.3 (those of profiles/ab_cluster_sweep.log).

(a) device ms of spk_cluster_agreement over the eight levels (spk_cluster_agreement_info: HIP events around all its
    launches);
(b) wall time of sweep.truth_table("cluster") against sweep.toPandas() followed by the pandas oracle of the tests
    (tests/agreement_common.py: group sizes per threshold over one row per record), on the same job and the same
    sweep frame, the two routes alternating in one process, and whether the two tables are identical.

Medians of `reps` runs after one warm-up, with the minimum and maximum of each.

    python tools/ab_cluster_agreement.py [reps] [out.log] [device-only]

Which step takes the device time (the sorts, the scans, the project's own kernels): run it `device-only` under
rocprofv3 --kernel-trace --stats, in a run of its own.
"""
import json
import os
import sys
import time

import numpy as np
import pandas as pd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402,F401
from agreement_common import agreement_oracle  # noqa: E402
from splink_amd.engine import Job  # noqa: E402
from splink_amd.frames import ExpectationFrame, GammaFrame  # noqa: E402
from splink_amd.labels import cluster_truth_rows  # noqa: E402
from splink_amd.params import Params  # noqa: E402
from splink_amd.session import AmdSession  # noqa: E402
from splink_amd.synthetic import cfg_settings, make_records  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
out_path = sys.argv[2] if len(sys.argv) > 2 and sys.argv[2] != "-" else None
device_only = len(sys.argv) > 3 and sys.argv[3] == "device-only"
records = int(os.environ.get("AB_RECORDS", "1000000"))
TS = [0.99, 0.95, 0.9, 0.8, 0.7, 0.6, 0.5, 0.3]
LABEL = "cluster"

cols = ["first_name", "surname", "dob", "city", "email"]
df = make_records(records, surname_vocab=15000, arrow=True)[["unique_id"] + cols + [LABEL]]
params = Params(cfg_settings(2), AmdSession(0))
st = params.settings
job = Job("dedupe_only", [df], "unique_id", 0)
job.ctx.enable_timing(True)
job.block(st["blocking_rules"])
gf = GammaFrame(job, st)
sweep = ExpectationFrame(gf, st, params.params["λ"], params._level_probabilities()).clusters_at_thresholds(TS)
sweep._run()
res = {"lib": os.path.basename(os.environ.get("SPLINK_AMD_LIB", "libsplink_hip.so")), "config": 2, "records": len(df), "pairs": int(job.n_pairs), "thresholds": TS, "reps": reps}


def spread(xs):
    return {"median": float(np.median(xs)), "min": float(min(xs)), "max": float(max(xs))}


def host_route():
    """What there was: every record's labels to pandas, then group sizes per threshold."""
    pdf = sweep.toPandas()
    ids = pd.factorize(df[LABEL].to_numpy())[0].astype(np.int64)
    rows = [agreement_oracle(pdf[f"cluster_id_{t!r}"].to_numpy(), ids, len(df), False) for t in TS]
    return cluster_truth_rows(np.stack(rows), TS)


device_ms, device_s, host_s = [], [], []
for i in range(reps + 1):
    t0 = time.perf_counter()
    got = sweep.truth_table(LABEL)
    t1 = time.perf_counter()
    ms = job.ctx.cluster_agreement_info()[1]
    if not device_only:
        t2 = time.perf_counter()
        host = host_route()
        t3 = time.perf_counter()
    if i:
        device_ms.append(ms)
        device_s.append(t1 - t0)
        if not device_only:
            host_s.append(t3 - t2)
res["spk_cluster_agreement_ms"] = spread(device_ms)
res["truth_table_s"] = spread(device_s)
res["table"] = got.to_dict(orient="list")
if not device_only:
    res["toPandas_then_pandas_s"] = spread(host_s)
    res["identical"] = bool(got.equals(host))
    res["speedup_median"] = res["toPandas_then_pandas_s"]["median"] / res["truth_table_s"]["median"]
print(json.dumps(res))
if out_path:
    with open(out_path, "w") as fh:
        json.dump(res, fh, indent=1)
