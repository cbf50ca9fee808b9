"""Pairs against labels: the device pass against the EM histogram and against the host route, at cfg2 (1 M records,
~46 M pairs, label = the synthetic records' ground-truth `cluster`).

(a) device time of spk_label_histogram (spk_label_info, HIP events around its launches) next to the device time of
    spk_em_histogram on the same codes (spk_ctx_kernel_ms), and the bytes the call must move -- P x (8 + code_bytes)
    streamed (both rows and the code of every pair), plus the label arrays (8 B per record read and 4 B written by the
    narrowing, 4 B per record gathered) -- over that time, next to the read-only streaming rate torch reaches on
    this device (tools/hbm_ceiling.py's read_only_sum figure, measured here the same way);
(b) wall time of df_e.truth_table("cluster") against the route it replaces: df_e.toPandas() with `cluster` retained,
    then numpy (codes from the gamma columns, truth from cluster_l / cluster_r, one bincount) and the same host
    table.  "cold" drops the job's cached host columns before every run (the device route factorises the label
    column again, the host route converts the retained input columns again); "warm" keeps them.

Each figure is the median of `reps` runs (`big_reps` for the host route) after one warm-up, with min and max, from
fresh frames.

    python tools/ab_labels.py [reps] [big_reps] [device-only]

The A/B of how a wave adds its keys (SPK_LABEL_AGG in csrc/spk_labels.hip: 0 one LDS atomic per pair, 1 ballot
aggregation with a shuffle, 2 with v_readlane): build variants with
    python tools/build_ab.py OUT.so spk_labels.hip -DSPK_LABEL_AGG=N
and run this tool with SPLINK_AMD_LIB naming each in turn, `device-only`, in one session.
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402,F401
from hbm_ceiling import timed  # noqa: E402
from splink_amd.engine import Job  # noqa: E402
from splink_amd.frames import ExpectationFrame, GammaFrame  # noqa: E402
from splink_amd.labels import LabelCounts, true_pairs_total  # noqa: E402
from splink_amd.params import Params  # noqa: E402
from splink_amd.session import AmdSession  # noqa: E402
from splink_amd.synthetic import cfg_settings, make_records  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
big_reps = int(sys.argv[2]) if len(sys.argv) > 2 else 2
device_only = len(sys.argv) > 3 and sys.argv[3] == "device-only"
LABEL = "cluster"

cols = ["first_name", "surname", "dob", "city", "email"]
df = make_records(1_000_000, surname_vocab=15000, arrow=True)[["unique_id"] + cols + [LABEL]]
settings = cfg_settings(2)
settings["additional_columns_to_retain"] = [LABEL]
params = Params(settings, AmdSession(0))
st = params.settings
job = Job("dedupe_only", [df], "unique_id", 0)
job.ctx.enable_timing(True)
job.block(st["blocking_rules"])
gf = GammaFrame(job, st)
lam, probs = params.params["λ"], params._level_probabilities()
names, levels = gf.meta


def spread(xs):
    return {"median": float(np.median(xs)), "min": float(min(xs)), "max": float(max(xs)), "n": len(xs)}


def host_route():
    """What the parent commit offers: every pair to pandas, then numpy."""
    pdf = ExpectationFrame(gf, st, lam, probs).toPandas()
    code = np.zeros(len(pdf), dtype=np.int64)
    stride = 1
    for name, L in zip(names, levels):
        code += (pdf[name].to_numpy(dtype=np.int64) + 1) * stride
        stride *= L + 1
    n_pat = stride
    a, b = pdf[LABEL + "_l"].to_numpy(), pdf[LABEL + "_r"].to_numpy()
    null = np.isnan(a.astype(np.float64)) | np.isnan(b.astype(np.float64))
    state = np.where(null, 2, (a == b).astype(np.int64))
    counts = np.bincount(state * n_pat + code, minlength=3 * n_pat).reshape(3, n_pat)
    mp = np.full(n_pat, np.nan)
    mp[code] = pdf["match_probability"].to_numpy()  # one score per pattern
    labels = df[LABEL].to_numpy()
    return LabelCounts(names, levels, counts, mp, "dedupe_only", true_pairs_total("dedupe_only", labels)).truth_table()


res = {"lib": os.path.basename(os.environ.get("SPLINK_AMD_LIB", "libsplink_hip.so")), "config": 2, "records": len(df),
       "pairs": int(job.n_pairs), "n_patterns": int(job.ctx.n_patterns()), "reps": reps, "big_reps": big_reps}

# ---- (a) device time and bandwidth
label_ms, em_ms = [], []
for i in range(reps + 1):
    ExpectationFrame(gf, st, lam, probs).label_counts(LABEL)
    pairs, ms = job.ctx.label_info()
    job.ctx.em_histogram(0)
    h = job.ctx.kernel_ms()["em_hist"]
    if i:
        label_ms.append(ms)
        em_ms.append(h)
code_bytes = 2 if res["n_patterns"] <= 65536 else 4
moved = res["pairs"] * (8 + code_bytes) + len(df) * (8 + 4 + 4)
x = torch.ones(int(2.9e9) // 8, dtype=torch.float64, device="cuda:0")
ceiling = x.numel() * 8 / timed(lambda: x.sum(), 20) / 1e9
del x
res["device"] = {"spk_label_histogram_ms": spread(label_ms), "spk_em_histogram_ms": spread(em_ms),
                 "bytes_moved": int(moved), "label_GBps_at_median": moved / (np.median(label_ms) * 1e-3) / 1e9,
                 "read_only_sum_GBps": ceiling,
                 "share_of_read_ceiling": moved / (np.median(label_ms) * 1e-3) / 1e9 / ceiling}

if device_only:
    print(json.dumps(res))
    sys.exit(0)

# ---- (b) wall time to the truth table
for mode in ("cold", "warm"):
    ts = []
    for i in range(reps + 1):
        if mode == "cold":
            job._host_cols = {}
        df_e = ExpectationFrame(gf, st, lam, probs)
        t0 = time.perf_counter()
        got = df_e.truth_table(LABEL)
        if i:
            ts.append(time.perf_counter() - t0)
    res.setdefault("truth_table_s", {})[mode] = spread(ts)
ts = []
for i in range(big_reps + 1):
    job._host_cols = {}
    t0 = time.perf_counter()
    host = host_route()
    if i:
        ts.append(time.perf_counter() - t0)
res["toPandas_then_numpy_s"] = spread(ts)
res["identical"] = bool(got.equals(host))
res["truth_table_rows"] = len(got)
res["speedup_cold_median"] = res["toPandas_then_numpy_s"]["median"] / res["truth_table_s"]["cold"]["median"]
print(json.dumps(res))
