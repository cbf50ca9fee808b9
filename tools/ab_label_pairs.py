"""Pairs against a table of labelled pairs: the device pass against the label-column pass and against the host route,
at cfg2 (1 M records, ~46 M pairs).  The label tables hold 10^3, 10^5 and 10^7 pairs, half of them candidate pairs
(drawn from the job's own pair set), half pairs of random records; a pair is a match iff its records share the
synthetic ground-truth `cluster`.

(a) device time of spk_label_pairs_histogram (spk_label_pairs_info: table clear, build, pattern table, counter clear,
    histogram) per label table, next to the device time of spk_label_histogram (spk_label_info) on the same pairs with
    the `cluster` column as labels, the two calls alternating in one loop; their ratio; the table's capacity and
    longest insert probe;
(b) wall time of df_e.truth_table_from_pairs(labels) at 10^5 labels against the route it replaces: df_e.toPandas(),
    a pandas merge with the labels on the unique ids, then numpy (codes from the gamma columns, one bincount) and the
    same host table.  "cold" drops the job's cached host columns before every run, "warm" keeps them.

Each figure is the median of `reps` runs (`big_reps` for the host route) after one warm-up, with min and max.

    python tools/ab_label_pairs.py [reps] [big_reps] [device-only]
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
from splink_amd.frames import ExpectationFrame, GammaFrame, _label_ids  # noqa: E402
from splink_amd.labels import PairLabelCounts  # noqa: E402
from splink_amd.params import Params  # noqa: E402
from splink_amd.session import AmdSession  # noqa: E402
from splink_amd.synthetic import cfg_settings, make_records  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
big_reps = int(sys.argv[2]) if len(sys.argv) > 2 else 2
device_only = len(sys.argv) > 3 and sys.argv[3] == "device-only"
SIZES = (10 ** 3, 10 ** 5, 10 ** 7)
WALL_SIZE = 10 ** 5

cols = ["first_name", "surname", "dob", "city", "email"]
df = make_records(1_000_000, surname_vocab=15000, arrow=True)[["unique_id"] + cols + ["cluster"]]
settings = cfg_settings(2)
params = Params(settings, AmdSession(0))
st = params.settings
job = Job("dedupe_only", [df], "unique_id", 0)
job.ctx.enable_timing(True)
job.block(st["blocking_rules"])
gf = GammaFrame(job, st)
lam, probs = params.params["λ"], params._level_probabilities()
m, u = job.flat_tables(probs)
names, levels = gf.meta
rng = np.random.Generator(np.random.PCG64(7))


def spread(xs):
    return {"median": float(np.median(xs)), "min": float(min(xs)), "max": float(max(xs)), "n": len(xs)}


def label_rows(n):
    """n distinct labelled pairs as device rows: n // 2 candidate pairs, the rest pairs of random records."""
    pl, pr = job.pair_rows()
    take = rng.choice(len(pl), n // 2, replace=False)
    n0 = len(df)
    l = np.concatenate([pl[take].astype(np.int64), rng.integers(0, n0, n - n // 2 + n // 8)])
    r = np.concatenate([pr[take].astype(np.int64), rng.integers(0, n0, n - n // 2 + n // 8)])
    key = np.minimum(l, r) << 32 | np.maximum(l, r)
    _, first = np.unique(key, return_index=True)
    first = np.sort(first[l[first] != r[first]])[:n]  # the candidates come first and are distinct already
    assert len(first) == n
    first = rng.permutation(first)
    cluster = job.host_values(0, "cluster")
    l, r = l[first], r[first]
    return l.astype(np.int32), r.astype(np.int32), (cluster[l] == cluster[r]).astype(np.uint8)


res = {"lib": os.path.basename(os.environ.get("SPLINK_AMD_LIB", "libsplink_hip.so")), "config": 2, "records": len(df),
       "pairs": int(job.n_pairs), "n_patterns": int(job.ctx.n_patterns()), "reps": reps, "big_reps": big_reps,
       "device": {}}

# ---- (a) device time, the two calls alternating
gf.ensure_codes()
ids0, ids1 = _label_ids(job, "cluster")
tables = {}
for n in SIZES:
    rows_l, rows_r, y = tables[n] = label_rows(n)
    pair_ms, column_ms = [], []
    for i in range(reps + 1):
        counts, _, code = job.ctx.label_pairs_histogram(rows_l, rows_r, y, float(lam), float(1 - lam), m, u)
        pairs, ms, capacity, probe = job.ctx.label_pairs_info()
        job.ctx.label_histogram(ids0, ids1, float(lam), float(1 - lam), m, u)
        if i:
            pair_ms.append(ms)
            column_ms.append(job.ctx.label_info()[1])
    res["device"][str(n)] = {
        "spk_label_pairs_histogram_ms": spread(pair_ms), "spk_label_histogram_ms": spread(column_ms),
        "ratio_of_medians": float(np.median(pair_ms) / np.median(column_ms)), "capacity": int(capacity),
        "table_bytes": int(capacity) * 12, "max_probe": int(probe), "labels_found": int((code >= 0).sum()),
        "labelled_candidates": int(counts[:2].sum())}

if device_only:
    print(json.dumps(res))
    sys.exit(0)

# ---- (b) wall time to the truth table
uid = job.host_values(0, "unique_id")
rows_l, rows_r, y = tables[WALL_SIZE]
labels = pd.DataFrame({"unique_id_l": uid[rows_l], "unique_id_r": uid[rows_r], "clerical_match_score": y.astype(float)})


def host_route():
    """What the parent commit offers: every pair to pandas, a merge with the labels, then numpy."""
    pdf = ExpectationFrame(gf, st, lam, probs).toPandas()
    a, b = pdf["unique_id_l"].to_numpy(), pdf["unique_id_r"].to_numpy()
    pdf["_lo"], pdf["_hi"] = np.minimum(a, b), np.maximum(a, b)
    a, b = labels["unique_id_l"].to_numpy(), labels["unique_id_r"].to_numpy()
    lab = pd.DataFrame({"_lo": np.minimum(a, b), "_hi": np.maximum(a, b),
                        "_y": (labels["clerical_match_score"].to_numpy() >= 0.5).astype(np.int64),
                        "_at": np.arange(len(labels))})
    merged = pdf.merge(lab, on=["_lo", "_hi"], how="left")
    code = np.zeros(len(merged), dtype=np.int64)
    stride = 1
    for name, L in zip(names, levels):
        code += (merged[name].to_numpy(dtype=np.int64) + 1) * stride
        stride *= L + 1
    n_pat = stride
    state = merged["_y"].fillna(2).to_numpy(dtype=np.int64)
    counts = np.bincount(state * n_pat + code, minlength=3 * n_pat).reshape(3, n_pat)
    mp = np.full(n_pat, np.nan)
    mp[code] = merged["match_probability"].to_numpy()  # one score per pattern
    label_code = np.full(len(labels), -1, dtype=np.int64)
    hit = merged["_at"].notna().to_numpy()
    label_code[merged["_at"].to_numpy()[hit].astype(np.int64)] = code[hit]
    return PairLabelCounts(names, levels, counts, mp, "dedupe_only", labels, lab["_y"].to_numpy(),
                           label_code).truth_table()


for mode in ("cold", "warm"):
    ts = []
    for i in range(reps + 1):
        if mode == "cold":
            job._host_cols = {}
        df_e = ExpectationFrame(gf, st, lam, probs)
        t0 = time.perf_counter()
        got = df_e.truth_table_from_pairs(labels)
        if i:
            ts.append(time.perf_counter() - t0)
    res.setdefault("truth_table_from_pairs_s", {})[mode] = spread(ts)
ts = []
for i in range(big_reps + 1):
    job._host_cols = {}
    t0 = time.perf_counter()
    host = host_route()
    if i:
        ts.append(time.perf_counter() - t0)
res["labels_in_wall_test"] = WALL_SIZE
res["toPandas_merge_numpy_s"] = spread(ts)
res["identical"] = bool(got.equals(host))
res["truth_table_rows"] = len(got)
res["speedup_cold_median"] = res["toPandas_merge_numpy_s"]["median"] / res["truth_table_from_pairs_s"]["cold"]["median"]
print(json.dumps(res))
