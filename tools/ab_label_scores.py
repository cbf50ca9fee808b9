"""Scores against labels, per pair: the fused device pass against the two passes it replaces and against the host
route.  link_only, two tables of `records / 2` synthetic records each (copies of one entity fall on both sides),
cfg2's comparisons with a term-frequency adjustment on surname (tools/ab_tf_select.py's job), label = the synthetic
records' ground-truth `cluster`.

(a) device time of spk_label_scores_tf_columns (spk_label_scores_info, HIP events around its launches) at T = the
    rows of df_e.truth_table (72 at cfg2) and at T = 1024, next to the two passes it fuses on the same pairs:
    tf_apply_columns(want_host=False, want_adj=False), which has no timer of its own and is taken by the host clock
    around the synchronising call, and spk_label_histogram (spk_label_info).  The three alternate in one loop.  Also
    the bytes the fused call must move: P x (8 + code_bytes) streamed (both rows and the code of every pair), the
    narrowed label ids (4 B per record) and the value ids (8 B per record and tf column) gathered.
(b) wall time of tf.truth_table("cluster") against the route it replaces: tf.toPandas() with `cluster` retained, then
    the same table in numpy.  Both from fresh frames, the job's cached host columns dropped before every run.

Each figure is the median of `reps` runs (`big_reps` for the host route) after one warm-up, with min and max.  One
JSON line, appended to the log.

    python tools/ab_label_scores.py [records] [reps] [big_reps] [log] [device-only]

The A/B of the grid cap (SPK_LABEL_SCORE_WG_PER_CU in csrc/spk_labels.hip, workgroups per compute unit): build a
variant with
    python tools/build_ab.py OUT.so spk_labels.hip -DSPK_LABEL_SCORE_WG_PER_CU=N
and run this tool with SPLINK_AMD_LIB naming each library in turn, `device-only`, in one session.
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
from splink_amd.frames import ExpectationFrame, GammaFrame, _label_ids  # noqa: E402
from splink_amd.labels import ScoreLabelCounts, true_pairs_total  # noqa: E402
from splink_amd.params import Params  # noqa: E402
from splink_amd.session import AmdSession  # noqa: E402
from splink_amd.synthetic import cfg_settings, make_records  # noqa: E402
from splink_amd.term_frequencies import make_adjustment_for_term_frequencies  # noqa: E402

records = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 7
big_reps = int(sys.argv[3]) if len(sys.argv) > 3 else 2
log_path = sys.argv[4] if len(sys.argv) > 4 else os.path.join(ROOT, "profiles", "ab_label_scores.log")
device_only = len(sys.argv) > 5 and sys.argv[5] == "device-only"
LABEL = "cluster"
TF = "tf_adjusted_match_prob"

cols = ["first_name", "surname", "dob", "city", "email"]
df = make_records(records, surname_vocab=15000)[["unique_id"] + cols + [LABEL]]
side = np.random.Generator(np.random.PCG64(1)).random(len(df)) < 0.5
tables = [df[side].reset_index(drop=True), df[~side].reset_index(drop=True)]
settings = cfg_settings(2)
settings["link_type"] = "link_only"
settings["additional_columns_to_retain"] = [LABEL]
next(c for c in settings["comparison_columns"] if c["col_name"] == "surname")["term_frequency_adjustments"] = True
amd = AmdSession(0)
params = Params(settings, amd)
st = params.settings
job = Job("link_only", tables, "unique_id", 0)
job.ctx.enable_timing(True)
job.block(st["blocking_rules"])
gf = GammaFrame(job, st)
lam, probs = params.params["λ"], params._level_probabilities()


def fresh_tf():
    return make_adjustment_for_term_frequencies(ExpectationFrame(gf, st, lam, probs), params, st, amd)


def spread(xs):
    return {"median": float(np.median(xs)), "min": float(min(xs)), "max": float(max(xs)), "n": len(xs)}


res = {"lib": os.path.basename(os.environ.get("SPLINK_AMD_LIB", "libsplink_hip.so")), "link_type": "link_only",
       "records": [len(t) for t in tables], "pairs": int(job.n_pairs), "n_patterns": int(job.ctx.n_patterns()),
       "reps": reps, "big_reps": big_reps}

# ---- (a) device time of the fused pass and of the two passes it replaces, alternating
tf = fresh_tf()
m, u = job.flat_tables(probs)
lab0, lab1 = _label_ids(job, LABEL)
t_rows = ExpectationFrame(gf, st, lam, probs).truth_table(LABEL)["threshold"].to_numpy()
t_max = np.linspace(0.0, 1.0, 1024)
fused = {len(t_rows): [], 1024: []}
apply_wall, hist_ms = [], []
for i in range(reps + 1):
    job.score(lam, probs, want_host=False)
    t0 = time.perf_counter()
    job.ctx.tf_apply_columns(tf.dev_cols, tf.tables, 0, job.n_pairs, want_adj=False, want_host=False)
    a = (time.perf_counter() - t0) * 1e3
    job.ctx.label_histogram(lab0, lab1)
    h = job.ctx.label_info()[1]
    ms = {}
    for t in (t_rows, t_max):
        job.ctx.label_scores_tf_columns(lab0, lab1, float(lam), float(1 - lam), m, u, tf.dev_cols, tf.tables, t)
        ms[len(t)] = job.ctx.label_scores_info()[1]
    if i:
        apply_wall.append(a)
        hist_ms.append(h)
        for k, v in ms.items():
            fused[k].append(v)
code_bytes = 2 if res["n_patterns"] <= 65536 else 4
n_rec = sum(len(t) for t in tables)
moved = res["pairs"] * (8 + code_bytes) + n_rec * (4 + 8 * len(tf.tables))
res["device"] = {
    "spk_label_scores_tf_columns_ms": {f"T={k}": spread(v) for k, v in fused.items()},
    "tf_apply_columns_device_resident_wall_ms": spread(apply_wall),
    "spk_label_histogram_ms": spread(hist_ms),
    "two_passes_median_ms": float(np.median(apply_wall) + np.median(hist_ms)),
    "bytes_moved": int(moved),
    "fused_GBps_at_median": {f"T={k}": moved / (np.median(v) * 1e-3) / 1e9 for k, v in fused.items()},
}

if device_only:
    line = json.dumps(res)
    print(line)
    with open(log_path, "a") as fh:
        fh.write(line + "\n")
    sys.exit(0)


# ---- (b) wall time to the truth table
def host_route():
    """What the parent commit offers: every pair to pandas, then numpy."""
    pdf = fresh_tf().toPandas()
    a, b = pdf[LABEL + "_l"].to_numpy(dtype=np.float64), pdf[LABEL + "_r"].to_numpy(dtype=np.float64)
    state = np.where(np.isnan(a) | np.isnan(b), 2, (a == b).astype(np.int64))
    score = pdf[TF].to_numpy()
    T = len(t_rows)
    b_ = np.searchsorted(t_rows, score, side="left")
    b_[np.isnan(score)] = T + 1
    counts = np.bincount(state * (T + 2) + b_, minlength=3 * (T + 2)).reshape(3, T + 2)
    totals = counts.sum(axis=1)
    all_true = true_pairs_total("link_only", tables[0][LABEL].to_numpy(), tables[1][LABEL].to_numpy())
    return ScoreLabelCounts(counts, t_rows, totals, "link_only", all_true).truth_table()


ts = []
for i in range(reps + 1):
    job._host_cols = {}
    frame = fresh_tf()
    t0 = time.perf_counter()
    got = frame.truth_table(LABEL)
    if i:
        ts.append(time.perf_counter() - t0)
res["truth_table_s"] = spread(ts)
ts = []
for i in range(big_reps + 1):
    job._pairs_host = None
    job._host_cols = {}
    t0 = time.perf_counter()
    host = host_route()
    if i:
        ts.append(time.perf_counter() - t0)
res["toPandas_then_numpy_s"] = spread(ts)
res["identical"] = bool(got.equals(host))
res["truth_table_rows"] = len(got)
res["speedup_median"] = res["toPandas_then_numpy_s"]["median"] / res["truth_table_s"]["median"]
line = json.dumps(res)
print(line)
with open(log_path, "a") as fh:
    fh.write(line + "\n")
