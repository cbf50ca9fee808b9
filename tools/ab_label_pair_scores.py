"""Scores against a table of labelled pairs, per pair: the fused device pass against the two parent passes whose work
it does and against the host route, at cfg2 (1 M records, ~46 M pairs, dedupe_only) with a term-frequency adjustment
on surname.  The label tables hold 10^3, 10^5 and 10^7 pairs, half of them candidate pairs (drawn from the job's own
pair set), half pairs of random records (tools/ab_label_pairs.py's recipe); a pair is a match iff its records share
the synthetic ground-truth `cluster`.

(a) device time of spk_label_pairs_scores_tf_columns (spk_label_pairs_scores_info: table clear, build, pattern table,
    counter clear, the counting kernel, the per-label kernel) per label table at T = 72 and T = 1024, next to
    spk_label_scores_tf_columns (spk_label_scores_info; the `cluster` column as labels: its gathers) and
    spk_label_pairs_histogram (spk_label_pairs_info; the same label table: its probes) on the same pairs, the calls
    alternating in one loop; the fused call over the sum of the two.
(b) device time of spk_label_pairs_scores_selection over a selection of about 1 % of the pairs (tf_adjusted_match_prob
    above its 99th percentile), per label table, at T = 72.
(c) wall time of tf.truth_table_from_pairs(labels) at 10^5 labels against the route it replaces: tf.toPandas() (the
    per-pair part over every pair, every pair to the host), a pandas merge with the labels on the unique ids, then
    the same table in numpy.  Skipped with `device-only`.

Each figure is the median of `reps` runs after one warm-up, with min and max (the host route: `big_reps` runs, without
a warm-up when that is 1).  One JSON line, printed and appended to the log.

    python tools/ab_label_pair_scores.py [reps] [big_reps] [log] [device-only]

The A/B of the pairs per lane and of the waves per SIMD the registers are held to (SPK_LABEL_PAIR_SCORE_PAIRS 4 | 8,
SPK_LABEL_PAIR_SCORE_WAVES in csrc/spk_labels.hip): build a variant with
    python tools/build_ab.py OUT.so spk_labels.hip -DSPK_LABEL_PAIR_SCORE_PAIRS=N -DSPK_LABEL_PAIR_SCORE_WAVES=W
and run this tool with SPLINK_AMD_LIB naming each library in turn, `device-only`, in one session.
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
from splink_amd import _native as N  # noqa: E402
from splink_amd.engine import Job  # noqa: E402
from splink_amd.frames import ExpectationFrame, GammaFrame, _label_ids  # noqa: E402
from splink_amd.labels import PairScoreLabelCounts  # noqa: E402
from splink_amd.params import Params  # noqa: E402
from splink_amd.session import AmdSession  # noqa: E402
from splink_amd.synthetic import cfg_settings, make_records  # noqa: E402
from splink_amd.term_frequencies import make_adjustment_for_term_frequencies  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
big_reps = int(sys.argv[2]) if len(sys.argv) > 2 else 1
log_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "ab_label_pair_scores.log")
device_only = len(sys.argv) > 4 and sys.argv[4] == "device-only"
SIZES = (10 ** 3, 10 ** 5, 10 ** 7)
WALL_SIZE = 10 ** 5
TF = "tf_adjusted_match_prob"

cols = ["first_name", "surname", "dob", "city", "email"]
df = make_records(1_000_000, surname_vocab=15000, arrow=True)[["unique_id"] + cols + ["cluster"]]
settings = cfg_settings(2)
next(c for c in settings["comparison_columns"] if c["col_name"] == "surname")["term_frequency_adjustments"] = True
amd = AmdSession(0)
params = Params(settings, amd)
st = params.settings
job = Job("dedupe_only", [df], "unique_id", 0)
job.ctx.enable_timing(True)
job.block(st["blocking_rules"])
gf = GammaFrame(job, st)
lam, probs = params.params["λ"], params._level_probabilities()
m, u = job.flat_tables(probs)
rng = np.random.Generator(np.random.PCG64(7))


def fresh_tf():
    return make_adjustment_for_term_frequencies(ExpectationFrame(gf, st, lam, probs), params, st, amd)


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
       "device": {}, "selection": {}}

# ---- (a) device time of the fused call and of the two parent calls, alternating
tf = fresh_tf()
gf.ensure_codes()
ids0, ids1 = _label_ids(job, "cluster")
la, om = float(lam), float(1 - lam)
t_all = {72: np.linspace(0.0, 1.0, 72), 1024: np.linspace(0.0, 1.0, 1024)}
tables = {}
for n in SIZES:
    rows_l, rows_r, y = tables[n] = label_rows(n)
    fused = {T: [] for T in t_all}
    column = {T: [] for T in t_all}
    hist = []
    for i in range(reps + 1):
        job.ctx.label_pairs_histogram(rows_l, rows_r, y)
        h = job.ctx.label_pairs_info()[1]
        ms = {}
        for T, t in t_all.items():
            job.ctx.label_scores_tf_columns(ids0, ids1, la, om, m, u, tf.dev_cols, tf.tables, t)
            c_ms = job.ctx.label_scores_info()[1]
            counts, pair, _ = job.ctx.label_pair_scores_tf_columns(rows_l, rows_r, y, la, om, m, u, tf.dev_cols,
                                                                   tf.tables, t)
            ms[T] = (c_ms, job.ctx.label_pair_scores_info()[1])
        if i:
            hist.append(h)
            for T, (c_ms, f_ms) in ms.items():
                column[T].append(c_ms)
                fused[T].append(f_ms)
    _, _, capacity, probe = job.ctx.label_pair_scores_info()
    res["device"][str(n)] = {
        "spk_label_pairs_scores_tf_columns_ms": {f"T={T}": spread(v) for T, v in fused.items()},
        "spk_label_scores_tf_columns_ms": {f"T={T}": spread(v) for T, v in column.items()},
        "spk_label_pairs_histogram_ms": spread(hist),
        "fused_over_sum_of_parents": {f"T={T}": float(np.median(fused[T]) / (np.median(column[T]) + np.median(hist)))
                                      for T in t_all},
        "capacity": int(capacity), "table_bytes": int(capacity) * 12, "max_probe": int(probe),
        "labels_found": int((pair >= 0).sum()), "labelled_pairs_counted": int(counts[:2].sum())}

# ---- (b) the selection call over about 1 % of the pairs
job.score(lam, probs, want_host=False)
job.ctx.tf_apply_columns(tf.dev_cols, tf.tables, 0, job.n_pairs, want_adj=False, want_host=False)
sample = np.concatenate([job.ctx.tf_copy(s, 1 << 20) for s in range(0, job.n_pairs - (1 << 20), job.n_pairs // 8)])
cut = float(np.nanquantile(sample, 0.99))
kept = job.ctx.select_tf_columns(la, om, m, u, tf.dev_cols, tf.tables, [(N.SEL_TF_MP, 0, N.SEL_OP[">"], cut)])
res["selection"]["kept"] = int(kept)
res["selection"]["fraction"] = kept / job.n_pairs
for n in SIZES:
    rows_l, rows_r, y = tables[n]
    sel_ms, col_ms = [], []
    for i in range(reps + 1):
        job.ctx.label_scores_selection(ids0, ids1, N.SEL_TF_MP, t_all[72])
        c_ms = job.ctx.label_scores_info()[1]
        job.ctx.label_pair_scores_selection(rows_l, rows_r, y, N.SEL_TF_MP, t_all[72])
        if i:
            col_ms.append(c_ms)
            sel_ms.append(job.ctx.label_pair_scores_info()[1])
    res["selection"][str(n)] = {"spk_label_pairs_scores_selection_ms": spread(sel_ms),
                                "spk_label_scores_selection_ms": spread(col_ms)}
job.ctx.select_release()


def finish():
    line = json.dumps(res)
    print(line)
    with open(log_path, "a") as fh:
        fh.write(line + "\n")


if device_only:
    finish()
    sys.exit(0)

# ---- (c) wall time to the truth table
uid = job.host_values(0, "unique_id")
rows_l, rows_r, y = tables[WALL_SIZE]
labels = pd.DataFrame({"unique_id_l": uid[rows_l], "unique_id_r": uid[rows_r], "clerical_match_score": y.astype(float)})
ts_given = t_all[72]


def host_route():
    """What the parent commit offers: every tf-scored pair to pandas, a merge with the labels, then numpy."""
    pdf = fresh_tf().toPandas()
    a, b = pdf["unique_id_l"].to_numpy(), pdf["unique_id_r"].to_numpy()
    pdf["_lo"], pdf["_hi"] = np.minimum(a, b), np.maximum(a, b)
    a, b = labels["unique_id_l"].to_numpy(), labels["unique_id_r"].to_numpy()
    lab = pd.DataFrame({"_lo": np.minimum(a, b), "_hi": np.maximum(a, b),
                        "_y": (labels["clerical_match_score"].to_numpy() >= 0.5).astype(np.int64),
                        "_at": np.arange(len(labels))})
    merged = pdf[["_lo", "_hi", TF]].merge(lab, on=["_lo", "_hi"], how="left")
    state = merged["_y"].fillna(2).to_numpy(dtype=np.int64)
    score = merged[TF].to_numpy()
    T = len(ts_given)
    b_ = np.searchsorted(ts_given, score, side="left")
    b_[np.isnan(score)] = T + 1
    counts = np.bincount(state * (T + 2) + b_, minlength=3 * (T + 2)).reshape(3, T + 2)
    hit = merged["_at"].notna().to_numpy()
    at = merged["_at"].to_numpy()[hit].astype(np.int64)
    pair = np.full(len(labels), -1, dtype=np.int64)
    pair[at] = np.flatnonzero(hit)
    label_score = np.full(len(labels), np.nan)
    label_score[at] = score[hit]
    return PairScoreLabelCounts(counts, ts_given, counts.sum(axis=1), "dedupe_only", labels, lab["_y"].to_numpy(),
                                label_score, TF, label_pair=pair).truth_table()


ts = []
for i in range(reps + 1):
    job._host_cols = {}
    frame = fresh_tf()
    t0 = time.perf_counter()
    got = frame.truth_table_from_pairs(labels, ts_given)
    if i:
        ts.append(time.perf_counter() - t0)
res["truth_table_from_pairs_s"] = spread(ts)
ts = []
for i in range(big_reps + 1 if big_reps > 1 else 1):  # one run: no warm-up (minutes of host work each)
    job._pairs_host = None
    job._host_cols = {}
    t0 = time.perf_counter()
    host = host_route()
    if i or big_reps <= 1:
        ts.append(time.perf_counter() - t0)
res["labels_in_wall_test"] = WALL_SIZE
res["toPandas_merge_numpy_s"] = spread(ts)
res["identical"] = bool(got.equals(host))
res["truth_table_rows"] = len(got)
res["speedup_median"] = res["toPandas_merge_numpy_s"]["median"] / res["truth_table_from_pairs_s"]["median"]
finish()
