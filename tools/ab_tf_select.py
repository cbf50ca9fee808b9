"""Selection on tf_adjusted_match_prob against the per-pair tf pass and against a full copy: link_only, two tables
of `records / 2` synthetic records each (copies of one entity fall on both sides), cfg2's comparisons with a
term-frequency adjustment on surname.

(a) wall time (host clock around the synchronising call) of select_tf_columns for `tf_adjusted_match_prob > t`
    against tf_apply_columns(want_host=False, want_adj=False), the cheapest per-pair tf pass there was before, on
    the same pairs and tables, alternating;
(b) wall time of tf.filter("tf_adjusted_match_prob > t").toPandas() against tf.toPandas() followed by the pandas
    mask, from fresh frames.

Medians with the spread (min .. max) after one warm-up each; no pass / fail figure.

    python tools/ab_tf_select.py [records] [threshold] [reps] [full_reps] [out.json]
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
from splink_amd.frames import ExpectationFrame, GammaFrame  # noqa: E402
from splink_amd.params import Params  # noqa: E402
from splink_amd.session import AmdSession  # noqa: E402
from splink_amd.synthetic import cfg_settings, make_records  # noqa: E402
from splink_amd.term_frequencies import make_adjustment_for_term_frequencies  # noqa: E402

records = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
thr = float(sys.argv[2]) if len(sys.argv) > 2 else 0.9
reps = max(int(sys.argv[3]) if len(sys.argv) > 3 else 7, 5)
full_reps = int(sys.argv[4]) if len(sys.argv) > 4 else 3
out_path = sys.argv[5] if len(sys.argv) > 5 else None

cols = ["first_name", "surname", "dob", "city", "email"]
df = make_records(records, surname_vocab=15000)[["unique_id"] + cols]
side = np.random.Generator(np.random.PCG64(1)).random(len(df)) < 0.5
tables = [df[side].reset_index(drop=True), df[~side].reset_index(drop=True)]
settings = cfg_settings(2)
settings["link_type"] = "link_only"
next(c for c in settings["comparison_columns"] if c["col_name"] == "surname")["term_frequency_adjustments"] = True
amd = AmdSession(0)
params = Params(settings, amd)
st = params.settings
job = Job("link_only", tables, "unique_id", 0)
job.block(st["blocking_rules"])
gf = GammaFrame(job, st)
lam, probs = params.params["λ"], params._level_probabilities()
cond = f"tf_adjusted_match_prob > {thr!r}"
res = {"link_type": "link_only", "records": [len(t) for t in tables], "pairs": int(job.n_pairs), "condition": cond,
       "reps": reps, "full_reps": full_reps}


def fresh_tf():
    return make_adjustment_for_term_frequencies(ExpectationFrame(gf, st, lam, probs), params, st, amd,
                                                retain_adjustment_columns=True)


def spread(ts):
    return {"median": float(np.median(ts)), "min": float(min(ts)), "max": float(max(ts))}


# (a) the selection against the per-pair tf pass, device-resident results, alternating
tf = fresh_tf()
m, u = job.flat_tables(probs)
term = [(N.SEL_TF_MP, 0, N.SEL_OP[">"], thr)]
t_apply, t_select = [], []
for i in range(reps + 1):
    t0 = time.perf_counter()
    job.ctx.tf_apply_columns(tf.dev_cols, tf.tables, 0, job.n_pairs, want_adj=False, want_host=False)
    t1 = time.perf_counter()
    k = job.ctx.select_tf_columns(float(lam), float(1 - lam), m, u, tf.dev_cols, tf.tables, term)
    t2 = time.perf_counter()
    if i:
        t_apply.append(t1 - t0)
        t_select.append(t2 - t1)
job.selection_owner = None
res["survivors"] = int(k)
res["tf_apply_columns_device_s"] = spread(t_apply)
res["select_tf_columns_s"] = spread(t_select)

# (b) wall time to a pandas frame of the survivors
ts = []
for i in range(reps + 1):
    job._host_cols = {}  # both paths convert the retained input columns again in every run
    f = fresh_tf().filter(cond)
    t0 = time.perf_counter()
    got = f.toPandas()
    if i:
        ts.append(time.perf_counter() - t0)
res["filter_toPandas_s"] = spread(ts)
ts = []
for i in range(full_reps):
    job._pairs_host = None
    job._host_cols = {}
    full = fresh_tf()
    t0 = time.perf_counter()
    pdf = full.toPandas()
    exp = pdf[pdf["tf_adjusted_match_prob"] > thr].reset_index(drop=True)
    ts.append(time.perf_counter() - t0)
res["full_toPandas_then_mask_s"] = spread(ts)
res["identical"] = bool(got.equals(exp))
print(json.dumps(res))
if out_path:
    with open(out_path, "w") as fh:
        json.dump(res, fh, indent=1)
