"""The first k pairs in score order against a plain selection and against the host sort, at cfg2 (1 M records, ~46 M
pairs).

(a) device time of spk_select_top, descending, for k = 100 and k = 100,000 (spk_select_top_info, HIP events around its
    launches): three passes over the codes;
(b) spk_select with `match_probability >= the cut of (a)` on the same codes (spk_select_info): two passes, about the
    same number of survivors (all pairs at the cut instead of tied_kept of them);
(c) the only route to the same rows without spk_select_top: that filter, toPandas() and a pandas sort, wall time;
(d) spk_select_top_of, descending by tf_adjusted_match_prob, k = 100,000, on a tf selection of a few million survivors
    (surname with term-frequency adjustments).
Each device figure is the median of `reps` alternating runs after one warm-up.  With `verify`, (a) at k = 100,000 is
compared once with the definition over the scores of every pair copied to the host.

    python tools/ab_select_top.py [reps] [verify]
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
from splink_amd import select as S  # noqa: E402
from splink_amd.engine import Job  # noqa: E402
from splink_amd.frames import ExpectationFrame, GammaFrame  # noqa: E402
from splink_amd.params import Params  # noqa: E402
from splink_amd.session import AmdSession  # noqa: E402
from splink_amd.synthetic import cfg_settings, make_records  # noqa: E402
from splink_amd.term_frequencies import make_adjustment_for_term_frequencies  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
verify = "verify" in sys.argv[2:]
KS = (100, 100_000)

cols = ["first_name", "surname", "dob", "city", "email"]
df = make_records(1_000_000, surname_vocab=15000, arrow=True)[["unique_id"] + cols]
settings = cfg_settings(2)
for c in settings["comparison_columns"]:
    if c["col_name"] == "surname":
        c["term_frequency_adjustments"] = True
amd = AmdSession(0)
params = Params(settings, amd)
st = params.settings
job = Job("dedupe_only", [df], "unique_id", 0)
job.ctx.enable_timing(True)
job.block(st["blocking_rules"])
gf = GammaFrame(job, st)
lam, probs = params.params["λ"], params._level_probabilities()
df_e = ExpectationFrame(gf, st, lam, probs)
m, u = job.flat_tables(probs)
lam, om = float(lam), float(1 - lam)


def med(xs):
    return {"median": float(np.median(xs)), "min": float(min(xs)), "max": float(max(xs))}


res = {"config": 2, "records": len(df), "pairs": int(job.n_pairs), "patterns": int(job.ctx.n_patterns()), "reps": reps}
for k in KS:
    top_ms, sel_ms = [], []
    for i in range(reps + 1):  # alternating, so both see the same machine
        kept = job.ctx.select_top(lam, om, m, u, [], N.TOP_DESC, k)
        eligible, n_kept, cut, tied, tied_kept, ms = job.ctx.select_top_info()
        survivors = job.ctx.select(lam, om, m, u, [(N.SEL_MP, 0, N.SEL_OP[">="], cut)])
        if i:
            top_ms.append(ms)
            sel_ms.append(job.ctx.select_info()[1])
    t0 = time.perf_counter()
    host = df_e.filter(f"match_probability >= {cut!r}").toPandas()
    host = host.iloc[S.top_order(host["match_probability"].to_numpy(), S.TOP_DESC)[:k]].reset_index(drop=True)
    wall_host = time.perf_counter() - t0
    t0 = time.perf_counter()
    dev = df_e.orderBy("match_probability", ascending=False).limit(k).toPandas()
    wall_dev = time.perf_counter() - t0
    r = {"kept": int(kept), "cut": cut, "tied": int(tied), "tied_kept": int(tied_kept),
         "a_spk_select_top_ms": med(top_ms), "b_spk_select_ms": med(sel_ms), "b_survivors": int(survivors),
         "c_filter_toPandas_sort_wall_s": wall_host, "orderBy_limit_toPandas_wall_s": wall_dev,
         "same_rows": bool(dev.equals(host))}
    r["a_over_b"] = r["a_spk_select_top_ms"]["median"] / r["b_spk_select_ms"]["median"]
    res[f"k={k}"] = r

tf = make_adjustment_for_term_frequencies(df_e, params, st, amd)
for t in (0.5, 0.1, 0.01, 1e-3, 1e-4, 1e-5, 0.0):
    f = tf.filter(f"tf_adjusted_match_prob > {t!r}")
    if f.count() >= 2_000_000:
        break
of_ms = []
for i in range(reps + 1):
    f._n = None  # select again: the narrowing replaced the survivors
    n = f._select()
    kept = job.ctx.select_top_of(N.SEL_TF_MP, N.TOP_DESC, KS[1])
    job.selection_owner = None
    if i:
        of_ms.append(job.ctx.select_top_info()[5])
res["d_spk_select_top_of"] = {"survivors": int(n), "tf_threshold": t, "k": KS[1], "kept": int(kept), "ms": med(of_ms)}

if verify:
    k = KS[1]
    assert job.ctx.select_top(lam, om, m, u, [], N.TOP_DESC, k) == k
    ordinal = job.ctx.select_copy(0, k, len(gf.meta[0]), rows=False, gammas=False, mp=False)[0]
    mp = job.score(lam, probs)
    res["identical_to_definition"] = bool(np.array_equal(ordinal, np.sort(S.top_order(mp, S.TOP_DESC)[:k])))
print(json.dumps(res))
