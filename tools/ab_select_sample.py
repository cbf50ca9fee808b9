"""The stratified sample against a plain selection, at cfg2 (1 M records, ~46 M pairs).

Device time of spk_select_sample (10 equal-width strata, quota 200, no terms; spk_select_sample_info, HIP events
around its launches) next to spk_select with the term `match_probability > 0.95` on the same codes (spk_select_info):
that one streams the codes through one count pass and one emit pass, the sample through 8 histogram passes, a count
pass and an emit pass, each of which also computes the pairs' keys.  Each figure is the median of `reps` runs after one
warm-up.  With `verify`, the sample is compared once with the definition (tools/emulate_select_sample.py) over the
scores of every pair copied to the host.

    python tools/ab_select_sample.py [reps] [verify]
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402,F401
import emulate_select_sample as emu  # noqa: E402
from splink_amd import _native as N  # noqa: E402
from splink_amd.engine import Job  # noqa: E402
from splink_amd.frames import GammaFrame  # noqa: E402
from splink_amd.params import Params  # noqa: E402
from splink_amd.session import AmdSession  # noqa: E402
from splink_amd.synthetic import cfg_settings, make_records  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
verify = "verify" in sys.argv[2:]
STRATA, QUOTA, SEED, PASSES = 10, 200, 0, 8 + 2

cols = ["first_name", "surname", "dob", "city", "email"]
df = make_records(1_000_000, surname_vocab=15000, arrow=True)[["unique_id"] + cols]
params = Params(cfg_settings(2), AmdSession(0))
st = params.settings
job = Job("dedupe_only", [df], "unique_id", 0)
job.ctx.enable_timing(True)
job.block(st["blocking_rules"])
gf = GammaFrame(job, st)
lam, probs = params.params["λ"], params._level_probabilities()
m, u = job.flat_tables(probs)
edges = [i / STRATA for i in range(STRATA + 1)]
quota = [QUOTA] * STRATA


def med(xs):
    return {"median": float(np.median(xs)), "min": float(min(xs)), "max": float(max(xs))}


sample_ms, select_ms = [], []
for i in range(reps + 1):  # alternating, so both see the same machine
    kept = job.ctx.select_sample(float(lam), float(1 - lam), m, u, [], edges, quota, SEED)
    n_strata, pop, cnt, ms = job.ctx.select_sample_info()
    survivors = job.ctx.select(float(lam), float(1 - lam), m, u, [(N.SEL_MP, 0, N.SEL_OP[">"], 0.95)])
    if i:
        sample_ms.append(ms)
        select_ms.append(job.ctx.select_info()[1])
res = {"config": 2, "records": len(df), "pairs": int(job.n_pairs), "patterns": int(job.ctx.n_patterns()), "reps": reps,
       "strata": STRATA, "quota": QUOTA, "population": [int(x) for x in pop], "sampled": [int(x) for x in cnt],
       "kept": int(kept), "spk_select_sample_ms": med(sample_ms), "passes_over_the_codes": PASSES,
       "spk_select_mp_gt_0.95_ms": med(select_ms), "spk_select_survivors": int(survivors),
       "spk_select_passes_over_the_codes": 2}
res["ratio"] = res["spk_select_sample_ms"]["median"] / res["spk_select_mp_gt_0.95_ms"]["median"]
res["ratio_per_pass"] = res["ratio"] / (PASSES / 2)
if verify:
    assert job.ctx.select_sample(float(lam), float(1 - lam), m, u, [], edges, quota, SEED) == kept
    ordinal = job.ctx.select_copy(0, kept, len(gf.meta[0]), rows=False, gammas=False, mp=False)[0]
    mp = job.score(lam, probs)
    want, _, want_pop, want_cnt = emu.sample(SEED, np.arange(len(mp), dtype=np.int64), mp, edges, quota)
    res["identical_to_definition"] = bool(np.array_equal(ordinal, np.nonzero(want)[0]) and
                                          np.array_equal(pop, want_pop) and np.array_equal(cnt, want_cnt))
print(json.dumps(res))
