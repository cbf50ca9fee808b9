"""Rates of jaccard_sim / cosine_distance next to the unmodified bench workload (cfg2), one process:
the comparison pass with the surname column replaced by (a) a jaccard_sim CASE and (b) a cosine_distance CASE
over QgramTokeniser(surname), and the bulk functions' pairs/s next to jaro_winkler_sim's on the same strings.

    python tools/ab_setsim.py [records]
"""
import copy
import os
import sys
import time

import numpy as np
import pandas as pd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402,F401  (torch's HIP runtime first, as bench.py)
from splink_amd import _native as N  # noqa: E402
from splink_amd.engine import Job  # noqa: E402
from splink_amd.params import Params  # noqa: E402
from splink_amd.session import AmdSession  # noqa: E402
from splink_amd.synthetic import cfg_settings, make_records  # noqa: E402

COLS = ["first_name", "surname", "dob", "city", "email"]
GUARD = "case when surname_l is null or surname_r is null then -1 "
JAC = "jaccard_sim(surname_l, surname_r)"
COS = "cosine_distance(QgramTokeniser(surname_l), QgramTokeniser(surname_r))"
VARIANTS = [
    ("cfg2", None),
    ("surname -> jaccard_sim", GUARD + f"when {JAC} >= 0.8 then 2 when {JAC} >= 0.5 then 1 else 0 end"),
    ("surname -> cosine_distance over bigrams", GUARD + f"when {COS} <= 0.2 then 2 when {COS} <= 0.5 then 1 else 0 end"),
]


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
    df = make_records(n, surname_vocab=int(os.environ.get("AB_VOCAB", "15000")), arrow=True)[["unique_id"] + COLS]
    base = cfg_settings(2)
    job = Job("dedupe_only", [df], "unique_id", 0)
    job.ctx.enable_timing(True)
    job.block(base["blocking_rules"])
    print(f"{n} records, {job.n_pairs} pairs", flush=True)
    for name, expr in VARIANTS:
        st = copy.deepcopy(base)
        if expr is not None:
            st["comparison_columns"][1] = {"custom_name": "surname_set", "custom_columns_used": ["surname"],
                                           "num_levels": 3, "case_expression": expr}
        st = Params(st, AmdSession(0)).settings
        job.gammas(st)
        ts = []
        for _ in range(5):
            job.gammas(st)
            ts.append(job.ctx.kernel_ms()["gamma"])
        job.ctx.sync()
        cells = job.ctx.gammas_exact_counts(len(COLS))
        print(f"{name}: gamma pass {np.median(ts):.3f} ms (min {min(ts):.3f}), template columns "
              f"{job.ctx.gammas_simple_count()}, exact cells {cells}", flush=True)
    # bulk functions on the surnames of the pairs themselves
    m = min(job.n_pairs, 2_000_000)
    l, r = job.ctx.pairs_copy(job.n_pairs - m, m)  # the last rule's pairs: the surnames differ
    sn = job.tables[0]["surname"].to_numpy(dtype=object)
    keep = ~(pd.isna(sn[l]) | pd.isna(sn[r]))
    left, right = list(sn[l][keep]), list(sn[r][keep])
    ctx = N.Context(0)
    for fn in ("jaro_winkler_sim", "jaccard_sim", "cosine_distance"):
        getattr(ctx, fn)(left[:1000], right[:1000])
        t0 = time.perf_counter()
        out = getattr(ctx, fn)(left, right)
        dt = time.perf_counter() - t0
        print(f"bulk {fn}: {len(left)} pairs in {dt * 1e3:.1f} ms end to end (host encoding and copies included), "
              f"{len(left) / dt:.3e} pairs/s, mean {np.nanmean(out):.4f}", flush=True)


if __name__ == "__main__":
    main()
