"""Best match per record against the selection and against the host route, at cfg2 (1 M records, ~46 M pairs).

(a) device time of spk_select_best for each mode (spk_select_best_info, HIP events around its launches) next to
    spk_select's time on the same pairs (spk_select_info), over the survivors of `match_probability > 0.9` and over
    every pair (no threshold);
(b) wall time of df_e.filter(cond).best_matches(per=...).toPandas() against the route without best_matches():
    df_e.filter(cond).toPandas(), then a stable pandas sort by score descending and drop_duplicates on the id
    (per="mutual": over the pairs of either side of a record, then the pairs that win both of theirs);
(c) the A/B of the run collapse: run this tool with the library as built and with SPLINK_AMD_LIB naming variants
    built by
        python tools/build_ab.py OUT.so spk_best.hip -DSPK_BEST_COLLAPSE=N
    (0: one atomic per pair, 1: collapse under per="l" only, 2: under every mode with left groups), in turn in one
    session, and compare the (a) figures; `label` names the run in the output.

Each figure is the median of `reps` runs (`big_reps` for the host route over every pair) after one warm-up, from
fresh frames (no cached result).

    python tools/ab_best.py [label] [reps] [big_reps] [device-only]
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
from splink_amd.frames import ExpectationFrame, FilteredFrame, GammaFrame  # noqa: E402
from splink_amd.params import Params  # noqa: E402
from splink_amd.select import Predicate  # noqa: E402
from splink_amd.session import AmdSession  # noqa: E402
from splink_amd.synthetic import cfg_settings, make_records  # noqa: E402

label = sys.argv[1] if len(sys.argv) > 1 else "collapse"
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 7
big_reps = int(sys.argv[3]) if len(sys.argv) > 3 else 2
device_only = len(sys.argv) > 4 and sys.argv[4] == "device-only"
MP = "match_probability"
PERS = ["l", "r", "either", "mutual"]

cols = ["first_name", "surname", "dob", "city", "email"]
df = make_records(1_000_000, surname_vocab=15000, arrow=True)[["unique_id"] + cols]
params = Params(cfg_settings(2), AmdSession(0))
st = params.settings
job = Job("dedupe_only", [df], "unique_id", 0)
job.ctx.enable_timing(True)
job.block(st["blocking_rules"])
gf = GammaFrame(job, st)
lam, probs = params.params["λ"], params._level_probabilities()


def filtered(thr):
    df_e = ExpectationFrame(gf, st, lam, probs)
    return FilteredFrame(df_e, Predicate()) if thr is None else df_e.filter(f"{MP} > {thr!r}")


def host_best(kept, per):
    """The route without best_matches(): the kept rows of filter(cond).toPandas(), in its order."""
    if per in ("l", "r"):
        first = kept.sort_values(MP, ascending=False, kind="stable").drop_duplicates("unique_id_" + per)
        return kept.loc[np.sort(first.index.to_numpy())].reset_index(drop=True)
    pos = np.arange(len(kept))
    long = pd.DataFrame({"id": np.concatenate([kept["unique_id_l"].to_numpy(), kept["unique_id_r"].to_numpy()]),
                         "pos": np.concatenate([pos, pos]), MP: np.concatenate([kept[MP].to_numpy()] * 2)})
    win = long.sort_values([MP, "pos"], ascending=[False, True], kind="stable").drop_duplicates("id")
    best = pd.Series(win["pos"].to_numpy(), index=win["id"].to_numpy())
    bl = best.reindex(kept["unique_id_l"].to_numpy()).to_numpy() == pos
    br = best.reindex(kept["unique_id_r"].to_numpy()).to_numpy() == pos
    return kept[(bl & br) if per == "mutual" else (bl | br)].reset_index(drop=True)


def med(xs):
    return {"median": float(np.median(xs)), "min": float(min(xs))}


res = {"label": label, "config": 2, "records": len(df), "pairs": int(job.n_pairs), "reps": reps, "big_reps": big_reps,
       "sizes": {}}
for name, thr in (("mp_gt_0.9", 0.9), ("no_threshold", None)):
    out = {"condition": f"{MP} > 0.9" if thr is not None else "every pair"}
    # (a) device time: spk_select, then spk_select_best over its survivors
    for per in PERS:
        sel_ms, best_ms = [], []
        for i in range(reps + 1):
            f = filtered(thr)
            out["survivors"] = int(f.count())
            s_ms = job.ctx.select_info()[1]
            b = f.best_matches(per=per)
            out.setdefault("kept", {})[per] = int(b.count())
            if i:
                sel_ms.append(s_ms)
                best_ms.append(job.ctx.select_best_info()[2])
        out.setdefault("spk_select_ms", {})[per] = med(sel_ms)
        out.setdefault("spk_select_best_ms", {})[per] = med(best_ms)
    b = filtered(thr).best_matches(per="mutual", ties="all")
    b.count()
    out["spk_select_best_ms_mutual_ties_all"] = float(job.ctx.select_best_info()[2])
    # (b) wall time to the best pairs as a pandas frame
    if not device_only:
        n_host = reps if thr is not None else big_reps
        for per in (("l", "mutual") if thr is not None else ("l",)):
            ts = []
            for i in range(reps + 1):
                f = filtered(thr)
                t0 = time.perf_counter()
                got = f.best_matches(per=per).toPandas()
                if i:
                    ts.append(time.perf_counter() - t0)
            out.setdefault("best_matches_toPandas_s", {})[per] = med(ts)
            ts = []
            for i in range(n_host + 1):
                job._host_cols = {}  # the host route converts the retained input columns again in every run
                f = filtered(thr)
                t0 = time.perf_counter()
                host = host_best(f.toPandas(), per)
                if i:
                    ts.append(time.perf_counter() - t0)
            out.setdefault("filter_toPandas_then_host_s", {})[per] = med(ts)
            out.setdefault("identical", {})[per] = bool(got.equals(host))
            del host, got, f
    res["sizes"][name] = out
print(json.dumps(res))
