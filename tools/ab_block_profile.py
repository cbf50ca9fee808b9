"""The blocking-rule profile against the blocking call, on cfg2's rules at 1 M records and on cfg5's two rules at the
size `bench.py --config 5` uses (1 M records generated with the address column).

(a) the key-level profile (max_enumerate = 0): wall time from a fresh job (upload of the key columns, key build,
    spk_block_profile) and the call's own HIP-event time (spk_block_profile_info, key-level part);
(b) the profile with every rule enumerated (max_enumerate < 0): the same, plus the HIP-event time of the count pass
    and the ordinals it walked -- their quotient is the rate DEFAULT_MAX_ENUMERATE is taken from;
(c) the route there was before for the same counts: Job.block on a fresh job (clustered, as block_using_rules runs
    it), reading n_pairs / n_candidates: wall time, and its split into keys and pairs (Job.timings);
(d) the largest-blocks step (limit 5, by candidates) on a job whose keys are built: the key-level HIP-event time with
    the bin cut, without it (every block sorted), and with limit 0 (no largest-blocks step at all).

The runs alternate inside one loop; each figure is the median of `reps` runs after one warm-up, with min and max.

    python tools/ab_block_profile.py [reps]
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
from splink_amd.compiler import compile_rule  # noqa: E402
from splink_amd.engine import Job  # noqa: E402
from splink_amd.synthetic import cfg_settings, make_records  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
KEYS = ["unique_id", "surname", "dob"]  # what the two rules read


def spread(xs):
    return {"median": float(np.median(xs)), "min": float(min(xs)), "max": float(max(xs)), "n": len(xs)}


def profile_fresh(df, rules, max_enumerate):
    t0 = time.perf_counter()
    job = Job("dedupe_only", [df], "unique_id", 0, cluster=False)
    job.ctx.enable_timing(True)
    specs = [compile_rule(r, job.schema) for r in rules]
    out = job.profile_rules(specs, max_enumerate=max_enumerate, limit=5)
    wall = time.perf_counter() - t0
    key_ms, enum_ms, ordinals = job.ctx.block_profile_info()
    job.ctx.close()
    return wall, key_ms, enum_ms, ordinals, out[0]


def block_fresh(df, rules):
    t0 = time.perf_counter()
    job = Job("dedupe_only", [df], "unique_id", 0)
    job.block(list(rules))
    wall = time.perf_counter() - t0
    out = (wall, job.timings["block_keys_s"], job.timings["block_pairs_s"], int(job.n_pairs), int(job.n_candidates))
    job.ctx.close()
    return out


def measure(config, df):
    rules = cfg_settings(config)["blocking_rules"]
    a_wall, a_key, b_wall, b_key, b_enum, c_wall, c_keys, c_pairs = [], [], [], [], [], [], [], []
    d_cut, d_all, d_none = [], [], []
    held = Job("dedupe_only", [df], "unique_id", 0, cluster=False)
    held.ctx.enable_timing(True)
    specs = [compile_rule(r, held.schema) for r in rules]
    sym = held._set_rule_keys(specs)

    def key_ms(cut, limit):
        held.ctx.block_profile_set_cut(cut)
        held.ctx.block_profile(0, sym, None, 0, 1, 0, N.LARGEST_BY_CANDIDATES, limit)
        return held.ctx.block_profile_info()[0]

    for i in range(reps + 1):
        a = profile_fresh(df, rules, 0)
        b = profile_fresh(df, rules, -1)
        c = block_fresh(df, rules)
        d = (key_ms(True, 5), key_ms(False, 5), key_ms(True, 0))
        if not i:
            continue
        a_wall.append(a[0]), a_key.append(a[1])
        b_wall.append(b[0]), b_key.append(b[1]), b_enum.append(b[2])
        c_wall.append(c[0]), c_keys.append(c[1]), c_pairs.append(c[2])
        d_cut.append(d[0]), d_all.append(d[1]), d_none.append(d[2])
    prof = b[4]
    assert int(prof["enumerated"].sum()) == c[3] and int(prof["candidates"].sum()) == c[4]
    return {
        "config": config, "records": len(df), "rules": rules, "reps": reps,
        "blocks": [int(x) for x in prof["blocks"]], "candidates": [int(x) for x in prof["candidates"]],
        "pairs": [int(x) for x in prof["enumerated"]], "n_pairs": c[3], "n_candidates": c[4],
        "a_key_level": {"fresh_job_wall_s": spread(a_wall), "key_ms": spread(a_key)},
        "b_with_enumeration": {"fresh_job_wall_s": spread(b_wall), "key_ms": spread(b_key), "enum_ms": spread(b_enum),
                               "ordinals": int(b[3]),
                               "ordinals_per_s_at_median": b[3] / (np.median(b_enum) * 1e-3)},
        "c_job_block": {"fresh_job_wall_s": spread(c_wall), "block_keys_s": spread(c_keys),
                        "block_pairs_s": spread(c_pairs), "pair_bytes": 8 * c[3]},
        "d_largest_blocks_key_ms": {"cut": spread(d_cut), "no_cut": spread(d_all), "limit_0": spread(d_none)},
    }


for config in (2, 5):
    table = make_records(1_000_000, surname_vocab=15000, with_address=config == 5, arrow=True)[KEYS]
    print(json.dumps(measure(config, table)), flush=True)
    del table
