"""u from random record pairs (no counterpart in the reference release; later releases:
estimate_u_using_random_sampling).

Blocked pairs are mostly agreeing pairs, so u = P(level | non-match) estimated from them by EM leans towards
agreement.  Random record pairs are nearly all non-matches: their comparison levels give u directly, and EM then
finds m and λ on the blocked pairs with u held fixed (Params.fix_u_probabilities).

The pairs are drawn on the device (spk_pairs_sample): draw i is a function of (seed, i, total draws) alone, so the
sample can be walked in batches under a memory cap and in contiguous shares by the ranks of a process group.  What
is kept per batch is the integer pattern histogram of its comparison pass; the sum of those does not depend on the
batch size, the rank count or the launch shape.  The draws are independent (sampling with replacement).
"""
from __future__ import annotations

import numpy as np
import pandas as pd

from .engine import Job, distributed_shard, session_device
from .frames import ComparisonFrame
from .labels import NON_MATCH, LabelCounts
from .settings import complete_settings_dict


def _sampling_job(settings, spark, df_l, df_r, df) -> Job:
    """The records on the device in input row order: no blocking rules, so no keys and no clustering."""
    from .blocking import _tables
    return Job(settings["link_type"], _tables(settings, df_l, df_r, df), settings["unique_id_column_name"],
               session_device(spark), shard=distributed_shard(), cluster=False)


def random_pairs(settings: dict, spark, n_draws: int, seed: int = 0, df_l=None, df_r=None, df=None):
    """`n_draws` random record pairs allowed by the link type, drawn on the device with replacement: the random
    counterpart of cartesian_block.  Under dedupe_only / link_and_dedupe a draw whose two records have equal or
    NULL unique ids (within one source) is dropped, as the link-type predicate drops the pair, so slightly fewer
    than n_draws pairs can come back."""
    settings = complete_settings_dict(settings, spark)
    job = _sampling_job(settings, spark, df_l, df_r, df)
    job.sample_pairs(int(n_draws), 0, int(n_draws), seed)
    return ComparisonFrame(job, settings)


def u_rows_from_histogram(gamma_names, n_levels, hist):
    """One row per (gamma column, level from -1 on) of a pattern histogram of non-matching pairs: its pair count
    and u = count_v / Σ_{v >= 0} count_v by the M-step's own arithmetic -- LabelCounts(...).m_step() with every
    pair labelled a non-match: the float32 cast, the NULL level (-1) outside the denominator and without a u
    (None), a level no pair shows at 0 as Params._populate_params leaves it."""
    hist = np.ascontiguousarray(hist, dtype=np.int64)
    zero = np.zeros_like(hist)
    counts = LabelCounts(gamma_names, n_levels, np.stack([hist, zero, zero]))
    _, pi_rows = counts.m_step()
    u = {(r["gamma_col"], r["gamma_value"]): r["new_probability_non_match"] for r in pi_rows}
    lev = counts.levels(np.arange(counts.n_patterns))
    out = []
    for k, (name, L) in enumerate(zip(counts.names, counts.n_levels)):
        for v in range(-1, L):
            n = int(counts.counts[NON_MATCH][lev[:, k] == v].sum())
            out.append({"gamma_col": name, "gamma_value": v, "count": n,
                        "u_probability": None if v < 0 else u.get((name, v), 0)})
    return out


def estimate_u_using_random_sampling(settings: dict, params, spark, max_pairs: int, seed: int = 0,
                                     batch_pairs: int = 1 << 28, fix: bool = True, df_l=None, df_r=None, df=None):
    """Estimate every u (prob_dist_non_match) of `params` from `max_pairs` random record pairs and, with fix=True,
    hold them fixed in the M-steps that follow.  The current parameters go to the history; m and λ are not
    touched.  The sample is walked in ranges of `batch_pairs` draws (a memory cap: 8 bytes of pair rows and 2-4
    of codes per draw), under a process group each rank over its contiguous share of the draws; the result does
    not depend on either.  Returns a DataFrame with one row per (gamma column, level): gamma_col, gamma_value
    (-1 = NULL, which has no u), count, u_probability."""
    max_pairs, batch_pairs = int(max_pairs), int(batch_pairs)
    if max_pairs < 1 or batch_pairs < 1:
        raise ValueError("estimate_u_using_random_sampling: max_pairs and batch_pairs must be positive")
    settings = complete_settings_dict(settings, spark)
    job = _sampling_job(settings, spark, df_l, df_r, df)
    rank, world = distributed_shard()
    lo, hi = max_pairs * rank // world, max_pairs * (rank + 1) // world
    # every rank runs the same number of batches (the histograms are summed over the ranks batch by batch): the
    # largest share's; a rank whose share ends sooner samples empty ranges
    n_batches = -(-(-(-max_pairs // world)) // batch_pairs)
    hist = None
    for b in range(n_batches):
        first = min(lo + b * batch_pairs, hi)
        job.sample_pairs(max_pairs, first, min(batch_pairs, hi - first), seed)
        job.gammas(settings)
        h = job.pattern_histogram()
        hist = h if hist is None else hist + h
    names, n_levels = job.code_meta
    rows = u_rows_from_histogram(names, n_levels, hist)
    params._save_params_to_iteration_history()
    for r in rows:
        if r["gamma_value"] >= 0:
            params._set_pi_value(r["gamma_col"], r["gamma_value"], "non_match", r["u_probability"])
    if fix:
        params.fix_u_probabilities = True
    return pd.DataFrame(rows, columns=["gamma_col", "gamma_value", "count", "u_probability"])
