"""What blocking rules would cost, before the pairs are generated (reference: splink/comparison_evaluation.py:12-35).

`get_largest_blocks` keeps the reference's signature and meaning: the rows per value of a rule's l-side key, largest
first.  `profile_blocking_rules` goes further, for the rules of a settings dict in order: per rule the rows with a
key, the blocks, the candidate pairs and the largest block, a histogram of block sizes, the largest blocks with their
key values, and -- where the candidate range is short enough to walk -- the pairs the rule would really emit after the
link-type predicate and the exclusion by earlier rules.  Everything is computed on the GPU from the sorted blocking
keys (spk_block_profile); no pair is materialised, so a rule that would exhaust the device's memory is profiled at
the cost of its key sort.
"""
from __future__ import annotations

import numpy as np
import pandas as pd

from . import _native as N
from .compiler import compile_rule
from .engine import Job, session_device
from .settings import complete_settings_dict

# Candidate ordinals of one rule up to which profile_blocking_rules also counts the pairs the rule emits.  Measured:
# spk_block's count pass walks 2.56e10 ordinals / s on an MI355X (cfg2's rules, 1 M records, 2026-10-20,
# tools/ab_block_profile.py, profiles/ab_block_profile.log); 2 s of that is 5.1e10, rounded down to a power of two.
DEFAULT_MAX_ENUMERATE = 1 << 35

_ROW_ID = "__row_position"


class HostFrame:
    """A small host-side result with the frame surface reference callers use (toPandas, count, columns)."""

    def __init__(self, df: pd.DataFrame):
        self._df = df.reset_index(drop=True)

    def toPandas(self) -> pd.DataFrame:  # noqa: N802 (Spark name)
        return self._df.copy()

    def to_pandas(self) -> pd.DataFrame:
        return self.toPandas()

    def count(self) -> int:
        return len(self._df)

    def __len__(self):
        return len(self._df)

    @property
    def columns(self):
        return list(self._df.columns)


def key_column_name(kexpr) -> str:
    """A key expression as the reference names its column: the rule's l-side text with `l.` removed."""
    text = kexpr.column
    for tr in kexpr.transforms:
        if tr[0] == "substr":
            text = f"substr({text}, {tr[1]})" if tr[2] >= 2 ** 31 - 1 else f"substr({text}, {tr[1]}, {tr[2]})"
        else:
            text = f"{tr[0]}({text})"
    return text


def _key_frame(job: Job, spec, rows) -> pd.DataFrame:
    """The l-side key values of the device rows `rows` of table 0, one column per key term of the rule: evaluated on
    the host, for these few rows only."""
    rows = np.asarray(rows, dtype=np.int64)
    inp = rows if job.perm[0] is None else np.asarray(job.perm[0])[rows]
    t = job.inputs[0].take(inp).reset_index(drop=True)
    out = {}
    for lexpr, _ in (spec.terms if spec is not None else []):
        name = key_column_name(lexpr)
        if name not in out:
            out[name] = job._key_values(t, lexpr).tolist()
    return pd.DataFrame(out, index=range(len(rows)))


def get_largest_blocks(blocking_rule: str, df, spark, limit: int = 5) -> HostFrame:
    """For one table, the `limit` largest blocks of a blocking rule: the rows per value of the rule's l-side key, rows
    with a NULL key left out, largest first (ties: in key order).  Columns: the l-side key expressions with `l.`
    removed, in the rule's order, then `count`.

    The rule is compiled as blocking compiles it, so `l.city = r.city and abs(l.age - r.age) < 5` is profiled on its
    key term (the reference's query breaks on it) and a rule without an equality raises ValueError."""
    from .blocking import as_pandas
    from .engine import schema_of
    limit = int(limit)
    if limit < 0:
        raise ValueError("get_largest_blocks: limit must not be negative")
    table = as_pandas(df)
    spec = compile_rule(blocking_rule, schema_of([table]))
    # the link-type predicate plays no part in a key-level profile: row position serves as the unique id
    table = table.assign(**{_ROW_ID: np.arange(len(table), dtype=np.int64)})
    job = Job("dedupe_only", [table], _ROW_ID, session_device(spark), cluster=False)
    _, _, largest = job.profile_rules([spec], max_enumerate=0, largest_by=N.LARGEST_BY_ROWS_L, limit=limit)
    top = largest[0]
    out = _key_frame(job, spec, top["row_l"])
    out["count"] = top["rows_l"].astype(np.int64)
    return HostFrame(out)


class BlockingProfile:
    """The result of profile_blocking_rules, on the host.

    rules: one row per rule -- rule, rows_l, rows_r (rows with a non-NULL key as the join's l- / r-side), blocks
    (distinct l-side key values), candidates (sum over blocks of n(n-1)/2 or nL * nR), largest_candidates (of one
    block), enumerated (nullable: the pairs left of the rule's candidates after the link-type predicate and the
    exclusion on the keys of earlier key-only rules; NA when the rule's range was too long to walk), pairs (nullable:
    `enumerated` where neither the rule nor an earlier one has a residual predicate, else NA -- the residual decides,
    and the profile does not evaluate it) and cumulative_pairs."""

    def __init__(self, rule_texts, has_residual, rules, hist, largest, key_frames):
        self.rule_texts = list(rule_texts)
        self._hist = np.asarray(hist, dtype=np.int64).reshape(len(self.rule_texts), N.PROFILE_BINS, 2)
        self._largest = list(largest)
        self._keys = list(key_frames)
        rules = np.asarray(rules, dtype=N.RULE_PROFILE_DTYPE)
        df = pd.DataFrame({"rule": self.rule_texts})
        for c in ("rows_l", "rows_r", "blocks", "candidates", "largest_candidates"):
            df[c] = rules[c].astype(np.int64)
        enumerated = pd.array([None if e < 0 else int(e) for e in rules["enumerated"].tolist()], dtype="Int64")
        df["enumerated"] = enumerated
        decided = ~np.logical_or.accumulate(np.asarray(has_residual, dtype=bool)) if len(has_residual) else \
            np.zeros(0, dtype=bool)
        df["pairs"] = pd.array([e if ok and e is not pd.NA else None for e, ok in zip(enumerated, decided)],
                               dtype="Int64")
        df["cumulative_pairs"] = df["pairs"].cumsum(skipna=False)
        self.rules = df

    def largest_blocks(self, r: int) -> pd.DataFrame:
        """Rule r's largest blocks by candidates: its key columns, then rows_l, rows_r, candidates."""
        out = self._keys[r].copy()
        for c in ("rows_l", "rows_r", "candidates"):
            out[c] = self._largest[r][c].astype(np.int64)
        return out

    def histogram(self, r: int) -> pd.DataFrame:
        """Rule r's blocks by the bit length of their candidate count (bin 0: no candidate; bin i: 2^(i-1) .. 2^i - 1),
        the non-empty bins: bin, blocks, candidates."""
        h = self._hist[r]
        bins = np.nonzero(h[:, 0])[0]
        return pd.DataFrame({"bin": bins.astype(np.int64), "blocks": h[bins, 0], "candidates": h[bins, 1]})

    def __repr__(self):
        return f"BlockingProfile(\n{self.rules.to_string()}\n)"


def profile_blocking_rules(settings: dict, spark, df_l=None, df_r=None, df=None, limit: int = 5,
                           max_enumerate: int = DEFAULT_MAX_ENUMERATE) -> BlockingProfile:
    """Profile the settings' blocking rules, in order, over the tables block_using_rules would take (no rules: the
    cartesian block), without generating a pair.  `limit`: largest blocks kept per rule.  `max_enumerate`: a rule
    whose candidate range is at most this long is also walked by blocking's count pass, which gives the pairs the
    rule emits (BlockingProfile.rules' `enumerated` / `pairs`); 0 never, negative always.  The default,
    DEFAULT_MAX_ENUMERATE = 2^35 ordinals, is 2 s of that pass at the 2.56e10 ordinals / s measured on an MI355X
    (cfg2's rules, 1 M records, 2026-10-20, tools/ab_block_profile.py), rounded down to a power of two.  Always the whole job: the profile is
    not split over the ranks of a process group."""
    from .blocking import _tables
    settings = complete_settings_dict(settings, spark)
    limit = int(limit)
    if limit < 0:
        raise ValueError("profile_blocking_rules: limit must not be negative")
    texts = list(settings.get("blocking_rules") or [])
    job = Job(settings["link_type"], _tables(settings, df_l, df_r, df), settings["unique_id_column_name"],
              session_device(spark), cluster=False)
    specs = [compile_rule(t, job.schema) for t in texts]
    rules, hist, largest = job.profile_rules(specs, max_enumerate=int(max_enumerate),
                                             largest_by=N.LARGEST_BY_CANDIDATES, limit=limit)
    if not specs:
        texts, specs = ["(no blocking rules: cartesian)"], [None]
    keys = [_key_frame(job, spec, top["row_l"]) for spec, top in zip(specs, largest)]
    residual = [spec is not None and spec.residual is not None for spec in specs]
    return BlockingProfile(texts, residual, rules, hist, largest, keys)
