"""Golden fixture for get_largest_blocks (run in the build container only).

Runs the reference's own comparison_evaluation.get_largest_blocks (comparison_evaluation.py:12-35) over sqlite,
through make_golden.py's SqliteSpark / SqliteFrame, for three key-only rules and two limits each, and writes the
table and the returned rows to tests/golden/largest_blocks.json.  Data only.

Usage:  PYTHONPATH=/root/reference python tests/golden/make_golden_blocks.py
"""
from __future__ import annotations

import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from make_golden import SqliteFrame, SqliteSpark, connect, dump, frame_json, q, to_table  # noqa: E402

from splink.comparison_evaluation import get_largest_blocks  # noqa: E402  (reference)

from splink_amd.synthetic import make_records  # noqa: E402

RULES = [
    "l.surname = r.surname",
    "l.city = r.city and l.dob = r.dob",
    "l.first_name = r.first_name AND l.surname = r.surname",
]
LIMITS = [5, 8]


def records():
    df = make_records(600, seed=11, surname_vocab=25, first_vocab=12, city_vocab=6)[
        ["unique_id", "first_name", "surname", "dob", "city"]].copy()
    df["dob"] = [None if d is None else str(d)[:4] for d in df["dob"].tolist()]  # the year: blocks of several rows
    return df


def main():
    df = records()
    con = connect()
    to_table(con, df, "records")
    spark = SqliteSpark(con)
    cases = []
    for rule in RULES:
        for limit in LIMITS:
            out = get_largest_blocks(rule, SqliteFrame(con, "select * from records"), spark, limit=limit)
            rows = q(con, out.sql)
            print(rule, limit, rows["count"].tolist())
            cases.append({"rule": rule, "limit": limit, "rows": frame_json(rows)})
    dump("largest_blocks", {"table": frame_json(df), "cases": cases})


if __name__ == "__main__":
    main()
