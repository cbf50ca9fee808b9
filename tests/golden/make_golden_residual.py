"""Golden fixture for blocking rules with residual predicates (run in the build container only).

The reference splices any join condition into `on {rule} {not_previous_rules}` (blocking.py:59-68,
145-154); this script runs four such rules -- equalities AND-ed with abs(), levenshtein() and `<`
residuals -- through the reference pipeline of make_golden.py (the reference's own SQL on sqlite) for the
three link types and writes tests/golden/residual_rules.json.  Data only.

Usage:  PYTHONPATH=/root/reference python tests/golden/make_golden_residual.py
"""
from __future__ import annotations

import os
import sys

import numpy as np
import pandas as pd

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from make_golden import dump, reference_pipeline  # noqa: E402

RULES = [
    "l.city = r.city and abs(l.age - r.age) < 5",
    "l.surname = r.surname and levenshtein(l.first_name, r.first_name) <= 1",
    "l.city = r.city",
    "l.surname = r.surname and l.age < r.age",
]

FIRST_NAMES = ["ann", "anne", "anna", "bob", "rob", "bobby", None, "cat", "kat", "cath"]
SURNAMES = ["smith", "smyth", "jones", None, "jonas"]
CITIES = ["a", "b", None]


def records(n=60):
    rng = np.random.default_rng(7)
    first = [FIRST_NAMES[i] for i in rng.integers(0, len(FIRST_NAMES), n)]
    sur = [SURNAMES[i] for i in rng.integers(0, len(SURNAMES), n)]
    city = [CITIES[i] for i in rng.integers(0, len(CITIES), n)]
    age = [float(a) if a <= 70 else None for a in rng.integers(20, 75, n)]
    return pd.DataFrame({"unique_id": list(range(n)), "first_name": first, "surname": sur, "city": city, "age": age})


def settings(link_type):
    return {
        "link_type": link_type,
        "proportion_of_matches": 0.3,
        "max_iterations": 2,
        "comparison_columns": [{"col_name": "first_name", "num_levels": 3}, {"col_name": "surname", "num_levels": 2}],
        "additional_columns_to_retain": ["city", "age"],
        "blocking_rules": list(RULES),
    }


def main():
    df = records()
    df_l = df.iloc[:35].reset_index(drop=True)
    df_r = df.iloc[25:].reset_index(drop=True)
    cases = {
        "dedupe_only": reference_pipeline(settings("dedupe_only"), False, df=df),
        "link_only": reference_pipeline(settings("link_only"), False, df_l=df_l, df_r=df_r),
        "link_and_dedupe": reference_pipeline(settings("link_and_dedupe"), False, df_l=df_l, df_r=df_r),
    }
    for name, g in cases.items():
        assert "error" not in g, (name, g["error"])
        g.pop("gammas", None)  # df_e carries the gamma columns; keeps the file small
        print(name, len(g["df_e"]["unique_id_l"]), "pairs")
    dump("residual_rules", cases)


if __name__ == "__main__":
    main()
