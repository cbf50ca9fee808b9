"""spk_pairs_sample restated on the host from the definition in include/splink_hip.h (Python integers, mod 2^64),
and the records / settings / host u arithmetic the sampling tests share."""
import numpy as np

M64 = (1 << 64) - 1
GOLDEN_GAMMA = 0x9E3779B97F4A7C15


def mix(x):
    """The splitmix64 finaliser."""
    x &= M64
    x ^= x >> 30
    x = (x * 0xBF58476D1CE4E5B9) & M64
    x ^= x >> 27
    x = (x * 0x94D049BB133111EB) & M64
    x ^= x >> 31
    return x


def word(seed, i, j):
    return mix((mix(seed) + GOLDEN_GAMMA * (3 * i + j + 1)) & M64)


def below(w, n):
    return (w * n) >> 64


def anchor(seed, i, total, n0):
    lo, hi = (i * n0) // total, ((i + 1) * n0) // total
    return lo + below(word(seed, i, 0), hi - lo) if hi > lo else lo


def sample(seed, total, first, count, n0, n1=None, rank=None, null_div=0):
    """(l, r) int32 arrays: the surviving draws among the ordinals [first, first + count) of a sample of `total`.
    n1 given: link_only (table 0 x table 1, every draw survives); else one table of n0 rows with `rank` per row
    and the NULL-unique-id layout `null_div` (0 = none)."""
    ls, rs = [], []
    link_only = n1 is not None
    if (link_only and (n0 == 0 or n1 == 0)) or (not link_only and n0 < 2):
        count = 0
    for i in range(first, first + count):
        a = anchor(seed, i, total, n0)
        w1 = word(seed, i, 1)
        if link_only:
            ls.append(a)
            rs.append(below(w1, n1))
            continue
        b = below(w1, n0 - 1)
        b += b >= a
        ra, rb = int(rank[a]), int(rank[b])
        if ra == rb:
            continue
        if null_div > 0 and ra // null_div == rb // null_div and \
                (ra % null_div == null_div - 1 or rb % null_div == null_div - 1):
            continue
        l, r = (a, b) if ra < rb else (b, a)
        ls.append(l)
        rs.append(r)
    return np.array(ls, dtype=np.int32), np.array(rs, dtype=np.int32)


# ---- the records and settings of the comparison-pass and u tests ---------------------------------------------
N_RECORDS = 300
N_DRAWS = 20000
U_SEED = 7


def records():
    """300 synthetic records with a numeric column (age, some NULL) next to the string ones."""
    from splink_amd.synthetic import make_records
    df = make_records(N_RECORDS, seed=11, surname_vocab=60, first_vocab=40, city_vocab=8)
    rng = np.random.Generator(np.random.PCG64(5))
    age = rng.integers(18, 60, N_RECORDS).astype(np.float64)
    age[rng.random(N_RECORDS) < 0.05] = np.nan
    df["age"] = age
    df["unique_id"] = rng.permutation(N_RECORDS).astype(np.int64)  # the id order is not the row order
    return df


def settings(rules=()):
    """cfg1-style: a Jaro-Winkler, a Levenshtein, an exact and a numeric comparison column.  All four read fields of
    a small vocabulary, so every level occurs among non-matching pairs: the closeness test's bound is the sampling
    error alone, and the true matches among the draws (0.2 % of all pairs) must stay well inside it."""
    from splink_amd.synthetic import _eq2, _jw3, _lev3
    return {
        "link_type": "dedupe_only", "proportion_of_matches": 0.05, "max_iterations": 4, "em_convergence": 1e-12,
        "retain_matching_columns": False, "retain_intermediate_calculation_columns": False,
        "blocking_rules": list(rules),
        "comparison_columns": [
            {"col_name": "first_name", "num_levels": 3, "case_expression": _jw3("first_name")},
            {"col_name": "surname", "num_levels": 3, "case_expression": _lev3("surname")},
            {"col_name": "city", "num_levels": 2, "case_expression": _eq2("city")},
            {"col_name": "age", "num_levels": 3,
             "case_expression": "case when age_l is null or age_r is null then -1 "
                                "when abs(age_l - age_r) < 1.5 then 2 when abs(age_l - age_r) < 10 then 1 else 0 end"},
        ],
    }


NAMES = ["gamma_first_name", "gamma_surname", "gamma_city", "gamma_age"]
LEVELS = [3, 3, 2, 3]


def oracle_gammas(df, l, r, st):
    """int8 [P, K]: the settings' CASE expressions over the pairs (l[i], r[i]) of `df`, by the SQL oracle."""
    import pandas as pd
    import oracle as orc
    pairs = pd.DataFrame({"row_l": np.asarray(l, dtype=np.int64), "row_r": np.asarray(r, dtype=np.int64)})
    cmp_df = orc.comparison_frame(pairs, df, df)
    g = orc.sql_gammas(cmp_df, [c["case_expression"] for c in st["comparison_columns"]])
    assert (g != -99).all()  # every CASE resolved to a level
    return g


def host_u(g, levels):
    """Per column the list of u per level 0..L-1 from a gamma matrix of non-matches: count_v / Σ_{v >= 0} count_v
    cast to float32, an unobserved level 0 (the reference's M-step with every pair a non-match), and the counts
    per level -1..L-1."""
    us, counts = [], []
    for k, L in enumerate(levels):
        c = np.array([(g[:, k] == v).sum() for v in range(-1, L)], dtype=np.int64)
        den = int(c[1:].sum())
        us.append([float(np.float32(int(c[v + 1]) / den)) if c[v + 1] else 0 for v in range(L)])
        counts.append(c)
    return us, counts
