"""Spark's substr on the device, outside pos >= 1: substr_range (spk_ingest.hip; UTF-8 bytes, hashes the blocking
key) and apply_substr (spk_interp.h; UTF-16 units with a surrogate-pair walk, serves comparison programs and residual
predicates), position 0, negative positions, a start before the string or past it, length 0 and the two-argument
form.  Also the ingest paths next to them: spk_rank_from_raw with ids over the whole int64 range, keys of three and
four terms, keys that are '' or differ only past a hash word, an all-NULL key column, a one-row side.

The expected values never pass through sqlite's substr (which is not Spark's there): tests/substr_common.py's port of
UTF8String.substringSQL computes every substring into a plain column, and oracle.block / oracle.sql_gammas run on
those columns -- so the oracle's link-type and NULL semantics are reused and only the substr is replaced."""
import functools
import random
import warnings

import numpy as np
import pandas as pd
import pytest

import exprgen as xg
import oracle as orc
import substr_common as sc
from test_gpu_exprfuzz import _split
from test_gpu_ingest import _arrow

pytestmark = pytest.mark.gpu
warnings.filterwarnings("ignore")

LINK_TYPES = ["dedupe_only", "link_only", "link_and_dedupe"]
RECORDS = sc.make_records()
# one cell per position, the lengths in turn: every link type and both column kinds run here
DIAGONAL = [(p, sc.GRID_LEN[(i + 1) % len(sc.GRID_LEN)]) for i, p in enumerate(sc.GRID_POS)]


@pytest.fixture(scope="module")
def amd():
    from splink_amd import AmdSession, _native
    if _native.device_count() == 0:
        pytest.fail("no HIP device visible: the -m gpu tests need an MI355X")
    return AmdSession(0)


def _device_pairs(job, col="unique_id"):
    """(col of the l row, col of the r row) of the job's pairs, sorted."""
    l, r = job.pair_rows()
    vl, vr = job.tables[0][col].to_numpy()[l], job.r_table()[col].to_numpy()[r]
    return sorted(zip(vl.tolist(), vr.tolist()))


def _oracle_pairs(link_type, kw, rules, col="unique_id"):
    st = {"link_type": link_type, "blocking_rules": list(rules), "unique_id_column_name": "unique_id"}
    pairs, left, right = orc.block(st, **kw)
    vl, vr = left[col].to_numpy()[pairs["row_l"].to_numpy(dtype=np.int64)], right[col].to_numpy()[pairs["row_r"].to_numpy(dtype=np.int64)]
    return sorted(zip(vl.tolist(), vr.tolist()))


def _blocked(link_type, inputs, rules, col="unique_id"):
    from splink_amd.engine import Job
    job = Job(link_type, inputs, "unique_id", 0)
    job.block(list(rules))
    ids = _device_pairs(job, col)
    assert len(ids) == len(set(ids))
    return ids


def _report(got, want, by_uid, what):
    """Fails with the first missing and the first extra pair and their records."""
    if got == want:
        return
    missing, extra = sorted(set(want) - set(got)), sorted(set(got) - set(want))
    lines = [f"{what}: {len(missing)} pairs missing, {len(extra)} extra"]
    for name, ps in (("missing", missing), ("extra", extra)):
        if ps:
            lines.append(f"  first {name}: l {by_uid[ps[0][0]]}  r {by_uid[ps[0][1]]}")
    pytest.fail("\n".join(lines))


def _non_null_pairs(link_type, kw, col):
    """Candidate pairs of rows whose `col` is not NULL, under the link type's predicate."""
    if link_type == "dedupe_only":
        n = int(kw["df"][col].notna().sum())
        return n * (n - 1) // 2
    nl, nr = int(kw["df_l"][col].notna().sum()), int(kw["df_r"][col].notna().sum())
    return nl * nr + (nl * (nl - 1) // 2 + nr * (nr - 1) // 2 if link_type == "link_and_dedupe" else 0)


# ---------------------------------------------------------------------------------------------------------------------
# a. blocking keys (substr_range)
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _cell(link_type, pos, length):
    """Inputs of the job, and the reference pairs of `substr(l.a, pos, length) = substr(r.a, pos, length)`."""
    full = sc.add_ref_substr(RECORDS, "ka", "a", pos, length)
    inputs, kw = _split(link_type, full)
    return inputs, kw, _oracle_pairs(link_type, kw, ["l.ka = r.ka"])


def _check_cell(link_type, pos, length, arrow):
    inputs, kw, want = _cell(link_type, pos, length)
    every = _non_null_pairs(link_type, kw, "a")
    if length == 0:
        assert len(want) == every  # all keys are ''
    else:
        assert 20 <= len(want) < 0.9 * every, (pos, length, len(want), every)
    call = lambda side: sc.substr_sql(f"{side}.a", pos, length)  # noqa: E731
    got = _blocked(link_type, [_arrow(t) for t in inputs] if arrow else inputs, [f"{call('l')} = {call('r')}"])
    _report(got, want, RECORDS.set_index("unique_id").to_dict("index"), f"{link_type} substr(a, {pos}, {length})")


@pytest.mark.parametrize("length", sc.GRID_LEN, ids=lambda n: "two-arg" if n is None else f"len{n}")
@pytest.mark.parametrize("pos", sc.GRID_POS, ids=lambda p: f"pos{p}")
def test_substr_key_grid_dedupe(amd, pos, length):
    """One job per (pos, len) with the single rule substr(l.a, pos, len) = substr(r.a, pos, len) on 300 records:
    a later rule's exclusion of earlier pairs would hide a wrong key."""
    _check_cell("dedupe_only", pos, length, arrow=False)


def test_substr_key_grid_is_not_vacuous():
    """On the reference alone: the grid yields many different pair sets, the len > 0 cells neither few pairs nor
    nearly all, and rows whose start is clamped from below zero or lies past the end."""
    sets = {(p, n): tuple(_cell("dedupe_only", p, n)[2]) for p in sc.GRID_POS for n in sc.GRID_LEN}
    assert len(set(sets.values())) >= 10
    lens = [len(v) for v in RECORDS["a"].tolist() if v is not None]
    assert any(n < 9 for n in lens) and any(n < 3 for n in lens)  # start = n + pos < 0 for pos -9, -3
    assert any(n <= 8 for n in lens) and any(n <= 3 for n in lens)  # start = pos - 1 >= n for pos 9, 4


@pytest.mark.parametrize("arrow", [False, True], ids=["object", "arrow"])
@pytest.mark.parametrize("cell", DIAGONAL, ids=lambda c: f"pos{c[0]}-len{c[1]}")
@pytest.mark.parametrize("link_type", LINK_TYPES)
def test_substr_key_diagonal_link_types_and_arrow(amd, link_type, cell, arrow):
    _check_cell(link_type, cell[0], cell[1], arrow)


THREE = ("substr(l.a,-2,1) = substr(r.a,-2,1) and substr(l.b,0,1) = substr(r.b,0,1) and l.c = r.c",
         "l.k1 = r.k1 and l.k2 = r.k2 and l.c = r.c")
# name -> (device rules, reference rules over the precomputed columns, {column: (source, pos, len, fn)})
RULE_CASES = {
    "asymmetric": (["substr(l.a, -3, 2) = substr(r.b, 2, 2)"], ["l.k1 = r.k2"],
                   {"k1": ("a", -3, 2, None), "k2": ("b", 2, 2, None)}),
    "one-sided": (["substring(l.a, -2) = r.b"], ["l.k1 = r.b"], {"k1": ("a", -2, None, None)}),
    "three-term": ([THREE[0]], [THREE[1]], {"k1": ("a", -2, 1, None), "k2": ("b", 0, 1, None)}),
    "four-term": ([THREE[0] + " and l.n = r.n"], [THREE[1] + " and l.n = r.n"],
                  {"k1": ("a", -2, 1, None), "k2": ("b", 0, 1, None)}),
    "two-rules": (["substr(l.a, -3, 2) = substr(r.a, -3, 2)", "substr(l.b, 0, 2) = substr(r.b, 0, 2)"],
                  ["l.k1 = r.k1", "l.k2 = r.k2"], {"k1": ("a", -3, 2, None), "k2": ("b", 0, 2, None)}),
    "host-keyed": (["lower(substr(l.a, -3, 3)) = lower(substr(r.a, -3, 3))"], ["l.k1 = r.k1"],
                   {"k1": ("a", -3, 3, str.lower)}),
}


@pytest.mark.parametrize("name", list(RULE_CASES))
@pytest.mark.parametrize("link_type", LINK_TYPES)
def test_substr_rules_match_oracle(amd, link_type, name):
    """Asymmetric and one-sided substr terms, keys of three and four terms (k_pack_ids and the re-densification
    more than once, NULLs in every term's column), two rules (the second excludes the first's pairs) and a
    host-keyed lower(substr(..)) term."""
    rules, ref_rules, cols = RULE_CASES[name]
    full = RECORDS
    for k, (src, pos, length, fn) in cols.items():
        full = sc.add_ref_substr(full, k, src, pos, length, fn)
    inputs, kw = _split(link_type, full)
    want = _oracle_pairs(link_type, kw, ref_rules)
    assert len(want) >= 10, (name, len(want))
    if name in ("three-term", "four-term"):  # every term decides: dropping one changes the pairs, and so does a NULL
        for drop in range(len(ref_rules[0].split(" and "))):
            terms = ref_rules[0].split(" and ")
            fewer = _oracle_pairs(link_type, kw, [" and ".join(terms[:drop] + terms[drop + 1:])])
            assert len(fewer) > len(want), (name, drop)
        assert all(full[c].isna().any() for c in ("k1", "k2", "c", "n"))
    if name == "two-rules":
        first, second = (_oracle_pairs(link_type, kw, [r]) for r in ref_rules)
        assert set(first) & set(second) and len(want) == len(set(first) | set(second))
    if name == "host-keyed":  # lower() joins values that differ in case only
        uncased = _split(link_type, sc.add_ref_substr(RECORDS, "k1", "a", -3, 3))[1]
        assert len(_oracle_pairs(link_type, uncased, ref_rules)) < len(want)
    got = _blocked(link_type, inputs, rules)
    _report(got, want, RECORDS.set_index("unique_id").to_dict("index"), f"{link_type} {name}")


# ---------------------------------------------------------------------------------------------------------------------
# b. comparison programs and residual predicates (apply_substr)
# ---------------------------------------------------------------------------------------------------------------------
def _o(col, pos, length, default=None):
    return lambda side: (col, side, pos, length, default)


# (levels, CASE text over {0} / {1} = the l- and r-side operand, operand) -- position <= 0, a negative position
# beyond most lengths, the two-argument form and length 0, under =, <, levenshtein, jaro_winkler_sim and an ifnull
PROGRAM_COLUMNS = [
    (2, "case when {0} = {1} then 1 else 0 end", _o("a", -3, 2)),
    (2, "case when {0} = {1} then 1 else 0 end", _o("a", 0, 2)),
    (3, "case when {0} < {1} then 1 when {0} = {1} then 2 else 0 end", _o("a", -2, None)),
    (3, "case when {0} is null or {1} is null then -1 when levenshtein({0}, {1}) <= 1 then 2 "
        "when levenshtein({0}, {1}) <= 3 then 1 else 0 end", _o("b", -70, 68)),
    (3, "case when jaro_winkler_sim({0}, {1}) >= 0.88 then 2 when jaro_winkler_sim({0}, {1}) >= 0.7 then 1 else 0 end",
     _o("a", -4, 4)),
    (2, "case when {0} = {1} then 1 else 0 end", _o("a", 3, 0)),
    (2, "case when {0} = {1} then 1 else 0 end", _o("a", -2, 1, "wxyz")),
    (3, "case when levenshtein({0}, {1}) <= 2 then 2 when {0} > {1} then 1 else 0 end", _o("a", -9, 7)),
    (3, "case when levenshtein({0}, {1}) <= 5 then 2 when jaro_winkler_sim({0}, {1}) >= 0.9 then 1 else 0 end",
     _o("b", -1028, None)),
    (2, "case when length({0}) >= 2 and {0} != {1} then 1 else 0 end", _o("b", 0, 64)),
]


def _program_case(df):
    """(settings columns for the device, CASE texts for the oracle, the frame with the precomputed operands)."""
    cols, ref_exprs, ref = [], [], df.copy()
    for i, (levels, text, operand) in enumerate(PROGRAM_COLUMNS):
        names = []
        for side in "lr":
            spec = operand(side)
            name = f"s{i}_{side}"
            ref[name] = pd.Series(sc.operand_values(df, *spec), dtype=object, index=df.index)
            names.append(name)
        cols.append(dict(name=f"c{i}", L=levels, expr=text.format(*(sc.operand_sql(*operand(s)) for s in "lr"))))
        ref_exprs.append(text.format(*names))
    return cols, ref_exprs, ref


def _cells_differ(mode, cols, got, want, df):
    assert got.shape == want.shape, (mode, got.shape, want.shape)
    bad = np.argwhere(got != want)
    if len(bad):
        i, k = bad[0]
        pytest.fail(f"{len(bad)} cells differ; first: " + xg.describe(
            "substr", mode, cols[k]["expr"], df.iloc[i][["a_l", "b_l"]].to_dict(), df.iloc[i][["a_r", "b_r"]].to_dict(),
            got[i, k], want[i, k]))


def test_substr_operands_in_comparison_programs(amd):
    """400 pairs with a surrogate pair before, at and after each cut, BMP-only rows, 0 / 1 / 63 / 64 / 65 units, a
    pair past the slow limit and NULLs: the default mode, the interpreter alone and every Levenshtein kernel."""
    from splink_amd.gammas import add_gammas
    from splink_amd.compiler import Schema, compile_comparisons
    rng = random.Random(8128)
    df = sc.make_pair_frame(rng, 400, xg.huge_pair(rng))
    cols, ref_exprs, ref = _program_case(df)
    want = orc.sql_gammas(ref, ref_exprs)
    assert (want != -99).all()
    for k in range(len(cols)):  # no column is constant: each level of each column occurs
        assert len(set(want[:, k].tolist())) == cols[k]["L"] + (1 if "then -1" in cols[k]["expr"] else 0), (k, cols[k])
    # the order ifnull(substr(x, ..), 'd') has no operand form: a clean refusal, not a wrong value
    with pytest.raises(ValueError, match="inside ifnull"):
        compile_comparisons(xg.settings([dict(name="c", L=2, expr="case when ifnull(substr(a_l, -2, 1), 'x') = a_r "
                                                                  "then 1 else 0 end")]), Schema({"a": "str"}))
    gf = add_gammas(df, xg.settings(cols), amd)
    _cells_differ("default", cols, gf.gamma_matrix(), want, df)
    job, st = gf.job, gf.settings
    try:
        for mode in (1, 0):
            job.ctx.gammas_set_simple(mode)
            job.gammas(st)
            _cells_differ(f"simple={mode}", cols, job.gammas_host(), want, df)
        job.ctx.gammas_set_simple(1)
        for kern in (0, 1, 2, 3):
            job.ctx.gammas_set_lev_kernel(kern)
            job.gammas(st)
            _cells_differ(f"lev_kernel={kern}", cols, job.gammas_host(), want, df)
    finally:
        job.ctx.gammas_set_simple(1)
        job.ctx.gammas_set_lev_kernel(2)


@pytest.mark.parametrize("link_type", LINK_TYPES)
def test_substr_in_residual_predicate(amd, link_type):
    """l.k = r.k and levenshtein(substr(l.a, -4), substr(r.a, -4)) <= 1 on 150 records: oracle.block with the
    predicate over the precomputed last four code points."""
    df = sc.make_records(150, seed=11)
    full = sc.add_ref_substr(df, "s4", "a", -4, None)
    inputs, kw = _split(link_type, full)
    want = _oracle_pairs(link_type, kw, ["l.k = r.k and levenshtein(l.s4, r.s4) <= 1"])
    keyed = _oracle_pairs(link_type, kw, ["l.k = r.k"])
    plain = _oracle_pairs(link_type, kw, ["l.k = r.k and levenshtein(l.a, r.a) <= 1"])
    assert 20 <= len(want) < len(keyed) and set(want) != set(plain)  # the predicate and its substr both decide
    got = _blocked(link_type, inputs, ["l.k = r.k and levenshtein(substr(l.a, -4), substr(r.a, -4)) <= 1"])
    _report(got, want, df.set_index("unique_id").to_dict("index"), f"{link_type} residual")


# ---------------------------------------------------------------------------------------------------------------------
# c. unique-id ranks over the whole int64 range (spk_rank_from_raw / k_i64_keys)
# ---------------------------------------------------------------------------------------------------------------------
I64_MIN, I64_MAX = -2 ** 63, 2 ** 63 - 1


def _rank_tables():
    """Left and right records {unique_id (nullable Int64), rid, k}: INT64_MIN, INT64_MIN + 1, -1, 0, 1, INT64_MAX - 1,
    INT64_MAX and a NULL id on each side among 15 ordinary ids per side, in shuffled row order, two key values."""
    rng = random.Random(5)
    ids_l = [I64_MIN, -1, 1, I64_MAX, None, 7] + list(range(100, 115))
    ids_r = [I64_MIN + 1, 0, I64_MAX - 1, I64_MAX, None, 7] + list(range(107, 122))
    out = []
    for tag, ids in (("l", ids_l), ("r", ids_r)):
        rng.shuffle(ids)
        out.append(pd.DataFrame({"unique_id": pd.array(ids, dtype="Int64"),
                                 "rid": [f"{tag}{i}" for i in range(len(ids))],
                                 "k": pd.Series([f"k{rng.randrange(2)}" for _ in ids], dtype=object)}))
    return out


@pytest.mark.parametrize("link_type", ["dedupe_only", "link_and_dedupe"])
def test_rank_of_extreme_and_null_ids(amd, link_type):
    """The pair set and its orientation (which row is l, which is r) under `l.id < r.id` in signed order, a NULL id
    (it shares the sort key ~0 with INT64_MAX) pairing only across sources."""
    df_l, df_r = _rank_tables()
    if link_type == "dedupe_only":
        both = pd.concat([df_l, df_r], ignore_index=True)
        inputs, kw = [both], dict(df=both)
    else:
        both = pd.concat([df_l.assign(_source_table="left"), df_r.assign(_source_table="right")], ignore_index=True)
        inputs, kw = [both], dict(df_l=df_l, df_r=df_r)
    want = _oracle_pairs(link_type, kw, ["l.k = r.k"], col="rid")
    rec = both.set_index("rid").to_dict("index")
    uid = lambda r: None if sc.is_null(rec[r]["unique_id"]) else int(rec[r]["unique_id"])  # noqa: E731
    assert any(uid(a) is not None and uid(b) is not None and uid(a) < 0 < uid(b) for a, b in want)
    with_null = [(a, b) for a, b in want if uid(a) is None or uid(b) is None]
    with_max = [(a, b) for a, b in want if I64_MAX in (uid(a), uid(b))]
    if link_type == "dedupe_only":
        assert not with_null and with_max
    else:
        assert with_null and all(a[0] == "l" and b[0] == "r" for a, b in with_null)
        assert any(a[0] != b[0] for a, b in with_max) and any(a[0] == b[0] for a, b in with_max)
    got = _blocked(link_type, inputs, ["l.k = r.k"], col="rid")
    _report(got, want, rec, f"{link_type} ranks")


# ---------------------------------------------------------------------------------------------------------------------
# d. plain-key edges
# ---------------------------------------------------------------------------------------------------------------------
def _edge_records(values, n, seed):
    rng = random.Random(seed)
    return pd.DataFrame({"unique_id": range(n), "a": pd.Series([rng.choice(values) for _ in range(n)], dtype=object)})


@pytest.mark.parametrize("arrow", [False, True], ids=["object", "arrow"])
@pytest.mark.parametrize("name,values", [
    ("empty-and-null", ["", None, "x"]),
    # one 8-byte hash word apart from its tail, lengths, and a trailing NUL byte
    ("byte9-length-nul", ["abcdefghi", "abcdefghj", "abcdefgh", "aaaaaaaa", "aaaaaaaaa", "abc", "abc\x00", "abc\x00\x00",
                          "", "\x00", None]),
])
def test_plain_key_edges(amd, name, values, arrow):
    df = _edge_records(values, 120, seed=3)
    want = _oracle_pairs("dedupe_only", dict(df=df), ["l.a = r.a"])
    by_uid = df.set_index("unique_id").to_dict("index")
    assert want and all(by_uid[a]["a"] == by_uid[b]["a"] for a, b in want)  # the oracle keeps all of these apart
    per_value = {v: sum(x == v for x in df["a"].tolist() if x is not None) for v in values if v is not None}
    assert all(c >= 2 for c in per_value.values()) and len(want) == sum(c * (c - 1) // 2 for c in per_value.values())
    got = _blocked("dedupe_only", [_arrow(df) if arrow else df], ["l.a = r.a"])
    _report(got, want, by_uid, name)


@pytest.mark.parametrize("link_type", LINK_TYPES)
def test_all_null_key_column(amd, link_type):
    """No pairs and no error; with a second rule on another column, that rule's pairs alone."""
    df = sc.make_records(60, seed=2).assign(a=pd.Series([None] * 60, dtype=object))
    inputs, kw = _split(link_type, df)
    assert _blocked(link_type, inputs, ["l.a = r.a"]) == []
    assert _blocked(link_type, inputs, ["substr(l.a, -2, 1) = substr(r.a, -2, 1)"]) == []
    want = _oracle_pairs(link_type, kw, ["l.a = r.a", "l.k = r.k"])
    assert len(want) >= 20
    assert _blocked(link_type, inputs, ["l.a = r.a", "l.k = r.k"]) == want


def test_one_row_right_table(amd):
    df = sc.make_records(80, seed=4)
    df_l = df.iloc[:79].reset_index(drop=True)
    for rules in (["l.k = r.k"], ["substr(l.a, -2, 1) = substr(r.a, -2, 1)"]):
        hits = []
        for i in (79, 0):  # a right row of its own, and a copy of a left row
            df_r = df.iloc[i:i + 1].reset_index(drop=True).assign(unique_id=1000)
            full_l, full_r = (sc.add_ref_substr(t, "ka", "a", -2, 1) for t in (df_l, df_r))
            want = _oracle_pairs("link_only", dict(df_l=full_l, df_r=full_r),
                                 ["l.k = r.k" if "substr" not in rules[0] else "l.ka = r.ka"])
            assert _blocked("link_only", [df_l, df_r], rules) == want
            hits.append(len(want))
        assert max(hits) >= 1
