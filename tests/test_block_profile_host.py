"""Host-side checks of the blocking-rule profile: the reference's largest-blocks fixture and the restatement the GPU
tests rely on, BlockingProfile's NA rules, the struct layouts, and the loud failure without a device."""
import re

import numpy as np
import pandas as pd
import pytest

import profile_common as pc
from conftest import ROOT, load_golden
from parity_common import frame

from splink_amd import _native as N
from splink_amd.comparison_evaluation import BlockingProfile, key_column_name

RULE_KEYS = {
    "l.surname = r.surname": ["surname"],
    "l.city = r.city and l.dob = r.dob": ["city", "dob"],
    "l.first_name = r.first_name AND l.surname = r.surname": ["first_name", "surname"],
}


@pytest.fixture(scope="module")
def fixture():
    return load_golden("largest_blocks")


def test_fixture_is_well_formed(fixture):
    table = frame(fixture["table"])
    assert list(table.columns) == ["unique_id", "first_name", "surname", "dob", "city"] and len(table) == 600
    assert (table["dob"].dropna().str.len() == 4).all()  # cut to the year (typos included)
    assert all(table[c].isna().any() for c in ("first_name", "surname", "dob", "city"))  # NULL keys to leave out
    cases = fixture["cases"]
    assert sorted((c["rule"], c["limit"]) for c in cases) == sorted((r, k) for r in RULE_KEYS for k in (5, 8))
    for c in cases:
        rows = c["rows"]
        assert list(rows) == RULE_KEYS[c["rule"]] + ["count"]
        counts = rows["count"]
        assert len(counts) == c["limit"] and counts == sorted(counts, reverse=True) and min(counts) >= 1
    by = {(c["rule"], c["limit"]): c["rows"]["count"] for c in cases}
    assert by[("l.surname = r.surname", 8)] == [38, 35, 32, 31, 30, 26, 23, 21]
    # the other two rules tie across the limit, which is why the parity tests compare multisets
    assert by[("l.city = r.city and l.dob = r.dob", 5)][-1] == by[("l.city = r.city and l.dob = r.dob", 8)][5]


def test_restatement_reproduces_the_fixture(fixture):
    table = frame(fixture["table"])
    for c in fixture["cases"]:
        cols = RULE_KEYS[c["rule"]]
        want = pc.figures(pc.key_tuples(table, [(col, None) for col in cols]))
        rows = c["rows"]
        assert rows["count"] == pc.top_k(want["per_block"], c["limit"], "rows_l")
        for i, n in enumerate(rows["count"]):
            key = tuple(rows[col][i] for col in cols)
            assert all(v is not None for v in key) and want["per_block"][key][0] == n


def test_restatement_figures_by_hand():
    keys = [("a",)] * 4 + [("b",)] + [None] * 2 + [("c",)] * 2
    f = pc.figures(keys)
    assert (f["rows_l"], f["rows_r"], f["blocks"], f["candidates"], f["largest_candidates"]) == (7, 7, 3, 7, 6)
    assert f["hist"][0] == [1, 0] and f["hist"][1] == [1, 1] and f["hist"][3] == [1, 6]
    g = pc.figures(keys, [("a",)] * 3 + [("d",)] + [None])
    assert (g["rows_l"], g["rows_r"], g["blocks"], g["candidates"], g["largest_candidates"]) == (7, 4, 3, 12, 12)
    assert g["hist"][0] == [2, 0] and g["hist"][4] == [1, 12]
    assert pc.top_k(g["per_block"], 2, "rows_l") == [4, 2] and pc.top_k(g["per_block"], 5, "candidates") == [12, 0, 0]
    df = pd.DataFrame({"s": ["abcd", "abxx", None, "a"]})
    assert pc.key_tuples(df, [("s", (1, 2))]) == [("ab",), ("ab",), None, ("a",)]


def _rules(enumerated):
    a = np.zeros(len(enumerated), dtype=N.RULE_PROFILE_DTYPE)
    a["rows_l"] = a["rows_r"] = 10
    a["blocks"] = 2
    a["candidates"] = [20 + i for i in range(len(enumerated))]
    a["largest_candidates"] = 15
    a["enumerated"] = enumerated
    return a


def _profile(enumerated, residual):
    n = len(enumerated)
    empty = np.zeros(0, dtype=N.BLOCK_ENTRY_DTYPE)
    return BlockingProfile([f"rule {i}" for i in range(n)], residual, _rules(enumerated),
                           np.zeros((n, N.PROFILE_BINS, 2), dtype=np.int64), [empty] * n, [pd.DataFrame()] * n)


def test_pairs_and_cumulative_pairs_na_rules():
    p = _profile([7, 5, 3], [False, False, False]).rules
    assert list(p.columns) == ["rule", "rows_l", "rows_r", "blocks", "candidates", "largest_candidates", "enumerated",
                               "pairs", "cumulative_pairs"]
    assert str(p["enumerated"].dtype) == str(p["pairs"].dtype) == str(p["cumulative_pairs"].dtype) == "Int64"
    assert p["pairs"].tolist() == [7, 5, 3] and p["cumulative_pairs"].tolist() == [7, 12, 15]
    # a residual decides the rule's own pairs and what it excludes from every later rule
    p = _profile([7, 5, 3], [False, True, False]).rules
    assert p["enumerated"].tolist() == [7, 5, 3]
    assert p["pairs"].tolist()[0] == 7 and p["pairs"].isna().tolist() == [False, True, True]
    assert p["cumulative_pairs"].isna().tolist() == [False, True, True]
    # a rule that was not enumerated (-1) has no pair count; later key-only rules keep theirs, the running sum does not
    p = _profile([7, -1, 3], [False, False, False]).rules
    assert p["enumerated"].isna().tolist() == [False, True, False]
    assert p["pairs"].isna().tolist() == [False, True, False] and p["pairs"].tolist()[2] == 3
    assert p["cumulative_pairs"].isna().tolist() == [False, True, True]
    assert p["candidates"].tolist() == [20, 21, 22]


def test_histogram_and_largest_blocks_frames():
    hist = np.zeros((1, N.PROFILE_BINS, 2), dtype=np.int64)
    hist[0, 0] = [3, 0]
    hist[0, 4] = [2, 25]
    top = np.zeros(2, dtype=N.BLOCK_ENTRY_DTYPE)
    top["rows_l"], top["rows_r"], top["candidates"] = [6, 5], [6, 5], [15, 10]
    p = BlockingProfile(["l.a = r.a"], [False], _rules([25]), hist, [top], [pd.DataFrame({"a": ["x", "y"]})])
    assert p.histogram(0).to_dict("list") == {"bin": [0, 4], "blocks": [3, 2], "candidates": [0, 25]}
    assert p.largest_blocks(0).to_dict("list") == {"a": ["x", "y"], "rows_l": [6, 5], "rows_r": [6, 5],
                                                   "candidates": [15, 10]}


def test_struct_layouts_and_constants():
    assert N.RULE_PROFILE_DTYPE.itemsize == 48 and N.BLOCK_ENTRY_DTYPE.itemsize == 32
    assert N.BLOCK_ENTRY_DTYPE.fields["row_l"][1] == 24
    with open(f"{ROOT}/include/splink_hip.h") as f:
        text = f.read()
    for name, value in (("SPK_PROFILE_BINS", N.PROFILE_BINS), ("SPK_LARGEST_BY_CANDIDATES", N.LARGEST_BY_CANDIDATES),
                        ("SPK_LARGEST_BY_ROWS_L", N.LARGEST_BY_ROWS_L)):
        assert re.search(r"#define\s+" + name + r"\s+" + str(value) + r"\b", text), name
    assert {"spk_block_profile", "spk_block_profile_info"} <= set(N.EXPORTS)


def test_key_column_names():
    from splink_amd.compiler import Schema, compile_rule
    spec = compile_rule("substr(l.surname, 1, 2) = substr(r.surname, 1, 2) and l.City = r.city and l.age < r.age",
                        Schema({"surname": "str", "city": "str", "age": "num"}))
    assert [key_column_name(l) for l, _ in spec.terms] == ["substr(surname, 1, 2)", "city"]
    assert spec.residual is not None


def test_api_is_exported():
    import splink_amd
    assert callable(splink_amd.get_largest_blocks) and callable(splink_amd.profile_blocking_rules)
    assert callable(splink_amd.Splink.profile_blocking_rules)
    d = splink_amd.DEFAULT_MAX_ENUMERATE
    assert d > 0 and d & (d - 1) == 0  # a power of two


def test_a_rule_without_an_equality_is_refused():
    from splink_amd import get_largest_blocks
    with pytest.raises(ValueError):
        get_largest_blocks("l.a < r.a", pd.DataFrame({"a": ["x", "y"]}), None)


def test_no_device_means_native_unavailable():
    if N.device_count() > 0:
        return
    from splink_amd import get_largest_blocks, profile_blocking_rules
    df = pd.DataFrame({"unique_id": [0, 1], "a": ["x", "y"]})
    with pytest.raises(N.NativeUnavailable):
        get_largest_blocks("l.a = r.a", df, None)
    settings = {"link_type": "dedupe_only", "blocking_rules": ["l.a = r.a"],
                "comparison_columns": [{"col_name": "a", "num_levels": 2}]}
    with pytest.raises(N.NativeUnavailable):
        profile_blocking_rules(settings, "supress_warnings", df=df)
