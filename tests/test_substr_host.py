"""Every host statement of Spark's substr against tests/substr_common.py's port of UTF8String.substringSQL:
table.spark_substr (host-keyed blocking terms, derived columns), derived.evaluate on substr inside a derived
expression, and the tests' own restatements in tests/exprgen.py and tests/profile_common.py -- which hold for
pos >= 1 and len >= 0 only, and must say so instead of answering.  All strings of 0-5 code points over 1-, 2-, 3-
and 4-byte characters, positions -7 .. 7, lengths -1 (Spark: empty), 0, 1, 2, 3, 6 and the two-argument form."""
import pandas as pd
import pytest

import exprgen as xg
import profile_common as pc
import substr_common as sc
from splink_amd import derived as D
from splink_amd import table as T
from splink_amd.compiler import Schema, compile_comparisons
from splink_amd.sqlexpr import parse

STRINGS = sc.small_strings(5)


def test_port_on_known_values():
    """The port itself on cases worked by hand from UTF8String.substringSQL / substring."""
    f = sc.spark_substring_sql
    assert len(STRINGS) == sum(5 ** k for k in range(6))
    assert f("abcdef", 1, 3) == f("abcdef", 0, 3) == "abc"   # position 0 is position 1
    assert f("abcdef", -3, 2) == "de" and f("abcdef", -2, sc.TWO_ARG) == "ef"
    assert f("abc", -9, 8) == "ab"      # start -6, until 2: the part before the string is lost, the length is not
    assert f("abc", -9, 6) == "" and f("abc", -9, 7) == "a"
    assert f("abc", 4, 1) == "" and f("abc", 3, 200) == "c"
    assert f("abc", 2, 0) == "" and f("abc", 2, -1) == ""
    assert f("a😀é€b", 2, 2) == "😀é" and f("a😀é€b", -2, 1) == "€" and f("a😀é€b", -4, sc.TWO_ARG) == "😀é€b"
    assert f("", 1, 1) == "" and f("", -1, 1) == "" and f("", 0, sc.TWO_ARG) == ""
    assert f("ab", 2, sc.TWO_ARG) == "b"  # start + length saturates at Integer.MAX_VALUE


def test_table_spark_substr_matches_port():
    bad = []
    for s in STRINGS:
        for p in sc.SMALL_POS:
            for n in sc.SMALL_LEN:
                got, want = T.spark_substr(s, p, n), sc.spark_substring_sql(s, p, n)
                if got != want:
                    bad.append((s, p, n, got, want))
    assert not bad, (len(bad), bad[:5])


@pytest.mark.parametrize("inner", ["lower(a)", "a"])
def test_derived_evaluate_matches_port(inner):
    """substr(lower(a), p, n) and substring(lower(a), p) as derived columns (derived.evaluate, per row), NULL rows
    included; the strings of 0-5 code points with an upper-case letter among them."""
    values = [s.replace("b", "B") for s in STRINGS] + [None, "ABCDEFGHIJ", "😀€éBa😀€éBa"]
    df = pd.DataFrame({"a": pd.Series(values, dtype=object)})
    low = (lambda v: v.lower()) if inner.startswith("lower") else (lambda v: v)
    bad = []
    for p in sc.SMALL_POS:
        for n in sc.SMALL_LEN:
            text = f"substring({inner}, {p})" if n == sc.TWO_ARG else f"substr({inner}, {p}, {n})"
            got = D.evaluate(parse(text), df, "str").to_numpy(dtype=object, na_value=None).tolist()
            want = [None if v is None else sc.spark_substring_sql(low(v), p, n) for v in values]
            bad += [(text, v, g, w) for v, g, w in zip(values, got, want) if g != w]
    assert not bad, (len(bad), bad[:5])


def _substr_operand(p, n):
    """The compiled operand of substr(a_l, p, n) (the two-argument form for n = TWO_ARG)."""
    call = f"substring(a_l, {p})" if n == sc.TWO_ARG else f"substr(a_l, {p}, {n})"
    cols = [dict(name="c0", L=2, expr=f"case when {call} = a_r then 1 else 0 end")]
    compiled = compile_comparisons(xg.settings(cols), Schema({"a": "str"}))
    (op,) = [o for o in compiled.operands if o.substr is not None]
    return compiled, op


def test_exprgen_emulation_substr_branch():
    """exprgen._operand's substr: the port's value for pos >= 1 and len >= 0, and an assertion (not a value) outside
    that, where Python slicing is not Spark's substr; the compiled operand sends position 0 to the device as 1."""
    strings = sc.small_strings(3) + ["abcdefgh", "a😀é€b😀a"]
    for p in range(1, 8):
        for n in (0, 1, 2, 3, 6, sc.TWO_ARG):
            compiled, op = _substr_operand(p, n)
            assert op.substr == (p, n)
            for s in strings:
                assert xg._operand(compiled, op, {"a_l": s, "a_r": "x"}) == sc.spark_substring_sql(s, p, n), (s, p, n)
            assert xg._operand(compiled, op, {"a_l": None, "a_r": "x"}) is None
    for p, n in ((0, 2), (-1, 2), (-7, 200), (2, -1), (-3, sc.TWO_ARG)):
        compiled, op = _substr_operand(p, n)
        with pytest.raises(AssertionError):
            xg._operand(compiled, op, {"a_l": "abc", "a_r": "x"})
    for p, sent in ((0, 1), (-3, -3), (5, 5)):
        compiled, _ = _substr_operand(p, 2)
        arr = compiled.native_operands({("a", "str"): 0})
        assert [(int(o["substr_start"]), int(o["substr_len"])) for o in arr if o["substr_start"] != 0] == [(sent, 2)]


def test_profile_common_key_function():
    """profile_common.key_tuples' substr term: the port's value for pos >= 1 and len >= 0, NULL stays NULL, and an
    assertion outside that."""
    values = sc.small_strings(3) + [None, "abcdefgh", "a😀é€b😀a"]
    df = pd.DataFrame({"a": pd.Series(values, dtype=object)})
    for p in range(1, 8):
        for n in (0, 1, 2, 3, 6, 200):
            got = pc.key_tuples(df, [("a", (p, n))])
            want = [None if v is None else (sc.spark_substring_sql(v, p, n),) for v in values]
            assert got == want, (p, n)
    for p, n in ((0, 2), (-1, 2), (-7, 200), (2, -1)):
        with pytest.raises(AssertionError):
            pc.key_tuples(df, [("a", (p, n))])


def test_blocking_records_are_not_vacuous():
    """The records and the grid of tests/test_gpu_substr.py, on the reference alone: some row's start is clamped
    from below zero, some row's start lies at or past its code-point count, and the grid's keys differ."""
    df = sc.make_records()
    a = [v for v in df["a"].tolist() if v is not None]
    assert len(df) == 300 and 20 <= 300 - len(a) <= 45 and "" in a
    assert {len(v) for v in a} >= set(range(9)) and max(len(v) for v in a) == 20
    assert any(len(v) < 9 for v in a) and any(len(v) >= 9 for v in a)          # pos -9: clamped / not clamped
    assert any(0 < len(v) < 3 for v in a) and any(len(v) <= 3 for v in a)        # pos -3 clamped, pos 4 past the end
    keys = {(p, n): tuple(sc.ref_values(df["a"].tolist(), p, n)) for p in sc.GRID_POS for n in sc.GRID_LEN}
    assert len(set(keys.values())) >= 10


def test_ifnull_over_substr_is_refused_cleanly():
    """ifnull(substr(x, ..), 'd') has no operand form (the device would cut the default too): a ValueError that says
    so, for a comparison column and for a residual predicate; the supported order compiles."""
    from splink_amd.compiler import compile_rules
    schema = Schema({"a": "str", "k": "str"})
    bad = "ifnull(substr({0}, -2, 1), 'x') = ifnull(substr({1}, -2, 1), 'x')"
    with pytest.raises(ValueError, match="inside ifnull"):
        compile_comparisons(xg.settings([dict(name="c", L=2, expr=f"case when {bad.format('a_l', 'a_r')} then 1 else 0 end")]),
                            schema)
    with pytest.raises(ValueError, match="inside ifnull"):
        compile_rules([f"l.k = r.k and {bad.format('l.a', 'r.a')}"], schema)
    good = "case when substr(ifnull(a_l, 'wxyz'), -2, 1) = substr(a_r, -2, 1) then 1 else 0 end"
    compiled = compile_comparisons(xg.settings([dict(name="c", L=2, expr=good)]), schema)
    assert {(o.substr, o.lit) for o in compiled.operands} == {((-2, 1), None), ((-2, 1), "wxyz")}
