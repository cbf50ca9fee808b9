"""Blocking rules with residual predicates, host side: rule compilation and the validity of the
reference fixture tests/golden/residual_rules.json (tests/golden/make_golden_residual.py)."""
import pytest

import residual_common as rc
from conftest import load_golden
from splink_amd import _native as N
from splink_amd.compiler import KeyExpr, MAX_RESIDUAL_RULES, Schema, compile_rule, compile_rules

SCHEMA = Schema({"unique_id": "num", "first_name": "str", "surname": "str", "city": "str", "age": "num"})
CASES = ["dedupe_only", "link_only", "link_and_dedupe"]


def test_rules_split_into_key_terms_and_residual():
    specs = [compile_rule(t, SCHEMA) for t in rc.GOLDEN_RULES]
    for spec, col in zip(specs, ["city", "surname", "city", "surname"]):
        plain = compile_rule(f"l.{col} = r.{col}", SCHEMA)
        assert spec.terms == plain.terms == [(KeyExpr(col), KeyExpr(col))]
        assert spec.symmetric and plain.symmetric
    assert [s.residual is not None for s in specs] == [True, True, False, True]
    # an asymmetric key keeps its flag next to a residual; the residual may come first in the text
    spec = compile_rule("l.age < r.age and l.first_name = r.surname", SCHEMA)
    assert not spec.symmetric and spec.residual is not None and len(spec.terms) == 1
    specs, rule_program, hidden = compile_rules(rc.GOLDEN_RULES, SCHEMA)
    assert rule_program == [0, 1, -1, 2]
    assert list(hidden.n_levels) == [2, 2, 2]
    # rules without residuals: no hidden programs at all (the spk_block path)
    assert compile_rules(["l.city = r.city", "l.surname = r.surname"], SCHEMA)[1:] == ([-1, -1], None)


def test_rules_still_rejected():
    for bad in ["l.age < r.age", "l.city = l.city", "abs(l.age - r.age) < 5 and l.city != r.city"]:
        with pytest.raises(ValueError):  # no key term
            compile_rule(bad, SCHEMA)
    with pytest.raises(ValueError, match="like"):
        compile_rules(["l.city = r.city and l.first_name like 'a%'"], SCHEMA)
    with pytest.raises(ValueError, match="initcap"):
        compile_rules(["l.city = r.city and initcap(l.first_name) = r.first_name"], SCHEMA)
    with pytest.raises(ValueError):  # an unqualified column
        compile_rules(["l.city = r.city and age < 5"], SCHEMA)
    with pytest.raises(ValueError):  # a string keyed against a number, next to a residual
        compile_rules(["l.city = r.age and l.age < r.age"], SCHEMA)
    eight = [f"l.city = r.city and abs(l.age - r.age) < {i + 1}" for i in range(MAX_RESIDUAL_RULES)]
    assert compile_rules(eight + ["l.city = r.city"], SCHEMA)[1] == list(range(8)) + [-1]
    with pytest.raises(ValueError, match="at most 8"):
        compile_rules(eight + ["l.surname = r.surname and l.age < r.age"], SCHEMA)


def test_hidden_program_of_rule_1():
    _, rule_program, hidden = compile_rules(rc.GOLDEN_RULES[:1], SCHEMA)
    assert rule_program == [0] and len(hidden.programs) == 1
    p = hidden.programs[0]
    assert (p["n_levels"], p["else_level"], p["n_when"]) == (2, 0, 1)
    w = int(p["first_when"])
    assert hidden.when_level[w] == 1
    instrs = hidden.instrs[hidden.when_first[w]: hidden.when_first[w] + hidden.when_n[w]]
    assert [int(i["op"]) for i in instrs] == [N.OP["STR_CMP"], N.OP["ABSDIFF"], N.OP["AND"]]
    key, absdiff = instrs[0], instrs[1]
    assert int(key["cmp"]) == N.CMP["="]
    ops = hidden.operands
    assert {(ops[key["a"]].name, ops[key["a"]].side), (ops[key["b"]].name, ops[key["b"]].side)} == \
        {("city", 0), ("city", 1)}
    assert int(absdiff["cmp"]) == N.CMP["<"] and float(absdiff["t"]) == 5.0
    assert {(ops[absdiff["a"]].name, ops[absdiff["a"]].side), (ops[absdiff["b"]].name, ops[absdiff["b"]].side)} == \
        {("age", 0), ("age", 1)}
    assert set(hidden.columns) == {("city", "str"), ("age", "num")}


@pytest.mark.parametrize("case", CASES)
def test_fixture_matches_brute_force_and_sees_each_bug(case):
    g = load_golden("residual_rules")[case]
    assert g["settings_in"]["blocking_rules"] == rc.GOLDEN_RULES
    frames = {k: rc.records(g[k]) for k in ("df", "df_l", "df_r") if k in g}
    L, R = rc.sides(case, **frames)
    emitted, stats = rc.brute_force(case, L, R, rc.GOLDEN_RULE_FNS)
    got = sorted((L[i]["_id"] + R[j]["_id"] for _, i, j in emitted), key=repr)
    assert got == rc.golden_pair_ids(g)
    assert len(set(got)) == len(got)
    for r, fn in enumerate(rc.GOLDEN_RULE_FNS):
        if fn[1] is not None:  # every residual rule rejects a key candidate and emits a pair
            assert stats[r]["rejected"] > 0 and stats[r]["emitted"] > 0, (r, stats[r])
    # pairs an implementation excluding on the key alone would lose; candidates whose residual is NULL
    assert sum(s["after_untrue_earlier"] for s in stats) > 0
    assert sum(s["null_residual"] for s in stats) > 0
