"""jaccard_sim, cosine_distance and the q-gram tokenisers on the host: the restatement's anchor values, the programs
the compiler emits for them in a case expression and in a blocking rule's residual, and the tokeniser of
derived.py against the restatement."""
import numpy as np
import pandas as pd
import pytest

import setsim_common as S
from splink_amd import _native as N
from splink_amd import derived as D
from splink_amd.compiler import Schema, compile_comparisons, compile_rules

SCHEMA = Schema({"unique_id": "num", "a": "str", "city": "str", "surname": "str"})
COSINE_QGRAMS = "cosine_distance(QgramTokeniser(a_l), Q3gramTokeniser(a_r))"


def test_restatement_reproduces_the_anchor_values():
    for a, b, v in S.JACCARD_ANCHORS:
        assert S.jaccard_sim(a, b) == v, (a, b, S.jaccard_sim(a, b))
    assert S.jaccard_sim("", "") == 0.0
    for a, b, v in S.COSINE_ANCHORS:
        assert S.cosine_distance(a, b) == v, (a, b, S.cosine_distance(a, b))
    for a, v in S.COSINE_SELF:
        assert S.cosine_distance(a, a) == v, (a, S.cosine_distance(a, a))
    assert S.cosine_distance("!!!", "abc") == 1.0
    for blank in ("", " ", "\t\n", "\u3000", "\u1680\u2000\u2006\u2008\u200a\u2028\u2029\u205f\x1c\x1f"):
        assert S.cosine_distance(blank, "abc") is None and S.cosine_distance("abc", blank) is None
    for not_blank in ("\u00a0", "\u2007", "\u202f", "\x0e", "\x1b", "\u200b"):
        assert S.cosine_distance(not_blank, "abc") == 1.0
    for s, q, want in S.QGRAM_EXAMPLES:
        assert S.qgram(s, q) == want


def _settings(exprs):
    return {"comparison_columns": [{"custom_name": f"c{i}", "num_levels": 3, "case_expression": e}
                                   for i, e in enumerate(exprs)]}


def _instrs(prog):
    return [(int(i["op"]), prog.operands[int(i["a"])], prog.operands[int(i["b"])], int(i["cmp"]), float(i["t"]))
            for i in prog.instrs if int(i["op"]) in (N.OP["JACCARD"], N.OP["COSINE"])]


def test_case_expression_compiles_to_the_new_opcodes():
    assert (N.OP["JACCARD"], N.OP["COSINE"]) == (12, 13)
    prog = compile_comparisons(_settings([
        "case when jaccard_sim(a_l, a_r) >= 0.43 then 2 when jaccard_sim(a_l, a_r) > 0.13 then 1 else 0 end",
        f"case when {COSINE_QGRAMS} < 0.3 then 2 when 0.5000000000000001 >= {COSINE_QGRAMS} then 1 else 0 end",
        "case when cosine_distance(substr(a_l, 2, 5), ifnull(a_r, 'x y')) = 0.5 then 2 "
        "when jaccard_sim(lower(a_l), 'smith') <= 0.5 then 1 else 0 end",
    ]), SCHEMA)
    ins = _instrs(prog)
    assert [(op, cmp, t) for op, _, _, cmp, t in ins] == [
        (12, N.CMP[">="], 0.43), (12, N.CMP[">"], 0.13), (13, N.CMP["<"], 0.3),
        (13, N.CMP["<="], 0.5000000000000001),  # the literal on the left: the comparison flipped
        (13, N.CMP["="], 0.5), (12, N.CMP["<="], 0.5)]
    a, b = ins[0][1], ins[0][2]
    assert (a.kind, a.side, a.name, a.form) == ("col", 0, "a", "str") and (b.kind, b.side, b.name) == ("col", 1, "a")
    assert ins[1][1] == a and ins[1][2] == b  # one operand pair: the device computes the value once per column
    a, b = ins[2][1], ins[2][2]
    assert (a.side, a.name, a.form) == (0, "qgramtokeniser(a)", "str")
    assert (b.side, b.name, b.form) == (1, "q3gramtokeniser(a)", "str")
    assert ins[3][1] == a and ins[3][2] == b
    a, b = ins[4][1], ins[4][2]
    assert (a.name, a.substr) == ("a", (2, 5)) and (b.name, b.lit) == ("a", "x y")
    a, b = ins[5][1], ins[5][2]
    assert a.name == "lower(a)" and (b.kind, b.lit) == ("str", "smith")
    assert set(prog.derived) == {"qgramtokeniser(a)", "q3gramtokeniser(a)", "lower(a)"}
    assert {("qgramtokeniser(a)", "str"), ("q3gramtokeniser(a)", "str"), ("a", "str")} <= set(prog.columns)


def test_blocking_rule_residual_compiles_to_the_new_opcodes():
    rules = ["l.city = r.city and jaccard_sim(l.surname, r.surname) >= 0.5",
             "l.city = r.city and cosine_distance(QgramTokeniser(l.a), Q3gramTokeniser(r.a)) < 0.3",
             "l.surname = r.surname"]
    specs, rule_program, hidden = compile_rules(rules, SCHEMA)
    assert rule_program == [0, 1, -1] and hidden.gamma_names == ["rule_0", "rule_1"]
    assert [s.residual is not None for s in specs] == [True, True, False]
    ins = _instrs(hidden)
    assert [(op, cmp, t) for op, _, _, cmp, t in ins] == [(12, N.CMP[">="], 0.5), (13, N.CMP["<"], 0.3)]
    assert [(o.side, o.name) for o in ins[0][1:3]] == [(0, "surname"), (1, "surname")]
    assert [(o.side, o.name) for o in ins[1][1:3]] == [(0, "qgramtokeniser(a)"), (1, "q3gramtokeniser(a)")]
    assert set(hidden.derived) == {"qgramtokeniser(a)", "q3gramtokeniser(a)"}
    # each hidden program is the whole rule: key equality AND the value test
    ops = [int(i["op"]) for i in hidden.instrs]
    assert ops == [N.OP["STR_CMP"], 12, N.OP["AND"], N.OP["STR_CMP"], 13, N.OP["AND"]]


@pytest.mark.parametrize("fn", sorted(S.Q_OF))
def test_tokeniser_agrees_with_the_restatement(fn):
    q = S.Q_OF[fn]
    base = "abcdefghij"
    values = ["", "a", base[:q - 1], base[:q], base[:q + 1], base, "two words", None,
              # a surrogate pair at a window edge: the first and the last window split one
              S.SURROGATE + base[:q], base[:q] + S.SURROGATE, base[:q - 1] + S.SURROGATE + "z", S.SURROGATE]
    prog = compile_comparisons(_settings(
        [f"case when jaccard_sim({fn}(a_l), {fn}(a_r)) > 0.5 then 1 else 0 end"]), SCHEMA)
    name = f"{fn.lower()}(a)"
    assert list(prog.derived) == [name]
    got = D.evaluate(prog.derived[name], pd.DataFrame({"a": pd.Series(values, dtype=object)}), "str")
    got = [None if pd.isna(x) else x for x in got.tolist()]
    want = [S.qgram(v, q) for v in values]
    assert got == want
    assert want[0] == "" and want[7] is None and want[1] == "a" and " " not in want[3] and want[4].count(" ") == 1
    assert "?" in want[8] and "?" in want[9] and S.SURROGATE in want[8]  # split at the edge, whole inside a window
    for v in values:
        if v is not None:
            assert D.qgram_tokenise(v, q) == S.qgram(v, q)


def test_tokenisers_nest_with_the_string_functions():
    prog = compile_comparisons(_settings([
        "case when cosine_distance(QgramTokeniser(lower(trim(a_l))), Q4gramTokeniser(substr(ifnull(a_r, 'none'), 1, 6)))"
        " < 0.5 then 1 else 0 end"]), SCHEMA)
    names = sorted(prog.derived)
    assert names == ["q4gramtokeniser(substr(ifnull(a, 'none'), 1, 6))", "qgramtokeniser(lower(trim(a)))"]
    df = pd.DataFrame({"a": pd.Series(["  JoHn ", None, "Smithson"], dtype=object)})
    assert D.evaluate(prog.derived[names[1]], df, "str").tolist()[0] == "jo oh hn"
    got = D.evaluate(prog.derived[names[0]], df, "str").tolist()
    assert got[1:] == ["none", "Smit mith iths"]


@pytest.mark.parametrize("expr", [
    "case when Dmetaphone(a_l) = Dmetaphone(a_r) then 1 else 0 end",
    "case when jaccard_sim(a_l, a_r) > jaccard_sim(a_r, a_l) then 1 else 0 end",
    "case when cosine_distance(a_l, a_r) < a_l then 1 else 0 end",
    "case when jaccard_sim(a_l, a_r) >= '0.5' then 1 else 0 end",
    "case when jaccard_sim(a_l) >= 0.5 then 1 else 0 end",
    "case when Q5ramTokeniser(a_l) = Q5ramTokeniser(a_r) then 1 else 0 end",
])
def test_unsupported_forms_still_raise(expr):
    with pytest.raises(ValueError):
        compile_comparisons(_settings([expr]), SCHEMA)


def test_native_functions_list_the_new_names():
    from splink_amd.session import NATIVE_FUNCTIONS
    assert {"jaccard_sim", "cosine_distance", "jaro_winkler_sim"} <= set(NATIVE_FUNCTIONS)
    assert {"spk_jaccard_sim", "spk_cosine_distance"} <= set(N.EXPORTS)
    assert np.dtype(N.INSTR_DTYPE).itemsize == 32
