"""The Jaro-Winkler ladders of tests/jw_ladder_common.py, checked without a device: they pin every pair of every
family, a one-ulp error of any value would change a level, the compiler hands the thresholds to the device bit for
bit, and the families reach the lengths, orders and kernels they are built for.

The reference is orc.jaro_winkler; tests/test_oracle_golden.py::test_string_values ties it bit for bit to the jar's
values in tests/golden/string_values.json, so that anchor is not repeated here."""
import copy
import math
import struct
import warnings

import numpy as np
import pytest

import jw_ladder_common as J

FORMS = (J.LADDER, J.MIXED_EQ)


def _bits(x):
    return struct.pack("<d", float(x))


@pytest.mark.parametrize("name", J.FAMILIES)
def test_every_pair_is_pinned_once(name):
    """Each non-NULL pair's own value is a rung of exactly one column of one call, in the narrow layout and again in
    the wide one; no pair is left out; 0.0 and 1.0 (the filter's TF_ZERO / TF_ONE decisions) are rungs too; no call
    is larger than the pattern space allows and a family stays within about 40 calls."""
    pairs, refs = J.family(name)
    assert any(v == 0.0 for v in refs) and any(v == 1.0 for v in refs)
    for form in FORMS:
        for n_cols in (J.NARROW_COLS, J.WIDE_COLS):
            calls = J.ladder_calls(refs, n_cols, form)
            pins = J.pinned(refs, calls)
            for (a, b), v, pin in zip(pairs, refs, pins):
                if a is None or b is None:
                    assert v is None and pin is None
                    continue
                assert pin is not None and len(pin) == 1, (a, b, v, pin)
                c, k, level = pin[0]
                assert calls[c]["rungs"][k][(5 - level) // 2] == v
                assert J.level_of(v, calls[c]["rungs"][k], form, equal=a == b) == (6 if form == J.MIXED_EQ and a == b
                                                                                     else level)
            for call in calls:
                assert len(call["rungs"]) == n_cols and 8 ** n_cols < 2 ** 31
                assert (8 ** n_cols <= J.CODE16_PATTERNS) == (n_cols == J.NARROW_COLS)
                for col in call["settings"]["comparison_columns"]:
                    assert col["case_expression"].count(" when ") == 1 + J.MAX_TESTS and col["num_levels"] == J.LEVELS
    assert len(J.family_calls(name)) <= 40


@pytest.mark.parametrize("name", J.FAMILIES)
def test_one_ulp_changes_the_pinning_level(name):
    """Replace a pair's reference value by its neighbours: the level of its pinning column changes both times, so the
    device's value cannot be one ulp off without a code differing."""
    pairs, refs = J.family(name)
    calls = J.family_calls(name)
    for (a, b), v, pin in zip(pairs, refs, J.pinned(refs, calls)):
        if v is None:
            continue
        assert len(pin) == 2  # the narrow and the wide layout
        for c, k, level in pin:
            rung = calls[c]["rungs"][k]
            assert J.level_of(v, rung) == level
            # (level + 1 and level - 1, except where the neighbour is itself the next rung of the column)
            assert J.level_of(math.nextafter(v, math.inf), rung) > level, (a, b, v)
            assert J.level_of(math.nextafter(v, -math.inf), rung) < level, (a, b, v)


def test_thresholds_survive_the_compiler():
    """compile_comparisons (no device) keeps every rung bit for bit as its test's threshold, `>` and `>=` as written,
    the levels and the test order, after complete_settings_dict as the device path applies it -- both column forms,
    over every call of every family (values down to the smallest, written with repr)."""
    from splink_amd import _native as N
    from splink_amd.compiler import Schema, compile_comparisons
    from splink_amd.settings import complete_settings_dict
    schema = Schema({"a": "str"})
    n_checked = 0
    for name in J.FAMILIES:
        for form in FORMS:
            for call in J.family_calls(name, form):
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")  # "no blocking rules": the ladders compare a pair table
                    st = complete_settings_dict(copy.deepcopy(call["settings"]), "supress_warnings")
                prog = compile_comparisons(st, schema)
                assert len(prog.programs) == len(call["rungs"])
                for p, rung in zip(prog.programs, call["rungs"]):
                    tests = J.rung_tests(rung, form)
                    skip = 1 if form == J.LADDER else 2  # the NULL guard (and `a_l = a_r`)
                    assert p["n_when"] == skip + len(tests) and p["else_level"] == 0 and p["n_levels"] == J.LEVELS
                    assert prog.when_level[p["first_when"]] == -1
                    for i, (cmp, t, level) in enumerate(tests):
                        w = p["first_when"] + skip + i
                        assert prog.when_n[w] == 1 and prog.when_level[w] == level
                        ins = prog.instrs[prog.when_first[w]]
                        assert ins["op"] == N.OP["JW"] and ins["cmp"] == N.CMP[cmp]
                        assert _bits(ins["t"]) == _bits(t), (t, float(ins["t"]))
                        n_checked += 1
    assert n_checked > 1000


def test_families_cover_the_edges():
    """The lengths on both sides of every length at which the device code changes (window range 0 / 1 at 3 / 4,
    w = 0.1 / 1/lmx at 10 / 11, one / two 32-unit halves at 32 / 33, exact / slow pass at 64 / 65, slow / huge pass at
    1024 / 1025), all three length orders, transpositions / 2 >= 2, rungs one ulp apart, and every kernel of
    jw_exact's dispatch in the family built for it."""
    longer, orders, kernels = set(), set(), {}
    max_t, values = 0, []
    for name in J.FAMILIES:
        pairs, refs = J.family(name)
        values += [v for v in refs if v is not None]
        kernels[name] = {}
        for (a, b), v in zip(pairs, refs):
            kern = J.kernel_of(a, b)
            kernels[name][kern] = kernels[name].get(kern, 0) + 1
            if a is None or b is None:
                continue
            la, lb = J.ulen(a), J.ulen(b)
            longer.add(max(la, lb))
            if a != b:
                orders.add((la > lb) - (la < lb))
            if max(la, lb) <= 300:
                m, t, prefix = J.jaro_parts(a, b)
                max_t = max(max_t, t)
                assert J.jaro_winkler_py(a, b) == v, (a, b)  # the plain-Python restatement agrees with the oracle
    assert {3, 4, 10, 11, 32, 33, 64, 65, 1024, 1025} <= longer
    assert orders == {-1, 0, 1}
    assert max_t >= 2
    assert J.ulp_neighbours(values)
    assert kernels["planes32"].get("planes2_u32", 0) >= 150
    assert set(kernels["planes32"]) <= {"planes2_u32", "equal", "null"}
    assert kernels["planes64"].get("planes2_u64", 0) >= 40 and set(kernels["planes64"]) <= {"planes2_u64", "equal"}
    for kern in ("planes_u32", "planes_u64", "small_global"):
        assert kernels["mixed"].get(kern, 0) >= 5, kernels["mixed"]
    assert kernels["slow"].get("slow", 0) >= 20 and kernels["huge"].get("huge", 0) >= 6
    # planes64: the shorter row on both sides of 32 units, with more than 32 matches where it is longer
    pairs, _ = J.family("planes64")
    short = [min(J.ulen(a), J.ulen(b)) for a, b in pairs]
    assert min(short) <= 32 and max(short) >= 33
    assert max(J.jaro_parts(a, b)[0] for a, b in pairs) > 32
    # mixed: the wide units meet the letters they share a low byte with
    pairs, _ = J.family("mixed")
    assert all(ord(w) & 0xFF == ord(c) and ord(w) >= 256 for c, w in J.WIDE.items())
    assert any(w in a + b for w in J.WIDE.values() for a, b in pairs if a and b)
    assert any(J.SURROGATE in (a or "") + (b or "") for a, b in pairs)


@pytest.mark.parametrize("name", J.FAMILIES)
def test_families_tell_operation_orders_apart(name):
    """jw_finish must evaluate the jar's expression in the jar's operation order.  Another order of the same sum or
    of the Winkler term changes the last bit of only a few values in a hundred, so every family holds pairs whose
    value differs under each of J.REORDERINGS (those past 64 units are built with known matches, transpositions and
    prefix, checked here against the oracle's value)."""
    pairs, refs = J.family(name)
    told = [0] * len(J.REORDERINGS)
    for (a, b), v in zip(pairs, refs):
        if v is None:
            continue
        if (a, b) in J.KNOWN_PARTS:
            parts = J.KNOWN_PARTS[(a, b)]
        elif max(J.ulen(a), J.ulen(b)) <= 64:
            parts = J.jaro_parts(a, b)
        else:
            continue
        variants = J.finish_variants(*parts, J.ulen(a), J.ulen(b))
        assert variants[0] == v, (a, b, parts)
        for r in range(len(J.REORDERINGS)):
            told[r] += variants[1 + r] != v
    assert all(told), dict(zip(J.REORDERINGS, told))


def test_level_of_matches_a_case_evaluation():
    """level_of against a literal reading of the CASE text: first WHEN that holds, ELSE 0."""
    rung = (0.9733333333333334, 0.9733333333333333, 0.5)
    expr = J.ladder_expression(rung)
    for t in rung:
        assert repr(t) in expr and float(repr(t)) == t
    want = {1.0: 6, rung[0]: 5, rung[1]: 3, 0.6: 2, 0.5: 1, 0.0: 0}
    for v, level in want.items():
        assert J.level_of(v, rung) == level
        assert J.level_of(v, rung, J.MIXED_EQ) == min(level, 5)
    assert J.level_of(None, rung) == -1 and J.level_of(0.1, rung, J.MIXED_EQ, equal=True) == 6
    got = J.expected_levels([("a", "b"), (None, "b"), ("a", "a")], [0.5, None, 1.0],
                            J.ladder_settings([0.5, 1.0, 0.0], 2, J.MIXED_EQ))
    assert got.tolist() == [[0, 3], [-1, -1], [6, 6]] and got.dtype == np.int8
