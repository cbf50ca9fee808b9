"""tests/exprgen.py on the host: for generated comparison columns and residual rules the compiler accepts
every expression, sqlite (oracle.connect) resolves every cell, and the plain-Python emulation of the compiled
RPN programs gives sqlite's level on every cell.  This is what lets tests/test_gpu_exprfuzz.py take sqlite
for the truth: a mismatch there is then in a kernel or in the host-side classification, not in the compiler
or the oracle.  The coverage counts keep the generator honest after a grammar change."""
import random
from collections import Counter

import numpy as np
import pytest

import exprgen as xg
import oracle as orc
from splink_amd.compiler import MAX_RESIDUAL_RULES, Schema, compile_comparisons, compile_rules

SCHEMA = Schema({"unique_id": "num", "a": "str", "b": "str", "x": "num", "y": "num", "k": "str"})
N_PAIRS = 320
PER_FAMILY = 200
VALUE_OPS = ["STR_CMP", "NUM_CMP", "JW", "LEV", "LEVRATIO", "ABSDIFF", "PERCDIFF", "LEN"]


@pytest.fixture(scope="module")
def frame():
    df = xg.make_pair_frame(random.Random(20261), N_PAIRS)
    assert all(df[c].dtype == np.float64 for c in ("x_l", "x_r", "y_l", "y_r"))
    return df, df.to_dict("records")


def _columns():
    rng = random.Random(4242)
    cols = [xg.column_g(rng, exact16=i % 10 == 0) for i in range(2 * PER_FAMILY)]
    cols += [xg.column_s(rng, cls=["jw", "lev", "eq", "num"][i % 4]) for i in range(PER_FAMILY)]
    cols += [xg.column_n(rng, kind=xg.N_KINDS[i % len(xg.N_KINDS)]) for i in range(PER_FAMILY)]
    for i, c in enumerate(cols):
        c["name"] = f"c{i}"
    return cols


def test_generated_columns_compile_resolve_and_emulate(frame):
    df, rows = frame
    cols = _columns()
    assert len(cols) >= 600 and all(sum(c["family"] == f for c in cols) >= 150 for f in "GSN")
    assert all(c["expr"] == c["expr"].lower() for c in cols)
    decided, levels, sizes = Counter(), Counter(), Counter()
    rejected, unresolved, mismatches = [], 0, []
    for lo in range(0, len(cols), 10):
        part = cols[lo:lo + 10]
        try:
            compiled = compile_comparisons(xg.settings(part), SCHEMA)
        except ValueError as e:
            rejected.append((lo, str(e)))
            continue
        for c, w in zip(part, range(len(part))):
            p = compiled.programs[w]
            got_sizes = compiled.when_n[p["first_when"]:p["first_when"] + p["n_when"]].tolist()
            assert got_sizes == c["sizes"], (c["expr"], got_sizes, c["sizes"])  # the generator's instruction count
            sizes.update(got_sizes)
        want = orc.sql_gammas(df, [c["expr"] for c in part])
        unresolved += int((want == -99).sum())
        for i, row in enumerate(rows):
            trace = []
            got = xg.emulate(compiled, row, trace)
            for (k, w, ins), g in zip(trace, got):
                if g != want[i, k]:
                    mismatches.append(xg.describe(4242, "emulator", part[k]["expr"], row, "", g, want[i, k]))
                levels[(g, "else" if w < 0 else "when")] += 1
                if w >= 0 and len(ins) == 1:  # a single-leaf WHEN: that leaf decided the cell
                    op = xg.OPNAME[int(ins[0]["op"])]
                    decided[(op, xg.CMPNAME[int(ins[0]["cmp"])]) if op in VALUE_OPS else (op, "")] += 1
    assert not rejected, rejected[:3]
    assert unresolved == 0
    assert not mismatches, (len(mismatches), mismatches[:3])
    # coverage of the generator: every comparator of every value leaf, the NULL tests and TRUE decided a cell
    # as a single-leaf WHEN; every level came from a WHEN and from an ELSE; WHENs of exactly 16 instructions exist
    missing = [(op, c) for op in VALUE_OPS for c in xg.CMPS if decided[(op, c)] == 0]
    missing += [(op, "") for op in ("ISNULL", "NOTNULL", "CONST") if decided[(op, "")] == 0]
    assert not missing, missing
    assert all(levels[(lv, how)] > 0 for lv in (-1, 0, 1, 2, 3) for how in ("when", "else")), levels
    assert sizes[16] >= 10 and max(sizes) == 16, sizes


def test_fixed_columns_compile_resolve_and_emulate(frame):
    df, rows = frame
    cols = xg.FIXED_COLUMNS
    compiled = compile_comparisons(xg.settings(cols), SCHEMA)
    want = orc.sql_gammas(df, [c["expr"] for c in cols])
    assert (want != -99).all()
    got = np.array([xg.emulate(compiled, row) for row in rows])
    assert (got == want).all(), np.argwhere(got != want)[:5]
    for k, c in enumerate(cols):  # no column is constant on the frame
        assert len(set(want[:, k].tolist())) >= 2, c["expr"]


def test_generated_residual_rules_compile_resolve_and_emulate(frame):
    df, rows = frame
    rng = random.Random(777)
    rules = [xg.residual_rule(rng, exact=i % 12 == 0) for i in range(120)]
    assert sum(n == 16 for _, n in rules) >= 5 and max(n for _, n in rules) == 16
    bad = []
    for lo in range(0, len(rules), MAX_RESIDUAL_RULES):
        part = rules[lo:lo + MAX_RESIDUAL_RULES]
        specs, rule_program, hidden = compile_rules([r for r, _ in part], SCHEMA)
        assert hidden is not None and rule_program == list(range(len(part)))
        assert hidden.when_n.tolist() == [n for _, n in part]
        want = orc.sql_gammas(df, [xg.rule_as_case(r) for r, _ in part])
        assert (want != -99).all()
        for i, row in enumerate(rows):
            got = xg.emulate(hidden, row)
            for k, g in enumerate(got):
                if g != want[i, k]:
                    bad.append(xg.describe(777, "emulator", part[k][0], row, "", g, want[i, k]))
    assert not bad, (len(bad), bad[:3])
