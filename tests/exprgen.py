"""Seeded generator of comparison columns and residual blocking rules over the whole grammar that
splink_amd/compiler.py compiles, with a plain-Python emulation of the compiled programs; shared by
tests/test_exprgen_host.py (generator, compiler, sqlite oracle and emulator agree: CPU) and
tests/test_gpu_exprfuzz.py (the kernels against the sqlite oracle).

Everything is driven by random.Random(seed).  Expressions are emitted in lower case, literals included:
the reference lower-cases a completed case_expression as a whole (case_statements.py:24-43), so a literal
with an upper-case letter would not survive into the SQL that either side runs.

Where sqlite and Spark differ the generator stays on common ground, so that sqlite can stand for Spark:
* no +-Infinity and no NaN as a value (`inf - inf` and NaN ordering differ between Spark, sqlite and IEEE);
* substr(x, p, n) only with p >= 1 and n >= 0 (position 0 and negative arguments differ; those are checked
  against a port of Spark's substringSQL instead: tests/substr_common.py, tests/test_substr_host.py,
  tests/test_gpu_substr.py);
* a string operand is never compared with a numeric one (sqlite's type affinity is not Spark's cast);
* `is null` is applied to columns (possibly wrapped), not to literals;
* lower() / trim() are the oracle's Python restatements on both sides (oracle.connect).

Columns (logical): strings `a` (0-12 units) and `b` (long: 60-70, 120-135 and one pair past 1024 units,
with a BMP code point above U+E000 next to a supplementary-plane one), float64 `x` and `y`, key `k`.
"""
import functools
import math
import re

import numpy as np
import pandas as pd

import oracle as orc
from splink_amd import _native as N
from splink_amd import derived as D

CMPS = ["=", "!=", "<", "<=", ">", ">="]
JW_T = [0, 0.5, 0.7, 0.88, 0.94, 1, -0.1, 1.2]
LEV_T = [0, 1, 2, 3.5, -1, 40]
RATIO_T = [0, 0.2, 0.3, 0.5, 1, 2, -0.1]
ABS_T = [0, 0.5, 1, 2, 3.5, 1e300, -1]
PERC_T = [0, 0.1, 0.5, 1, 2, -1]
LEN_T = [0, 1, 5, 6.5, 12, 64, 130]
NUM_VALUES = [0.0, -0.0, 1.0, 2.0, -2.0, 1.5, 3.5, 1e300, -1e300]
STR_LITS = ["martha", "é", "", "zz", "a", "😀bcd"]
NUM_LITS = ["0", "1", "1.5", "-2", "3.5", "1e300"]

# ---------------------------------------------------------------------------------------------------------
# data
# ---------------------------------------------------------------------------------------------------------
A_BASES = ["martha", "marhta", "jones", "jonas", "dixon", "dicksonx", "dwayne", "duane", "é", "josé", "jose", "a",
           "Š", " anna", "anna ", "ANNA", "anna", "abcdefghijkl", "zz"]
A_ALPHA = list("abcdeéŠšAn ")
B_ALPHA = list("abcdefghij klmnop,.0123é")


def _mutate(rng, s, k, alpha, max_len):
    s = list(s)
    for _ in range(k):
        op = rng.randrange(3)
        i = rng.randrange(len(s) + 1)
        if (op == 0 or not s) and len(s) < max_len:
            s.insert(i, rng.choice(alpha))
        elif op == 1 and s:
            del s[min(i, len(s) - 1)]
        elif s:
            s[min(i, len(s) - 1)] = rng.choice(alpha)
    return "".join(s)


def _b_bases(rng):
    def text(n):
        return "".join(rng.choice(B_ALPHA) for _ in range(n))
    out = [text(rng.randint(60, 66)) for _ in range(3)] + [text(rng.randint(120, 128)) for _ in range(2)]
    out += [text(20), text(40)]
    # code-point order vs UTF-16 unit order: U+FF21 < U+1F600, but 0xFF21 > 0xD83D
    out += ["Ａ😀bcd", "😀Ａbcd", "Ａbcd", "😀bcd", "😀bcd" + text(58)]
    return out


def _a_value(rng, empty):
    r = rng.random()
    if r < 0.08:
        return None
    if empty and r < 0.14:
        return ""
    v = _mutate(rng, rng.choice(A_BASES), rng.choice([0, 0, 0, 1, 1, 2]), A_ALPHA, 12)
    return v if (v or empty) else "a"


def _b_value(rng, bases):
    r = rng.random()
    if r < 0.08:
        return None
    if r < 0.11:
        return ""
    base = rng.choice(bases)
    return _mutate(rng, base, rng.choice([0, 0, 1, 2, 3, 6, 12]), B_ALPHA, 135)


def _num_value(rng):
    return float("nan") if rng.random() < 0.12 else rng.choice(NUM_VALUES)


def huge_pair(rng):
    """Two strings past 1024 UTF-16 units a few edits apart (the huge pass of the exact kernels)."""
    s = "".join(rng.choice(B_ALPHA) for _ in range(1030))
    return s, _mutate(rng, s, 5, B_ALPHA, 1100)


def make_records(rng, n, empty_a=True, n_keys=6, huge=False):
    """n records {unique_id, a, b, x, y, k}; numeric columns float64 (NULL as NaN), never object dtype: an
    object column reaches sqlite as TEXT and every numeric comparison would become a text comparison."""
    bases = _b_bases(rng)
    rows = []
    for i in range(n):
        rows.append({"unique_id": i, "a": _a_value(rng, empty_a), "b": _b_value(rng, bases),
                     "x": _num_value(rng), "y": _num_value(rng),
                     "k": None if rng.random() < 0.06 else f"k{rng.randrange(n_keys)}"})
    if huge and n >= 2:
        # one in each half: link_only and link_and_dedupe split the records there
        rows[0]["b"], rows[n // 2]["b"] = huge_pair(rng)
        rows[0]["k"] = rows[n // 2]["k"] = "k0"
    df = pd.DataFrame(rows)
    df["x"] = df["x"].astype(np.float64)
    df["y"] = df["y"].astype(np.float64)
    for c in ("a", "b", "k"):
        df[c] = df[c].astype(object)
    return df


def make_pair_frame(rng, n):
    """A comparison frame, one pair per row (a_l, a_r, b_l, ...): the right side is the left value, a mutation
    of it or an independent draw, so that distances and similarities land on both sides of the thresholds."""
    bases = _b_bases(rng)
    rows = []
    for i in range(n):
        row = {}
        al = _a_value(rng, True)
        r = rng.random()
        ar = al if r < 0.2 else (_a_value(rng, True) if r < 0.5 or al is None else
                                 _mutate(rng, al, rng.choice([1, 1, 2, 3]), A_ALPHA, 12))
        bl = _b_value(rng, bases)
        r = rng.random()
        br = bl if r < 0.15 else (_b_value(rng, bases) if r < 0.4 or bl is None else
                                  _mutate(rng, bl, rng.choice([1, 2, 3, 6, 20, 50]), B_ALPHA, 135))
        xl, yl = _num_value(rng), _num_value(rng)
        xr = xl if rng.random() < 0.3 else _num_value(rng)
        yr = yl if rng.random() < 0.3 else _num_value(rng)
        kl = None if rng.random() < 0.06 else f"k{rng.randrange(3)}"
        kr = kl if rng.random() < 0.6 else (None if rng.random() < 0.1 else f"k{rng.randrange(3)}")
        row.update(a_l=al, a_r=ar, b_l=bl, b_r=br, x_l=xl, x_r=xr, y_l=yl, y_r=yr, k_l=kl, k_r=kr)
        rows.append(row)
    rows[0]["b_l"], rows[0]["b_r"] = huge_pair(rng)
    # one unit apart, the differing units with equal low bytes (U+0061 / U+0161)
    rows[1]["a_l"], rows[1]["a_r"] = "a", "š"
    rows[2]["a_l"], rows[2]["a_r"] = "mšrtha", "martha"
    rows[3]["b_l"], rows[3]["b_r"] = "Ａbcd", "😀bcd"
    df = pd.DataFrame(rows)
    for c in ("x_l", "x_r", "y_l", "y_r"):
        df[c] = df[c].astype(np.float64)
    for c in ("a_l", "a_r", "b_l", "b_r", "k_l", "k_r"):
        df[c] = df[c].astype(object)
    return df


# ---------------------------------------------------------------------------------------------------------
# expressions (comparison form: <col>_l / <col>_r)
# ---------------------------------------------------------------------------------------------------------
def _str_operand(rng, col=None, side=None, plain=False):
    col = col or rng.choice("ab")
    side = side or rng.choice("lr")
    s = f"{col}_{side}"
    if plain or rng.random() < 0.7:
        return s
    r = rng.random()
    if r < 0.25:
        s = f"lower({s})"
    elif r < 0.45:
        s = f"trim({s})"
    if rng.random() < 0.4:
        s = f"ifnull({s}, '{rng.choice(STR_LITS)}')"
    if rng.random() < 0.45 or s == f"{col}_{side}":
        s = f"substr({s}, {rng.choice([1, 1, 2, 3, 60])}, {rng.choice([0, 1, 3, 5, 64, 200])})"
    return s


def _num_operand(rng, col=None, side=None, plain=False):
    col = col or rng.choice("xy")
    side = side or rng.choice("lr")
    s = f"{col}_{side}"
    if plain or rng.random() < 0.8:
        return s
    return f"ifnull({s}, {rng.choice(NUM_LITS)})"


def _ratio(a, b):
    return f"levenshtein({a}, {b})/((length({a}) + length({b}))/2)"


def _perc(a, b):
    return f"abs({a} - {b})/abs(case when {a} > {b} then {a} else {b} end)"


def _num(t):
    return repr(t) if isinstance(t, float) else str(t)


LEAF_KINDS = ["isnull", "strcmp", "numcmp", "jw", "lev", "levratio", "absdiff", "percdiff", "len", "const",
              "lit_str", "lit_num"]


def leaf(rng, kind=None):
    """One leaf test (one RPN instruction) of a random kind with a random comparator."""
    kind = kind or rng.choice(LEAF_KINDS)
    c = rng.choice(CMPS)
    if kind == "isnull":
        o = _str_operand(rng) if rng.random() < 0.5 else _num_operand(rng)
        return f"{o} is {'not ' if rng.random() < 0.5 else ''}null"
    if kind == "strcmp":
        return f"{_str_operand(rng)} {c} {_str_operand(rng)}"
    if kind == "numcmp":
        return f"{_num_operand(rng)} {c} {_num_operand(rng)}"
    if kind == "jw":
        return f"jaro_winkler_sim({_str_operand(rng)}, {_str_operand(rng)}) {c} {_num(rng.choice(JW_T))}"
    if kind == "lev":
        return f"levenshtein({_str_operand(rng)}, {_str_operand(rng)}) {c} {_num(rng.choice(LEV_T))}"
    if kind == "levratio":
        return f"{_ratio(_str_operand(rng), _str_operand(rng))} {c} {_num(rng.choice(RATIO_T))}"
    if kind == "absdiff":
        return f"abs({_num_operand(rng)} - {_num_operand(rng)}) {c} {_num(rng.choice(ABS_T))}"
    if kind == "percdiff":
        return f"{_perc(_num_operand(rng), _num_operand(rng))} {c} {_num(rng.choice(PERC_T))}"
    if kind == "len":
        return f"length({_str_operand(rng)}) {c} {_num(rng.choice(LEN_T))}"
    if kind == "const":
        return rng.choice(["true", "false", "null"])
    if kind == "lit_str":
        o, lit = _str_operand(rng), f"'{rng.choice(STR_LITS)}'"
        return f"{o} {c} {lit}" if rng.random() < 0.7 else f"{lit} {c} {o}"
    o, lit = _num_operand(rng), rng.choice(NUM_LITS)
    return f"{o} {c} {lit}" if rng.random() < 0.7 else f"{lit} {c} {o}"


def predicate(rng, depth=2, budget=16):
    """(text, RPN instruction count <= budget): an AND / OR / NOT tree of n-ary nodes, at most `depth` deep."""
    if depth == 0 or budget < 3 or rng.random() < 0.3:
        if budget >= 2 and rng.random() < 0.15:
            return f"not ({leaf(rng)})", 2
        return leaf(rng), 1
    m = min(rng.randint(2, 4), (budget + 1) // 2)
    spare = budget - (2 * m - 1)  # beyond one instruction per child and the m - 1 connectives
    parts, used = [], m - 1
    for i in range(m):
        give = spare if i == m - 1 else rng.randint(0, spare)
        text, n = predicate(rng, depth - 1, 1 + give)
        spare -= n - 1
        used += n
        parts.append(f"({text})")
    text = f" {rng.choice(['and', 'or'])} ".join(parts)
    if used < budget and rng.random() < 0.15:
        return f"not ({text})", used + 1
    return text, used


def predicate_exact(rng, total):
    """A predicate of exactly `total` RPN instructions (14 or 16: the device's limit is 16 per WHEN)."""
    def node(m):
        return "(" + f" {rng.choice(['and', 'or'])} ".join(f"({leaf(rng)})" for _ in range(m)) + ")", 2 * m - 1
    a, na = node(4)
    b, nb = node(3)
    op = rng.choice(["and", "or"])
    if total == 16:
        return f"{a} {op} {b} {rng.choice(['and', 'or'])} (not ({leaf(rng)}))", na + nb + 2 + 2
    assert total == 14
    return f"not ({a} {op} {b})", na + nb + 1 + 1


def _case(whens, else_level):
    return "case " + " ".join(f"when {p} then {lv}" for p, lv in whens) + f" else {else_level} end"


def _levels(rng, L, n):
    return [rng.randint(-1, L - 1) for _ in range(n)]


def column_g(rng, exact16=False):
    L = rng.randint(2, 4)
    n = rng.randint(1, 4)
    preds, sizes = [], []
    for i in range(n):
        text, size = predicate_exact(rng, 16) if (exact16 and i == 0) else predicate(rng, 2, 16)
        preds.append(text)
        sizes.append(size)
    lv = _levels(rng, L, n + 1)
    return dict(family="G", cls=None, L=L, expr=_case(list(zip(preds, lv)), lv[-1]), sizes=sizes, simple=False)


def _guard(rng, col):
    s = ("l", "r") if rng.random() < 0.5 else ("r", "l")
    return f"{col}_{s[0]} is null or {col}_{s[1]} is null"


def _s_test(rng, cls, col):
    l, r = f"{col}_l", f"{col}_r"
    if cls == "jw":
        return f"jaro_winkler_sim({l}, {r}) {rng.choice(['>', '>='])} {_num(rng.choice(JW_T))}"
    if cls == "lev":
        k = rng.random()
        if k < 0.55:
            return f"levenshtein({l}, {r}) {rng.choice(CMPS)} {_num(rng.choice(LEV_T))}"
        if k < 0.8:
            return f"{_ratio(l, r)} {rng.choice(['<', '<='])} {_num(rng.choice(RATIO_T))}"
        return f"{l} {rng.choice(['=', '!='])} {r}"
    if cls == "eq":
        return f"{l} {rng.choice(['=', '!='])} {r}"
    k = rng.random()
    if k < 0.34:
        return f"{l} {rng.choice(CMPS)} {r}"
    if k < 0.67:
        return f"abs({l} - {r}) {rng.choice(CMPS)} {_num(rng.choice(ABS_T))}"
    return f"{_perc(l, r)} {rng.choice(CMPS)} {_num(rng.choice(PERC_T))}"


def column_s(rng, cls=None, col=None):
    """Filter-shaped: the NULL guard (either side first), then 1-6 single-leaf tests on the same plain pair."""
    cls = cls or rng.choice(["jw", "lev", "eq", "num"])
    col = col or (rng.choice("xy") if cls == "num" else rng.choice("ab"))
    L = rng.randint(2, 4)
    n = rng.randint(1, 6)
    tests = [_s_test(rng, cls, col) for _ in range(n)]
    if cls == "lev" and not any("levenshtein" in t for t in tests):  # all `=` / `!=` would be class EQ
        tests[rng.randrange(n)] = f"levenshtein({col}_l, {col}_r) {rng.choice(CMPS)} {_num(rng.choice(LEV_T))}"
    lv = _levels(rng, L, n + 2)
    whens = [(_guard(rng, col), lv[0])] + list(zip(tests, lv[1:]))
    return dict(family="S", cls=cls, L=L, expr=_case(whens, lv[-1]), sizes=[3] + [1] * n, simple=True)


N_KINDS = ["jw_cmp", "ratio_gt", "swapped", "seven", "guard_other", "str_order"]


def column_n(rng, kind=None):
    """Near misses of the filter shape: every one must fall to the interpreter."""
    kind = kind or rng.choice(N_KINDS)
    col = rng.choice("ab")
    l, r = f"{col}_l", f"{col}_r"
    L = rng.randint(2, 4)
    n = 7 if kind == "seven" else rng.randint(1, 6)
    base_cls = rng.choice(["jw", "lev", "eq"]) if kind in ("seven", "guard_other") else \
        ("jw" if kind == "jw_cmp" else "lev")
    tests = [_s_test(rng, base_cls, col) for _ in range(n)]
    i = rng.randrange(n)
    guard_col = col
    if kind == "jw_cmp":
        tests[i] = f"jaro_winkler_sim({l}, {r}) {rng.choice(['<', '<=', '=', '!='])} {_num(rng.choice(JW_T))}"
    elif kind == "ratio_gt":
        tests[i] = f"{_ratio(l, r)} {rng.choice(['>', '>='])} {_num(rng.choice(RATIO_T))}"
    elif kind == "swapped":
        tests[i] = rng.choice([f"levenshtein({r}, {l}) {rng.choice(CMPS)} {_num(rng.choice(LEV_T))}",
                               f"jaro_winkler_sim({r}, {l}) {rng.choice(['>', '>='])} {_num(rng.choice(JW_T))}",
                               f"{r} = {l}"])
    elif kind == "guard_other":
        guard_col = "b" if col == "a" else "a"
    elif kind == "str_order":
        tests[i] = f"{l} {rng.choice(['<', '<=', '>', '>='])} {r}"
    lv = _levels(rng, L, n + 2)
    whens = [(_guard(rng, guard_col), lv[0])] + list(zip(tests, lv[1:]))
    return dict(family="N", cls=kind, L=L, expr=_case(whens, lv[-1]), sizes=[3] + [1] * n, simple=False)


SLOTS = {"jw": 4, "lev": 3, "eq": 6, "num": 4}  # spk_gamma.h FJ_MAX, FL_MAX, FE_MAX, FN_MAX


def job(rng, overflow=None, s_col=None):
    """A list of at most 12 columns mixing the three families (so one packed code word takes adds from the
    filter, exact, slow and interpreter passes).  overflow: None, or "jw" / "lev" / "num" for a job with one
    S column more of that class than the filter kernel has slots (5 / 4 / 5).  s_col: the string column of
    the string S columns (the blocked jobs put them on the blocking key's column)."""
    cols = []
    if overflow:
        cols += [column_s(rng, overflow, s_col if overflow != "num" else None) for _ in range(SLOTS[overflow] + 1)]
    n_s = rng.randint(2, 4) if not overflow else rng.randint(0, 2)
    for _ in range(n_s):
        cls = rng.choice([c for c in SLOTS if c != overflow])
        if sum(c["cls"] == cls for c in cols) >= SLOTS[cls]:
            continue
        cols.append(column_s(rng, cls, s_col if cls != "num" else None))
    cols += [column_n(rng) for _ in range(rng.randint(1, 3))]
    cols += [column_g(rng, exact16=rng.random() < 0.2) for _ in range(rng.randint(2, 12 - len(cols)) if len(cols) < 10
                                                                      else 1)]
    cols = cols[:12]
    rng.shuffle(cols)
    for i, c in enumerate(cols):
        c["name"] = f"c{i}"
    return cols


def expected_simple(cols):
    """Columns the filter kernel takes: the S columns, each class cut at the kernel's slots of that class
    (spk_gammas counts the filter's columns after layout_image returned the surplus to the interpreter)."""
    return sum(min(sum(c["cls"] == cls for c in cols if c["family"] == "S"), SLOTS[cls]) for cls in SLOTS)


def _fixed():
    """Hand-written columns run next to the random ones: each comparator family of the filter classes once,
    whatever the seeds draw (the `levenshtein > t` test that a "small distance passes" cut would get wrong,
    `=` / `!=` on a distance, thresholds outside the value range, unsorted levels), a Kleene NOT over
    NULL OR FALSE, and a near miss."""
    g = "{c}_l is null or {c}_r is null"
    lev, jw = "levenshtein({c}_l, {c}_r)", "jaro_winkler_sim({c}_l, {c}_r)"
    perc = _perc("x_l", "x_r")
    rows = [
        ("S", "lev", 2, "a", f"case when {g} then -1 when {lev} > 2 then 1 else 0 end"),
        ("S", "lev", 4, "a", f"case when a_r is null or a_l is null then 0 when {lev} = 1 then 2 when {lev} >= 3.5 then 0 "
                             f"when {lev} != 0 then 1 when {lev} < -1 then 3 else 3 end"),
        ("S", "lev", 4, "b", f"case when {g} then -1 when {lev} > 40 then 0 when {_ratio('b_l', 'b_r')} < 0.2 then 2 "
                             f"when {{c}}_l != {{c}}_r then 1 else 3 end"),
        ("S", "jw", 4, "a", f"case when {g} then -1 when {jw} > 1 then 0 when {jw} >= 1 then 3 when {jw} > 0.88 then 1 "
                            f"when {jw} >= 0 then 2 else 0 end"),
        ("S", "jw", 3, "b", f"case when {g} then 1 when {jw} >= 1.2 then 0 when {jw} >= 0.94 then 2 when {jw} > -0.1 then 0 "
                            f"else 1 end"),
        ("S", "eq", 2, "a", f"case when {g} then 1 when {{c}}_l != {{c}}_r then 0 when {{c}}_l = {{c}}_r then 1 else -1 end"),
        ("S", "num", 3, "x", f"case when {g} then -1 when {perc} > 1 then 0 when x_l >= x_r then 2 "
                             f"when abs(x_l - x_r) != 3.5 then 1 else 0 end"),
        ("G", None, 3, "a", "case when not ((a_l < a_r) or (false)) then 1 when not ((b_l = b_r) and (true)) then 2 "
                            "else 0 end"),
        ("N", "jw_cmp", 3, "a", f"case when {g} then -1 when {jw} < 0.88 then 0 when levenshtein(a_r, a_l) <= 1 then 1 "
                                f"else 2 end"),
    ]
    return [dict(name=f"f{i}", family=f, cls=cls, L=L, expr=e.format(c=c), simple=f == "S")
            for i, (f, cls, L, c, e) in enumerate(rows)]


FIXED_COLUMNS = _fixed()


def columns_used(expr):
    return sorted(set(re.findall(r"\b([abxyk])_[lr]\b", expr)))


def settings(cols, link_type="dedupe_only", rules=None):
    st = {"link_type": link_type, "proportion_of_matches": 0.1,
          "comparison_columns": [{"custom_name": c["name"], "custom_columns_used": columns_used(c["expr"]) or ["a"],
                                  "num_levels": c["L"], "case_expression": c["expr"]} for c in cols],
          "retain_matching_columns": False, "retain_intermediate_calculation_columns": False}
    if rules is not None:
        st["blocking_rules"] = list(rules)
    return st


# ---------------------------------------------------------------------------------------------------------
# residual rules
# ---------------------------------------------------------------------------------------------------------
def as_rule(text):
    """<col>_l / <col>_r -> l.<col> / r.<col>."""
    return re.sub(r"\b([abxyk])_([lr])\b", r"\2.\1", text)


def residual_rule(rng, exact=False):
    """`l.k = r.k and (<predicate>)`: the key term and its AND take 2 of the 16 instructions."""
    text, n = predicate_exact(rng, 14) if exact else predicate(rng, 2, 14)
    return as_rule(f"k_l = k_r and ({text})"), n + 2


def residual_rules(rng, n, sample):
    """n residual rules that each hold for some and fail for some of the key-equal pairs of `sample` (a pair
    frame): random trees are often constant (`levenshtein(..) >= -1`), and a rule that keeps every candidate or
    none says little about the filter.  The second rule has exactly 16 instructions."""
    keyed = (sample["k_l"] == sample["k_r"]).to_numpy(dtype=bool)
    out = []
    while len(out) < n:
        cand = [residual_rule(rng, exact=j % 2 == 0) for j in range(8)]
        lv = orc.sql_gammas(sample, [rule_as_case(r) for r, _ in cand])
        for j, (rule, size) in enumerate(cand):
            if 0.05 <= lv[keyed, j].mean() <= 0.95 and (len(out) != 1 or size == 16) and len(out) < n:
                out.append(rule)
    return out


def rule_as_case(rule):
    """The whole rule as a comparison column over <col>_l / <col>_r (level 1 = ifnull(rule, false))."""
    return "case when " + re.sub(r"\b([lr])\.([abxyk])\b", r"\2_\1", rule) + " then 1 else 0 end"


# ---------------------------------------------------------------------------------------------------------
# emulator of a CompiledComparisons (the semantics of spk_interp.h eval_pred / eval_column)
# ---------------------------------------------------------------------------------------------------------
OPNAME = {v: k for k, v in N.OP.items()}
CMPNAME = {0: "=", 1: "!=", 2: "<", 3: "<=", 4: ">", 5: ">="}


def _null(v):
    return v is None or v is pd.NA or (isinstance(v, float) and math.isnan(v))


def _cmp(a, b, c):
    return [a == b, a != b, a < b, a <= b, a > b, a >= b][c]


def _k_and(a, b):
    if a is False or b is False:
        return False
    return None if (a is None or b is None) else True


def _k_or(a, b):
    if a is True or b is True:
        return True
    return None if (a is None or b is None) else False


def _operand(compiled, o, row):
    """Value of an OperandSpec for a comparison-frame row; None = NULL."""
    if o.kind == "str":
        return o.lit
    if o.kind == "num":
        return None if math.isnan(o.num) else o.num
    suffix = "_r" if o.side else "_l"
    if o.name in compiled.derived:
        rec = {k[:-2]: v for k, v in row.items() if k.endswith(suffix)}
        v = D.eval_row(compiled.derived[o.name], rec)
    else:
        v = row[o.name + suffix]
    if _null(v):
        v = None
    if o.form == "num":
        if v is None:
            return o.num if o.has_num_default else None
        return float(v)
    if v is None:
        v = o.lit
    if v is not None and o.substr is not None:
        p, n = o.substr
        assert p >= 1 and n >= 0
        v = v[p - 1:p - 1 + n]
    return v


_jw = functools.lru_cache(maxsize=None)(orc.jaro_winkler)
_lev = functools.lru_cache(maxsize=None)(orc.levenshtein)


def _leaf_value(compiled, ins, row):
    op, c, t = OPNAME[int(ins["op"])], int(ins["cmp"]), float(ins["t"])
    if op == "CONST":
        return {0: False, 1: True, 2: None}[int(ins["i0"])]
    a = _operand(compiled, compiled.operands[int(ins["a"])], row)
    if op in ("ISNULL", "NOTNULL"):
        return (a is None) == (op == "ISNULL")
    if op == "LEN":
        return None if a is None else _cmp(float(len(a)), t, c)
    b = _operand(compiled, compiled.operands[int(ins["b"])], row)
    if a is None or b is None:
        return None
    if op in ("STR_CMP", "NUM_CMP"):
        return _cmp(a, b, c)  # Python orders str by code point, as Spark's UTF-8 byte order does
    if op == "JW":
        return _cmp(_jw(a, b), t, c)
    if op == "LEV":
        return _cmp(float(_lev(a, b)), t, c)
    if op == "LEVRATIO":
        den = (len(a) + len(b)) / 2.0
        return None if den == 0.0 else _cmp(_lev(a, b) / den, t, c)
    if op == "ABSDIFF":
        return _cmp(abs(a - b), t, c)
    assert op == "PERCDIFF"
    d = abs(a if a > b else b)
    return None if d == 0.0 else _cmp(abs(a - b) / d, t, c)


def emulate(compiled, row, trace=None):
    """Levels of every column program of `compiled` for one comparison-frame row (a mapping `<col>_l` /
    `<col>_r` -> value): an RPN stack over Kleene logic, the first WHEN that is TRUE decides.  With `trace`
    (a list) the deciding WHEN of each column is appended as (column, WHEN index or -1 for ELSE, the WHEN's
    instructions)."""
    out = []
    for k, (L, else_level, n_when, first_when) in enumerate(compiled.programs.tolist()):
        level, hit = else_level, (-1, None)
        for w in range(first_when, first_when + n_when):
            st = []
            ins = compiled.instrs[compiled.when_first[w]:compiled.when_first[w] + compiled.when_n[w]]
            for i in ins:
                op = OPNAME[int(i["op"])]
                if op == "AND":
                    b, a = st.pop(), st.pop()
                    st.append(_k_and(a, b))
                elif op == "OR":
                    b, a = st.pop(), st.pop()
                    st.append(_k_or(a, b))
                elif op == "NOT":
                    a = st.pop()
                    st.append(None if a is None else not a)
                else:
                    st.append(_leaf_value(compiled, i, row))
            assert len(st) == 1
            if st[0] is True:
                level, hit = int(compiled.when_level[w]), (w - first_when, ins)
                break
        out.append(level)
        if trace is not None:
            trace.append((k,) + hit)
    return out


def _short(rec):
    """A record for a message: strings past 200 units (the huge pair) cut to their head and their length."""
    if not isinstance(rec, dict):
        return rec
    return {k: (f"{v[:40]}...[{len(v)} units]" if isinstance(v, str) and len(v) > 200 else v) for k, v in rec.items()}


def describe(seed, mode, expr, rec_l, rec_r, got, want):
    """The message of a failed cell: enough for a two-row repro, not a dump of the job."""
    return (f"seed {seed} mode {mode}: got {got} want {want}\n  expr: {expr}\n  l: {_short(rec_l)}\n"
            f"  r: {_short(rec_r)}")
