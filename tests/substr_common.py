"""Spark's substr / substring, stated once and independently of the product: a port of UTF8String.substringSQL and
UTF8String.substring(start, until) over the UTF-8 bytes, the values and the (pos, len) grid of the substr tests,
and helpers that put precomputed substrings into a frame as plain columns -- so that oracle.block and
oracle.sql_gammas check the device with no substr() of their own (sqlite's differs from Spark's for position 0, for
negative positions and for a start before the string).

Shared by tests/test_substr_host.py (the host implementations and the tests' own restatements against this port) and
tests/test_gpu_substr.py (substr_range in spk_ingest.hip and apply_substr in spk_interp.h against it)."""
import itertools
import random

import pandas as pd

INT_MAX, INT_MIN = 2 ** 31 - 1, -2 ** 31
TWO_ARG = INT_MAX  # substr(x, pos) is substringSQL(pos, Integer.MAX_VALUE)


def _bytes_of_first_byte(b):
    """UTF8String.numBytesForFirstByte: the length of the code point a byte starts (1 for a byte that starts none)."""
    if b < 0xC0:
        return 1
    if b < 0xE0:
        return 2
    if b < 0xF0:
        return 3
    return 4 if b < 0xF8 else 1


def _num_chars(raw):
    i = n = 0
    while i < len(raw):
        i += _bytes_of_first_byte(raw[i])
        n += 1
    return n


def _substring(raw, start, until):
    """UTF8String.substring(start, until) on code points."""
    num_bytes = len(raw)
    if until <= start or start >= num_bytes:
        return b""
    i = c = 0
    while i < num_bytes and c < start:
        i += _bytes_of_first_byte(raw[i])
        c += 1
    j = i
    while i < num_bytes and c < until:
        i += _bytes_of_first_byte(raw[i])
        c += 1
    return raw[j:i] if i > j else b""


def spark_substring_sql(s, pos, length):
    """UTF8String.substringSQL(pos, length) of `s`: 1-based, position 0 is position 1, a negative position counts
    from the end (and may start before the string: the part before it is lost, the length still counts from
    there), `start + length` saturates at the int32 range."""
    raw = s.encode("utf-8")
    n = _num_chars(raw)
    start = pos - 1 if pos > 0 else (n + pos if pos < 0 else 0)
    end = start + length
    if end > INT_MAX:
        end = INT_MAX
    elif end < INT_MIN:
        end = INT_MIN
    return _substring(raw, start, end).decode("utf-8")


# ---------------------------------------------------------------------------------------------------------------------
# the exhaustive small cases of the host tests
# ---------------------------------------------------------------------------------------------------------------------
ALPHABET = ["a", "b", "é", "€", "😀"]  # 1-, 1-, 2-, 3- and 4-byte code points
SMALL_POS = list(range(-7, 8))
SMALL_LEN = [-1, 0, 1, 2, 3, 6, TWO_ARG]


def small_strings(max_len=5):
    """Every string of 0 .. max_len code points over ALPHABET."""
    return ["".join(t) for k in range(max_len + 1) for t in itertools.product(ALPHABET, repeat=k)]


# ---------------------------------------------------------------------------------------------------------------------
# the blocking-key tests' records and grid
# ---------------------------------------------------------------------------------------------------------------------
GRID_POS = [-9, -3, -1, 0, 1, 2, 4, 9]
GRID_LEN = [0, 1, 3, 200, None]  # None: the two-argument form

# lengths 0 .. 8 code points over 1- to 4-byte characters; 9 .. 20 code points, so that the hash reads whole 8-byte
# words and tails; values that share all but the last code point, and values that share all but the first
POOL_A = [
    "", "a", "é", "€", "😀",
    "ab", "é€", "hé",
    "abc", "abd", "a😀b", "xbc",
    "abcd", "xbcd", "é€😀a",
    "abcde", "abcdé", "😀bcde",
    "martha", "marthé", "mártha",
    "abcdefg", "é€😀aé€😀",
    "abcdefgh", "abcdefgé", "😀😀😀😀😀😀😀😀", "xbcdefgh",
    "abcdefghi", "abcdefghj", "éééééééééé", "ééééééééé€",
    "abcdefghijkl", "xbcdefghijkl", "€😀€😀€😀€😀€😀€😀",
    "abcdefghijklmnop", "abcdefghijklmnopq", "abcdefghijklmnopqrst", "😀abcdefghijklmnopqr€",
    "abcdefghijklmnopqrsé", "mabcdefghi",
    "ABC", "Martha", "MARTHÉ", "xBCD",  # lower() of a substr joins these with the lower-case values
]
# half of POOL_A, and values that equal substrings of POOL_A's values
POOL_B = POOL_A[::2] + ["de", "dé", "ha", "bc", "gh", "gé", "hi", "hj", "kl", "st", "b", "😀😀", "xab", "zbc", "qcd",
                        "yhi", "éé", "é€😀"]


def _draw(rng, pool, p_null):
    return None if rng.random() < p_null else rng.choice(pool)


def make_records(n=300, seed=7):
    """n records {unique_id, a, b, c, k, n}: `a` from POOL_A and `b` from POOL_B with 10 % NULL each, `c` one of
    two and `k` one of six strings, `n` (nullable Int64) one of two integers, all with NULLs."""
    rng = random.Random(seed)
    rows = []
    for i in range(n):
        rows.append({"unique_id": i, "a": _draw(rng, POOL_A, 0.1), "b": _draw(rng, POOL_B, 0.1),
                     "c": _draw(rng, ["c0", "c1"], 0.08), "n": _draw(rng, [-5, 2 ** 40], 0.08),
                     "k": _draw(rng, [f"k{j}" for j in range(6)], 0.06)})
    df = pd.DataFrame(rows)
    for c in ("a", "b", "c", "k"):
        df[c] = df[c].astype(object).where(df[c].notna(), None)
    df["n"] = pd.array([None if v is None or v != v else int(v) for v in df["n"].tolist()], dtype="Int64")
    return df


def is_null(v):
    return v is None or v is pd.NA or (isinstance(v, float) and v != v)


def ref_values(values, pos, length):
    """spark_substring_sql over a list of values; NULL stays NULL.  length None: the two-argument form."""
    ln = TWO_ARG if length is None else length
    return [None if is_null(v) else spark_substring_sql(v, pos, ln) for v in values]


def add_ref_substr(df, name, col, pos, length, fn=None):
    """A copy of `df` with the column `name` = substr(col, pos, length) by the port (then fn, e.g. str.lower)."""
    vals = ref_values(df[col].tolist(), pos, length)
    if fn is not None:
        vals = [None if v is None else fn(v) for v in vals]
    out = df.copy()
    out[name] = pd.Series(vals, dtype=object, index=df.index)
    return out


def substr_sql(operand, pos, length):
    """The SQL text of a substr call; length None: substring(operand, pos)."""
    return f"substring({operand}, {pos})" if length is None else f"substr({operand}, {pos}, {length})"


# ---------------------------------------------------------------------------------------------------------------------
# the comparison-program tests' pair frame
# ---------------------------------------------------------------------------------------------------------------------
BMP = list("abcdeé€Ｚ ")
ASTRAL = ["😀", "𝒜", "🙂"]  # two UTF-16 units each


def text_of_units(rng, units, p_astral):
    """A string of exactly `units` UTF-16 units; each step draws a supplementary-plane character with p_astral."""
    out, left = [], units
    while left:
        if left >= 2 and rng.random() < p_astral:
            out.append(rng.choice(ASTRAL))
            left -= 2
        else:
            out.append(rng.choice(BMP))
            left -= 1
    return "".join(out)


# a surrogate pair before, at and after the cuts of positions -4 .. 4 and lengths 1 .. 4
CUT_CASES = ["😀abc", "a😀bc", "ab😀c", "abc😀", "😀😀😀😀", "a😀", "😀a", "😀", "ab😀cd😀ef", "😀b😀c😀d😀", "abcd😀", "😀abcd",
             "abc😀de", "ab😀cde", "a😀bcde", "abcde😀f", "abcdef", "é€Ｚa", "", "a", "ab", "abc", "abcd", "abcde"]


def _mutate(rng, s, k, alpha):
    s = list(s)
    for _ in range(k):
        op, i = rng.randrange(3), rng.randrange(len(s) + 1)
        if op == 0 or not s:
            s.insert(i, rng.choice(alpha))
        elif op == 1:
            del s[min(i, len(s) - 1)]
        else:
            s[min(i, len(s) - 1)] = rng.choice(alpha)
    return "".join(s)


def make_pair_frame(rng, n, huge):
    """n pairs {a_l, a_r, b_l, b_r}: `a` short (CUT_CASES, texts of 0 .. 12 units), `b` long (63, 64, 65 and 120 ..
    130 units, with and without supplementary-plane characters, and the pair `huge` past 1024 units in row 0); the
    right value is the left one, a mutation of it or an independent draw; 8 % NULL on either side."""
    def a_value():
        return rng.choice(CUT_CASES) if rng.random() < 0.5 else text_of_units(rng, rng.randint(0, 12), 0.25)

    b_bases = [text_of_units(rng, u, p) for u in (63, 64, 65, 63, 64, 65, 1, 0, 120, 130) for p in (0.0, 0.3)]

    def right_of(v, draw, alpha):
        r = rng.random()
        if r < 0.2:
            return v
        return draw() if r < 0.45 else _mutate(rng, v, rng.choice([1, 1, 2, 3]), alpha)

    rows = []
    for i in range(n):
        al, bl = a_value(), rng.choice(b_bases)
        row = dict(a_l=al, a_r=right_of(al, a_value, BMP + ASTRAL), b_l=bl,
                   b_r=right_of(bl, lambda: rng.choice(b_bases), BMP + ASTRAL))
        for c in row:
            if rng.random() < 0.08:
                row[c] = None
        rows.append(row)
    rows[0]["b_l"], rows[0]["b_r"] = huge
    for i, s in enumerate(CUT_CASES):  # every cut case once against itself and once against its neighbour
        rows[1 + 2 * i].update(a_l=s, a_r=s)
        rows[2 + 2 * i].update(a_l=s, a_r=CUT_CASES[(i + 1) % len(CUT_CASES)])
    for i, u in enumerate((0, 1, 63, 64, 65)):  # the unit lengths around the 64-unit kernels, equal and one edit apart
        for j, p in enumerate((0.0, 0.3)):
            s = text_of_units(rng, u, p)
            rows[60 + 4 * i + 2 * j].update(b_l=s, b_r=s)
            rows[61 + 4 * i + 2 * j].update(b_l=s, b_r=_mutate(rng, s, 1, BMP + ASTRAL))
    df = pd.DataFrame(rows)
    for c in df.columns:
        df[c] = df[c].astype(object).where(df[c].notna(), None)
    return df


def operand_sql(col, side, pos, length, default=None):
    """substr(<col>_<side>, pos, length), over ifnull(<col>_<side>, '<default>') when a default is given."""
    inner = f"{col}_{side}" if default is None else f"ifnull({col}_{side}, '{default}')"
    return substr_sql(inner, pos, length)


def operand_values(df, col, side, pos, length, default=None):
    vals = [default if is_null(v) else v for v in df[f"{col}_{side}"].tolist()]
    return ref_values(vals, pos, length)
