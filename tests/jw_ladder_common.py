"""Pair families and threshold ladders that pin Jaro-Winkler values to the bit (no GPU here).

A comparison column only tells on which side of its thresholds a value lies.  To see the value itself, the
ladders here put the thresholds ON the reference values of the pairs under test: a column takes three rungs
v1 > v2 > v3 and asks `> v1`, `>= v1`, `> v2`, `>= v2`, `> v3`, `>= v3`, so a pair whose value is exactly v2
gets level 3, one ulp above it level 4, one ulp below it level 2.  Every expectation comes from orc.jaro_winkler
and Python comparisons; the families are the smallest strings at which each device kernel can still go wrong
(spk_strsim.h jw_exact's dispatch, restated in kernel_of()).

Used by tests/test_jw_ladder_host.py (the ladders pin every pair, a one-ulp error would show, the thresholds
survive the compiler) and tests/test_gpu_jw_values.py (the device gives these levels in every comparison path).
"""
import math

import numpy as np

import oracle as orc

MAX_TESTS = 6            # spk_gamma.h: tests of a template column after its NULL guard
LEVELS = MAX_TESTS + 1   # levels 0..6 of a ladder column; with -1 (NULL) a column counts 8 patterns
FILTER_JW_SLOTS = 4      # spk_gamma.h FJ_MAX: Jaro-Winkler columns the filter kernel takes; more go to the interpreter
NARROW_COLS = 4          # 8^4 patterns: uint16 packed codes, every column in the filter kernel and jw_cell
WIDE_COLS = 10           # 8^10 = 2^30 patterns (< 2^31): uint32 codes; columns 5..10 run the interpreter
CODE16_PATTERNS = 65536  # spk_gamma.hip set_pattern_space: 2-byte codes up to this many patterns
LADDER, MIXED_EQ = "ladder", "mixed_eq"
FAMILIES = ("planes32", "planes64", "mixed", "slow", "huge")

ALPHA_2 = list("ab")
ALPHA_8 = list("abcdefgh")
ALPHA_NAME = list("abcdefghijklmnopqrstuvwxyz") + list(" '-")
ALPHA_LATIN1 = list("abcdefgh") + ["é", "ü"]   # U+00E9 / U+00FC: plane 7 is in use
# units >= 256 equal in their low byte to an ASCII letter of the other side: a kernel that compared bytes, or
# planes of a row that has none, would match them
WIDE = {"a": "š", "c": "ţ", "`": "Š"}   # š U+0161, ţ U+0163, Š U+0160
SURROGATE = chr(0x28462)  # UTF-16 D861 DC62: both units' low bytes are letters ('a', 'b')


def ulen(s):
    """Length in UTF-16 units, what the device kernels and the jar count."""
    return len(s.encode("utf-16-le", "surrogatepass")) // 2


def _units(s):
    return list(np.frombuffer(s.encode("utf-16-le", "surrogatepass"), dtype=np.uint16))


def draw(rng, alpha, n):
    return "".join(alpha[int(i)] for i in rng.integers(0, len(alpha), n))


def mutate(rng, s, k, alpha, cap):
    """k random edits -- insert, delete, substitute, adjacent swap -- then at most `cap` characters."""
    s = list(s)
    for _ in range(k):
        op = int(rng.integers(4))
        i = int(rng.integers(len(s) + 1))
        c = alpha[int(rng.integers(len(alpha)))]
        if op == 0 or not s:
            s.insert(i, c)
        elif op == 1:
            del s[min(i, len(s) - 1)]
        elif op == 2 or len(s) < 2:
            s[min(i, len(s) - 1)] = c
        else:
            j = min(i, len(s) - 2)
            s[j], s[j + 1] = s[j + 1], s[j]
    return "".join(s[:cap])


def _orient(a, b, how):
    """0: as drawn, 1: swapped, 2: equal lengths (then the jar's `max` is the SECOND string)."""
    if how == 1:
        return b, a
    if how == 2:
        n = min(len(a), len(b))
        return a[:n], b[:n]
    return a, b


def jaro_parts(a, b):
    """(matches, transpositions / 2, common prefix) of commons-text 1.4 JaroWinklerDistance.matches(), in plain
    Python over UTF-16 units: what the coverage conditions of the host test are stated in."""
    x, y = _units(a), _units(b)
    mx, mn = (x, y) if len(x) > len(y) else (y, x)
    rng = max(len(mx) // 2 - 1, 0)
    idx = [-1] * len(mn)
    flags = [False] * len(mx)
    m = 0
    for mi, c in enumerate(mn):
        for xi in range(max(mi - rng, 0), min(mi + rng + 1, len(mx))):
            if not flags[xi] and c == mx[xi]:
                idx[mi] = xi
                flags[xi] = True
                m += 1
                break
    ms1 = [mn[i] for i in range(len(mn)) if idx[i] != -1]
    ms2 = [mx[i] for i in range(len(mx)) if flags[i]]
    t = sum(1 for p, q in zip(ms1, ms2) if p != q)
    prefix = 0
    for p, q in zip(x, y):
        if p != q:
            break
        prefix += 1
    return m, t // 2, prefix


REORDERINGS = ("x + (y + z)", "(x + z) + y", "sum * (1 / 3)", "j + w * (prefix * (1 - j))")


def finish_variants(m, t, prefix, lf, ls):
    """[the jar's value, then what each of REORDERINGS -- the same real-number expression in another operation
    order -- would give] from matches, transpositions / 2, prefix and the two lengths.  The families hold pairs
    whose value differs under each of them, so a device expression in another order cannot pass."""
    if m == 0:
        return [0.0] * (1 + len(REORDERINGS))
    x, y, z = m / lf, m / ls, (m - t) / m
    w = min(0.1, 1.0 / max(lf, ls))

    def winkler(j, alt=False):
        if j < 0.7:
            return j
        return j + w * (prefix * (1.0 - j)) if alt else j + (w * prefix) * (1.0 - j)

    j = ((x + y) + z) / 3
    return [winkler(j), winkler((x + (y + z)) / 3), winkler(((x + z) + y) / 3), winkler(((x + y) + z) * (1 / 3)),
            winkler(j, alt=True)]


def jaro_winkler_py(a, b):
    """The jar's expression over jaro_parts, in its operation order (a second restatement next to the C oracle)."""
    return finish_variants(*jaro_parts(a, b), ulen(a), ulen(b))[0]


KNOWN_PARTS = {}  # (a, b) -> (m, t, prefix) of the pairs built by substituted_pairs (long strings: no Python matching)


def substituted_pairs(lengths, base=0x4E00):
    """Pairs of a (n distinct units from `base` on) and b (a without its last d units and with k units from position
    `first` on replaced by 'z'), in either order: every other unit matches its own position, so m = n - d - k, no
    transpositions, prefix = first.  For each of REORDERINGS the first (n, d, k, first) found, n among `lengths`,
    whose value differs under it."""
    out = []
    for r in range(1, 1 + len(REORDERINGS)):
        found = None
        for n in lengths:
            for d in (0, 1, 2, 3, 5):
                for k in range(1, min(80, n // 3)):
                    for first in (n // 3, n // 2, n // 5, 7):
                        lf, ls = (n, n - d) if r % 2 else (n - d, n)
                        v = finish_variants(n - d - k, 0, first, lf, ls)
                        if v[r] != v[0] and found is None:
                            found = (n, d, k, first)
        assert found is not None, (lengths, r)
        n, d, k, first = found
        a = "".join(chr(base + i) for i in range(n))
        b = list(a[:n - d])
        step = max(1, (n - d - first) // k)
        for i in range(k):
            b[first + i * step] = "z"
        pair = (a, "".join(b)) if r % 2 else ("".join(b), a)
        KNOWN_PARTS[pair] = (n - d - k, 0, first)
        out.append(pair)
    return out


def has_planes(s):
    """Rows that carry bit-planes (spk_internal.h CPF_PLANES): at most 64 units, all below 256."""
    u = _units(s)
    return len(u) <= 64 and all(c < 256 for c in u)


def kernel_of(a, b):
    """The device code that evaluates jaro_winkler_sim(a, b) for two table rows, by the dispatch of jw_cell /
    jw_exact (spk_strsim.h) and the slow and huge passes: what each family is built to reach."""
    if a is None or b is None:
        return "null"
    la, lb = ulen(a), ulen(b)
    if a == b:
        return "equal"
    if max(la, lb) > 1024:
        return "huge"
    if max(la, lb) > 64:
        return "slow"
    mx, mn = (a, b) if la > lb else (b, a)
    word = "u32" if ulen(mx) <= 32 else "u64"
    if has_planes(mx) and has_planes(mn):
        return f"planes2_{word}"
    if has_planes(mx):
        return f"planes_{word}"
    return "small_global"


# ---- families --------------------------------------------------------------------------------------------------
def _planes32():
    rng = np.random.Generator(np.random.PCG64(3201))
    out = []
    k = 0
    for alpha in (ALPHA_2, ALPHA_8, ALPHA_NAME):
        for n in (1, 2, 3, 4, 5, 10, 11, 16, 31, 32):
            for edits in (1, 2, 3, 6):
                a = draw(rng, alpha, n)
                out.append(_orient(a, mutate(rng, a, edits, alpha, 32), k % 3))
                k += 1
            out.append((draw(rng, alpha, n), draw(rng, alpha, n)))  # a full re-draw
    # shared prefixes of 0..lmn units (the jar does not cap the prefix at 4), on both sides of w = 0.1 / 1/lmx
    for n, base in ((5, "abcde"), (10, "abcdefghij"), (11, "abcdefghijk")):
        for pre in range(n + 1):
            tail = "".join("z" if (i - pre) % 3 == 0 else base[i] for i in range(pre, n))
            out.append((base, base[:pre] + tail) if pre % 2 else (base[:pre] + tail, base + "a"))
    out += [
        # greedy first-free matching over repeated letters
        ("aaaa", "aaa"), ("aabaa", "abaaa"), ("abab", "baba"), ("aaabbb", "bbbaaa"), ("banana", "ananab"),
        ("abababababab", "babababababa"),
        # transpositions / 2 >= 2
        ("abcdefgh", "badcfehg"), ("abcdefghij", "bacdfeghji"),
        # longer length 10: range = 4; 'q' can match at distance 4 and not at distance 5
        ("qaaaaaaaaa", "bbbbqbbbbb"), ("qaaaaaaaaa", "bbbbbqbbbb"), ("bbbbqbbbbb", "qaaaaaaaa"),
        ("bbbbbqbbbb", "qaaaaaaaa"),
        # longer length <= 3: range = 0, only equal positions match
        ("ab", "ba"), ("abc", "bca"), ("abc", "abd"), ("abc", "xbc"), ("a", "ab"), ("b", "ab"), ("abc", "c"),
        # longer length 4 / 5: range = 1
        ("abcd", "bacd"), ("abcd", "cdab"), ("abcde", "badce"),
        # no common unit, identical, empty
        ("abc", "xyz"), ("aaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaa", "bbbbbbbbbbbbbbbbbbbbbbbbbbbbbbbb"), ("smith", "smith"),
        ("a", "a"), ("abcdefghabcdefghabcdefghabcdefgh", "abcdefghabcdefghabcdefghabcdefgh"), ("", ""), ("", "abc"),
        ("abc", ""),
        # the reference's own examples
        ("smith", "smithe"), ("linacre", "linaker"),
        # NULL rows
        (None, "abc"), ("abc", None), (None, None),
    ]
    return out


def _planes64():
    rng = np.random.Generator(np.random.PCG64(6401))
    out = []
    k = 0
    for n in (33, 34, 47, 63, 64):
        a = draw(rng, ALPHA_LATIN1, n)
        for edits in (1, 3, 6):  # the shorter row has 33..64 units too: both halves of jw_planes2<u64> run
            out.append(_orient(a, mutate(rng, a, edits, ALPHA_LATIN1, 64), k % 3))
            k += 1
        for m in (20, 32):       # the shorter row has <= 32 units: its second half loop does not run
            out.append(_orient(a, mutate(rng, a[:m], 2, ALPHA_LATIN1, 32), k % 2))
            k += 1
        out.append((a[n - 30:], a))                           # a suffix: most of its units lie outside the window
        out.append((a, a[:n // 2] + draw(rng, ALPHA_LATIN1, n - n // 2)))  # equal lengths, half re-drawn
        out.append((draw(rng, ALPHA_LATIN1, n), draw(rng, ALPHA_LATIN1, n - 1)))
    a = draw(rng, ALPHA_LATIN1, 64)
    out += [
        (a, a[:40] + draw(rng, ALPHA_LATIN1, 24)),            # 40 of 64 units shared as a prefix
        (a[:40] + draw(rng, ALPHA_LATIN1, 7), a),
        (a, a[:63] + "z"), ("z" + a[1:], a), (a[:33], a[:32] + "z"),
        (a[1:] + a[:1], a),                                   # a rotation: > 32 matches, all one unit off
        ("".join(a[i ^ 1] for i in range(64)), a),            # every adjacent pair swapped
        ("ab" * 32, "ba" * 32), ("é" * 40, "ü" * 40 + "é"), ("é" * 33, "é" * 34), (a, a),
        ("é" * 64, "ü" * 64),                                 # no common unit
    ]
    out += substituted_pairs(range(64, 40, -1), base=0xA1)    # Latin-1; values that depend on the operation order
    return out


def _widen(rng, s, how):
    """s with one or two letters replaced by a unit >= 256 of the same low byte, or (how = 2, where the row stays
    within 64 units) a surrogate pair inserted."""
    t = list(s)
    spots = [i for i, c in enumerate(t) if c in WIDE]
    if (how == 2 and ulen(s) + 2 <= 64) or not spots:
        t.insert(int(rng.integers(len(t) + 1)), SURROGATE)
        return "".join(t)
    for i in rng.choice(spots, size=min(len(spots), 1 + how), replace=False):
        t[int(i)] = WIDE[t[int(i)]]
    return "".join(t)


def _mixed():
    rng = np.random.Generator(np.random.PCG64(2561))
    alpha = list("abc`")
    out = []
    k = 0
    for n in (1, 2, 3, 4, 7, 12, 20, 31, 32, 33, 40, 62, 64):
        for wide_on_longer in (False, True):
            for rep in range(2):
                a = draw(rng, alpha, n)
                b = mutate(rng, a, 1 + k % 3, alpha, 64) or "a"
                long_, short = (a, b) if len(a) > len(b) else (b, a)
                if wide_on_longer:   # the longer row has no planes: jw_small over global memory
                    long_ = _widen(rng, long_, k % 3)
                else:                # only the longer row has planes: jw_planes, the shorter through UnitReader
                    short = _widen(rng, short, k % 3 if ulen(short) + 2 <= ulen(long_) else k % 2)
                out.append((long_, short) if rep else (short, long_))
                k += 1
    out += [
        ("abcd", "šbcd"), ("šbcd", "abcd"), ("abca", "abţa"), ("abţa", "abcab"),
        ("``a", "Š`a"), (SURROGATE + "ab", "abab"), ("abab", SURROGATE + "ab"), ("ab", SURROGATE),
        ("šţ", "ac"),                               # no common unit, the low bytes all equal
        ("šb" * 16, "šb" * 16), (None, "š"), ("ţ", None),
    ]
    return out


def _slow():
    rng = np.random.Generator(np.random.PCG64(1024))
    alpha = ALPHA_8 + [" "]
    out = []
    for n in (65, 100, 128, 129, 300, 1023, 1024):
        a = draw(rng, alpha, n)
        out.append((a, mutate(rng, a, 2, alpha, 1024)))
        out.append((mutate(rng, a, 8, alpha, 1024), a))
        out.append((a, mutate(rng, a[:40], 2, alpha, 64)))    # one side within the exact pass's 64 units
    out += substituted_pairs((300, 299, 250))                # values that depend on the expression's operation order
    a = draw(rng, alpha, 65)
    out += [(a, a[:64]), (a[:64], a), (a, a), ("a" * 70, "b" * 70), (a, a[:64] + "š")]
    return out


def _huge():
    rng = np.random.Generator(np.random.PCG64(1500))
    alpha = ALPHA_8 + [" "]
    out = []
    for n in (1025, 1500):
        a = draw(rng, alpha, n)
        out.append((a, mutate(rng, a, 4, alpha, 1500)))
        out.append((a[:1000] + draw(rng, alpha, n - 1000), a))
        out.append((a[:30], a))
    out += substituted_pairs((1100, 1099, 1200))
    out += [(a, a), ("a" * 1025, "b" * 1024)]
    return out


_BUILDERS = {"planes32": _planes32, "planes64": _planes64, "mixed": _mixed, "slow": _slow, "huge": _huge}
_CACHE = {}


def family(name):
    """The family's pairs [(a, b)] and their reference values [float | None], computed once."""
    if name not in _CACHE:
        pairs = _BUILDERS[name]()
        _CACHE[name] = (pairs, [orc.jaro_winkler(a, b) for a, b in pairs])
    return _CACHE[name]


# ---- ladders ---------------------------------------------------------------------------------------------------
_GUARD = "case when a_l is null or a_r is null then -1 "
_JW = "jaro_winkler_sim(a_l, a_r)"
_M = [0.05, 0.05, 0.1, 0.1, 0.1, 0.2, 0.4]
_U = [0.4, 0.2, 0.1, 0.1, 0.1, 0.05, 0.05]


def rung_tests(rung, form=LADDER):
    """[(cmp, threshold, level)] of one column after its guard (and, in the mixed form, after `a_l = a_r`)."""
    v1, v2, v3 = rung
    tests = [(">", v1, 6), (">=", v1, 5), (">", v2, 4), (">=", v2, 3), (">", v3, 2), (">=", v3, 1)]
    return tests if form == LADDER else tests[1:]


def ladder_expression(rung, form=LADDER, jw=_JW, guard=_GUARD):
    assert rung[0] > rung[1] > rung[2]
    head = "" if form == LADDER else "when a_l = a_r then 6 "
    return (guard + head + " ".join(f"when {jw} {c} {t!r} then {lv}" for c, t, lv in rung_tests(rung, form))
            + " else 0 end")


def level_of(v, rung, form=LADDER, equal=False):
    """The level a column gives a pair whose Jaro-Winkler value is v (None: a NULL side): Python comparisons only."""
    if v is None:
        return -1
    if form == MIXED_EQ and equal:
        return 6
    for c, t, lv in rung_tests(rung, form):
        if (v > t) if c == ">" else (v >= t):
            return lv
    return 0


def ladder_settings(values, n_cols, form=LADDER, jw=_JW):
    """One call: n_cols ladder columns over a_l / a_r whose rungs are `values` (distinct, at most 3 x n_cols; in
    descending order three to a column).  Missing rungs are filled with 2.0, 3.0 ..., which no value reaches.
    `jw` is the SQL text of the compared value (views and literals: tests/test_gpu_jw_values.py).
    Returns {"settings", "rungs", "form"}."""
    values = sorted(set(values), reverse=True)
    assert len(values) <= 3 * n_cols and all(0.0 <= v <= 1.0 for v in values)
    fill = 3 * n_cols - len(values)
    values = [float(2 + i) for i in reversed(range(fill))] + values
    rungs = [tuple(values[3 * k:3 * k + 3]) for k in range(n_cols)]
    cols = [{"custom_name": f"j{k}", "custom_columns_used": ["a"], "num_levels": LEVELS,
             "case_expression": ladder_expression(r, form, jw), "m_probabilities": list(_M),
             "u_probabilities": list(_U)}
            for k, r in enumerate(rungs)]
    assert (LEVELS + 1) ** n_cols < 2 ** 31  # the pattern space spk_gammas accepts
    return {"settings": {"link_type": "dedupe_only", "comparison_columns": cols}, "rungs": rungs, "form": form}


def ladder_calls(values, n_cols, form=LADDER, jw=_JW):
    """The distinct values split over as many calls as they need."""
    values = sorted(set(v for v in values if v is not None), reverse=True)
    step = 3 * n_cols
    return [ladder_settings(values[i:i + step], n_cols, form, jw) for i in range(0, len(values), step)]


def family_calls(name, form=LADDER):
    """The family's ladder calls: every value once in the narrow layout (uint16 codes) and once in the wide one
    (uint32 codes)."""
    refs = family(name)[1]
    return ladder_calls(refs, NARROW_COLS, form) + ladder_calls(refs, WIDE_COLS, form)


def expected_levels(pairs, refs, call):
    """The whole code matrix of one call: len(pairs) x columns, int8."""
    out = np.empty((len(pairs), len(call["rungs"])), dtype=np.int8)
    for i, ((a, b), v) in enumerate(zip(pairs, refs)):
        for k, rung in enumerate(call["rungs"]):
            out[i, k] = level_of(v, rung, call["form"], equal=a is not None and a == b)
    return out


def pinned(refs, calls):
    """For each pair the (call, column, level) whose rung is the pair's own value -- every one of them, so a caller
    can check there is exactly one per layout; None for a pair with a NULL side."""
    where = {}
    for c, call in enumerate(calls):
        for k, rung in enumerate(call["rungs"]):
            for r, v in enumerate(rung):
                where.setdefault(v, []).append((c, k, 5 - 2 * r))
    return [None if v is None else list(where.get(v, [])) for v in refs]


def ulp_neighbours(values):
    """Pairs of distinct values one ulp apart."""
    vs = sorted(set(v for v in values if v is not None))
    return [(x, y) for x, y in zip(vs, vs[1:]) if math.nextafter(x, math.inf) == y]
