"""jaccard_sim, cosine_distance and the q-gram tokenisers of the reference's UDF jar
(jars/scala-udf-similarity-0.0.6.jar), restated in plain Python from the specification recovered from its class
files (parity unpinned: the jar is not executable): the checker of tests/test_setsim_host.py and
tests/test_gpu_setsim.py.  Strings are Java Strings: everything works on UTF-16 code units.  Nothing here
imports the package under test.
"""
import math
import random

# Character.isWhitespace, as code units (every such character is in the BMP)
WHITESPACE = (set(range(9, 14)) | set(range(28, 33)) | {0x1680} | set(range(0x2000, 0x2007)) |
              set(range(0x2008, 0x200B)) | {0x2028, 0x2029, 0x205F, 0x3000})
SURROGATE = "\U0001F600"  # one code point, two units


def units(s):
    b = s.encode("utf-16-le", "surrogatepass")
    return [b[i] | (b[i + 1] << 8) for i in range(0, len(b), 2)]


def ulen(s):
    return len(units(s))


def jaccard_sim(a, b):
    """JaccardSimilarity.call -> commons-text 1.4 JaccardSimilarity.apply: Math.round(x * 100.0) / 100.0 of
    x = |A n B| / |A u B| over the sets of distinct units; 0.0 when either string is empty."""
    ua, ub = units(a), units(b)
    if not ua or not ub:
        return 0.0
    sa, sb = set(ua), set(ub)
    x = float(len(sa & sb)) / float(len(sa | sb))
    v = x * 100.0
    r = math.floor(v)  # Math.round: round half up to a long
    if v - r >= 0.5:
        r += 1
    return r / 100.0


def is_word(u):
    return 48 <= u <= 57 or 65 <= u <= 90 or 97 <= u <= 122 or u == 95


def tokens(s):
    """RegexTokenizer: every maximal run of [A-Za-z0-9_] (pattern (\\w)+, find() / group(0)), case-sensitive."""
    out, cur = [], []
    for u in units(s):
        if is_word(u):
            cur.append(u)
        elif cur:
            out.append(tuple(cur))
            cur = []
    if cur:
        out.append(tuple(cur))
    return out


def is_blank(s):
    return all(u in WHITESPACE for u in units(s))


def cosine_distance(a, b):
    """CosineDistance.call -> commons-text 1.4 CosineDistance.apply; None where the reference throws
    IllegalArgumentException("Invalid text") (a blank operand)."""
    if is_blank(a) or is_blank(b):
        return None
    ca, cb = {}, {}
    for t in tokens(a):
        ca[t] = ca.get(t, 0) + 1
    for t in tokens(b):
        cb[t] = cb.get(t, 0) + 1
    dot = sum(ca[t] * cb[t] for t in ca if t in cb)  # a long
    d1 = float(sum(c * c for c in ca.values()))
    d2 = float(sum(c * c for c in cb.values()))
    cos = 0.0 if d1 <= 0.0 or d2 <= 0.0 else float(dot) / (math.sqrt(d1) * math.sqrt(d2))
    return 1.0 - cos


def _window_text(w):
    out, i = [], 0
    while i < len(w):
        u = w[i]
        if 0xD800 <= u < 0xDC00 and i + 1 < len(w) and 0xDC00 <= w[i + 1] < 0xE000:
            out.append(chr(0x10000 + ((u - 0xD800) << 10) + (w[i + 1] - 0xDC00)))
            i += 2
        else:
            out.append("?" if 0xD800 <= u < 0xE000 else chr(u))  # Java's UTF-8 encoder: '?' for an unpaired surrogate
            i += 1
    return "".join(out)


def qgram(s, q):
    """new StringOps(s).sliding(q).toList.mkString(" "): None for NULL, '' for '', the whole string up to q units."""
    if s is None:
        return None
    u = units(s)
    if not u:
        return ""
    if len(u) <= q:
        return _window_text(u)
    return " ".join(_window_text(u[i:i + q]) for i in range(len(u) - q + 1))


Q_OF = {"QgramTokeniser": 2, "Q2gramTokeniser": 2, "Q3gramTokeniser": 3, "Q4gramTokeniser": 4, "Q5gramTokeniser": 5,
        "Q6gramTokeniser": 6}

JACCARD_ANCHORS = [("night", "nacht", 0.43), ("abcdefgh", "a", 0.13), ("abcdefgh", "abc", 0.38), ("aaa", "a", 1.0),
                   ("abc", "xyz", 0.0), ("", "a", 0.0)]
COSINE_ANCHORS = [("john smith", "john smyth", 0.5000000000000001), ("a a b", "a b b", 0.20000000000000018),
                  ("jo oh hn", "jo on", 0.5917517095361371)]
COSINE_SELF = [("john smith", 2.220446049250313e-16), ("a b c", -2.220446049250313e-16)]
QGRAM_EXAMPLES = [("john", 2, "jo oh hn"), ("ab", 3, "ab")]


# ---- SQL three-valued logic over the values ---------------------------------------------------------------------
def value_test(v, op, t):
    """`v op t` for a value test; None (NULL) when the value is (a NULL operand, a blank text under cosine)."""
    if v is None:
        return None
    return {"<": v < t, "<=": v <= t, ">": v > t, ">=": v >= t, "=": v == t, "!=": v != t}[op]


def case_level(whens, else_level):
    """First WHEN whose predicate is TRUE (FALSE and NULL fall through)."""
    for pred, level in whens:
        if pred is True:
            return level
    return else_level


# ---- strings for the device tests --------------------------------------------------------------------------------
LENGTH_EDGES = (63, 64, 65, 1023, 1024, 1025, 1500)  # around MAXU and SLOW_LIMIT, and well past


def words(rng, n_units, alphabet="abcdef", longest=6):
    """A text of exactly n_units units: words of 1..longest letters over a small alphabet, one space between them."""
    out = []
    left = n_units
    while left > 0:
        k = min(left, rng.randint(1, longest))
        out.append("".join(rng.choice(alphabet) for _ in range(k)))
        left -= k
        if left > 1:
            left -= 1
        elif left == 1:  # no room for a space and a letter both: one more letter on the last word
            out[-1] += rng.choice(alphabet)
            left = 0
    s = " ".join(out)
    assert len(s) == n_units, (len(s), n_units)
    return s


def distinct(n, start=0x100):
    """n distinct BMP units, none a surrogate, a word character or whitespace."""
    out, c = [], start
    while len(out) < n:
        if not (0xD800 <= c < 0xE000) and c not in WHITESPACE:
            out.append(chr(c))
        c += 1
    return "".join(out)


def value_pairs():
    """About 400 pairs for the bulk functions: the issue's list of shapes."""
    rng = random.Random(20240601)
    p = [(a, b) for a, b, _ in JACCARD_ANCHORS] + [(a, b) for a, b, _ in COSINE_ANCHORS]
    p += [(s, s) for s, _ in COSINE_SELF]
    p += [("", ""), ("", "abc"), ("abc", ""), ("abc def", "abc def"), ("john smith jones", "john smith jones"),
          ("abc", "xyz"), ("abc def", "uvw xyz"), ("a" * 30, "a"), ("a" * 30, "a" * 7), ("a" * 30, "b" * 30)]
    # |A n B| / |A u B| times 100 ends in exactly .5
    base8 = "abcdefgh"
    p += [(base8, base8[:k]) for k in (1, 3, 5, 7)] + [(base8[:k] * 2, base8) for k in (1, 3, 5, 7)]
    d200 = distinct(200)
    p += [(d200, d200[17]), (d200[17] * 3, d200)]
    # surrogate pairs: two units each; the high units are shared, the low units differ
    p += [(SURROGATE, SURROGATE), (SURROGATE + "ab", "\U0001F601" + "ab"), ("ab" + SURROGATE + "cd", "ab cd"),
          (SURROGATE * 3, "\U0001F601\U0001F602")]
    # no word character; blank texts
    p += [("!!!", "abc"), ("abc", "!!!"), ("!!!", "???"), ("éè", "éè"), ("-- --", "a -- b")]
    p += [(" ", "abc"), ("abc", "   "), ("\t", "abc"), ("\t \n", "abc"), ("\u3000", "abc"), ("abc", "\u3000\u3000"),
          ("\u2003\u2028", "abc"), (" ", " ")]
    p += [("\u00a0", "abc"), ("\u2007", "abc"), ("\u202f", "a b")]  # no-break spaces: not whitespace, no token either
    # tokens repeated up to 40 times; one token of 70 units
    for k in (2, 5, 17, 40):
        p += [(" ".join(["ab"] * k), "ab cd"), (" ".join(["ab"] * k + ["cd"] * 3), " ".join(["cd"] * k + ["ab"]))]
    t70 = "".join(rng.choice("abcdef") for _ in range(70))
    p += [(t70, t70), (t70, t70[:69]), (t70 + " x", "x " + t70), (t70, t70[:35] + " " + t70[35:])]
    p += [("Ab ab AB", "ab"), ("a_b a-b", "a_b a b"), ("x1 x2 x1", "x1")]
    # the length edges, on either side and on both
    for n in LENGTH_EDGES:
        long1, long2 = words(rng, n), words(rng, n)
        p += [(long1, words(rng, 12)), (words(rng, 12), long1), (long1, long2), (long1, long1)]
        d = distinct(n)
        p += [(d, d[5:40]), (d[3:30], d), (d, distinct(n, 0x100 + n // 2))]
    p += [(distinct(1500), words(rng, 1500)), (words(rng, 64), distinct(65))]
    # random strings over a 6-letter alphabet with spaces
    while len(p) < 400:
        a = "".join(rng.choice("abcdef ") for _ in range(rng.randint(1, 40)))
        b = "".join(rng.choice("abcdef ") for _ in range(rng.randint(1, 40)))
        p.append((a, b))
    return p
