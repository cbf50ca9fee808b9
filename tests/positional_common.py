"""Host restatement of the positional Levenshtein sketch (k_pos_rows, spk_ctx.hip) and of the bound ev_lev
(spk_filter.hip) derives from two of them, with the string generators the host and GPU tests share.

A row of n code points splits into the halves [0, ceil(n/2)) and [ceil(n/2), n).  Each half counts its units
in 30 buckets (a letter each, case folded; digits by bit 0; every other unit by bit 1) with 2-bit saturating
counts (3 = three or more).  The 16-byte row is  length | half-1 low plane << 8 | half-1 high plane << 38 |
half-2 low plane << 68 | half-2 high plane << 98;  length 255 = NULL, 254 = no sketch (254 or more code
points, or a surrogate pair)."""
import numpy as np

NB = 30
MASK = (1 << NB) - 1
LEN_NULL, LEN_NONE = 255, 254


def pos_bucket(u):
    if 97 <= u <= 122:
        return u - 97
    if 65 <= u <= 90:
        return u - 65
    if 48 <= u <= 57:
        return 26 + (u & 1)
    return 28 + ((u >> 1) & 1)


def pos_row(s):
    """The 128-bit row of a string as an int."""
    if s is None:
        return LEN_NULL
    n = len(s)
    if n >= LEN_NONE or any(ord(c) >= 0x10000 for c in s):
        return LEN_NONE
    h = (n + 1) // 2
    row = n
    for half, part in enumerate((s[:h], s[h:])):
        cnt = [0] * NB
        for c in part:
            b = pos_bucket(ord(c))
            cnt[b] = min(cnt[b] + 1, 3)
        lo = sum((c & 1) << b for b, c in enumerate(cnt))
        hi = sum((c >> 1) << b for b, c in enumerate(cnt))
        row |= (lo << (8 + 60 * half)) | (hi << (38 + 60 * half))
    return row


def row_counts(row):
    """(length, counts of half 1, counts of half 2) of a row with a sketch."""
    out = []
    for half in range(2):
        lo = (row >> (8 + 60 * half)) & MASK
        hi = (row >> (38 + 60 * half)) & MASK
        out.append(np.array([((lo >> b) & 1) + 2 * ((hi >> b) & 1) for b in range(NB)], dtype=np.int64))
    return row & 255, out[0], out[1]


def inter_ub(ca, cb, la, lb):
    """Upper bound of the multiset intersection of two strings of la / lb units from their saturating bucket
    counts.  The units of a that b cannot match number at least Σ max(0, ca - cb) over the stored counts (a
    bucket saturated in b hides at least three units there, more than an unsaturated count of a; one saturated
    in a has at least three; one saturated in both adds 0), so the intersection is at most
    la - Σ (ca - min(ca, cb)), and likewise from b's side."""
    mins = int(np.minimum(ca, cb).sum())
    return mins + min(la - int(ca.sum()), lb - int(cb.sum()))


def two_segment_term(A1, A2, B1, B2, I1, I2, j):
    """The issue's summand at the split point j of b (a1 against b[0, j), a2 against b[j, |b|))."""
    B = B1 + B2
    d = j - B1
    return (max(A1, j) - min(I1 + max(d, 0), A1, j)) + (max(A2, B - j) - min(I2 + max(-d, 0), A2, B - j))


def two_segment_brute(A1, A2, B1, B2, I1, I2):
    return min(two_segment_term(A1, A2, B1, B2, I1, I2, j) for j in range(B1 + B2 + 1))


def _side(Ax, Bx, Ix, Ay, By, Iy):
    """min over d in [0, By] of  max(Ax, Bx + d) - min(Ix + d, Ax)  +  max(Ay, By - d) - min(Iy, By - d).
    With Ix <= min(Ax, Bx) and Iy <= min(Ay, By) the two summands are max(Ax - Ix - d, Bx - Ix, Bx - Ax + d) and
    max(By - Iy - d, Ay - Iy, Ay - By + d): each falls, stays flat on [Ax - Bx, Ax - Ix] / [By - Ay, By - Iy], then
    rises, all with slope one, so the sum is convex and smallest where the flats meet or between them."""
    d = min(max(Ax - Bx, By - Ay), Ax - Ix, By - Iy)
    d = min(max(d, 0), By)
    return max(Ax - Ix - d, Bx - Ix, Bx - Ax + d) + max(By - Iy - d, Ay - Iy, Ay - By + d)


def two_segment_closed(A1, A2, B1, B2, I1, I2):
    return min(_side(A1, B1, I1, A2, B2, I2), _side(A2, B2, I2, A1, B1, I1))


def halves(n):
    return (n + 1) // 2, n // 2


def pos_terms(ra, rb):
    """(length gap, whole-string bag bound, two-segment bound, (A1, A2, B1, B2, I1, I2)) of two rows with sketches."""
    na, a1, a2 = row_counts(ra)
    nb, b1, b2 = row_counts(rb)
    (A1, A2), (B1, B2) = halves(na), halves(nb)
    I1, I2 = inter_ub(a1, b1, A1, B1), inter_ub(a2, b2, A2, B2)
    whole = max(na, nb) - inter_ub(np.minimum(a1 + a2, 3), np.minimum(b1 + b2, 3), na, nb)
    return abs(na - nb), whole, two_segment_closed(A1, A2, B1, B2, I1, I2), (A1, A2, B1, B2, I1, I2)


def pos_bound(a, b):
    """The filter's lower bound of lev(a, b) from the two rows; None when a row has no sketch (or is NULL)."""
    ra, rb = pos_row(a), pos_row(b)
    if (ra & 255) >= LEN_NONE or (rb & 255) >= LEN_NONE:
        return None
    gap, whole, seg, _ = pos_terms(ra, rb)
    return max(gap, whole, seg)


# ---- the whole-string sketch the positional one replaces (sketch_bucket / sketch_inter_ub, spk_internal.h) ----
def unit_bucket(u):
    if u < 128:
        if 97 <= u <= 122:
            return u - 97
        if 65 <= u <= 90:
            return u - 65
        if 48 <= u <= 57:
            return 26 + (u - 48) % 3
        return 29 + u % 3
    return (((u * 2654435761) & 0xFFFFFFFF) >> 16) & 31


def unit_bound(a, b):
    ca, cb = np.zeros(32, dtype=np.int64), np.zeros(32, dtype=np.int64)
    for s, c in ((a, ca), (b, cb)):
        for ch in s:
            k = unit_bucket(ord(ch))
            c[k] = min(c[k] + 1, 3)
    return max(abs(len(a) - len(b)), max(len(a), len(b)) - inter_ub(ca, cb, len(a), len(b)))


def ratio_cut(a, b, t=0.3):
    """Largest distance v with v / ((la + lb) / 2) <= t in fp64 (the ratio templates' test)."""
    den = (len(a) + len(b)) / 2.0
    v = -1
    while den > 0 and (v + 1) / den <= t:
        v += 1
    return v


# ---- generators ------------------------------------------------------------------------------------------
_DOMAINS = ["example.com", "mail.co.uk", "post.net", "inbox.org", "webmail.com", "fastmail.io", "letters.uk",
            "corp.example", "home.net", "uni.ac.uk"]
_SYL = ["ba", "chen", "dro", "fi", "gru", "ha", "jo", "kai", "lea", "mou", "ny", "pe", "ri", "sha", "sto", "thu", "vi",
        "wa", "ye", "zo", "nd", "ll", "rt", "x", "ck"]


def _name(rng, lo, hi):
    while True:
        w = "".join(_SYL[int(i)] for i in rng.integers(0, len(_SYL), int(rng.integers(1, 5))))
        if lo <= len(w) <= hi:
            return w


def email_pairs(rng, n):
    """first.surname##@domain pairs that share the surname (the pairs a surname blocking rule emits)."""
    out = []
    for _ in range(n):
        sur = _name(rng, 3, 14)
        e = [f"{_name(rng, 3, 12)}.{sur}{int(rng.integers(1, 100)):02d}@{_DOMAINS[int(rng.integers(len(_DOMAINS)))]}"
             for _ in range(2)]
        out.append((e[0], e[1]))
    return out


_ALPHA = list("abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789 ,.-@_") + list("éßüñçÿ")


def _rand(rng, k, alpha=_ALPHA):
    return "".join(alpha[int(i)] for i in rng.integers(0, len(alpha), k))


def adversarial_pairs(rng, n):
    """Random pairs of every shape the bound has a case for: short and odd lengths, letters repeated past the
    counters' saturation in one half (on one side and on both), Latin-1 units, front insertions that shift the
    midpoint, swapped halves, related strings a few edits apart, and rows that get no sketch."""
    out = []
    for i in range(n):
        kind = i % 10
        if kind == 0:  # lengths 0, 1, 2 and odd lengths
            out.append((_rand(rng, int(rng.integers(0, 4))), _rand(rng, int(rng.choice([0, 1, 2, 3, 5, 7, 9])))))
        elif kind == 1:  # one letter >= 3 times in one half of a; in b's too every other time
            c = _ALPHA[int(rng.integers(26))]
            a = c * int(rng.integers(3, 7)) + _rand(rng, int(rng.integers(4, 12)))
            b = (c * int(rng.integers(3, 7)) if rng.integers(2) else "") + _rand(rng, int(rng.integers(4, 14)))
            if rng.integers(2):
                a, b = a[::-1], b[::-1]  # the run in the second half
            out.append((a, b))
        elif kind == 2:  # Latin-1 units
            out.append((_rand(rng, int(rng.integers(1, 20)), list("éßüñçÿabc")), _rand(rng, int(rng.integers(1, 20)), list("éßüñçÿabc"))))
        elif kind == 3:  # k units inserted at the front, k = 1 .. 8
            a = _rand(rng, int(rng.integers(2, 30)))
            out.append((a, _rand(rng, 1 + (i // 10) % 8) + a))
        elif kind == 4:  # halves swapped
            a = _rand(rng, int(rng.integers(2, 30)))
            h = (len(a) + 1) // 2
            out.append((a, a[h:] + a[:h]))
        elif kind == 5:  # a few edits apart
            a = _rand(rng, int(rng.integers(5, 40)))
            b = list(a)
            for _ in range(int(rng.integers(1, 6))):
                p = int(rng.integers(len(b) + 1))
                op = int(rng.integers(3))
                if op == 0:
                    b.insert(p, _rand(rng, 1))
                elif b and op == 1:
                    del b[min(p, len(b) - 1)]
                elif b:
                    b[min(p, len(b) - 1)] = _rand(rng, 1)
            out.append((a, "".join(b)))
        elif kind == 6:  # unrelated, unequal lengths
            out.append((_rand(rng, int(rng.integers(0, 60))), _rand(rng, int(rng.integers(0, 60)))))
        elif kind == 7:  # small alphabets: many saturated buckets
            out.append((_rand(rng, int(rng.integers(1, 40)), list("ab1.")), _rand(rng, int(rng.integers(1, 40)), list("ab1."))))
        elif kind == 8:  # no sketch: a surrogate pair, or 254 code points and more
            a = _rand(rng, int(rng.integers(1, 20)))
            out.append((a + "\U0001F600" if rng.integers(2) else _rand(rng, int(rng.integers(254, 260))), a))
        else:  # the longest rows that still get one
            out.append((_rand(rng, int(rng.integers(250, 254))), _rand(rng, int(rng.integers(240, 254)))))
    return out


def threshold_pairs(rng, n, t=0.3):
    """Pairs whose distance is exactly the ratio cut and one more: substitutions by units the string lacks,
    all in the first half, all in the second, or as a front insertion."""
    out = []
    fresh = "0123456789"
    for i in range(n):
        a = _rand(rng, int(rng.integers(8, 40)), list("abcdefghijklmnopqrstuvwxyz"))
        where = i % 3
        for extra in (0, 1):
            if where == 2:  # front insertion of k units: the cut of the lengthened pair
                k = 0
                while ratio_cut(a, "x" * (len(a) + k + 1), t) >= k + 1:
                    k += 1
                k += extra
                b = "".join(fresh[(q + i) % 10] for q in range(k)) + a
            else:
                k = min(ratio_cut(a, a, t) + extra, len(a) // 2)
                pos = range(k) if where == 0 else range(len(a) - k, len(a))
                b = list(a)
                for q in pos:
                    b[q] = fresh[(q + i) % 10]
                b = "".join(b)
            out.append((a, b))
    return out
