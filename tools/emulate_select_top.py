"""Host emulation of spk_select_top / spk_select_top_of (numpy, no GPU): the key, the radix select's passes on
patterns and on pairs, and the two-class emit rule.

The device keeps the first k eligible pairs in the order

    ascending:   score(a) < score(b), or equal scores (two NULLs are equal) and ordinal(a) < ordinal(b)
    descending:  the same with score(a) > score(b)
    first:       ordinal(a) < ordinal(b)

with NULL (NaN) smaller than every number and -0.0 equal to +0.0.  Both score orders become "smallest key first" under

    image(s):    0 for a NULL; else with u the score's 64 bits and -0.0 read as +0.0:  ~u if u's sign bit is set,
                 u | 2^63 otherwise
    key(s):      image(s) ascending, ~image(s) descending

A radix select finds the key of the k-th element, most significant byte first: pass d histograms byte d of the keys
that agree with the prefix in the bytes above it, weighted (k_top_pat_hist: the elements are the eligible patterns,
the weights their pairs) or not (k_topof_hist: the elements are the survivors); the pick (k_top_pick) takes the byte
at which the running count reaches what is left of k, extends the prefix by it and reduces the remainder by the count
below it.  Pass 0 counts every element, so it also gives the total, and settles k = 0 (none kept) and k >= total (all
kept).  After 8 passes the prefix is the cut key, the remainder r is how many elements at the cut are kept and the
last chosen bin is how many there are.  The emit rule (k_top / k_topof): an element above the cut (key < cut) is kept;
one at the cut is kept iff fewer than r elements at the cut precede it in ordinal order; a chunk's output starts at
(above before it) + min(at the cut before it, r).  `top_by_passes` restates exactly that; `top_by_definition` sorts.

    python tools/emulate_select_top.py            # the two agree on random and crafted scores
"""
import numpy as np

MASK = (1 << 64) - 1
FIRST, ASC, DESC = 0, 1, 2          # SPK_TOP_FIRST, SPK_TOP_ASC, SPK_TOP_DESC
OUT, ABOVE, AT = 0, 1, 2            # spk_select.hip: TOP_OUT, TOP_ABOVE, TOP_AT
ACTIVE, ALL, EMPTY, FIRSTK = 0, 1, 2, 3   # TS_FLAG
PASSES, DIGITS = 8, 256
CHUNK = 2048                        # SEL_CHUNK


def image(score):
    """The order-preserving image of every score, uint64: 0 for NaN."""
    s = np.array(score, dtype=np.float64, copy=True).reshape(-1)
    null = np.isnan(s)
    s[s == 0.0] = 0.0  # -0.0 -> +0.0
    u = s.view(np.uint64)
    neg = (u >> np.uint64(63)) != 0
    img = np.where(neg, ~u, u | np.uint64(1 << 63))
    return np.where(null, np.uint64(0), img).astype(np.uint64)


def key(score, order):
    """The key the select runs on: smallest first in the order asked for."""
    img = image(score)
    return ~img if order == DESC else img


def key_score(k, order):
    """The score a key stands for (NaN: NULL)."""
    img = (~np.uint64(k)) if order == DESC else np.uint64(k)
    if int(img) == 0:
        return float("nan")
    u = (img & np.uint64((1 << 63) - 1)) if (int(img) >> 63) else ~img
    return float(np.array([u], dtype=np.uint64).view(np.float64)[0])


def _cut_figures(score, eligible, kept, order, k):
    """(eligible, kept, cut score or None, tied, tied_kept) of a kept mask under the definition."""
    score = np.asarray(score, dtype=np.float64)
    n_el, n_kept = int(eligible.sum()), int(kept.sum())
    if order == FIRST or k == 0 or k >= n_el:
        return n_el, n_kept, None, 0, 0
    kk = key(score, order)
    cut = kk[kept].max()
    at = eligible & (kk == cut)
    s = key_score(cut, order)
    return n_el, n_kept, (None if s != s else s), int(at.sum()), int((at & kept).sum())


def top_by_definition(score, eligible, order, k):
    """(kept mask, figures): the first min(k, eligible) eligible elements (given in ascending ordinal) by a stable sort
    with NULL lowest."""
    score = np.asarray(score, dtype=np.float64)
    eligible = np.asarray(eligible, dtype=bool)
    idx = np.nonzero(eligible)[0]
    if order != FIRST:
        s = score[idx]
        null = np.isnan(s)
        val = np.where(null, -np.inf, s) + 0.0
        pos = np.arange(len(idx))
        o = np.lexsort((pos, val, ~null)) if order == ASC else np.lexsort((pos, -val, null))
        idx = idx[o]
    kept = np.zeros(len(score), dtype=bool)
    kept[idx[:min(int(k), len(idx))]] = True
    return kept, _cut_figures(score, eligible, kept, order, int(k))


def pick_digit(hist, k):
    """(digit, elements below it, elements in it): the first digit at which the running count of `hist` reaches k >= 1."""
    run = np.cumsum(hist.astype(np.int64))
    g = int(np.searchsorted(run, k, side="left"))
    return g, (int(run[g - 1]) if g else 0), int(hist[g])


def radix_select(keys, weights, k):
    """(flag, cut key, remainder, tied, total) of the weighted select over `keys` (uint64) with integer `weights`."""
    keys = np.asarray(keys, dtype=np.uint64)
    weights = np.asarray(weights, dtype=np.int64)
    prefix, remain, tied, flag, total = np.uint64(0), 0, 0, ACTIVE, 0
    for d in range(PASSES):
        shift = np.uint64(56 - 8 * d)
        take = weights > 0
        if d > 0:
            if flag != ACTIVE:
                break
            above = shift + np.uint64(8)
            take = take & ((keys >> above) == (prefix >> above))
        hist = np.bincount(((keys[take] >> shift) & np.uint64(255)).astype(np.int64), weights=weights[take],
                           minlength=DIGITS).astype(np.int64)
        if d == 0:
            total = int(hist.sum())
            remain = min(int(k), total)
            flag = EMPTY if remain == 0 else ALL if remain == total else ACTIVE
            if flag != ACTIVE:
                break
        g, below, inside = pick_digit(hist, remain)
        prefix |= np.uint64(g) << shift
        remain -= below
        if d == PASSES - 1:
            tied = inside
    return flag, prefix, remain, tied, total


def classes(keys, eligible, flag, cut):
    """The class of every element: k_top_classes / k_topof's top_class."""
    keys = np.asarray(keys, dtype=np.uint64)
    if flag == ALL:
        cls = np.full(len(keys), ABOVE)
    elif flag == EMPTY:
        cls = np.full(len(keys), OUT)
    elif flag == FIRSTK:
        cls = np.full(len(keys), AT)
    else:
        cls = np.where(keys < cut, ABOVE, np.where(keys == cut, AT, OUT))
    return np.where(np.asarray(eligible, dtype=bool), cls, OUT)


def emit(cls, r, chunk=CHUNK):
    """(kept mask, output position of every kept element): the count / scan / emit with two counts per chunk."""
    n = len(cls)
    n_chunks = (n + chunk - 1) // chunk
    above = np.zeros(n_chunks + 1, dtype=np.int64)
    at = np.zeros(n_chunks + 1, dtype=np.int64)
    for c in range(n_chunks):
        part = cls[c * chunk:(c + 1) * chunk]
        above[c] = (part == ABOVE).sum()
        at[c] = (part == AT).sum()
    above_off = np.concatenate([[0], np.cumsum(above)[:-1]])
    at_off = np.concatenate([[0], np.cumsum(at)[:-1]])
    kept = np.zeros(n, dtype=bool)
    where = np.full(n, -1, dtype=np.int64)
    for c in range(n_chunks):
        run = above_off[c] + min(at_off[c], r)
        at_run = at_off[c]
        for i in range(c * chunk, min((c + 1) * chunk, n)):
            keep = cls[i] == ABOVE or (cls[i] == AT and at_run < r)
            at_run += cls[i] == AT
            if keep:
                kept[i] = True
                where[i] = run
                run += 1
        assert run == above_off[c + 1] + min(at_off[c + 1], r)
    return kept, where


def _figures(order, k, flag, cut, remain, tied, eligible_total, kept):
    if order == FIRST or flag != ACTIVE:
        return eligible_total, int(kept.sum()), None, 0, 0
    s = key_score(cut, order)
    return eligible_total, int(kept.sum()), (None if s != s else s), tied, remain


def top_of_by_passes(score, order, k, chunk=CHUNK):
    """spk_select_top_of over survivors with stored scores: (kept mask, figures)."""
    score = np.asarray(score, dtype=np.float64)
    n = len(score)
    every = np.ones(n, dtype=bool)
    if order == FIRST:
        kept, _ = emit(classes(np.zeros(n, dtype=np.uint64), every, FIRSTK, 0), int(k), chunk)
        return kept, (n, int(kept.sum()), None, 0, 0)
    keys = key(score, order)
    flag, cut, remain, tied, total = radix_select(keys, np.ones(n, dtype=np.int64), k)
    kept, _ = emit(classes(keys, every, flag, cut), remain if flag == ACTIVE else 0, chunk)
    return kept, _figures(order, k, flag, cut, remain, tied, total, kept)


def top_by_passes(code, pattern_score, pattern_eligible, order, k, chunk=CHUNK):
    """spk_select_top over pairs with pattern codes `code`: the score and the eligibility are functions of the
    pattern.  (kept mask, figures)."""
    code = np.asarray(code, dtype=np.int64)
    pattern_score = np.asarray(pattern_score, dtype=np.float64)
    pattern_eligible = np.asarray(pattern_eligible, dtype=bool)
    n_pat = len(pattern_score)
    if order == FIRST:
        tab = classes(np.zeros(n_pat, dtype=np.uint64), pattern_eligible, FIRSTK, 0)
        kept, _ = emit(tab[code], int(k), chunk)
        return kept, (int(pattern_eligible[code].sum()), int(kept.sum()), None, 0, 0)
    cnt = np.bincount(code, minlength=n_pat).astype(np.int64)          # k_top_hist
    keys = key(pattern_score, order)
    flag, cut, remain, tied, total = radix_select(keys, np.where(pattern_eligible, cnt, 0), k)
    tab = classes(keys, pattern_eligible, flag, cut)                    # k_top_classes
    kept, _ = emit(tab[code], remain if flag == ACTIVE else 0, chunk)   # k_top
    return kept, _figures(order, k, flag, cut, remain, tied, total, kept)


def _selftest():
    rng = np.random.Generator(np.random.PCG64(1))
    for n in (0, 1, 63, 64, 65, 4097):
        for distinct in (3, 600):
            values = np.concatenate([rng.random(distinct), [np.nan, -0.0, 0.0]])
            code = rng.integers(0, len(values), n)
            score = values[code]
            el = rng.random(len(values)) < 0.8
            for order in (FIRST, ASC, DESC):
                for k in (0, 1, n // 2, n, n + 5):
                    a = top_by_definition(score, el[code], order, k)
                    b = top_by_passes(code, values, el, order, k, chunk=64)
                    assert np.array_equal(a[0], b[0]) and a[1] == b[1], (n, distinct, order, k, a[1], b[1])
                    a = top_by_definition(score, np.ones(n, dtype=bool), order, k)
                    b = top_of_by_passes(score, order, k, chunk=64)
                    assert np.array_equal(a[0], b[0]) and a[1] == b[1], (n, distinct, order, k, a[1], b[1])
        print(f"n = {n}: passes == definition")


if __name__ == "__main__":
    _selftest()
