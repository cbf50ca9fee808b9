"""Shared by the tests of labels given as a table of pairs (spk_label_pairs_histogram and the frames above it).

Expected counts never go through a hash: a Python dict of canonical (lo, hi) -> state, then
np.bincount(state * n_patterns + code).  The hash and the capacity rule that include/splink_hip.h documents are
restated here only to construct keys that collide (home_slot); no expectation is computed with them."""
import numpy as np

M64 = (1 << 64) - 1
UNKNOWN = 2


def n_patterns(levels):
    return int(np.prod([L + 1 for L in levels]))


def codes_of(g, levels):
    stride = np.cumprod([1] + [L + 1 for L in levels[:-1]])
    return ((np.asarray(g, dtype=np.int64).reshape(-1, len(levels)) + 1) * stride).sum(axis=1)


def make_ctx(rows_l, rows_r, g, levels, n0, n1=None):
    """A context with loaded pairs and levels, as test_gpu_labels.py::make_ctx makes one; n1: link_only."""
    from splink_amd import _native as N
    c = N.Context(0)
    if n1 is not None:
        c.set_link_type(N.LINK_TYPES["link_only"])
        c.table_create(1, n1, 1)
    c.table_create(0, n0, 1)
    c.pairs_load(np.asarray(rows_l, dtype=np.int32), np.asarray(rows_r, dtype=np.int32))
    c.gammas_load(levels, np.asarray(g, dtype=np.int8).reshape(len(rows_l), len(levels)))
    return c


def random_case(rng, P, levels, n0, n1=None, groups=40, nulls=0.15):
    """test_gpu_labels.random_case's recipe: random rows, random levels, label ids per record with NULLs."""
    rows_l = rng.integers(0, n0, P)
    rows_r = rng.integers(0, n0 if n1 is None else n1, P)
    g = np.stack([rng.integers(-1, L, P) for L in levels], axis=1) if P else np.zeros((0, len(levels)), np.int64)
    ids0 = rng.integers(0, groups, n0).astype(np.int64)
    ids0[rng.random(n0) < nulls] = -rng.integers(1, 1 << 40)  # any negative id is NULL
    ids1 = None
    if n1 is not None:
        ids1 = rng.integers(0, groups, n1).astype(np.int64)
        ids1[rng.random(n1) < nulls] = -1
    return rows_l, rows_r, g, ids0, ids1


def m_u(levels, rng):
    tot = sum(levels)
    return rng.random(tot) * 0.9 + 0.05, rng.random(tot) * 0.9 + 0.05


def canonical(l, r, one_table):
    l, r = int(l), int(r)
    return (min(l, r), max(l, r)) if one_table else (l, r)


def expected(rows_l, rows_r, g, levels, lab_l, lab_r, is_match, one_table):
    """(counts int64 [3, n_patterns], label_code int64 [n_labels]) by dict lookup and bincount."""
    truth = {canonical(a, b, one_table): (i, int(y)) for i, (a, b, y) in enumerate(zip(lab_l, lab_r, is_match))}
    assert len(truth) == len(lab_l), "the test's own labels repeat a pair"
    code = codes_of(g, levels) if len(rows_l) else np.zeros(0, dtype=np.int64)
    rows_l, rows_r = np.asarray(rows_l, dtype=np.int64), np.asarray(rows_r, dtype=np.int64)
    lo, hi = (np.minimum(rows_l, rows_r), np.maximum(rows_l, rows_r)) if one_table else (rows_l, rows_r)
    # the dict is asked once per distinct candidate pair
    distinct, inverse = np.unique(lo * (1 << 32) + hi, return_inverse=True)
    hits = [truth.get((int(k) >> 32, int(k) & 0xFFFFFFFF)) for k in distinct]
    state = np.array([UNKNOWN if h is None else h[1] for h in hits], dtype=np.int64)[inverse.reshape(-1)]
    label = np.array([-1 if h is None else h[0] for h in hits], dtype=np.int64)[inverse.reshape(-1)]
    label_code = np.full(len(lab_l), -1, dtype=np.int64)
    np.maximum.at(label_code, label[label >= 0], code[label >= 0])
    n_pat = n_patterns(levels)
    return np.bincount(state * n_pat + code, minlength=3 * n_pat).reshape(3, n_pat), label_code


def distinct_pairs(rng, n, n0, n1=None, avoid=()):
    """n distinct labelled pairs of random rows, canonically distinct from each other and from `avoid`; never l == r
    on one table."""
    one_table = n1 is None
    seen = {canonical(a, b, one_table) for a, b in avoid}
    out = []
    while len(out) < n:
        a, b = int(rng.integers(0, n0)), int(rng.integers(0, n0 if one_table else n1))
        if (one_table and a == b) or canonical(a, b, one_table) in seen:
            continue
        seen.add(canonical(a, b, one_table))
        out.append((a, b))
    return out


def mixed_labels(rng, n, rows_l, rows_r, n0, n1=None):
    """n labels, about half of them candidate pairs (where the pair set has that many distinct ones without l == r),
    the rest pairs that are not candidates; random order on one table; random match flags."""
    one_table = n1 is None
    a, b = np.asarray(rows_l, dtype=np.int64), np.asarray(rows_r, dtype=np.int64)
    lo, hi = (np.minimum(a, b), np.maximum(a, b)) if one_table else (a, b)
    every = [(int(k) >> 32, int(k) & 0xFFFFFFFF) for k in np.unique(lo * (1 << 32) + hi)]
    keys = [k for k in every if not (one_table and k[0] == k[1])]
    take = min(n // 2, len(keys))
    picked = [keys[i] for i in rng.permutation(len(keys))[:take]]
    rest = []
    seen = set(every)
    while len(picked) + len(rest) < n:
        a, b = int(rng.integers(0, n0)), int(rng.integers(0, n0 if one_table else n1))
        if (one_table and a == b) or canonical(a, b, one_table) in seen:
            continue
        seen.add(canonical(a, b, one_table))
        rest.append((a, b))
    pairs = picked + rest
    pairs = [pairs[i] for i in rng.permutation(len(pairs))] if pairs else pairs
    if one_table:  # either order of a labelled pair
        pairs = [(b, a) if rng.random() < 0.5 else (a, b) for a, b in pairs]
    lab_l = np.array([p[0] for p in pairs], dtype=np.int32)
    lab_r = np.array([p[1] for p in pairs], dtype=np.int32)
    return lab_l, lab_r, rng.integers(0, 2, len(pairs)).astype(np.uint8), take


# ---- the documented table, restated to construct colliding keys only ------------------------------------------------
def fmix64(k):
    k ^= k >> 33
    k = (k * 0xff51afd7ed558ccd) & M64
    k ^= k >> 33
    k = (k * 0xc4ceb9fe1a85ec53) & M64
    k ^= k >> 33
    return k


def capacity_of(n_labels):
    cap = 64
    while cap < 2 * n_labels:
        cap *= 2
    return cap


def home_slot(lo, hi, capacity):
    return fmix64((int(lo) << 31) | int(hi)) & (capacity - 1)
