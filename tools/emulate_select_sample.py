"""Host emulation of spk_select_sample (numpy, no GPU): the key, the strata, and the radix select's passes.

The device keeps, per stratum of match_probability, the quota[b] eligible pairs with the smallest keys

    mix(x):        x ^= x >> 30; x *= 0xBF58476D1CE4E5B9; x ^= x >> 27; x *= 0x94D049BB133111EB; x ^= x >> 31
    key(seed, p):  mix(mix(seed) + 0x9E3779B97F4A7C15 * (p + 1))        (64-bit wrap-around, p the pair's ordinal)

and finds the quota[b]-th smallest key of every stratum without storing anything per pair: 8 passes, most
significant byte first.  Pass d histograms byte d of the keys that agree with their stratum's prefix in the bytes
above it (k_sample<SMP_HIST>); the pick (k_sample_pick) takes the byte at which the running count reaches what is left
of the quota, extends the prefix by it and reduces the remainder by the count below it.  Pass 0 counts every key, so
it also gives the population, and settles the strata that need no selecting: population <= quota (kept whole,
threshold all ones) and quota 0 (none kept).  `select_by_passes` restates exactly that; `select_by_definition` sorts.

    python tools/emulate_select_sample.py            # the two agree on random and crafted keys
"""
import numpy as np

MASK = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15
MAX_STRATA = 64   # SPK_SAMPLE_MAX_STRATA
NONE = 255        # spk_select.hip: SMP_NONE, the stratum of a pair that is never sampled
PASSES, DIGITS = 8, 256


def mix(x):
    """mix() over a numpy uint64 array (or anything that converts to one); wraps like the device's arithmetic."""
    x = np.array(x, dtype=np.uint64, copy=True)
    with np.errstate(over="ignore"):
        x ^= x >> np.uint64(30)
        x *= np.uint64(0xBF58476D1CE4E5B9)
        x ^= x >> np.uint64(27)
        x *= np.uint64(0x94D049BB133111EB)
        x ^= x >> np.uint64(31)
    return x


def keys(seed, ordinals):
    """key(seed, p) of every pair ordinal p, uint64."""
    p = np.asarray(ordinals).astype(np.uint64)
    with np.errstate(over="ignore"):
        return mix(mix(np.uint64(int(seed) & MASK)) + np.uint64(GOLDEN) * (p + np.uint64(1)))


def strata_of(mp, edges):
    """Stratum of every score under ascending `edges` (left-closed, the last right-closed too); NONE for a NaN or a
    score outside [edges[0], edges[-1]].  int64."""
    mp = np.asarray(mp, dtype=np.float64)
    edges = np.asarray(edges, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        inside = (mp >= edges[0]) & (mp <= edges[-1])
    b = np.searchsorted(edges[1:-1], np.where(inside, mp, edges[0]), side="right")  # inner edges <= x
    return np.where(inside, b, NONE).astype(np.int64)


def select_by_definition(key, stratum, quota):
    """(kept mask, population, kept count): per stratum the min(quota, population) smallest keys, by sorting."""
    key = np.asarray(key, dtype=np.uint64)
    stratum = np.asarray(stratum, dtype=np.int64)
    kept = np.zeros(len(key), dtype=bool)
    pop = np.zeros(len(quota), dtype=np.int64)
    cnt = np.zeros(len(quota), dtype=np.int64)
    for b, q in enumerate(quota):
        idx = np.nonzero(stratum == b)[0]
        pop[b] = len(idx)
        take = idx[np.argsort(key[idx], kind="stable")[:int(q)]]
        kept[take] = True
        cnt[b] = len(take)
    return kept, pop, cnt


def pick_digit(hist, k):
    """(digit, keys below it): the first digit at which the running count of `hist` [256] reaches k >= 1."""
    run = np.cumsum(hist.astype(np.int64))
    g = int(np.searchsorted(run, k, side="left"))
    return g, int(run[g - 1]) if g else 0


def select_by_passes(key, stratum, quota):
    """(kept mask, population, kept count, thresholds, flags): the device's passes.  flags: 0 selected by threshold,
    1 kept whole, 2 none kept."""
    key = np.asarray(key, dtype=np.uint64)
    stratum = np.asarray(stratum, dtype=np.int64)
    n = len(quota)
    assert 1 <= n <= MAX_STRATA
    prefix = np.zeros(n, dtype=np.uint64)
    remain = np.zeros(n, dtype=np.int64)
    thr = np.full(n, MASK, dtype=np.uint64)
    flag = np.zeros(n, dtype=np.int64)
    pop = np.zeros(n, dtype=np.int64)
    cnt = np.zeros(n, dtype=np.int64)
    in_stratum = stratum < n
    for d in range(PASSES):
        shift = np.uint64(56 - 8 * d)
        hist = np.zeros((n, DIGITS), dtype=np.int64)
        for b in range(n):
            take = in_stratum & (stratum == b)
            if d > 0:
                if flag[b] != 0:
                    continue
                above = shift + np.uint64(8)
                take = take & ((key >> above) == (prefix[b] >> above))
            hist[b] = np.bincount(((key[take] >> shift) & np.uint64(255)).astype(np.int64), minlength=DIGITS)
        for b in range(n):
            if d == 0:
                pop[b] = hist[b].sum()
                cnt[b] = remain[b] = min(int(quota[b]), int(pop[b]))
                flag[b] = 2 if cnt[b] == 0 else 1 if cnt[b] == pop[b] else 0
            if flag[b] != 0:
                continue
            g, below = pick_digit(hist[b], int(remain[b]))
            prefix[b] |= np.uint64(g) << shift
            remain[b] -= below
            if d == PASSES - 1:
                thr[b] = prefix[b]
    kept = np.zeros(len(key), dtype=bool)
    for b in range(n):
        if flag[b] != 2:
            kept |= in_stratum & (stratum == b) & (key <= thr[b])
    return kept, pop, cnt, thr, flag


def sample(seed, ordinals, mp, edges, quota, eligible=None):
    """The sample of the pairs `ordinals` with scores `mp`: (kept mask, stratum per pair, population, kept count).
    eligible: the pairs that pass the call's terms (all by default)."""
    stratum = strata_of(mp, edges)
    if eligible is not None:
        stratum = np.where(np.asarray(eligible, dtype=bool), stratum, NONE)
    kept, pop, cnt = select_by_definition(keys(seed, ordinals), stratum, quota)
    return kept, stratum, pop, cnt


def _selftest():
    rng = np.random.Generator(np.random.PCG64(1))
    cases = []
    k = rng.integers(0, 1 << 63, 5000, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, 5000, dtype=np.uint64)
    cases.append(("random", np.unique(k), 10))
    base = np.uint64(0xA5A5A5A5A5A5A5A5)
    for bits in (8, 16, 56):
        low = np.arange(300 if bits < 56 else 200, dtype=np.uint64) * np.uint64(max(1, (1 << (64 - bits)) // 300))
        cases.append((f"shared {bits} bits", (base & ~np.uint64((1 << (64 - bits)) - 1)) | low, 1))
    for name, key, n in cases:
        stratum = rng.integers(0, n, len(key))
        for q in (0, 1, 7, len(key)):
            a = select_by_definition(key, stratum, [q] * n)
            b = select_by_passes(key, stratum, [q] * n)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]), (name, q)
        print(f"{name}: {len(key)} keys, {n} strata: passes == definition")


if __name__ == "__main__":
    _selftest()
