"""The pair-set contract of spk_block.hip (its header comment) restated on the host in exact integers.

Two restatements, independent of each other and of the kernel:

  * expected_pairs: brute force, every candidate of every block in nested Python loops (small inputs only);
  * Plan: by ordinal range.  Plan.pairs(g_lo, g_hi) gives the ordered (l, r) sequence of the global candidate
    ordinals [g_lo, g_hi) in O(range + rows), so a thin shard of a space of 2^32 or 10^15 ordinals costs what its
    few thousand pairs cost.  Totals and prefixes are Python ints, a triangular block's row comes from math.isqrt
    and from searchsorted on the exact int64 row starts: no floating point decides anything.

The cases of tests/test_gpu_block_ordinals.py are defined here too, so that tests/test_ordinal_host.py can check on
the CPU, with the reference alone, that each of them can tell a wrong kernel from a right one."""
import math
from dataclasses import dataclass, field

import numpy as np

DEDUPE, LINK_ONLY, LINK_AND_DEDUPE = 0, 1, 2


# ---- brute force ---------------------------------------------------------------------------------------------
def expected_pairs(link_type, keys_l, keys_r, rank, sym=None, null_div=0):
    """keys_l[r] / keys_r[r]: rule r's key per row of the l / r table (-1 NULL); rank: per row of the one table
    (dedupe, link_and_dedupe) or None (link_only); sym[r]: rule r is a symmetric self-join (default: every rule);
    null_div > 0: rank = src * null_div + r with r == null_div - 1 for a NULL unique id.  Returns the (l, r)
    sequence and the candidate count: rule after rule, blocks by ascending key, rows inside a block in stable
    (key, rank) order (r side of a bipartite rule: (key, row)), ordinals l-major, then the rank predicate and the
    earlier-rule exclusion."""
    out, n_cand = [], 0
    for r, (kl, kr) in enumerate(zip(keys_l, keys_r)):
        def view(k, rk):
            rows = np.nonzero(k >= 0)[0]
            return rows[np.lexsort((rows, rk[rows], k[rows]))]
        tri = link_type != LINK_ONLY and (sym is None or bool(sym[r]))
        zl, zr = np.zeros(len(kl), np.int64), np.zeros(len(kr), np.int64)
        vl = view(kl, zl if rank is None else rank)
        vr = view(kr, zr)
        for key in np.unique(kl[vl]):
            bl = vl[kl[vl] == key]
            if tri:
                cand = [(x, y) for a, x in enumerate(bl) for y in bl[a + 1:]]
            else:
                br = vr[kr[vr] == key]
                cand = [(x, y) for x in bl for y in br]
            n_cand += len(cand)
            for x, y in cand:
                if rank is not None:
                    rx, ry = int(rank[x]), int(rank[y])
                    if rx == ry or (not tri and not rx < ry):
                        continue
                    if null_div > 0 and rx // null_div == ry // null_div and \
                            null_div - 1 in (rx % null_div, ry % null_div):
                        continue
                if any(keys_l[j][x] >= 0 and keys_l[j][x] == keys_r[j][y] for j in range(r)):
                    continue
                out.append((int(x), int(y)))
    return np.array(out, dtype=np.int64).reshape(-1, 2), n_cand


# ---- exact integer pieces --------------------------------------------------------------------------------------
def shard_range(total, s, S):
    """Global ordinals [g_lo, g_hi) of shard s of S."""
    total, s, S = int(total), int(s), int(S)
    return total * s // S, total * (s + 1) // S


def shard_of(total, S, g):
    """The shard of S that holds global ordinal g."""
    s = int(g) * int(S) // int(total)
    while shard_range(total, s, S)[1] <= g:
        s += 1
    lo, hi = shard_range(total, s, S)
    assert lo <= g < hi
    return s


def straddling(total, g, margin=1000):
    """(S, s): the first shard count from thin_S(total) on at which the shard holding ordinal g has at least `margin`
    ordinals on either side of it."""
    S = thin_S(total)
    while True:
        s = shard_of(total, S, g)
        lo, hi = shard_range(total, s, S)
        if lo + margin <= g < hi - margin:
            return S, s
        S += 1


def tri_start(a, n):
    """First ordinal of row a of a triangular block of n rows (Python ints)."""
    a, n = int(a), int(n)
    return a * (2 * n - a - 1) // 2


def tri_row(w, n):
    """Row of ordinal w: the largest a with tri_start(a) <= w, i.e. floor((t - sqrt(t^2 - 8w)) / 2) with t = 2n - 1,
    from the integer square root."""
    w, n = int(w), int(n)
    t = 2 * n - 1
    d = t * t - 8 * w
    root = math.isqrt(d)
    if root * root < d:
        root += 1
    a = (t - root) // 2
    assert 0 <= a < n - 1 and tri_start(a, n) <= w < tri_start(a + 1, n), (w, n, a)
    return a


def tri_decode(w, n):
    """(a, c), a < c < n: the view positions of ordinal w inside a triangular block."""
    a = tri_row(w, n)
    return a, a + 1 + (int(w) - tri_start(a, n))


def tri_decode_range(w0, w1, n):
    """tri_decode of every ordinal of [w0, w1) as int64 arrays: the rows the range touches by isqrt at its two ends,
    the ordinals inside by searchsorted on those rows' exact starts (a * (2n - a - 1) < 2^63 for n < 2^31)."""
    n = int(n)
    assert 0 <= w0 < w1 <= n * (n - 1) // 2 and n < 2 ** 31
    a0, a1 = tri_row(w0, n), tri_row(w1 - 1, n)
    rows = np.arange(a0, a1 + 1, dtype=np.int64)
    starts = rows * (2 * n - rows - 1) // 2
    w = np.arange(w0, w1, dtype=np.int64)
    i = np.searchsorted(starts, w, side="right") - 1
    a = rows[i]
    return a, a + 1 + (w - starts[i])


def _order(v):
    """np.argsort(v, kind="stable").  Distinct values of a dense range (ranks that are a permutation) are placed
    by one scatter instead, which is what keeps a 48 M row view cheap."""
    n = len(v)
    if n == 0:
        return np.zeros(0, np.int64)
    lo, hi = int(v.min()), int(v.max())
    if lo == hi:
        return np.arange(n, dtype=np.int64)
    if hi - lo < 2 * n + 16 and n < 2 ** 31:
        slot = np.full(hi - lo + 1, -1, np.int32)
        slot[v if lo == 0 else v - lo] = np.arange(n, dtype=np.int32)
        out = slot[slot >= 0]
        if len(out) == n:
            return out
    return np.argsort(v, kind="stable")


def _view(k, rank):
    """Rows with key >= 0 in stable (key, rank, row) order; rank None: (key, row)."""
    rows = np.flatnonzero(k >= 0)
    everything = len(rows) == len(k)
    if rank is not None:
        o = _order(rank if everything else rank[rows])
        rows = o if everything else rows[o]
    return rows[_order(k[rows])]


class _Rule:
    def __init__(self, kl, kr, rank, tri):
        self.tri = tri
        self.vl = _view(kl, rank)
        skl = kl[self.vl]
        heads = np.flatnonzero(np.r_[True, skl[1:] != skl[:-1]]) if len(skl) else np.zeros(0, np.int64)
        self.bstart = np.r_[heads, len(skl)].astype(np.int64)
        n = np.diff(self.bstart)
        if tri:
            self.vr, self.rstart, self.n_r = self.vl, self.bstart[:-1], n
            cand = n * (n - 1) // 2
        else:
            self.vr = _view(kr, None)
            skr = kr[self.vr]
            bkeys = skl[heads]
            self.rstart = np.searchsorted(skr, bkeys, side="left").astype(np.int64)
            self.n_r = np.searchsorted(skr, bkeys, side="right").astype(np.int64) - self.rstart
            cand = n * self.n_r
        off = [0]
        for c in cand.tolist():
            off.append(off[-1] + c)
        self.total = off[-1]
        assert self.total < 2 ** 63
        self.off = np.array(off, dtype=np.int64)  # [B + 1] exclusive prefix, then the total


class Plan:
    """The candidate-ordinal space of one blocking job.  total, rule_off: Python ints."""

    def __init__(self, link_type, keys_l, keys_r, rank, sym=None, null_div=0):
        self.link_type, self.keys_l, self.keys_r, self.rank, self.null_div = link_type, keys_l, keys_r, rank, null_div
        self.rules = []
        self.rule_off = [0]
        for r, (kl, kr) in enumerate(zip(keys_l, keys_r)):
            tri = link_type != LINK_ONLY and (sym is None or bool(sym[r]))
            R = _Rule(kl, kr, None if link_type == LINK_ONLY else rank, tri)
            self.rules.append(R)
            self.rule_off.append(self.rule_off[-1] + R.total)
        self.total = self.rule_off[-1]

    def _keep(self, r, tri, x, y):
        keep = np.ones(len(x), dtype=bool)
        if self.link_type != LINK_ONLY:
            rx, ry = self.rank[x], self.rank[y]
            keep &= (rx != ry) if tri else (rx < ry)
            d = self.null_div
            if d > 0:
                keep &= ~((rx // d == ry // d) & ((rx % d == d - 1) | (ry % d == d - 1)))
        for j in range(r):
            kl = self.keys_l[j][x]
            keep &= ~((kl >= 0) & (kl == self.keys_r[j][y]))
        return keep

    def candidates(self, g_lo, g_hi):
        """Every candidate of the global ordinals [g_lo, g_hi), in order: (m, 2) rows and the kept mask."""
        g_lo, g_hi = max(int(g_lo), 0), min(int(g_hi), self.total)
        xs, ys, ks = [], [], []
        for r, R in enumerate(self.rules):
            q, q1 = max(g_lo - self.rule_off[r], 0), min(g_hi - self.rule_off[r], R.total)
            if q1 <= q:
                continue
            b = int(np.searchsorted(R.off, q, side="right")) - 1  # off[b] <= q < off[b + 1]: never candidate-free
            while q < q1:
                while int(R.off[b + 1]) <= q:
                    b += 1
                o, bs, n = int(R.off[b]), int(R.bstart[b]), int(R.bstart[b + 1] - R.bstart[b])
                w0, w1 = q - o, min(q1, int(R.off[b + 1])) - o
                if R.tri:
                    a, c = tri_decode_range(w0, w1, n)
                    x, y = R.vl[bs + a], R.vl[bs + c]
                else:
                    a, c = np.divmod(np.arange(w0, w1, dtype=np.int64), int(R.n_r[b]))
                    x, y = R.vl[bs + a], R.vr[int(R.rstart[b]) + c]
                x, y = x.astype(np.int64), y.astype(np.int64)
                xs.append(x)
                ys.append(y)
                ks.append(self._keep(r, R.tri, x, y))
                q = o + w1
        if not xs:
            return np.zeros((0, 2), np.int64), np.zeros(0, bool)
        return np.stack([np.concatenate(xs), np.concatenate(ys)], axis=1), np.concatenate(ks)

    def pairs(self, g_lo, g_hi):
        cand, keep = self.candidates(g_lo, g_hi)
        return cand[keep]

    def shard(self, s, S):
        return self.pairs(*shard_range(self.total, s, S))


# ---- the GPU cases ---------------------------------------------------------------------------------------------
def perm_rank(n):
    """i * m % n with gcd(m, n) = 1: a permutation of the rows that costs one multiply."""
    m = int(n * 0.6180339887) | 1
    while math.gcd(m, n) != 1:
        m += 2
    return (np.arange(n, dtype=np.int64) * m) % n


def null_every(n_valid, every, key=0):
    """A key column with every `every`-th row NULL and n_valid rows of `key`: view position != row."""
    k = np.full(n_valid * every // (every - 1) + every, key, dtype=np.int64)
    k[::every] = -1
    return k[:np.flatnonzero(k >= 0)[n_valid - 1] + 1]


def five_kinds(total, S):
    return {"first": 0, "2^31": shard_of(total, S, 2 ** 31), "2^32": shard_of(total, S, 2 ** 32), "middle": S // 2,
            "last": S - 1}


@dataclass
class Case:
    name: str
    link_type: int
    total: int            # closed form from the construction (Python int)
    S: int
    shards: dict          # label -> shard
    make: object          # () -> dict(keys_l, keys_r, rank); cached by arrays()
    sym: list = field(default_factory=lambda: [1])
    null_div: int = 0
    runs: list = field(default_factory=list)  # tuples of consecutive shards that must concatenate to their union
    drops: bool = False   # the predicates drop some of the candidates of every chosen shard and keep others
    marks: dict = field(default_factory=dict)  # facts the host checks pin (rule prefix, block boundary ...)
    _arrays: dict = None
    _plan: Plan = None

    def arrays(self):
        if self._arrays is None:
            self._arrays = self.make()
        return self._arrays

    def plan(self):
        if self._plan is None:
            a = self.arrays()
            self._plan = Plan(self.link_type, a["keys_l"], a["keys_r"], a["rank"], self.sym, self.null_div)
        return self._plan

    def range(self, s):
        return shard_range(self.total, s, self.S)


S20 = 2 ** 20


def thin_S(total):
    """The shard count at which a shard holds 4096 ordinals (2^20 for the totals just above 2^32)."""
    return total // 4096


N_TRI = 92683                      # n(n-1)/2 = 4 295 022 903 > 2^32
N_BIP = 65537                      # 65537^2 = 4 295 098 369 > 2^32; C(65537, 2) = 2^31 + 32768
N_LARGE = 48_000_000               # (2n-1)^2 > 2^53 from n = 47 453 134 on
S_MAX = 2 ** 31 - 1                # n_shards is a C int


def _one_block(n, rank_of):
    def make():
        k = np.zeros(n, dtype=np.int64)
        return dict(keys_l=[k], keys_r=[k], rank=rank_of(n))
    return make


def case_a():
    total = N_TRI * (N_TRI - 1) // 2
    sh = five_kinds(total, S20)
    s32 = sh["2^32"]
    return Case("a_one_triangle", DEDUPE, total, S20, sh, _one_block(N_TRI, perm_rank), runs=[(s32 - 1, s32, s32 + 1)])


def case_b():
    """rank = perm // 3: view positions 3k, 3k+1, 3k+2 hold equal ranks, so a row a = 3k starts with two dropped pairs.
    A thin shard inside one row of ~50 000 pairs drops nothing; the shards here hold a row start each: the first, the
    nearest such row starts below and above ordinal 2^32, and the last (the final rows of the triangle)."""
    total = N_TRI * (N_TRI - 1) // 2
    a = tri_row(2 ** 32, N_TRI)
    a -= a % 3
    sh = {"first": 0, "row_start_below_2^32": shard_of(total, S20, tri_start(a, N_TRI)),
          "row_start_above_2^32": shard_of(total, S20, tri_start(a + 3, N_TRI)), "last": S20 - 1}
    return Case("b_equal_ranks", DEDUPE, total, S20, sh, _one_block(N_TRI, lambda n: perm_rank(n) // 3), drops=True,
                marks={"row_below": a})


def case_c_one_key():
    def make():
        return dict(keys_l=[null_every(N_BIP, 7)], keys_r=[null_every(N_BIP, 5)], rank=None)
    total = N_BIP * N_BIP
    return Case("c_bipartite_one_key", LINK_ONLY, total, S20, five_kinds(total, S20), make)


def _c_sizes():
    """~600 keys; every 50th has l rows and no r rows, every 50th + 25 r rows and no l rows."""
    n_l = [2800 + (i * 37) % 200 for i in range(600)]
    n_r = [2850 + (i * 53) % 150 for i in range(600)]
    for i in range(0, 600, 50):
        n_r[i] = 0
        n_l[i + 25] = 0
    return n_l, n_r


def case_c_blocks():
    n_l, n_r = _c_sizes()

    def make():
        rng = np.random.default_rng(31)

        def col(sizes, nulls):
            k = np.r_[np.repeat(np.arange(len(sizes), dtype=np.int64) * 3 + 1, sizes), np.full(nulls, -1, np.int64)]
            return k[rng.permutation(len(k))]
        return dict(keys_l=[col(n_l, 5000)], keys_r=[col(n_r, 3000)], rank=None)
    total = sum(a * b for a, b in zip(n_l, n_r))
    S = thin_S(total)
    return Case("c_bipartite_blocks", LINK_ONLY, total, S, five_kinds(total, S), make)


def _d_sizes():
    """~600 blocks of ~4000 rows; after every 10th, a run of 1..12 singleton blocks."""
    sizes = []
    for i in range(600):
        sizes.append(3900 + (i * 37) % 300)
        if i % 10 == 9:
            sizes += [1] * (1 + (i // 10) % 12)
    return sizes


def case_d():
    sizes = _d_sizes()
    cand = [n * (n - 1) // 2 for n in sizes]
    total = sum(cand)
    off = [0]
    for c in cand:
        off.append(off[-1] + c)
    # ordinals past 2^32 at which a run of singletons sits: the next block's first ordinal
    at = [off[b] for b in range(1, len(sizes)) if sizes[b] == 1 and sizes[b - 1] > 1 and 2 ** 32 < off[b] < total]
    found = None
    for S in range(thin_S(total), thin_S(total) + 200000):  # a shard's first ordinal is total * s // S: ~1 in 4096 (S, run) pairs fit
        for g in at:
            s = -(-g * S // total)
            if total * s // S == g:
                found = (S, s, g)
                break
        if found:
            break
    S, s_run, g_run = found

    def make():
        n = sum(sizes)
        keys = np.repeat(np.arange(len(sizes), dtype=np.int64) * 2 + 3, sizes)
        keys = keys[np.random.default_rng(41).permutation(n)]
        return dict(keys_l=[keys], keys_r=[keys], rank=perm_rank(n))
    sh = five_kinds(total, S)
    sh["singletons_first"] = s_run
    sh["singletons_last"] = s_run - 1
    return Case("d_many_triangles", DEDUPE, total, S, sh, make, marks={"run_at": g_run, "sizes": sizes})


N_E = 100000


def _e_keys(perm):
    """One table of N_E rows, one key with N_TRI l rows and N_BIP r rows (6 074 165 771 candidates).  The l rows
    are those whose perm is below N_TRI (key 5 on the others: an l block without r rows), the r rows the last N_BIP
    rows (key 9 before).  The l view is in rank order, so ordinal 2^32 lies at an l row of middling rank (about a third
    of its r rows rank higher), and the last l row still has the r rows with perm >= N_TRI above it."""
    i = np.arange(N_E, dtype=np.int64)
    return np.where(perm < N_TRI, 0, 5), np.where(i >= N_E - N_BIP, 0, 9)


def case_e_dedupe():
    def make():
        rank = perm_rank(N_E)
        kl, kr = _e_keys(rank)
        return dict(keys_l=[kl], keys_r=[kr], rank=rank)
    total = N_TRI * N_BIP
    S = thin_S(total)
    sh = {"2^32": shard_of(total, S, 2 ** 32), "last": S - 1}
    return Case("e_nonsym_dedupe", DEDUPE, total, S, sh, make, sym=[0], drops=True)


def case_e_link_and_dedupe(sym):
    """rank = src * div + r; the second half of the table is source 1; some unique ids are NULL (r = div - 1), which
    sorts them to the end of their source.  Symmetric: one triangle of N_TRI rows, whose ordinal 2^32 lies 334 rows
    before the end, so only every 1000th id is NULL (46 in source 1): the shard at 2^32 and the last one then hold
    rows with and without an id.  Non-symmetric: _e_keys, every 11th id NULL, except on the l rows of source 1 (a
    NULL id there would be the last l row, and the last shard all dropped).  The l rows of source 0 with a NULL id
    get a shard of their own: the one around the first of them meeting the first r row of source 1, where the pairs
    of its own source are dropped for the NULL id and those across the sources are kept by the source alone."""
    n = N_TRI if sym else N_E
    div = n + 1
    i = np.arange(n, dtype=np.int64)
    perm = perm_rank(n)
    if sym:
        null = i % 1000 == 4
    else:
        null = (i % 11 == 4) & ((i < n // 2) | (perm >= N_TRI))
    rank = (i >= n // 2) * div + np.where(null, div - 1, perm)

    def make():
        if sym:
            k = np.zeros(n, dtype=np.int64)
            return dict(keys_l=[k], keys_r=[k], rank=rank)
        kl, kr = _e_keys(perm)
        return dict(keys_l=[kl], keys_r=[kr], rank=rank)
    total = n * (n - 1) // 2 if sym else N_TRI * N_BIP
    S = thin_S(total)
    sh = {"2^32": shard_of(total, S, 2 ** 32), "last": S - 1}
    if not sym:
        a = int(((perm < N_TRI) & (i < n // 2) & ~null).sum())  # l view: source 0 with an id, then its NULL ids
        c = n // 2 - (n - N_BIP)                                # r view (row order): first row of source 1
        sh["l_null_id"] = shard_of(total, S, a * N_BIP + c)
    return Case("e_link_and_dedupe_" + ("sym" if sym else "nonsym"), LINK_AND_DEDUPE, total, S, sh, make,
                sym=[sym], null_div=div, drops=True)


def case_f(n_rules):
    """Rule 0: two blocks of N_BIP rows and 3000 NULL keys, shuffled.  Rules 1 and 2: blocks of ~34 and ~41 rows on
    every 41st / 29th row, which cut across rule 0's blocks (and its NULLs)."""
    n = 2 * N_BIP + 3000
    i = np.arange(n, dtype=np.int64)
    k1 = np.where(i % 41 == 0, (i // 41) % 97, -1)
    k2 = np.where(i % 29 == 0, (i // 29) % 113, -1)
    def tri(k):
        return sum(c * (c - 1) // 2 for c in np.bincount(k[k >= 0]).tolist())
    totals = [2 * (N_BIP * (N_BIP - 1) // 2), tri(k1), tri(k2)][:n_rules]
    total = sum(totals)

    def make():
        k0 = np.r_[np.zeros(N_BIP, np.int64), np.full(N_BIP, 7, np.int64), np.full(3000, -1, np.int64)]
        k0 = k0[np.random.default_rng(61).permutation(n)]
        keys = [k0, k1, k2][:n_rules]
        return dict(keys_l=keys, keys_r=keys, rank=perm_rank(n) // 2)
    S, s = straddling(total, totals[0])
    sh = {"straddles_rule_0_1": s, "inside_rule_1": shard_of(total, S, totals[0] + totals[1] // 2)}
    if n_rules == 3:
        sh["inside_rule_2"] = shard_of(total, S, totals[0] + totals[1] + totals[2] // 2)
    return Case(f"f_{n_rules}_rules", DEDUPE, total, S, sh, make, sym=[1] * n_rules, drops=True,
                marks={"rule_totals": totals})


def case_g():
    total = N_TRI * (N_TRI - 1) // 2
    sh = {"last": S_MAX - 1, "middle": S_MAX // 2, "first_past_2^63": 2 ** 63 // total + 1}
    return Case("g_int128_bounds", DEDUPE, total, S_MAX, sh, _one_block(N_TRI, perm_rank))


def case_h():
    n = N_LARGE
    total = n * (n - 1) // 2
    sh = {"first": 0, "last": S_MAX - 1, "row_n/2": shard_of(total, S_MAX, tri_start(n // 2, n)),
          "rows_near_end": shard_of(total, S_MAX, tri_start(n - 2000, n))}
    return Case("h_large_block", DEDUPE, total, S_MAX, sh, _one_block(n, perm_rank), marks={"n": n})


CASES = {
    "a": case_a, "b": case_b, "c_one_key": case_c_one_key, "c_blocks": case_c_blocks, "d": case_d,
    "e_dedupe": case_e_dedupe, "e_lad_nonsym": lambda: case_e_link_and_dedupe(0),
    "e_lad_sym": lambda: case_e_link_and_dedupe(1), "f2": lambda: case_f(2), "f3": lambda: case_f(3),
    "g": case_g, "h": case_h,
}
