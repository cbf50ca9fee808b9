"""Host checks of tests/ordinal_common.py: the by-range reference equals the brute force, the triangular decode
is exact at the row boundaries of blocks up to 2^31 - 1 rows, and every case of tests/test_gpu_block_ordinals.py
meets the condition that makes it worth running on the GPU (so that none of them can pass vacuously)."""
import numpy as np
import pytest

import ordinal_common as oc
from ordinal_common import DEDUPE, LINK_AND_DEDUPE, LINK_ONLY, Plan, expected_pairs, shard_range, tri_decode, \
    tri_decode_range, tri_row, tri_start


# ---- the range reference equals the brute force -----------------------------------------------------------------
def random_job(kind, seed):
    """Up to ~60 rows, 1 to 3 rules: NULL keys, singleton (candidate-free) blocks, equal ranks; per kind an l block
    without r rows, a non-symmetric rule under dedupe, NULL unique ids under link_and_dedupe."""
    rng = np.random.default_rng(seed)
    n = int(rng.integers(2, 61))
    n_rules = int(rng.integers(1, 4))

    def keys(m, values):
        k = rng.choice(values, size=m)
        k[rng.random(m) < 0.15] = -1
        return k.astype(np.int64)
    values = np.array([2, 3, 5, 11, 12, 40, 41])[:int(rng.integers(2, 8))]
    if kind == "link_only":
        m = int(rng.integers(1, 61))
        keys_l = [keys(n, values) for _ in range(n_rules)]
        keys_r = [keys(m, values[1:]) for _ in range(n_rules)]  # values[0]: l rows and never an r row
        return dict(link_type=LINK_ONLY, keys_l=keys_l, keys_r=keys_r, rank=None, sym=[1] * n_rules, null_div=0)
    sym = [1] * n_rules if kind in ("dedupe", "lad") else [int(x) for x in rng.integers(0, 2, size=n_rules)]
    if kind.endswith("nonsym"):
        sym[int(rng.integers(0, n_rules))] = 0
    keys_l = [keys(n, values) for _ in range(n_rules)]
    keys_r = [kl if s else keys(n, values) for kl, s in zip(keys_l, sym)]
    rank = rng.permutation(n).astype(np.int64) // int(rng.integers(1, 4))
    if kind.startswith("lad"):
        div = n + 1
        r = np.where(rng.random(n) < 0.2, div - 1, rank)
        rank = (np.arange(n) >= n // 2) * div + r
        return dict(link_type=LINK_AND_DEDUPE, keys_l=keys_l, keys_r=keys_r, rank=rank, sym=sym, null_div=div)
    return dict(link_type=DEDUPE, keys_l=keys_l, keys_r=keys_r, rank=rank, sym=sym, null_div=0)


@pytest.mark.parametrize("kind", ["dedupe", "link_only", "dedupe_nonsym", "lad", "lad_nonsym"])
def test_range_reference_equals_brute_force(kind):
    seen = dict(cand=0, kept=0, dropped=0, empty_block=0, l_without_r=0)
    for seed in range(40):
        job = random_job(kind, seed)
        want, n_cand = expected_pairs(**job)
        plan = Plan(**job)
        assert plan.total == n_cand
        whole = plan.pairs(0, plan.total)
        assert whole.shape == want.shape and (whole == want).all(), (kind, seed)
        for S in (1, 3, 7):
            parts = [plan.shard(s, S) for s in range(S)]
            assert [shard_range(n_cand, s, S)[0] for s in range(1, S)] == [shard_range(n_cand, s, S)[1]
                                                                           for s in range(S - 1)]
            got = np.concatenate(parts)
            assert got.shape == want.shape and (got == want).all(), (kind, seed, S)
        rng = np.random.default_rng(1000 + seed)
        for _ in range(6):  # arbitrary sub-ranges: three that tile the space, and the middle one alone
            g1, g2 = sorted(int(g) for g in rng.integers(0, n_cand + 1, size=2))
            a, b, c = plan.pairs(0, g1), plan.pairs(g1, g2), plan.pairs(g2, n_cand)
            assert (np.concatenate([a, b, c]) == want).all(), (kind, seed, g1, g2)
            cand, keep = plan.candidates(g1, g2)
            assert len(cand) == g2 - g1 and int(keep.sum()) == len(b)
        seen["cand"] += n_cand
        seen["kept"] += len(want)
        seen["dropped"] += n_cand - len(want)
        for R in plan.rules:
            seen["empty_block"] += int((np.diff(R.off) == 0).sum())
            seen["l_without_r"] += int((R.n_r == 0).sum())
    # the inputs had what they are meant to have
    assert seen["kept"] > 1000 and seen["empty_block"] > 0
    if kind != "link_only":
        assert seen["dropped"] > 100
    else:
        assert seen["l_without_r"] > 0


# ---- triangular decode --------------------------------------------------------------------------------------------
def test_tri_decode_every_ordinal_small():
    for n in range(2, 41):
        want = [(a, c) for a in range(n) for c in range(a + 1, n)]
        assert [tri_decode(w, n) for w in range(len(want))] == want
        a, c = tri_decode_range(0, len(want), n)
        assert list(zip(a.tolist(), c.tolist())) == want
        for w0 in range(0, len(want), 7):
            a, c = tri_decode_range(w0, min(w0 + 5, len(want)), n)
            assert list(zip(a.tolist(), c.tolist())) == want[w0:w0 + 5]


@pytest.mark.parametrize("n", [oc.N_TRI, oc.N_LARGE, 2 ** 31 - 1])
def test_tri_decode_row_boundaries_large(n):
    total = n * (n - 1) // 2
    a_first = n - 61
    for a in range(a_first, n - 1):
        start = total - (n - a) * (n - a - 1) // 2  # what the rows from a on hold, counted from the end
        assert tri_start(a, n) == start
        assert tri_decode(start - 1, n) == (a - 1, n - 1)
        assert tri_decode(start, n) == (a, a + 1)
        if a + 2 < n:
            assert tri_decode(start + 1, n) == (a, a + 2)
    assert tri_row(0, n) == 0 and tri_decode(n - 2, n) == (0, n - 1) and tri_decode(n - 1, n) == (1, 2)
    want = [(a_first - 1, n - 1)] + [(a, c) for a in range(a_first, n) for c in range(a + 1, n)]
    a, c = tri_decode_range(tri_start(a_first, n) - 1, total, n)
    assert list(zip(a.tolist(), c.tolist())) == want


# ---- the GPU cases discriminate -----------------------------------------------------------------------------------
def wrap64(x):
    return (x + 2 ** 63) % 2 ** 64 - 2 ** 63


def trunc_div(a, b):
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


@pytest.mark.parametrize("name", list(oc.CASES))
def test_gpu_case_discriminates(name):
    case = oc.CASES[name]()
    assert case.total > 2 ** 32
    assert case.S < 2 ** 31 and all(0 <= s < case.S for s in case.shards.values())
    ranges = {label: case.range(s) for label, s in case.shards.items()}
    assert all(hi > lo for lo, hi in ranges.values())
    for label, g in (("2^31", 2 ** 31), ("2^32", 2 ** 32)):
        if label in ranges:
            assert ranges[label][0] <= g < ranges[label][1]
    if "last" in ranges:
        assert ranges["last"][1] == case.total
    for run in case.runs:
        assert all(b == a + 1 for a, b in zip(run, run[1:]))
        assert case.range(run[0])[0] < 2 ** 32 < case.range(run[-1])[1]

    if name == "h":  # checked on the closed forms: no 48 M row arrays on the host
        n = case.marks["n"]
        assert (2 * n - 1) ** 2 > 2 ** 53 and n >= 47_453_134
        assert (2 * 47_453_134 - 1) ** 2 > 2 ** 53 >= (2 * 47_453_133 - 1) ** 2
        assert all(hi - lo <= 540_000 for lo, hi in ranges.values())
        assert tri_row(ranges["first"][1] - 1, n) == 0
        lo, hi = ranges["row_n/2"]
        assert lo <= tri_start(n // 2, n) < hi
        for label in ("rows_near_end", "last"):
            lo, hi = ranges[label]
            assert tri_row(hi - 1, n) - tri_row(lo, n) >= 5
        return

    plan = case.plan()
    assert plan.total == case.total
    thin = 3 if name == "g" else 4100
    for label, (lo, hi) in ranges.items():
        cand, keep = plan.candidates(lo, hi)
        assert len(cand) == hi - lo <= thin
        if case.drops:
            assert 0 < int(keep.sum()) < len(cand), label
        else:
            assert keep.all(), label
        if case.link_type != LINK_ONLY or name == "c_one_key":
            # view position and row differ: taking one for the other shows
            assert (cand[:, 0] != cand[:, 1]).any()

    if name == "b":  # pairs are dropped within three rows of ordinal 2^32, on either side of it
        a = case.marks["row_below"]
        assert tri_start(a, oc.N_TRI) <= 2 ** 32 < tri_start(a + 3, oc.N_TRI)
        assert ranges["row_start_below_2^32"][0] <= tri_start(a, oc.N_TRI) < ranges["row_start_below_2^32"][1]
        assert ranges["row_start_above_2^32"][0] <= tri_start(a + 3, oc.N_TRI) < ranges["row_start_above_2^32"][1]
    if name in ("c_one_key", "c_blocks"):
        a = case.arrays()
        assert (a["keys_l"][0] < 0).any() and (a["keys_r"][0] < 0).any()  # NULL rows: view position != row
    if name in ("c_blocks", "d"):
        R = plan.rules[0]
        assert len(R.off) - 1 >= 580 and int(np.diff(R.off).max()) < 2 ** 24  # the prefix, not one block, crosses
    if name == "c_blocks":
        assert int((plan.rules[0].n_r == 0).sum()) >= 10
    if name == "d":
        R, g = plan.rules[0], case.marks["run_at"]
        assert g > 2 ** 32 and ranges["singletons_first"][0] == g == ranges["singletons_last"][1]
        b = int(np.searchsorted(R.off, g, side="left"))
        assert R.off[b] == g and R.off[b + 1] == g and R.off[b - 1] < g  # candidate-free blocks sit at ordinal g
        assert int((np.diff(R.off) == 0).sum()) > 300
    if name.startswith("e_lad"):
        rank, d = case.arrays()["rank"], case.null_div
        assert (rank % d == d - 1).any() and set((rank // d).tolist()) == {0, 1}
        if "l_null_id" in ranges:  # one l row of source 0 with a NULL id, r rows of both sources
            cand, keep = plan.candidates(*ranges["l_null_id"])
            assert (rank[cand[:, 0]] == d - 1).all() and set((rank[cand[:, 1]] // d).tolist()) == {0, 1}
            assert (keep == (rank[cand[:, 1]] // d == 1)).all()
    if name.startswith("f"):
        totals = case.marks["rule_totals"]
        assert totals == [R.total for R in plan.rules] and totals[0] > 2 ** 32
        lo, hi = ranges["straddles_rule_0_1"]
        assert lo + 1000 <= totals[0] < hi - 1000
        first = totals[0]
        for r in range(1, len(totals)):
            lo, hi = ranges[f"inside_rule_{r}"]
            assert first <= lo and hi <= first + totals[r]
            # the earlier rules' keys exclude some of this rule's candidates here, and not all of them
            a = case.arrays()
            null = np.full(len(a["rank"]), -1, np.int64)
            alone = Plan(DEDUPE, [null] * r + [a["keys_l"][r]], [null] * r + [a["keys_r"][r]], a["rank"])
            kept_alone, kept = len(alone.pairs(lo - first, hi - first)), len(plan.pairs(lo, hi))
            assert 0 < kept < kept_alone
            first += totals[r]
    if name == "g":
        for label, s in case.shards.items():
            lo, hi = ranges[label]
            assert 2 <= hi - lo <= 3
            # total narrowed to 32 bits gives other bounds on every shard
            assert (case.total % 2 ** 32) * s // case.S != lo
            if label != "middle":  # total * shard is 2^62 at S // 2: it fits; the other two need the 128-bit product
                assert case.total * s >= 2 ** 63
                assert trunc_div(wrap64(case.total * s), case.S) != lo
                assert trunc_div(wrap64(case.total * (s + 1)), case.S) != hi
