"""spk_block at the edges of its compaction chunks (2048 candidate ordinals per workgroup, 8 per thread), on a
bare context: candidate counts one below, at and one above a chunk, a block that spans two chunks, runs of
candidate-free blocks at a chunk start, bipartite joins, rules that exclude each other, shards, and the state the
pair set's replacement leaves.  The expected value is a NumPy restatement of the contract in the header comment
of spk_block.hip, compared as an ordered sequence."""
import numpy as np
import pytest

from ordinal_common import DEDUPE, LINK_ONLY, expected_pairs  # the contract, restated (brute force)

pytestmark = pytest.mark.gpu

CHUNK = 2048  # spk_block.hip EN_CHUNK


@pytest.fixture(scope="module")
def native():
    from splink_amd import _native
    if _native.device_count() == 0:
        pytest.fail("no HIP device visible: the -m gpu tests need an MI355X")
    return _native


def load(native, link_type, keys_l, keys_r, rank):
    ctx = native.Context(0)
    ctx.set_link_type(link_type)
    n_l, n_r = len(keys_l[0]), len(keys_r[0])
    ctx.table_create(0, n_l, 0)
    if link_type == LINK_ONLY:
        ctx.table_create(1, n_r, 0)
    else:
        ctx.table_set_rank(0, rank)
    for r, (kl, kr) in enumerate(zip(keys_l, keys_r)):
        ctx.table_set_key(0, r, 0, kl)
        ctx.table_set_key(1 if link_type == LINK_ONLY else 0, r, 1, kr)
    return ctx


def run(native, link_type, keys_l, keys_r, rank, shards=1):
    """The pairs of every shard, concatenated, and the candidate total (equal on every shard)."""
    ctx = load(native, link_type, keys_l, keys_r, rank)
    parts, totals = [], set()
    for s in range(shards):
        n_pairs, n_cand = ctx.block(link_type, [1] * len(keys_l), s, shards)
        assert ctx.pairs_count() == n_pairs
        l, r = ctx.pairs_copy(0, n_pairs)
        parts.append(np.stack([l, r], axis=1).astype(np.int64))
        totals.add(n_cand)
    assert len(totals) == 1
    return np.concatenate(parts), totals.pop(), ctx


def check(native, link_type, keys_l, keys_r, rank, shards=1):
    want, n_cand = expected_pairs(link_type, keys_l, keys_r, rank)
    got, total, ctx = run(native, link_type, keys_l, keys_r, rank, shards)
    assert total == n_cand
    assert got.shape == want.shape and (got == want).all(), np.nonzero((got != want).any(axis=1))[0][:10]
    return want, n_cand, ctx


def blocks_to_keys(sizes, seed):
    """One key per block (ascending with the block's position), the rows shuffled; distinct ranks, shuffled."""
    rng = np.random.default_rng(seed)
    keys = np.repeat(np.arange(len(sizes), dtype=np.int64) * 3 + 1, sizes)
    keys = keys[rng.permutation(len(keys))]
    return keys, rng.permutation(len(keys)).astype(np.int64)


# ---- symmetric dedupe, one rule -------------------------------------------------------------------------------
SINGLES_AT_CHUNK = [1, 1, 64, 1, 8, 1, 1, 1, 3, 2] + [1] * 11 + [3, 1]


@pytest.mark.parametrize("sizes,n_cand", [
    ([64, 8, 3], CHUNK - 1),
    ([64, 8, 3, 2], CHUNK),
    ([64, 8, 3, 2, 2], CHUNK + 1),
    ([65], 2080),                  # one block over two chunks
    (SINGLES_AT_CHUNK, CHUNK + 3),  # candidate-free blocks before, between and after; 11 of them at ordinal 2048
])
def test_dedupe_chunk_edges(native, sizes, n_cand):
    keys, rank = blocks_to_keys(sizes, seed=len(sizes))
    want, total, _ = check(native, DEDUPE, [keys], [keys], rank)
    assert total == n_cand == len(want)  # distinct ranks: every candidate is a pair


def test_dedupe_equal_ranks_drop_pairs(native):
    keys, rank = blocks_to_keys([64, 8, 3, 2, 2], seed=11)
    rank = rank // 3  # runs of three equal ranks: the rank predicate drops pairs on both sides of the chunk edge
    want, total, _ = check(native, DEDUPE, [keys], [keys], rank)
    assert total == CHUNK + 1 and 0 < len(want) < total


@pytest.mark.parametrize("keys", [np.array([4], np.int64), np.full(50, -1, np.int64)], ids=["one_row", "all_null"])
def test_dedupe_no_pairs(native, keys):
    want, total, ctx = check(native, DEDUPE, [keys], [keys], np.arange(len(keys), dtype=np.int64))
    assert total == 0 and len(want) == 0
    assert ctx.pairs_count() == 0  # a valid, empty pair set
    l, r = ctx.pairs_copy(0, 0)
    assert len(l) == 0 and len(r) == 0


# ---- bipartite (link_only, two tables) --------------------------------------------------------------------------
def shuffled(keys, seed):
    keys = np.asarray(keys, dtype=np.int64)
    return keys[np.random.default_rng(seed).permutation(len(keys))]


@pytest.mark.parametrize("kl,kr,n_cand", [
    ([5] * 32, [5] * 64, CHUNK),
    ([5] * 32 + [9], [5] * 64 + [9], CHUNK + 1),
    # key 2 has l rows and no r rows, between keys 1 and 3 that have both; keys 0 and 4 only on the r side
    ([1] * 3 + [2] * 2 + [3] * 4 + [-1], [0] * 2 + [1] * 5 + [3] * 2 + [4] * 3 + [-1] * 2, 3 * 5 + 4 * 2),
], ids=["32x64", "32x64+1x1", "l_block_without_r"])
def test_link_only_chunk_edges(native, kl, kr, n_cand):
    kl, kr = shuffled(kl, 1), shuffled(kr, 2)
    want, total, _ = check(native, LINK_ONLY, [kl], [kr], None)
    assert total == n_cand == len(want)


# ---- several rules -------------------------------------------------------------------------------------------
def rule_keys(n_rules, n=200):
    """Rule 0 in blocks of ten with some NULLs; the last rule in blocks of ~28 that lose the pairs rule 0 has;
    with three rules the middle one has distinct keys, so no candidates at all."""
    i = np.arange(n, dtype=np.int64)
    k0 = np.where(i % 13 == 5, -1, i % 20)
    k_last = np.where(i % 17 == 3, -1, i % 7)
    keys = [k0, k_last] if n_rules == 2 else [k0, i + 100, k_last]
    rank = np.random.default_rng(n_rules).permutation(n).astype(np.int64) // 2  # some equal ranks
    return keys, rank


@pytest.mark.parametrize("n_rules", [2, 3])
def test_rules_exclude_earlier_keys(native, n_rules):
    keys, rank = rule_keys(n_rules)
    want, total, _ = check(native, DEDUPE, keys, keys, rank)
    per_rule = [expected_pairs(DEDUPE, [k], [k], rank) for k in keys]
    assert total == sum(c for _, c in per_rule) > CHUNK
    # the last rule loses candidates to rule 0's key, and keeps some
    assert 0 < len(want) - len(per_rule[0][0]) < len(per_rule[-1][0])
    if n_rules == 3:
        assert per_rule[1][1] == 0


# ---- shards --------------------------------------------------------------------------------------------------
def test_three_shards_concatenate(native):
    keys, rank = blocks_to_keys([64, 8, 3, 2, 2], seed=5)
    check(native, DEDUPE, [keys], [keys], rank, shards=3)
    keys, rank = rule_keys(3)
    check(native, DEDUPE, keys, keys, rank, shards=3)


# ---- state ---------------------------------------------------------------------------------------------------
def test_pair_set_replaced_then_dropped(native):
    keys, rank = rule_keys(2)
    _, _, ctx = check(native, DEDUPE, keys, keys, rank)
    rows_l = np.array([7, 0, 199, 3, 3], dtype=np.int32)
    rows_r = np.array([8, 199, 0, 3, 4], dtype=np.int32)
    ctx.pairs_load(rows_l, rows_r)
    assert ctx.pairs_count() == 5
    l, r = ctx.pairs_copy()
    assert (l == rows_l).all() and (r == rows_r).all()
    ctx.table_create(0, 10, 0)
    with pytest.raises(RuntimeError) as e:
        ctx.pairs_count()
    assert "spk_pairs_count failed (-4)" in str(e.value) and "no pairs" in str(e.value)
