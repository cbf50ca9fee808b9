"""sample_pairs without a device: the key, the emulated radix select against the definition, the arguments."""
import numpy as np
import pytest

from select_sample_common import emulator

M64 = (1 << 64) - 1


def py_mix(x):
    x ^= x >> 30
    x = (x * 0xBF58476D1CE4E5B9) & M64
    x ^= x >> 27
    x = (x * 0x94D049BB133111EB) & M64
    x ^= x >> 31
    return x


def py_key(seed, p):
    return py_mix((py_mix(seed) + 0x9E3779B97F4A7C15 * (p + 1)) & M64)


ORDINALS = (0, 1, 2 ** 31, 2 ** 40)
FIXED = {0: (0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x706EDE5CFCDC9A1C, 0x1937167E168D9372),
         1: (0xBFEF8030DDC2D772, 0x5F552CE482F2AA47, 0xEEF8885F38F68B2D, 0xF0B96BE858B2A574),
         M64: (0xA577782BC52A9F5A, 0xB485244380E590BE, 0xCB3A607555D8E38E, 0x83E0AD93349E6601)}


# ---- 1. the key ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", sorted(FIXED))
def test_key_fixed_vectors(seed):
    emu = emulator()
    got = emu.keys(seed, np.array(ORDINALS, dtype=np.int64))
    assert got.dtype == np.uint64
    assert [int(k) for k in got] == [py_key(seed, p) for p in ORDINALS] == list(FIXED[seed])


def test_key_is_the_first_splitmix64_output_at_seed_0():
    assert py_key(0, 0) == py_mix(0x9E3779B97F4A7C15) == 0xE220A8397B1DCDAF


@pytest.mark.parametrize("seed,first", [(0, 0), (7, 2 ** 31 - 2 ** 15), (M64, 2 ** 40)])
def test_keys_are_distinct(seed, first):
    emu = emulator()
    p = np.arange(first, first + 2 ** 16, dtype=np.int64)
    k = emu.keys(seed, p)
    assert len(np.unique(k)) == len(p)
    for i in (0, 1, 4095, 2 ** 16 - 1):
        assert int(k[i]) == py_key(seed, first + i)


# ---- 2. the emulated passes against the definition ----------------------------------------------------------
def agree(key, stratum, quota):
    emu = emulator()
    kept_d, pop_d, cnt_d = emu.select_by_definition(key, stratum, quota)
    kept_p, pop_p, cnt_p, thr, flag = emu.select_by_passes(key, stratum, quota)
    assert np.array_equal(kept_d, kept_p)
    assert np.array_equal(pop_d, pop_p) and np.array_equal(cnt_d, cnt_p)
    for b, q in enumerate(quota):
        assert cnt_p[b] == min(q, pop_p[b]) == int(kept_p[np.asarray(stratum) == b].sum())
        assert flag[b] == (2 if cnt_p[b] == 0 else 1 if cnt_p[b] == pop_p[b] else 0)
        if flag[b] == 0:  # the threshold is the quota-th smallest key itself
            assert int(thr[b]) == int(np.sort(np.asarray(key)[np.asarray(stratum) == b])[q - 1])
    return kept_p, pop_p, cnt_p


def random_keys(n, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    k = np.unique(rng.integers(0, 1 << 63, 2 * n, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, 2 * n, dtype=np.uint64))
    rng.shuffle(k)
    return k[:n], rng


@pytest.mark.parametrize("n_strata", [1, 10, 64])
def test_passes_on_random_keys(n_strata):
    key, rng = random_keys(6000, n_strata)
    stratum = rng.integers(0, n_strata, len(key))
    stratum[stratum == n_strata // 2] = emulator().NONE if n_strata > 1 else 0  # an empty stratum; pairs in none
    pop = np.bincount(stratum[stratum < n_strata], minlength=n_strata)
    if n_strata > 1:
        assert pop[n_strata // 2] == 0 and (stratum == emulator().NONE).any()
    for quota in ([0] * n_strata, [1] * n_strata, [17] * n_strata, list(pop), list(np.maximum(pop - 1, 0)),
                  list(pop + 1), [int(q) for q in rng.integers(0, 200, n_strata)]):
        kept, _, cnt = agree(key, stratum, [int(q) for q in quota])
        assert kept.sum() == cnt.sum()


@pytest.mark.parametrize("bits", [8, 16, 56])
def test_passes_on_keys_with_a_shared_prefix(bits):
    """One stratum whose keys share their `bits` leading bits, next to a stratum of random keys."""
    free = 64 - bits
    rng = np.random.Generator(np.random.PCG64(bits))
    n = 200 if bits == 56 else 500
    low = rng.choice(1 << min(free, 40), n, replace=False).astype(np.uint64) if free > 8 else \
        rng.choice(256, n, replace=False).astype(np.uint64)
    shared = (np.uint64(0xC3A5F00DDEADBEEF) >> np.uint64(free) << np.uint64(free)) | low
    assert len(np.unique(shared >> np.uint64(free))) == 1 and len(np.unique(shared)) == n
    other, _ = random_keys(300, bits)
    key = np.concatenate([shared, other])
    stratum = np.concatenate([np.zeros(n, dtype=np.int64), np.ones(len(other), dtype=np.int64)])
    for q0 in (0, 1, 2, n // 2, n - 1, n, n + 1):
        agree(key, stratum, [q0, 11])


def test_passes_on_keys_that_differ_in_the_last_digit_only():
    key = np.uint64(0x0123456789ABCD00) + np.arange(256, dtype=np.uint64)[::-1]
    stratum = np.zeros(256, dtype=np.int64)
    for q in (0, 1, 2, 128, 255, 256, 257):
        kept, pop, cnt = agree(key, stratum, [q])
        assert pop[0] == 256 and cnt[0] == min(q, 256)
        assert np.array_equal(np.nonzero(kept)[0], np.arange(256)[256 - cnt[0]:])  # the smallest keys are the last rows


def test_extreme_keys():
    key = np.array([0, 1, M64, M64 - 1, 1 << 63, (1 << 63) - 1], dtype=np.uint64)
    for q in range(8):
        agree(key, np.zeros(len(key), dtype=np.int64), [q])


def test_sample_from_seed_and_ordinals():
    emu = emulator()
    n = 5000
    rng = np.random.Generator(np.random.PCG64(5))
    mp = rng.random(n)
    mp[::97] = np.nan
    mp[5], mp[6] = 0.25, 1.0   # on an inner edge: the stratum to its right; on the last edge: the last stratum
    edges = [0.0, 0.25, 0.5, 1.0]
    eligible = rng.random(n) < 0.7
    eligible[5] = eligible[6] = True
    kept, stratum, pop, cnt = emu.sample(3, np.arange(n), mp, edges, [5, 50, 10 ** 6], eligible)
    assert stratum[5] == 1 and stratum[6] == 2 and (stratum[::97] == emu.NONE).all()
    assert not kept[~eligible].any() and not kept[np.isnan(mp)].any()
    assert list(cnt) == [5, 50, pop[2]] and kept[stratum == 2].all()
    # the same seed with larger quotas: a superset
    more = emu.sample(3, np.arange(n), mp, edges, [50, 51, 0], eligible)[0]
    assert (more[kept & (stratum < 2)]).all() and not more[stratum == 2].any()
    # the passes give the same sample from (seed, ordinals)
    by_passes = emu.select_by_passes(emu.keys(3, np.arange(n)), stratum, [5, 50, 10 ** 6])[0]
    assert np.array_equal(kept, by_passes)
    assert not np.array_equal(kept, emu.sample(4, np.arange(n), mp, edges, [5, 50, 10 ** 6], eligible)[0])


# ---- 3. sample_pairs' arguments -----------------------------------------------------------------------------
def test_sample_args():
    from splink_amd.select import SAMPLE_MAX_STRATA, sample_args, sample_strata
    assert SAMPLE_MAX_STRATA == emulator().MAX_STRATA == 64
    edges, quota, seed = sample_args(200, 10, 0)
    assert edges == [i / 10 for i in range(11)] and edges[0] == 0.0 and edges[-1] == 1.0
    assert quota == [200] * 10 and seed == 0
    assert sample_args([1, 0, 3], (0.0, 0.5, 0.9, 1.0), 2 ** 64 - 1) == ([0.0, 0.5, 0.9, 1.0], [1, 0, 3], 2 ** 64 - 1)
    assert sample_args(np.int64(4), np.array([0.1, 0.2]), np.uint64(9)) == ([0.1, 0.2], [4], 9)
    assert len(sample_args(0, 64)[0]) == 65
    for strata in (0, 65, -1, True, [0.5], [], [0.0, 0.5, 0.5, 1.0], [0.0, 0.6, 0.5], [0.0, float("nan"), 1.0],
                   [0.0, float("inf")], list(range(66)), "abc", None, 2.5):
        with pytest.raises(ValueError, match="sample_pairs"):
            sample_args(10, strata, 0)
    for per in (-1, [1, 2], [1, 2, 3, 4], [1, -2, 3], [1, 2.5, 3], 2.0, None, True, 2 ** 63, "7"):
        with pytest.raises(ValueError, match="sample_pairs"):
            sample_args(per, [0.0, 0.3, 0.6, 1.0], 0)
    for seed in (-1, 2 ** 64, 1.0, None, True, "0"):
        with pytest.raises(ValueError, match="sample_pairs"):
            sample_args(10, 10, seed)
    # the host's strata of sampled scores: left-closed, the last one closed on the right
    mp = np.array([0.0, 0.3, 0.2999999999999999, 0.6, 1.0, 0.9999999999999999])
    assert list(sample_strata(mp, [0.0, 0.3, 0.6, 1.0])) == [0, 1, 0, 2, 2, 2]
    assert list(emulator().strata_of(mp, [0.0, 0.3, 0.6, 1.0])) == [0, 1, 0, 2, 2, 2]
    assert list(sample_strata(np.array([0.5, 1.0]), [0.5, 1.0])) == [0, 0]


def test_sample_pairs_refusals_without_a_device():
    """The refusals that depend on the frame alone are raised before anything touches the device."""
    from splink_amd.frames import BestMatchFrame, ExpectationFrame, FilteredFrame, SampleFrame
    from splink_amd.select import Predicate

    class FakeJob:
        n_shards = 1
        passthrough = None

    def filtered(parent_cls, n_shards=1):
        parent = object.__new__(parent_cls)
        parent.job = FakeJob()
        parent.job.n_shards = n_shards
        parent.settings = {}
        parent.gammas = parent
        return FilteredFrame(parent, Predicate())

    ok = filtered(ExpectationFrame).sample_pairs(per_stratum=3, strata=[0.0, 0.5, 1.0], seed=1)
    assert isinstance(ok, SampleFrame) and ok._n is None  # lazy: nothing has run
    with pytest.raises(ValueError, match="sample_pairs"):
        filtered(ExpectationFrame).sample_pairs(per_stratum=-1)
    with pytest.raises(ValueError, match="unscored"):
        filtered(FilteredFrame).sample_pairs()
    with pytest.raises(ValueError, match="sharded"):
        filtered(ExpectationFrame, n_shards=2).sample_pairs()
    for name in ("filter", "where", "best_matches", "clusters", "clusters_at_thresholds", "sample_pairs"):
        with pytest.raises(ValueError, match="sample frame"):
            getattr(ok, name)()
    best = object.__new__(BestMatchFrame)
    with pytest.raises(ValueError, match="best-match"):
        best.sample_pairs()
    from splink_amd.term_frequencies import TfFilteredFrame
    with pytest.raises(ValueError, match="term-frequency"):
        object.__new__(TfFilteredFrame).sample_pairs()
