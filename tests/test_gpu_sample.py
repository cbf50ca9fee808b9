"""Random record pairs drawn on the device (spk_pairs_sample) and u estimated from them.

The pairs are compared bit for bit with the host restatement of the definition (tests/sample_common.py); the
comparison pass over them, u, and the EM that holds u fixed are compared with the CPU oracle."""
import copy
import warnings

import numpy as np
import pytest

import sample_common as sc

pytestmark = pytest.mark.gpu
warnings.filterwarnings("ignore")


@pytest.fixture(scope="module")
def amd():
    from splink_amd import AmdSession, _native
    if _native.device_count() == 0:
        pytest.fail("no HIP device visible: the -m gpu tests need an MI355X")
    return AmdSession(0)


def _chunk():
    from splink_amd import _native as N
    return N.SAMPLE_CHUNK


def make_ctx(link_type, n0, n1=None, rank=None, null_div=0):
    from splink_amd import _native as N
    c = N.Context(0)
    c.set_link_type(N.LINK_TYPES[link_type])
    c.table_create(0, n0, 1)
    if n1 is not None:
        c.table_create(1, n1, 1)
    if rank is not None:
        c.table_set_rank(0, np.asarray(rank, dtype=np.int64))
        c.table_set_rank_null(0, null_div)
    return c


def ranks(n, kind, seed=0, right_from=None):
    """(rank per row, null_div): distinct unique ids, duplicated ones, or NULL ids in the spk_table_set_rank_null
    layout; right_from: rows from there on are the second source of link_and_dedupe."""
    rng = np.random.Generator(np.random.PCG64(seed))
    src = np.zeros(n, dtype=np.int64) if right_from is None else (np.arange(n) >= right_from).astype(np.int64)
    if kind == "distinct":
        r, div, nulls = rng.permutation(n).astype(np.int64), n + 1, False
    elif kind == "duplicated":
        r, div, nulls = rng.integers(0, max(n // 2, 1), n).astype(np.int64), n + 1, False
    else:
        r, div, nulls = rng.permutation(n).astype(np.int64), n + 1, True
        r[rng.random(n) < 0.25] = div - 1
        r[0] = div - 1
    return src * div + r, (div if nulls else 0)


def totals():
    c = _chunk()
    return [0, 1, 63, 64, 65, c - 1, c, c + 1, 3 * c + 5]


CASES = [("dedupe_only", "distinct"), ("dedupe_only", "duplicated"), ("dedupe_only", "null"),
         ("link_and_dedupe", "null")]


@pytest.mark.parametrize("n0", [1, 2, 3, 97])
@pytest.mark.parametrize("link_type,kind", CASES, ids=[f"{a}-{b}" for a, b in CASES])
def test_one_table_pairs_equal_the_restatement(link_type, kind, n0, amd):
    from splink_amd import _native as N
    rank, div = ranks(n0, kind, seed=n0, right_from=(n0 // 3 if link_type == "link_and_dedupe" else None))
    c = make_ctx(link_type, n0, rank=rank, null_div=div)
    assert c.pairs_sample_info() == (-1, -1, -1.0)
    kept_any = 0
    for total in totals():
        seed = 1000 + total
        n = c.pairs_sample(N.LINK_TYPES[link_type], seed, total, 0, total)
        l, r = c.pairs_copy(0, n)
        wl, wr = sc.sample(seed, total, 0, total, n0, rank=rank, null_div=div)
        assert n == len(wl) == c.pairs_count(), (total, n, len(wl))
        assert np.array_equal(l, wl) and np.array_equal(r, wr), total
        assert c.pairs_sample_info() == (total, n, -1.0)
        kept_any += n
    if n0 == 1:
        assert kept_any == 0  # one row: no pairs, and no hang
    elif kind == "distinct":
        assert kept_any == sum(totals())  # nothing to drop
    elif n0 == 97:
        assert 0 < kept_any < sum(totals())  # some draws dropped, most kept
    c.close()


@pytest.mark.parametrize("n1", [1, 97])
@pytest.mark.parametrize("n0", [1, 2, 3, 97])
def test_link_only_pairs_equal_the_restatement(n0, n1, amd):
    from splink_amd import _native as N
    c = make_ctx("link_only", n0, n1)
    c.enable_timing(True)
    for total in totals():
        n = c.pairs_sample(N.LINK_TYPES["link_only"], 77, total, 0, total)
        assert n == total  # every draw survives
        l, r = c.pairs_copy(0, n)
        wl, wr = sc.sample(77, total, 0, total, n0, n1=n1)
        assert np.array_equal(l, wl) and np.array_equal(r, wr), total
        draws, kept, ms = c.pairs_sample_info()
        assert (draws, kept) == (total, total) and (ms > 0.0 if total else ms == 0.0)
    c.close()


@pytest.mark.parametrize("link_type", ["dedupe_only", "link_and_dedupe", "link_only"])
def test_ranges_concatenate_to_the_whole_sample(link_type, amd):
    from splink_amd import _native as N
    n0, total = 97, 3 * _chunk() + 5
    lt = N.LINK_TYPES[link_type]
    if link_type == "link_only":
        c = make_ctx(link_type, n0, 41)
    else:
        rank, div = ranks(n0, "null", seed=4, right_from=(40 if link_type == "link_and_dedupe" else None))
        c = make_ctx(link_type, n0, rank=rank, null_div=div)
    n = c.pairs_sample(lt, 5, total, 0, total)
    whole = c.pairs_copy(0, n)
    cuts = [0, 7, _chunk() + 130, total - 1, total]  # uneven, not on a workgroup's boundary; the last of one draw
    parts, kept = [], 0
    for a, b in zip(cuts, cuts[1:]):
        k = c.pairs_sample(lt, 5, total, a, b - a)
        assert c.pairs_sample_info()[:2] == (b - a, k)
        parts.append(c.pairs_copy(0, k))
        kept += k
    assert kept == n and (link_type == "link_only" or 0 < n < total)
    assert np.array_equal(np.concatenate([p[0] for p in parts]), whole[0])
    assert np.array_equal(np.concatenate([p[1] for p in parts]), whole[1])
    assert c.pairs_sample(lt, 5, total, total, 0) == 0  # the empty range at the end
    c.close()


@pytest.mark.parametrize("link_type", ["dedupe_only", "link_and_dedupe", "link_only"])
def test_sampled_pairs_are_pairs_of_the_cartesian_block(link_type, amd):
    from splink_amd import _native as N
    n0, n1 = 60, (35 if link_type == "link_only" else None)
    lt = N.LINK_TYPES[link_type]
    rank, div = (None, 0) if n1 else ranks(n0, "null", seed=8, right_from=(25 if link_type == "link_and_dedupe" else None))
    c = make_ctx(link_type, n0, n1, rank=rank, null_div=div)
    c.table_set_key(0, 0, 0, np.zeros(n0, dtype=np.int64))  # no rules: one key for every row
    c.table_set_key(1 if n1 else 0, 0, 1, np.zeros(n1 or n0, dtype=np.int64))
    n_all, _ = c.block(lt, [1])
    legal = set(zip(*[a.tolist() for a in c.pairs_copy(0, n_all)]))
    assert len(legal) == n_all > 0
    n = c.pairs_sample(lt, 21, 6000, 0, 6000)
    got = set(zip(*[a.tolist() for a in c.pairs_copy(0, n)]))
    assert got <= legal and len(got) > n_all // 2
    c.close()


def test_error_paths_leave_no_pair_set(amd):
    from splink_amd import _native as N
    D = N.LINK_TYPES["dedupe_only"]

    def no_pairs(c):
        with pytest.raises(RuntimeError, match="no pairs"):
            c.pairs_count()
        assert c.pairs_sample_info() == (-1, -1, -1.0)

    c = N.Context(0)
    with pytest.raises(RuntimeError, match="tables not loaded"):  # SPK_E_STATE
        c.pairs_sample(D, 0, 10, 0, 10)
    no_pairs(c)
    c.table_create(0, 8, 1)
    with pytest.raises(RuntimeError, match="rank not set"):  # SPK_E_STATE: dedupe needs ranks
        c.pairs_sample(D, 0, 10, 0, 10)
    with pytest.raises(RuntimeError, match="tables not loaded"):  # link_only needs table 1
        c.pairs_sample(N.LINK_TYPES["link_only"], 0, 10, 0, 10)
    no_pairs(c)
    c.set_link_type(D)
    c.table_set_rank(0, np.arange(8, dtype=np.int64))
    assert c.pairs_sample(D, 0, 10, 0, 10) == 10 and c.pairs_count() == 10
    for total, first, count in [(-1, 0, 0), (10, -1, 1), (10, 0, -1), (10, 5, 6), (10, 11, 0)]:  # SPK_E_INVALID
        assert c.pairs_sample(D, 0, 10, 0, 10) == 10
        with pytest.raises(ValueError, match="range"):
            c.pairs_sample(D, 0, total, first, count)
        no_pairs(c)
    with pytest.raises(ValueError, match="link_type"):
        c.pairs_sample(3, 0, 10, 0, 10)
    assert c.pairs_sample(D, 0, 10, 0, 10) == 10
    with pytest.raises(ValueError, match="63 bits"):  # SPK_E_LIMIT: total_draws x n0
        c.pairs_sample(D, 0, 1 << 60, 0, 10)
    no_pairs(c)
    assert c.pairs_sample(D, 0, (1 << 60) - 1, (1 << 59), 10) == 10  # the largest sample these 8 rows allow
    l, r = c.pairs_copy(0, 10)
    wl, wr = sc.sample(0, (1 << 60) - 1, 1 << 59, 10, 8, rank=np.arange(8))
    assert np.array_equal(l, wl) and np.array_equal(r, wr)
    c.close()


# ---- the comparison pass, u, and the EM that holds it --------------------------------------------------------
@pytest.fixture(scope="module")
def world():
    """The 300 records, the restated 20,000 draws of seed U_SEED and the oracle's gammas over them, shared by the
    tests below (read only)."""
    df = sc.records()
    st = sc.settings()
    rank = df["unique_id"].to_numpy().astype(np.int64)  # distinct integer ids: the rank order is the id order
    l, r = sc.sample(sc.U_SEED, sc.N_DRAWS, 0, sc.N_DRAWS, len(df), rank=rank)
    g = sc.oracle_gammas(df, l, r, st)
    return {"df": df, "l": l, "r": r, "g": g, "u": sc.host_u(g, sc.LEVELS)}


def test_comparison_pass_on_a_sampled_set(amd, world):
    from splink_amd import add_gammas, random_pairs
    frame = random_pairs(copy.deepcopy(sc.settings()), amd, sc.N_DRAWS, seed=sc.U_SEED, df=world["df"])
    job = frame.job
    assert job.n_pairs == len(world["l"]) == sc.N_DRAWS and job.perm[0] is None
    l, r = job.ctx.pairs_copy(0, job.n_pairs)
    assert np.array_equal(l, world["l"]) and np.array_equal(r, world["r"])
    gf = add_gammas(frame, copy.deepcopy(sc.settings()), amd)
    assert list(gf.meta[0]) == sc.NAMES and list(gf.meta[1]) == sc.LEVELS
    got = gf.gamma_matrix()
    assert got.shape == world["g"].shape and np.array_equal(got, world["g"])
    assert len({tuple(v) for v in world["g"].tolist()}) > 20  # a pattern space worth comparing
    hist = job.pattern_histogram()
    assert hist.dtype == np.int64 and hist.sum() == sc.N_DRAWS
    pdf = gf.toPandas()
    assert len(pdf) == sc.N_DRAWS and (pdf["unique_id_l"] < pdf["unique_id_r"]).all()


@pytest.fixture
def nccl_group():
    import socket
    import torch
    import torch.distributed as dist
    torch.cuda.set_device(0)
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1,
                            device_id=torch.device("cuda:0"))
    yield dist
    dist.destroy_process_group()


def test_pattern_histogram_through_the_all_reduce(amd, world, nccl_group):
    """force_reduce, as tests/test_gpu_dist.py sets it for the EM histogram: the sampled set's histogram goes through
    the RCCL all-reduce at one rank and comes back the same, for a range of the sample and for an empty one."""
    import oracle as orc
    from splink_amd import add_gammas, random_pairs
    frame = random_pairs(copy.deepcopy(sc.settings()), amd, sc.N_DRAWS, seed=sc.U_SEED, df=world["df"])
    job = frame.job
    gf = add_gammas(frame, copy.deepcopy(sc.settings()), amd)
    want = np.zeros(int(np.prod([L + 1 for L in sc.LEVELS])), dtype=np.int64)
    orc.pattern_codes(world["g"], sc.LEVELS, hist=want, want_codes=False)
    local = job.pattern_histogram()
    job.force_reduce = True
    reduced = job.pattern_histogram()
    assert np.array_equal(local, want) and np.array_equal(reduced, want)
    job.sample_pairs(sc.N_DRAWS, sc.N_DRAWS, 0, sc.U_SEED)  # a rank whose share has run out
    job.gammas(gf.settings)
    assert job.n_pairs == 0 and not job.pattern_histogram().any()
    job.force_reduce = False


def _linker(amd, df, rules=()):
    from splink_amd import Splink
    return Splink(copy.deepcopy(sc.settings(rules)), amd, df=df)


def _u_of(params_dict):
    return [[params_dict["π"][n]["prob_dist_non_match"][f"level_{v}"]["probability"] for v in range(L)]
            for n, L in zip(sc.NAMES, sc.LEVELS)]


def _m_of(params_dict):
    return [[params_dict["π"][n]["prob_dist_match"][f"level_{v}"]["probability"] for v in range(L)]
            for n, L in zip(sc.NAMES, sc.LEVELS)]


def test_u_end_to_end(amd, world):
    from splink_amd import estimate_u_using_random_sampling
    linker = _linker(amd, world["df"])
    m0, lam0 = _m_of(linker.params.params), linker.params.params["λ"]
    u_before = _u_of(linker.params.params)
    table = linker.estimate_u_using_random_sampling(sc.N_DRAWS, seed=sc.U_SEED)
    want_u, want_counts = world["u"]
    assert _u_of(linker.params.params) == want_u != u_before  # exactly the host's u from the oracle's gammas
    assert _m_of(linker.params.params) == m0 and linker.params.params["λ"] == lam0
    assert len(linker.params.param_history) == 1 and _u_of(linker.params.param_history[0]) == u_before
    assert linker.params.fix_u_probabilities is True
    assert list(table.columns) == ["gamma_col", "gamma_value", "count", "u_probability"]
    assert len(table) == sum(L + 1 for L in sc.LEVELS)
    for k, (name, L) in enumerate(zip(sc.NAMES, sc.LEVELS)):
        rows = table[table["gamma_col"] == name]
        assert rows["gamma_value"].tolist() == list(range(-1, L))
        assert rows["count"].tolist() == want_counts[k].tolist()
        assert np.isnan(rows["u_probability"].iloc[0]) and rows["u_probability"].tolist()[1:] == want_u[k]
    # the same in batches of 1000 draws, and without fixing
    other = _linker(amd, world["df"])
    t2 = estimate_u_using_random_sampling(other.settings, other.params, amd, sc.N_DRAWS, seed=sc.U_SEED,
                                          batch_pairs=1000, fix=False, df=world["df"])
    assert _u_of(other.params.params) == want_u and other.params.fix_u_probabilities is False
    assert t2.equals(table)
    with pytest.raises(ValueError):
        estimate_u_using_random_sampling(other.settings, other.params, amd, 0, df=world["df"])


RULES = ["l.city = r.city", "l.first_name = r.first_name"]


def _blocked_hist(df, st):
    """The oracle's pattern histogram of the rule-blocked pairs."""
    import oracle as orc
    full = dict(st, unique_id_column_name="unique_id")
    pairs, left, right = orc.block(full, df=df)
    g = sc.oracle_gammas(df, pairs["row_l"].to_numpy(), pairs["row_r"].to_numpy(), st)
    hist = np.zeros(int(np.prod([L + 1 for L in sc.LEVELS])), dtype=np.int64)
    orc.pattern_codes(g, sc.LEVELS, hist=hist, want_codes=False)
    return hist


def test_em_with_fixed_u(amd, world):
    import oracle as orc
    from parity_common import rel_close
    df, (want_u, _) = world["df"], world["u"]
    st = sc.settings(RULES)
    hist = _blocked_hist(df, st)
    assert hist.sum() > 500
    linker = _linker(amd, df, RULES)
    linker.estimate_u_using_random_sampling(sc.N_DRAWS, seed=sc.U_SEED)
    lam, m = linker.params.params["λ"], _m_of(linker.params.params)
    linker.get_scored_comparisons()
    history = linker.params.param_history[1:] + [linker.params.params]  # [0]: before the sampled u
    assert len(history) == st["max_iterations"] + 1
    assert all(_u_of(p) == want_u for p in history)  # every iteration has the sampled u
    for it, p in enumerate(history[1:]):
        stats = orc.em_stats_hist(hist, sc.LEVELS, lam, m, want_u)
        lam, m, moved_u = orc.m_step(stats, sc.LEVELS)  # the u it would move to is dropped: u stays the sampled one
        assert moved_u != want_u
        assert rel_close(p["λ"], lam), (it, p["λ"], lam)
        for a, b in zip(sum(_m_of(p), []), sum(m, [])):
            assert rel_close(a, b), (it, a, b)
    # fix=False: the first M-step moves u, so the flag is what holds it
    free = _linker(amd, df, RULES)
    free.estimate_u_using_random_sampling(sc.N_DRAWS, seed=sc.U_SEED, fix=False)
    assert _u_of(free.params.params) == want_u
    free.get_scored_comparisons()
    assert _u_of(free.params.param_history[2]) != want_u


def test_the_estimate_is_close_to_the_exact_u(amd, world):
    """Every level's sampled u within 6 binomial standard errors (+ 1 / n) of the exact u over all 44,850 pairs
    of the 300 records with the true matches (equal synthetic cluster) removed."""
    from splink_amd import add_gammas, complete_settings_dict
    from splink_amd.blocking import cartesian_block
    df = world["df"]
    st = copy.deepcopy(sc.settings())
    st["additional_columns_to_retain"] = ["cluster"]
    st = complete_settings_dict(st, amd)
    pdf = add_gammas(cartesian_block(st, amd, df=df), st, amd).toPandas()
    assert len(pdf) == 300 * 299 // 2
    non = pdf[pdf["cluster_l"] != pdf["cluster_r"]]
    assert 0 < len(pdf) - len(non) < 500
    linker = _linker(amd, df)
    table = linker.estimate_u_using_random_sampling(sc.N_DRAWS, seed=sc.U_SEED)
    for name, L in zip(sc.NAMES, sc.LEVELS):
        g = non[name].to_numpy()
        rows = table[table["gamma_col"] == name]
        n_nonnull = int(rows["count"].iloc[1:].sum())
        for v in range(L):
            p = float((g == v).sum()) / float((g >= 0).sum())
            got = float(rows["u_probability"].iloc[v + 1])
            bound = 6 * np.sqrt(p * (1 - p) / n_nonnull) + 1 / n_nonnull
            print(name, v, "exact", p, "sampled", got, "bound", bound)
            assert abs(got - p) <= bound, (name, v, p, got, bound)
