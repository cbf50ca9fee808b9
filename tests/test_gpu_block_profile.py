"""The blocking-rule profile on the device (spk_block_profile, comparison_evaluation.py): the reference's
get_largest_blocks fixture, the per-rule pair counts against the SQL oracle and against the blocking call itself, the
key-level figures against tests/profile_common.py, candidate spaces past 2^32, the untouched context, the errors."""
import ctypes
import time

import numpy as np
import pandas as pd
import pytest

import profile_common as pc
from conftest import load_golden
from parity_common import frame

from splink_amd.comparison_evaluation import get_largest_blocks, profile_blocking_rules

pytestmark = pytest.mark.gpu

LINK_TYPES = ["dedupe_only", "link_only", "link_and_dedupe"]
KEY_FIELDS = ("rows_l", "rows_r", "blocks", "candidates", "largest_candidates")


@pytest.fixture(scope="module")
def amd():
    from splink_amd import AmdSession, _native
    if _native.device_count() == 0:
        pytest.fail("no HIP device visible: the -m gpu tests need an MI355X")
    return AmdSession(0)


# ---- 1. the reference's fixture -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden_blocks():
    g = load_golden("largest_blocks")
    return frame(g["table"]), g["cases"]


def check_largest(got, table, want_rows):
    cols = [c for c in want_rows if c != "count"]
    assert list(got.columns) == cols + ["count"]
    assert got["count"].tolist() == want_rows["count"]  # the multiset: no tie order is pinned
    sizes = table.dropna(subset=cols).groupby(cols).size()
    seen = set()
    for row in got.itertuples(index=False):
        key = tuple(row[:-1])
        assert all(v is not None and v == v for v in key) and key not in seen
        seen.add(key)
        assert int(sizes[key if len(key) > 1 else key[0]]) == row[-1]


@pytest.mark.parametrize("case", range(6))
def test_get_largest_blocks_matches_the_reference(amd, golden_blocks, case):
    table, cases = golden_blocks
    c = cases[case]
    out = get_largest_blocks(c["rule"], table, amd, limit=c["limit"])
    got = out.toPandas()
    assert out.count() == c["limit"] and out.columns == list(got.columns) and out.to_pandas().equals(got)
    check_largest(got, table, c["rows"])


def test_get_largest_blocks_without_a_unique_id_and_with_a_residual(amd, golden_blocks):
    table, cases = golden_blocks
    c = cases[3]  # l.city = r.city and l.dob = r.dob, limit 8
    bare = table.drop(columns=["unique_id"])
    check_largest(get_largest_blocks(c["rule"], bare, amd, limit=c["limit"]).toPandas(), table, c["rows"])
    # profiled on its key terms: the same blocks as the key-only rule
    res = get_largest_blocks("l.surname = r.surname and levenshtein(l.first_name, r.first_name) <= 2", bare, amd, 8)
    check_largest(res.toPandas(), table, cases[1]["rows"])
    assert get_largest_blocks("l.surname = r.surname", bare, amd, limit=0).count() == 0
    assert get_largest_blocks("l.surname = r.surname", bare, amd, limit=1000).count() == table["surname"].nunique()


# ---- 2. per-rule pair counts against the SQL oracle ----------------------------------------------------------------
ORACLE_RULES = ["l.city = r.city", "l.first_name = r.surname", "substr(l.surname,1,2) = substr(r.surname,1,2)"]


def people(n, seed):
    """n records: 6 cities (blocks of ~n/6 rows), first names and surnames from one vocabulary (so that first_name =
    surname joins), NULLs in every key column, NULL and repeated unique ids."""
    rng = np.random.default_rng(seed)
    names = np.array(["adam", "adele", "bo", "bob", "carl", "carla", "dee", "dev", "ed", "eda", "flo", "fay"],
                     dtype=object)
    cities = np.array(["ayr", "bath", "cork", "deal", "ely", "fife"], dtype=object)

    def pick(vocab, p_null):
        v = vocab[rng.integers(0, len(vocab), n)].copy()
        v[rng.random(n) < p_null] = None
        return v

    uid = rng.permutation(n).astype(object)
    uid[rng.integers(0, n, 8)] = uid[rng.integers(0, n, 8)]  # repeated ids
    uid[rng.integers(0, n, 6)] = None
    return pd.DataFrame({"unique_id": uid, "first_name": pick(names, 0.05), "surname": pick(names, 0.05),
                         "city": pick(cities, 0.04)})


def oracle_settings(link_type, rules):
    return {"link_type": link_type, "blocking_rules": list(rules),
            "comparison_columns": [{"col_name": "first_name", "num_levels": 2}, {"col_name": "surname", "num_levels": 2}],
            "additional_columns_to_retain": ["city"]}


def job_tables(link_type, df):
    if link_type == "dedupe_only":
        return dict(df=df)
    return dict(df_l=df.iloc[:230].reset_index(drop=True), df_r=df.iloc[170:].reset_index(drop=True))


@pytest.mark.parametrize("link_type", LINK_TYPES)
def test_enumerated_per_rule_matches_the_oracle(amd, link_type):
    import oracle as orc
    tables = job_tables(link_type, people(400, 5))
    totals = [len(orc.block(oracle_settings(link_type, ORACLE_RULES[:k + 1]), **tables)[0]) for k in range(3)]
    want = [totals[0], totals[1] - totals[0], totals[2] - totals[1]]
    assert all(w > 0 for w in want)
    p = profile_blocking_rules(oracle_settings(link_type, ORACLE_RULES), amd, limit=3, max_enumerate=-1, **tables)
    print(link_type, p.rules.to_string())
    assert p.rules["rule"].tolist() == ORACLE_RULES
    assert p.rules["enumerated"].tolist() == want
    assert p.rules["pairs"].tolist() == want and p.rules["cumulative_pairs"].tolist() == totals
    # more than one count-pass workgroup (2048 ordinals) per rule, and a block that straddles a workgroup border
    assert (p.rules["candidates"] > 2048).all()
    assert 0 < p.largest_blocks(0)["candidates"].iloc[-1] and p.rules["blocks"].iloc[0] == 6
    # no rules: the cartesian block
    cart = profile_blocking_rules(oracle_settings(link_type, []), amd, max_enumerate=-1, **tables)
    n_cart = len(orc.block(oracle_settings(link_type, []), **tables)[0])
    assert len(cart.rules) == 1 and cart.rules["blocks"].tolist() == [1]
    assert cart.rules["enumerated"].tolist() == [n_cart] and cart.rules["pairs"].tolist() == [n_cart]
    assert list(cart.largest_blocks(0).columns) == ["rows_l", "rows_r", "candidates"]


# ---- 3. against the blocking call itself -----------------------------------------------------------------------
def blocked_job(link_type, df, rules):
    from splink_amd.blocking import _tables
    from splink_amd.compiler import compile_rule
    from splink_amd.engine import Job
    from splink_amd.settings import complete_settings_dict
    st = complete_settings_dict(oracle_settings(link_type, rules), "supress_warnings")
    job = Job(link_type, _tables(st, **{"df_l": None, "df_r": None, "df": None, **job_tables(link_type, df)}),
              "unique_id", 0)
    job.block(list(rules))
    sym = [1 if compile_rule(r, job.schema).symmetric else 0 for r in rules]
    return job, sym


def same_key_level(a, b):
    for f in KEY_FIELDS:
        assert a[0][f].tolist() == b[0][f].tolist(), f
    assert (a[1] == b[1]).all()
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a[2], b[2]))


@pytest.mark.parametrize("link_type", ["dedupe_only", "link_only"])
def test_profile_agrees_with_block(amd, link_type):
    from splink_amd import _native as N
    job, sym = blocked_job(link_type, people(400, 5), ORACLE_RULES)
    lt = N.LINK_TYPES[link_type]
    whole = job.ctx.block_profile(lt, sym, None, 0, 1, -1, N.LARGEST_BY_CANDIDATES, 4)
    rules = whole[0]
    assert int(rules["enumerated"].sum()) == job.n_pairs and int(rules["candidates"].sum()) == job.n_candidates
    assert job.ctx.block_profile_info()[2] == job.n_candidates
    # shards: the same key-level outputs, and the shards' counts add up to the whole
    for S in (3, 7):
        parts = [job.ctx.block_profile(lt, sym, None, s, S, -1, N.LARGEST_BY_CANDIDATES, 4) for s in range(S)]
        for part in parts:
            same_key_level(part, whole)
        assert sum(p[0]["enumerated"] for p in parts).tolist() == rules["enumerated"].tolist()
        # each shard's sum is what spk_block emits for that shard (the middle one is checked)
        n_pairs, _ = job.ctx.block(lt, sym, S // 2, S)
        assert int(parts[S // 2][0]["enumerated"].sum()) == n_pairs
    # a cap between two rules' ranges: only the rules at or below it are enumerated
    cands = sorted(int(c) for c in rules["candidates"])
    assert cands[0] < cands[1]
    capped = job.ctx.block_profile(lt, sym, None, 0, 1, (cands[0] + cands[1]) // 2, N.LARGEST_BY_CANDIDATES, 4)
    same_key_level(capped, whole)
    small = int(np.argmin(rules["candidates"]))
    for r in range(3):
        assert int(capped[0]["enumerated"][r]) == (int(rules["enumerated"][r]) if r == small else -1)
    assert job.ctx.block_profile_info()[2] == cands[0]
    never = job.ctx.block_profile(lt, sym, None, 0, 1, 0, N.LARGEST_BY_CANDIDATES, 4)
    same_key_level(never, whole)
    assert never[0]["enumerated"].tolist() == [-1, -1, -1] and job.ctx.block_profile_info()[2] == 0
    # the measurement switch changes no result
    job.ctx.block_profile_set_cut(False)
    same_key_level(job.ctx.block_profile(lt, sym, None, 0, 1, 0, N.LARGEST_BY_CANDIDATES, 4), whole)
    job.ctx.block_profile_set_cut(True)


# ---- 4. rules with residual predicates ----------------------------------------------------------------------
# tests/test_gpu_residual.py's MEDIUM_RULES
MEDIUM_RULES = ["l.surname = r.surname and levenshtein(l.first_name, r.first_name) <= 2",
                "l.dob = r.dob and l.city != r.city",
                "l.surname = r.surname"]


def test_residual_rules_enumerate_what_block_residual_enumerates(amd):
    from splink_amd import _native as N
    from splink_amd.engine import Job
    from splink_amd.synthetic import make_records
    df = make_records(2000, seed=23, surname_vocab=100, first_vocab=30, city_vocab=20)[
        ["unique_id", "first_name", "surname", "dob", "city", "email"]]
    df["dob"] = df["dob"].str[:4]
    job = Job("dedupe_only", [df], "unique_id", 0)
    job.block(MEDIUM_RULES)
    enumerated, _ = job.ctx.block_residual_info()
    assert enumerated > job.n_pairs > 0
    rules, _, _ = job.ctx.block_profile(0, [1, 1, 1], [0, 1, -1], 0, 1, -1, N.LARGEST_BY_CANDIDATES, 0)
    assert int(rules["enumerated"].sum()) == enumerated
    assert int(rules["candidates"].sum()) == job.n_candidates
    # rule 2 repeats rule 0's key; rule 0 has a program, so it excludes nothing
    assert int(rules["enumerated"][2]) > 0
    # without the programs rule 0's key excludes all of rule 2
    plain, _, _ = job.ctx.block_profile(0, [1, 1, 1], None, 0, 1, -1, N.LARGEST_BY_CANDIDATES, 0)
    assert int(plain["enumerated"][2]) == 0 and plain["enumerated"][0] == rules["enumerated"][0]
    st = {"link_type": "dedupe_only", "blocking_rules": ["l.city = r.city and l.dob = r.dob"] + MEDIUM_RULES,
          "comparison_columns": [{"col_name": "first_name", "num_levels": 2}, {"col_name": "surname", "num_levels": 2}],
          "additional_columns_to_retain": ["city", "dob"]}
    p = profile_blocking_rules(st, amd, df=df, max_enumerate=-1).rules
    assert p["enumerated"].notna().all()
    assert p["pairs"].isna().tolist() == [False, True, True, True]
    assert p["pairs"].iloc[0] == p["enumerated"].iloc[0] == p["cumulative_pairs"].iloc[0]
    assert p["cumulative_pairs"].isna().tolist() == [False, True, True, True]


# ---- 5. key-level figures -------------------------------------------------------------------------------------
def shapes(n, seed, shift=0):
    """Blocks of many sizes: `a` in blocks of 1, 1, 2, 3, 5, 9, 17, 40 rows ... plus NULLs; `b` strings whose first
    two characters make ~8 blocks; `c` mostly values that `a` never takes; `z` NULL in every row."""
    rng = np.random.default_rng(seed)
    sizes = [1, 1, 1, 2, 3, 5, 9, 17, 40]
    a = np.concatenate([np.full(s, f"v{i + shift}", dtype=object) for i, s in enumerate(sizes)])
    a = np.concatenate([a, rng.choice(np.array(["p", "q", "r"], dtype=object), n - len(a))])
    a[rng.random(n) < 0.1] = None
    b = np.array([rng.choice(list("abcd")) + rng.choice(list("xy")) + str(i % 7) for i in range(n)], dtype=object)
    b[rng.random(n) < 0.1] = None
    c = np.where(rng.random(n) < 0.2, "v7", np.array([f"w{i % 5}" for i in range(n)], dtype=object)).astype(object)
    order = rng.permutation(n)
    return pd.DataFrame({"unique_id": np.arange(n), "a": a[order], "b": b[order], "c": c[order],
                         "z": np.full(n, np.nan)})


KEY_RULES = [("l.a = r.a", [("a", None)], [("a", None)]),
             ("substr(l.b, 1, 2) = substr(r.b, 1, 2)", [("b", (1, 2))], [("b", (1, 2))]),
             ("l.a = r.c", [("a", None)], [("c", None)]),
             ("l.z = r.z", [("z", None)], [("z", None)]),
             ("l.a = r.a and substr(l.b, 2, 1) = substr(r.b, 2, 1)", [("a", None), ("b", (2, 1))],
              [("a", None), ("b", (2, 1))])]


@pytest.mark.parametrize("link_type", ["dedupe_only", "link_only"])
def test_key_level_figures(amd, link_type):
    from splink_amd import _native as N
    from splink_amd.compiler import compile_rule
    from splink_amd.engine import Job
    df_l = shapes(300, 3)
    tables = [df_l] if link_type == "dedupe_only" else [df_l, shapes(260, 4, shift=2)]
    df_r = tables[-1]
    job = Job(link_type, tables, "unique_id", 0, cluster=False)
    specs = [compile_rule(text, job.schema) for text, _, _ in KEY_RULES]
    want = []
    for (text, el, er), spec in zip(KEY_RULES, specs):
        kl = pc.key_tuples(df_l, el)
        tri = link_type == "dedupe_only" and spec.symmetric
        want.append((pc.figures(kl, None if tri else pc.key_tuples(df_r, er)), kl))
    # the shapes the issue names: one-row blocks, l-keys without an r partner, a rule without any key
    assert want[0][0]["hist"][0][0] >= 1 and want[3][0]["blocks"] == 0
    assert any(v[1] == 0 for v in want[2][0]["per_block"].values())
    for by, name in ((N.LARGEST_BY_CANDIDATES, "candidates"), (N.LARGEST_BY_ROWS_L, "rows_l")):
        for limit in (0, 4, 1000):
            rules, hist, largest = job.profile_rules(specs, max_enumerate=0, largest_by=by, limit=limit)
            assert rules["enumerated"].tolist() == [-1] * len(specs)
            for r, (w, kl) in enumerate(want):
                pc.check_rule(rules[r], hist[r], largest[r], w, limit, name, lambda row, kl=kl: kl[row])
    assert len(largest[3]) == 0 and not hist[3].any()


def bare_context(N, link_type, keys_l, keys_r=None, rank=None):
    ctx = N.Context(0)
    lt = N.LINK_TYPES[link_type]
    ctx.set_link_type(lt)
    ctx.table_create(0, len(keys_l), 0)
    if link_type == "link_only":
        ctx.table_create(1, len(keys_r), 0)
        ctx.table_set_key(1, 0, 1, keys_r)
    else:
        ctx.table_set_rank(0, np.arange(len(keys_l), dtype=np.int64) if rank is None else rank)
        ctx.table_set_rank_null(0, 0)
        ctx.table_set_key(0, 0, 1, keys_l)
    ctx.table_set_key(0, 0, 0, keys_l)
    return ctx, lt


@pytest.mark.parametrize("link_type", ["dedupe_only", "link_only"])
def test_empty_tables(amd, link_type):
    from splink_amd import _native as N
    none = np.zeros(0, dtype=np.int64)
    for keys_l, keys_r in ((none, none), (none, np.zeros(3, dtype=np.int64)), (np.zeros(3, dtype=np.int64), none)):
        if link_type == "dedupe_only" and len(keys_l) != len(keys_r):
            continue
        ctx, lt = bare_context(N, link_type, keys_l, keys_r)
        rules, hist, largest = ctx.block_profile(lt, [1], None, 0, 1, -1, N.LARGEST_BY_CANDIDATES, 3)
        r = rules[0]
        assert (int(r["rows_l"]), int(r["rows_r"])) == (len(keys_l), len(keys_r))
        assert int(r["blocks"]) == (1 if len(keys_l) else 0)
        assert int(r["candidates"]) == int(r["largest_candidates"]) == int(r["enumerated"]) == 0
        assert hist[0, 1:].sum() == 0 and hist[0, 0].tolist() == [int(r["blocks"]), 0]
        assert len(largest[0]) == int(r["blocks"])
        ctx.close()


# ---- 6. past 2^32 candidates ------------------------------------------------------------------------------------
def check_big(ctx, lt, N, n_l, n_r, total):
    before = ctx.memory()
    t0 = time.perf_counter()
    rules, hist, largest = ctx.block_profile(lt, [1], None, 0, 1, -1, N.LARGEST_BY_CANDIDATES, 2)
    seconds = time.perf_counter() - t0
    print(f"{total} ordinals profiled with enumeration in {seconds:.3f} s")
    r = rules[0]
    assert total > 2 ** 32
    assert int(r["candidates"]) == int(r["enumerated"]) == int(r["largest_candidates"]) == total
    assert (int(r["rows_l"]), int(r["rows_r"]), int(r["blocks"])) == (n_l, n_r, 1)
    want_hist = np.zeros((N.PROFILE_BINS, 2), dtype=np.int64)
    want_hist[33] = [1, total]
    assert total.bit_length() == 33 and (hist[0] == want_hist).all()
    assert len(largest[0]) == 1
    e = largest[0][0]
    assert (int(e["rows_l"]), int(e["rows_r"]), int(e["candidates"])) == (n_l, n_r, total)
    assert ctx.block_profile_info()[2] == total  # three slabs of at most 2^31 ordinals
    after = ctx.memory()
    assert after == before and after["pairs"] == 0
    with pytest.raises(RuntimeError):
        ctx.pairs_count()  # and no pair set appeared


def test_dedupe_cartesian_past_2_32(amd):
    from splink_amd import _native as N
    n = 92683
    ctx, lt = bare_context(N, "dedupe_only", np.zeros(n, dtype=np.int64),
                           rank=np.random.default_rng(1).permutation(n).astype(np.int64))
    check_big(ctx, lt, N, n, n, 4295022903)
    ctx.close()


def test_link_only_constant_key_past_2_32(amd):
    from splink_amd import _native as N
    n = 65537
    ctx, lt = bare_context(N, "link_only", np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64))
    check_big(ctx, lt, N, n, n, 4295098369)
    ctx.close()


# ---- 7. the context is left as it was ---------------------------------------------------------------------------
def test_profile_leaves_the_context_untouched(amd):
    from splink_amd import Splink
    from splink_amd import _native as N
    from splink_amd.synthetic import cfg_settings, make_records
    df = make_records(1500, seed=5, surname_vocab=60, first_vocab=80, city_vocab=30)[
        ["unique_id", "first_name", "surname", "dob", "city", "email"]]
    settings = cfg_settings(2, max_iterations=3)
    linker = Splink(settings, amd, df=df)
    df_e = linker.get_scored_comparisons()
    kept = df_e.filter("match_probability > 0.3")
    n_kept = kept.count()
    job = df_e.job
    ctx, n, K = job.ctx, job.n_pairs, len(settings["comparison_columns"])
    assert 0 < n_kept < n

    def snapshot():
        return (ctx.pairs_copy(0, n), ctx.gammas_copy(K, 0, n), ctx.select_copy(0, n_kept, K), ctx.memory(),
                ctx.select_info()[0], ctx.pairs_count())

    def same(a, b):
        if isinstance(a, (tuple, list)):
            return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
        if isinstance(a, np.ndarray):
            return a.dtype == b.dtype and a.tobytes() == b.tobytes()
        return a == b

    before = snapshot()
    rules, _, _ = ctx.block_profile(N.LINK_TYPES["dedupe_only"], [1, 1], None, 0, 1, -1, N.LARGEST_BY_CANDIDATES, 5)
    assert int(rules["enumerated"].sum()) == n and int(rules["candidates"].sum()) == job.n_candidates
    # under another link type as well: the context's own is handed back
    ctx.block_profile(N.LINK_TYPES["link_and_dedupe"], [1, 1], None, 1, 3, -1, N.LARGEST_BY_ROWS_L, 2)
    assert same(snapshot(), before)  # select_copy refuses a stale selection: it is still current
    assert kept.count() == n_kept and job.selection_owner is kept
    want = kept.toPandas()
    assert len(want) == n_kept
    # a linker that profiles its rules first scores as one that does not (a fresh linker: EM moves a linker's params)
    first = df_e.toPandas()
    other = Splink(cfg_settings(2, max_iterations=3), amd, df=df)
    p = other.profile_blocking_rules(limit=3)
    assert p.rules["pairs"].sum() == n and p.rules["cumulative_pairs"].iloc[-1] == n
    assert list(p.largest_blocks(0).columns) == ["surname", "rows_l", "rows_r", "candidates"]
    assert p.histogram(1)["blocks"].sum() == p.rules["blocks"].iloc[1]
    again = other.get_scored_comparisons().toPandas()
    pd.testing.assert_frame_equal(again, first, check_exact=True)


# ---- 8. errors ---------------------------------------------------------------------------------------------------
def test_error_codes(amd):
    from splink_amd import _native as N
    keys = np.array([0, 0, 1, -1], dtype=np.int64)
    ctx, lt = bare_context(N, "dedupe_only", keys)
    lib, h = ctx._lib, ctx._h
    sym = np.ones(2, dtype=np.int32)
    rules = np.zeros(2, dtype=N.RULE_PROFILE_DTYPE)
    largest = np.zeros((2, 4), dtype=N.BLOCK_ENTRY_DTYPE)
    n_largest = np.zeros(2, dtype=np.int32)

    def call(link_type=lt, n_rules=1, shard=0, n_shards=1, largest_by=0, limit=4, out_largest=largest,
             out_n=n_largest):
        p = lambda a: ctypes.c_void_p(0) if a is None else ctypes.c_void_p(a.ctypes.data)  # noqa: E731
        return lib.spk_block_profile(h, ctypes.c_int(link_type), ctypes.c_int(n_rules), p(sym), p(None),
                                     ctypes.c_int(shard), ctypes.c_int(n_shards), ctypes.c_int64(-1),
                                     ctypes.c_int(largest_by), ctypes.c_int(limit), p(rules), p(None), p(out_largest),
                                     p(out_n))

    assert call() == N.SPK_OK and int(rules[0]["enumerated"]) == 1 and int(n_largest[0]) == 2
    assert ctx.block_profile_info()[2] == 1
    assert call(limit=0, out_largest=None, out_n=None) == N.SPK_OK
    for bad in (dict(limit=-1), dict(out_largest=None), dict(out_n=None), dict(largest_by=2), dict(largest_by=-1),
                dict(shard=1), dict(shard=-1), dict(n_shards=0), dict(link_type=3), dict(link_type=-1),
                dict(n_rules=0), dict(n_rules=33)):
        assert call(**bad) == N.SPK_E_INVALID, bad
        assert ctx.block_profile_info() == (-1.0, -1.0, -1)
    assert call(n_rules=2) == N.SPK_E_STATE  # rule 1 has no keys
    assert call(link_type=N.LINK_TYPES["link_only"]) == N.SPK_E_STATE  # table 1 is not loaded
    with pytest.raises(ValueError):
        ctx.block_profile(lt, [1], None, 0, 1, 0, 7, 1)
    with pytest.raises(RuntimeError, match=r"\(-4\)"):
        ctx.block_profile(lt, [1, 1], None, 0, 1, 0, 0, 1)
    assert call() == N.SPK_OK  # and the context still works
    ctx.close()
    # no rank under dedupe_only / link_and_dedupe
    ctx = N.Context(0)
    ctx.table_create(0, 4, 0)
    ctx.table_set_key(0, 0, 0, keys)
    ctx.table_set_key(0, 0, 1, keys)
    for link_type in ("dedupe_only", "link_and_dedupe"):
        with pytest.raises(RuntimeError, match=r"\(-4\)"):
            ctx.block_profile(N.LINK_TYPES[link_type], [1], None, 0, 1, 0, 0, 1)
    # timing: HIP-event milliseconds once it is on
    ctx.table_set_rank(0, np.arange(4, dtype=np.int64))
    ctx.block_profile(0, [1], None, 0, 1, -1, 0, 1)
    assert ctx.block_profile_info()[:2] == (-1.0, -1.0)
    ctx.enable_timing(True)
    ctx.block_profile(0, [1], None, 0, 1, -1, 0, 1)
    key_ms, enum_ms, ordinals = ctx.block_profile_info()
    assert key_ms > 0 and enum_ms > 0 and ordinals == 1
    ctx.close()
