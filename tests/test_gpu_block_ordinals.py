"""spk_block's pair set past 2^31 and 2^32 candidate ordinals, and past the block size at which the triangular
decode's discriminant (2n-1)^2 no longer fits a double's mantissa.  A shard is a range of ordinals, so a thin
shard of a huge ordinal space holds a few thousand pairs: each case blocks a few chosen shards of a space of more
than 2^32 candidates on a bare context and compares the candidate total, the pair count and the ordered pair
sequence with the exact-integer reference of tests/ordinal_common.py, where the cases are defined
(tests/test_ordinal_host.py checks there that each of them discriminates).  The last two tests tie the result to
the path users run: a sharded Job, its pairs and its comparison vectors."""
import time

import numpy as np
import pandas as pd
import pytest

import ordinal_common as oc
from ordinal_common import DEDUPE, LINK_ONLY, Plan, shard_of, shard_range, straddling, thin_S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def native():
    from splink_amd import _native
    if _native.device_count() == 0:
        pytest.fail("no HIP device visible: the -m gpu tests need an MI355X")
    return _native


def load(native, case):
    a = case.arrays()
    ctx = native.Context(0)
    ctx.set_link_type(case.link_type)
    ctx.table_create(0, len(a["keys_l"][0]), 0)
    if case.link_type == LINK_ONLY:
        ctx.table_create(1, len(a["keys_r"][0]), 0)
    else:
        ctx.table_set_rank(0, a["rank"])
        ctx.table_set_rank_null(0, case.null_div)
    for r, (kl, kr) in enumerate(zip(a["keys_l"], a["keys_r"])):
        ctx.table_set_key(0, r, 0, kl)
        ctx.table_set_key(1 if case.link_type == LINK_ONLY else 0, r, 1, kr)
    return ctx


def block_shard(ctx, case, s):
    n_pairs, n_cand = ctx.block(case.link_type, case.sym, s, case.S)
    assert ctx.pairs_count() == n_pairs
    l, r = ctx.pairs_copy(0, n_pairs)
    return np.stack([l, r], axis=1).astype(np.int64), n_pairs, n_cand


def same_sequence(got, want, what):
    assert len(got) == len(want), (what, len(got), len(want))
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert len(bad) == 0, (what, len(bad), bad[:5], got[bad[:5]], want[bad[:5]])


@pytest.mark.parametrize("name", list(oc.CASES))
def test_shards_match_reference(native, name):
    t0 = time.perf_counter()
    case = oc.CASES[name]()
    case.arrays()
    t1 = time.perf_counter()
    plan = case.plan()
    t2 = time.perf_counter()
    ctx = load(native, case)
    t3 = time.perf_counter()
    print(f"{case.name}: total {case.total}, S {case.S}; arrays {t1 - t0:.2f} s, host plan {t2 - t1:.2f} s, "
          f"upload {t3 - t2:.2f} s")
    try:
        assert plan.total == case.total
        by_shard = {}
        for label, s in list(case.shards.items()) + [("run", s) for run in case.runs for s in run]:
            if s in by_shard:
                continue
            t = time.perf_counter()
            got, n_pairs, n_cand = block_shard(ctx, case, s)
            t_block = time.perf_counter() - t
            want = plan.shard(s, case.S)
            lo, hi = case.range(s)
            print(f"  shard {s} ({label}): ordinals [{lo}, {hi}), {n_pairs} pairs, expected {len(want)}; "
                  f"block {t_block * 1e3:.1f} ms")
            assert n_cand == case.total, (label, n_cand)
            assert n_pairs == len(want), (label, n_pairs, len(want))
            same_sequence(got, want, label)
            by_shard[s] = got
        for run in case.runs:  # consecutive shards tile the union of their ranges
            union = plan.pairs(case.range(run[0])[0], case.range(run[-1])[1])
            same_sequence(np.concatenate([by_shard[s] for s in run]), union, run)
    finally:
        ctx.close()


# ---- job level ----------------------------------------------------------------------------------------------------
CFG2_COLS = ["first_name", "surname", "dob", "city", "email"]
CFG2_SPECS = [("jw", 3, [0.94, 0.88]), ("jw", 3, [0.94, 0.88]), ("eq", 2, []), ("eq", 2, []), ("lev", 3, [0.3])]
N_B, N_NULL = 300, 417  # the two-rule job: rule 0's second block, and its NULL keys


@pytest.fixture(scope="module")
def amd(native):
    from splink_amd import AmdSession
    return AmdSession(0)


@pytest.fixture(scope="module")
def records():
    """N_TRI + N_B + N_NULL synthetic records in shuffled order, the unique ids a permutation of the rows.  blk0:
    one value on N_TRI records, another on N_B, NULL on the rest; blk1: one value on ~80 records of each of the
    three groups, NULL elsewhere (one block that cuts across blk0's: pairs inside a blk0 block are excluded, the
    others kept)."""
    from splink_amd.synthetic import make_records
    n = oc.N_TRI + N_B + N_NULL
    df = make_records(n, seed=23, surname_vocab=800, first_vocab=400, city_vocab=100)[["unique_id"] + CFG2_COLS]
    i = np.arange(n)
    j = i - oc.N_TRI
    blk0 = np.where(i < oc.N_TRI, "aaa", np.where(j < N_B, "bbb", None)).astype(object)
    in1 = np.where(i < oc.N_TRI, i % 1150 == 3, np.where(j < N_B, j % 4 == 0, (j - N_B) % 5 == 0))
    order = np.random.default_rng(23).permutation(n)
    df["blk0"] = blk0[order]
    df["blk1"] = np.where(in1, "x", None).astype(object)[order]
    df["unique_id"] = oc.perm_rank(n)
    return df


def check_job(amd, job, plan, s, S):
    import oracle as orc
    from splink_amd.settings import complete_settings_dict
    from splink_amd.synthetic import cfg_settings
    want = plan.shard(s, S)
    assert job.n_candidates == plan.total
    l, r = job.pair_rows()
    same_sequence(np.stack([l, r], axis=1).astype(np.int64), want, "job pairs")
    st = complete_settings_dict(cfg_settings(2), amd)
    job.gammas(st)
    table = job.tables[0]
    cols = [orc.StrCol(table[c].tolist()) for c in CFG2_COLS]
    ref = orc.template_gammas(CFG2_SPECS, cols, cols, want[:, 0], want[:, 1])
    got = job.gammas_host()
    assert got.shape == ref.shape and (got == ref).all(), np.nonzero((got != ref).any(axis=1))[0][:10]
    return want


def test_job_cartesian_shard_at_2_32(amd, records):
    """A dedupe job without blocking rules over N_TRI records is one block of more than 2^32 candidates."""
    from splink_amd.engine import Job
    df = records.iloc[:oc.N_TRI].reset_index(drop=True)
    n = len(df)
    total = n * (n - 1) // 2
    S = thin_S(total)
    s = shard_of(total, S, 2 ** 32)
    job = Job("dedupe_only", [df], "unique_id", 0, shard=(s, S))
    job.block([])
    table = job.tables[0]
    assert table["unique_id"].equals(df["unique_id"])  # no rule, no clustering
    k = np.zeros(n, dtype=np.int64)
    plan = Plan(DEDUPE, [k], [k], table["unique_id"].to_numpy(np.int64))
    assert plan.total == total > 2 ** 32
    want = check_job(amd, job, plan, s, S)
    assert len(want) == shard_range(total, s, S)[1] - shard_range(total, s, S)[0] > 4000  # distinct ids: all kept


def test_job_two_rules_shard_across_the_rule_boundary(amd, records):
    """Rule 0 has more than 2^32 candidates; the shard holds its last ordinals and rule 1's first.  Blocking keys
    are ids in hash order, which the host cannot know: rule 0's block order is read off the job's table (clustered by
    rule 0's key), and rule 1 has one block."""
    from splink_amd.engine import Job
    n1 = int(records["blk1"].notna().sum())
    totals = [oc.N_TRI * (oc.N_TRI - 1) // 2 + N_B * (N_B - 1) // 2, n1 * (n1 - 1) // 2]
    total = sum(totals)
    S, s = straddling(total, totals[0])
    lo, hi = shard_range(total, s, S)
    assert totals[0] > 2 ** 32 and lo + 1000 <= totals[0] < hi - 1000
    job = Job("dedupe_only", [records], "unique_id", 0, shard=(s, S))
    job.block(["l.blk0 = r.blk0", "l.blk1 = r.blk1"])
    table = job.tables[0]
    assert sorted(table["unique_id"]) == sorted(records["unique_id"])
    k0 = pd.factorize(table["blk0"])[0].astype(np.int64)  # ids by first appearance, -1 for NULL
    assert (np.diff(k0[k0 >= 0]) >= 0).all() and k0.max() == 1  # the table is clustered: blocks are contiguous
    k1 = np.where(table["blk1"].notna().to_numpy(), 0, -1).astype(np.int64)
    plan = Plan(DEDUPE, [k0, k1], [k0, k1], table["unique_id"].to_numpy(np.int64))
    assert plan.rule_off == [0, totals[0], total]
    cand, keep = plan.candidates(totals[0], hi)  # rule 1's part: rule 0's key excludes some of it, not all
    assert 0 < int(keep.sum()) < len(cand)
    check_job(amd, job, plan, s, S)
