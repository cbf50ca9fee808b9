"""Blocking rules with residual predicates on the device (spk_block_residual): reference parity on
tests/golden/residual_rules.json, a medium-sized sharded job against a pandas restatement, the state the
filter leaves for the comparison pass, the link-type edges, and the unchanged path of plain rules."""
import copy
import warnings

import numpy as np
import pandas as pd
import pytest

import residual_common as rc
from conftest import load_golden
from parity_common import check_history, compare_frames, frame

pytestmark = pytest.mark.gpu
warnings.filterwarnings("ignore")

CASES = ["dedupe_only", "link_only", "link_and_dedupe"]


@pytest.fixture(scope="module")
def amd():
    from splink_amd import AmdSession, _native
    if _native.device_count() == 0:
        pytest.fail("no HIP device visible: the -m gpu tests need an MI355X")
    return AmdSession(0)


# ---- 1. golden pipeline parity ------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_pipeline_matches_reference(case, amd):
    from splink_amd import Splink
    g = load_golden("residual_rules")[case]
    linker = Splink(copy.deepcopy(g["settings_in"]), "supress_warnings", df=frame(g.get("df")),
                    df_l=frame(g.get("df_l")), df_r=frame(g.get("df_r")))
    df_e = linker.get_scored_comparisons()
    compare_frames(df_e.toPandas(), g["df_e"], g["df_e_columns"])
    check_history(linker.params, g)


# ---- 2 / 3. medium size: shards, several compaction workgroups, the state after the filter ------------------
MEDIUM_RULES = ["l.surname = r.surname and levenshtein(l.first_name, r.first_name) <= 2",
                "l.dob = r.dob and l.city != r.city",
                "l.surname = r.surname"]
MEDIUM_KEYS = ["surname", "dob", "surname"]
RF_CHUNK = 2048  # pairs per compaction workgroup (spk_block.hip RF_CHUNK)


@pytest.fixture(scope="module")
def medium():
    """7,000 synthetic records with small vocabularies (dob cut to its year: 80 values), the one-shard job on
    MEDIUM_RULES, and the pandas restatement: merge on the key, the residual row-wise, minus the pairs an earlier
    rule emitted in full."""
    from splink_amd.engine import Job
    from splink_amd.synthetic import make_records
    df = make_records(7000, seed=23, surname_vocab=100, first_vocab=30, city_vocab=20)[
        ["unique_id", "first_name", "surname", "dob", "city", "email"]]
    df["dob"] = df["dob"].str[:4]
    job = Job("dedupe_only", [df], "unique_id", 0)
    job.block(MEDIUM_RULES)
    try:  # the hidden predicate pass must leave no codes a caller could read as comparison vectors
        job.ctx.gammas_copy(1, 0, 1)
        codes_dropped = False
    except RuntimeError as e:  # SPK_E_STATE, and no other failure
        codes_dropped = "spk_gammas_copy failed (-4)" in str(e) and "no gammas" in str(e)
    table = job.tables[0]  # pair rows index the clustered table
    lev = {}

    def lev_le2(a, b):
        if rc.null(a) or rc.null(b):
            return None
        if (a, b) not in lev:
            lev[(a, b)] = rc.levenshtein(a, b)
        return lev[(a, b)] <= 2

    residuals = [lambda m: [lev_le2(a, b) is True for a, b in zip(m["first_name_l"], m["first_name_r"])],
                 lambda m: [rc.cmp("!=", a, b) is True for a, b in zip(m["city_l"], m["city_r"])],
                 None]
    t = table.reset_index().rename(columns={"index": "row"})
    seen, per_rule, key_candidates = set(), [], []
    for key, res in zip(MEDIUM_KEYS, residuals):
        side = t.dropna(subset=[key])
        m = side.merge(side, on=key, suffixes=("_l", "_r"))
        m = m[m["unique_id_l"] < m["unique_id_r"]]
        key_candidates.append(len(m))
        if res is not None:
            m = m[np.array(res(m), dtype=bool)]
        pairs = set(zip(m["row_l"].tolist(), m["row_r"].tolist())) - seen
        per_rule.append(pairs)
        seen |= pairs
    return dict(df=df, job=job, table=table, per_rule=per_rule, key_candidates=key_candidates,
                codes_dropped=codes_dropped)


def test_medium_rules_shards_and_order(amd, medium):
    from splink_amd.engine import Job
    job, per_rule, cand = medium["job"], medium["per_rule"], medium["key_candidates"]
    l1, r1 = job.pair_rows()
    one = np.stack([l1, r1], axis=1)
    # as a set: the pandas restatement
    assert len(one) == sum(len(p) for p in per_rule)
    got = set(map(tuple, one.tolist()))
    assert len(got) == len(one) and got == set().union(*per_rule)
    # per rule a contiguous range, in rule order
    rule_of = {p: k for k, pairs in enumerate(per_rule) for p in pairs}
    seq = np.array([rule_of[p] for p in map(tuple, one.tolist())])
    assert (np.diff(seq) >= 0).all()
    # the fixture exercises what it should: every rule has >= 50,000 key candidates, every residual rejects and
    # keeps pairs, each rule's survivors span several compaction workgroups, and rule 2 (key-only) emits pairs
    # that key-match rule 0 without satisfying it
    assert min(cand) >= 50000, cand
    assert all(len(p) > 2 * RF_CHUNK for p in per_rule), [len(p) for p in per_rule]
    assert len(per_rule[0]) < cand[0] and len(per_rule[1]) < cand[1]
    assert len(per_rule[2]) > 0
    # n_candidates: the key-candidate ordinals, as spk_block counts them for the equality parts alone
    plain = Job("dedupe_only", [medium["df"]], "unique_id", 0)
    plain.block([f"l.{k} = r.{k}" for k in MEDIUM_KEYS])
    assert job.n_candidates == plain.n_candidates == sum(cand)
    # enumerated before the filter: rules 0 and 1 carry predicates, so no earlier rule excludes on its key and
    # every key candidate that passes the link-type predicate is enumerated
    enumerated, filter_ms = job.ctx.block_residual_info()
    assert enumerated == sum(cand) and enumerated >= job.n_pairs
    assert filter_ms == -1.0  # timing is off
    assert plain.ctx.block_residual_info() == (-1, -1.0)  # no residual call on that context
    # three shards: cut on the key-candidate ordinals, one boundary strictly inside a rule; concatenated they are
    # the one-shard list, in its order
    total = sum(cand)
    bounds = [total * s // 3 for s in (1, 2)]
    edges = np.cumsum([0] + cand)
    assert any(edges[k] < b < edges[k + 1] for b in bounds for k in range(3))
    parts = []
    for s in range(3):
        js = Job("dedupe_only", [medium["df"]], "unique_id", 0, shard=(s, 3))
        js.block(MEDIUM_RULES)
        assert js.n_candidates == total
        assert js.tables[0]["unique_id"].equals(medium["table"]["unique_id"])
        parts.append(np.stack(js.pair_rows(), axis=1))
        assert len(parts[-1]) == js.n_pairs > 0
    assert (np.concatenate(parts) == one).all()


@pytest.mark.parametrize("mode", [1, 21])
def test_state_after_the_filter(amd, medium, mode):
    """gammas() on the filtered pairs against a second context that loads the same row pairs: rule ranges, rule
    1's view positions and the blocking-key implied levels kept in step with the pairs, nothing of the hidden
    predicate pass left behind."""
    from splink_amd.engine import Job
    from splink_amd.settings import complete_settings_dict
    from splink_amd.synthetic import cfg_settings
    job = medium["job"]
    st = complete_settings_dict(cfg_settings(2), amd)  # first_name / surname JW-3, dob / city exact-2, email Lev-3
    assert medium["codes_dropped"]
    l, r = job.pair_rows()
    other = Job("dedupe_only", [medium["table"][list(medium["df"].columns)]], "unique_id", 0, cluster=False)
    other.load_pairs(l, r)
    other.gammas(st)
    want = other.gammas_host()
    job.ctx.gammas_set_simple(mode)
    job.gammas(st)
    got = job.gammas_host()
    job.ctx.gammas_set_simple(1)
    assert got.shape == want.shape and (got == want).all(), np.nonzero((got != want).any(axis=1))[0][:10]
    if mode == 21:
        assert job.ctx.gammas_view_regions() > 0
    # surname: implied by the key of rules 0 and 2 for their (surviving) pairs
    imp = job.ctx.gammas_implied_pairs(5)
    n0, n2 = len(medium["per_rule"][0]), len(medium["per_rule"][2])
    assert imp[1] == max(n0, n2) > 0, (imp, n0, n2)
    assert (got[:n0, 1] == 2).all()  # rule 0's pairs: equal surnames


# ---- 4. link types at the edges ------------------------------------------------------------------------------
@pytest.mark.parametrize("link_type", ["link_and_dedupe", "link_only"])
def test_null_unique_id_and_asymmetric_residual(amd, link_type):
    from splink_amd.engine import Job
    g = load_golden("residual_rules")["link_and_dedupe"]
    df_l, df_r = frame(g["df_l"]), frame(g["df_r"])
    df_l["unique_id"] = df_l["unique_id"].astype(object)
    df_r["unique_id"] = df_r["unique_id"].astype(object)
    df_l.loc[3, "unique_id"] = None
    df_r.loc[[0, 20], "unique_id"] = None
    rules = ["l.surname = r.surname and l.age < r.age", "l.city = r.city and abs(l.age - r.age) <= 3", "l.surname = r.surname"]
    fns = [(rc.eq("surname"), lambda l, r: rc.cmp("<", l["age"], r["age"])),
           (rc.eq("city"), lambda l, r: None if rc.null(l["age"]) or rc.null(r["age"]) else abs(l["age"] - r["age"]) <= 3),
           (rc.eq("surname"), None)]
    rows_l = [dict(zip(df_l.columns, v)) for v in df_l.itertuples(index=False, name=None)]
    rows_r = [dict(zip(df_r.columns, v)) for v in df_r.itertuples(index=False, name=None)]
    if link_type == "link_only":
        inputs = [df_l, df_r]
        L, R = [dict(x, _id=("l", i)) for i, x in enumerate(rows_l)], [dict(x, _id=("r", i)) for i, x in enumerate(rows_r)]
    else:
        inputs = [pd.concat([df_l.assign(_source_table="left"), df_r.assign(_source_table="right")],
                            ignore_index=True)]
        L = [dict(x, _source_table="left", _id=i) for i, x in enumerate(rows_l)] + \
            [dict(x, _source_table="right", _id=len(rows_l) + i) for i, x in enumerate(rows_r)]
        R = L
    emitted, stats = rc.brute_force(link_type, L, R, fns)
    assert all(s["emitted"] > 0 for s in stats) and stats[0]["rejected"] > 0 and stats[0]["null_residual"] > 0
    job = Job(link_type, inputs, "unique_id", 0)
    job.block(rules)
    l, r = job.pair_rows()
    # device rows -> input rows through the job's permutation
    pl = job.perm[0] if job.perm[0] is not None else np.arange(len(inputs[0]))
    rs = job.r_side()
    pr = job.perm[rs] if job.perm[rs] is not None else np.arange(len(inputs[rs]))
    got = sorted(zip(pl[l].tolist(), pr[r].tolist()))
    assert got == sorted((i, j) for _, i, j in emitted)
    assert job.n_pairs == len(emitted)


# ---- 5. rules without residuals: the unchanged path ----------------------------------------------------------
def test_plain_rules_take_spk_block(amd, medium, monkeypatch):
    from splink_amd import _native as N
    from splink_amd.engine import Job
    calls = []
    real_block, real_residual = N.Context.block, N.Context.block_residual
    monkeypatch.setattr(N.Context, "block", lambda self, *a, **k: calls.append("block") or real_block(self, *a, **k))
    monkeypatch.setattr(N.Context, "block_residual",
                        lambda self, *a, **k: calls.append("residual") or real_residual(self, *a, **k))
    plain_rules = ["l.surname = r.surname", "l.dob = r.dob", "l.first_name = r.first_name and l.city = r.city"]
    job = Job("dedupe_only", [medium["df"]], "unique_id", 0)
    job.block(plain_rules)
    assert calls == ["block"]
    want = job.pair_rows()
    # the new entry point with no program anywhere: spk_block's pairs
    empty = N.Context.gammas_args(np.zeros(0, N.PROGRAM_DTYPE), [], [], [], np.zeros(0, N.INSTR_DTYPE),
                                  np.zeros(0, N.OPERAND_DTYPE), np.zeros(1, np.int64), np.zeros(0, np.uint8))
    n_pairs, n_cand = real_residual(job.ctx, N.LINK_TYPES["dedupe_only"], [1, 1, 1], [-1, -1, -1], empty)
    assert (n_pairs, n_cand) == (job.n_pairs, job.n_candidates)
    got = job.ctx.pairs_copy(0, n_pairs)
    assert (got[0] == want[0]).all() and (got[1] == want[1]).all()
    job2 = Job("dedupe_only", [medium["df"]], "unique_id", 0)
    job2.block(MEDIUM_RULES[:1])
    assert calls == ["block", "residual"]


# ---- 6. the compaction's chunk edges at small size -------------------------------------------------------------
SMALL_N = 65  # one key: rule 0 enumerates 65 * 64 / 2 = 2080 candidates -- two compaction workgroups, nine slabs
SMALL_RULES = ["l.k = r.k and l.v < r.v", "l.k2 = r.k2"]  # rule 1 is key-only and carries view positions
SMALL_FNS = [(rc.eq("k"), lambda l, r: rc.cmp("<", l["v"], r["v"])), (rc.eq("k2"), None)]
RF_SLAB = 256  # pairs per slab of a compaction workgroup (spk_block.hip RF_THREADS)


def small_frame(keep):
    """65 records in unique-id order under one key, so rule 0's candidate ordinals are the pairs (i, j), i < j,
    i-major; `v` decides which of them `l.v < r.v` keeps."""
    from splink_amd.synthetic import make_records
    df = make_records(SMALL_N, seed=41, surname_vocab=6, first_vocab=6, city_vocab=4)[
        ["unique_id", "first_name", "surname", "dob", "city", "email"]]
    i = np.arange(SMALL_N)
    df["unique_id"] = i
    df["k"] = "a"
    df["k2"] = [f"g{x % 5}" for x in i]
    if keep == "none":
        v = np.zeros(SMALL_N)
    elif keep == "all":
        v = i.astype(np.float64)
    elif keep == "one":  # descending but for rows 60, 61: the pair (60, 61), ordinal 2070 of 2080
        v = -i.astype(np.float64)
        v[[60, 61]] = v[[61, 60]]
    else:
        v = np.random.default_rng(7).integers(0, 4, SMALL_N).astype(np.float64)
    df["v"] = v
    return df


@pytest.mark.parametrize("keep", ["none", "one", "all", "mix"])
def test_small_rule_at_the_chunk_edges(amd, keep):
    from splink_amd.engine import Job
    from splink_amd.settings import complete_settings_dict
    from splink_amd.synthetic import cfg_settings
    df = small_frame(keep)
    L = [dict(zip(df.columns, v), _id=i) for i, v in enumerate(df.itertuples(index=False, name=None))]
    emitted, stats = rc.brute_force("dedupe_only", L, L, SMALL_FNS)
    n_cand = SMALL_N * (SMALL_N - 1) // 2
    assert n_cand == 2080 and stats[0]["candidates"] == n_cand and stats[1]["candidates"] == 5 * 13 * 12 // 2
    want0 = [(i, j) for k, i, j in emitted if k == 0]
    assert len(want0) == {"none": 0, "one": 1, "all": n_cand}.get(keep, len(want0))
    assert (stats[1]["emitted"] == 0) == (keep == "all")
    if keep == "one":
        assert want0 == [(60, 61)]
    if keep == "mix":  # kept and rejected candidates in the first slab, between ordinals 256 and 2048, and past 2048
        kept = np.zeros(n_cand, dtype=bool)
        kept[[i * (2 * SMALL_N - i - 1) // 2 + j - i - 1 for i, j in want0]] = True
        for part in (kept[:RF_SLAB], kept[RF_SLAB:RF_CHUNK], kept[RF_CHUNK:]):
            assert part.any() and not part.all()
    job = Job("dedupe_only", [df], "unique_id", 0)
    job.block(SMALL_RULES)
    assert job.n_pairs == len(emitted) and job.n_candidates == n_cand + stats[1]["candidates"]
    assert job.ctx.block_residual_info()[0] == n_cand + stats[1]["candidates"]  # rule 0 does not exclude on its key
    l, r = job.pair_rows()
    perm = job.perm[0] if job.perm[0] is not None else np.arange(SMALL_N)
    got = list(zip(perm[l].tolist(), perm[r].tolist()))
    # rule 0: the survivors in ordinal order
    assert got[:len(want0)] == want0
    # rule 1: block after block (their order is the device's key ids'), l-major inside a block
    got1 = got[len(want0):]
    groups = list(dict.fromkeys(i % 5 for i, _ in got1))
    want1 = sorted(((i, j) for k, i, j in emitted if k == 1), key=lambda p: (groups.index(p[0] % 5), p))
    assert got1 == want1
    if keep != "mix":
        return
    # the state after the filter, as test_state_after_the_filter: rule ranges and rule 1's view positions
    st = complete_settings_dict(cfg_settings(2), amd)
    other = Job("dedupe_only", [job.tables[0][list(df.columns)]], "unique_id", 0, cluster=False)
    other.load_pairs(l, r)
    other.gammas(st)
    want = other.gammas_host()
    job.ctx.gammas_set_simple(21)
    job.gammas(st)
    codes = job.gammas_host()
    job.ctx.gammas_set_simple(1)
    assert codes.shape == want.shape and (codes == want).all(), np.nonzero((codes != want).any(axis=1))[0][:10]
    assert job.ctx.gammas_view_regions() > 0
