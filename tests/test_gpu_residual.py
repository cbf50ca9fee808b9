"""Blocking rules with residual predicates on the device (spk_block_residual): reference parity on
tests/golden/residual_rules.json, a medium-sized sharded job against a pandas restatement, the state the
filter leaves for the comparison pass, the link-type edges, and the unchanged path of plain rules."""
import copy
import math
import warnings

import numpy as np
import pandas as pd
import pytest

import residual_common as rc
from conftest import load_golden

pytestmark = pytest.mark.gpu
warnings.filterwarnings("ignore")

CASES = ["dedupe_only", "link_only", "link_and_dedupe"]


@pytest.fixture(scope="module")
def amd():
    from splink_amd import AmdSession, _native
    if _native.device_count() == 0:
        pytest.fail("no HIP device visible: the -m gpu tests need an MI355X")
    return AmdSession(0)


# ---- the comparison of tests/test_gpu_parity.py (compare_frames / check_history), copied -------------------
def frame(d):
    return pd.DataFrame(d) if d else None


def rel_close(a, b, tol=1e-9):
    """Relative closeness; NULL (None) and NaN are the same missing value."""
    a = None if (isinstance(a, float) and math.isnan(a)) else a
    b = None if (isinstance(b, float) and math.isnan(b)) else b
    if a is None or b is None:
        return a is None and b is None
    return abs(a - b) <= tol * max(abs(a), abs(b), 1e-300)


def sort_like_golden(df):
    keys = [k for k in ("_source_table_l", "unique_id_l", "_source_table_r", "unique_id_r") if k in df.columns]
    rest = [c for c in df.columns if c.startswith("gamma_")]
    return df.sort_values(keys + rest, kind="mergesort").reset_index(drop=True)


def compare_frames(got: pd.DataFrame, exp: dict, columns):
    assert list(got.columns) == list(columns)
    got = sort_like_golden(got)
    for c in columns:
        gv, ev = got[c].tolist(), exp[c]
        assert len(gv) == len(ev), c
        for a, b in zip(gv, ev):
            if isinstance(b, float) or (isinstance(a, float) and not isinstance(b, str)):
                a = None if a is None else float(a)
                assert rel_close(a, b), (c, a, b)
            else:
                if isinstance(a, float) and math.isnan(a):
                    a = None
                assert a == b, (c, a, b)


def check_history(params, g):
    hist = params.param_history[1:] + [params.params]
    assert len(hist) == len(g["iterations"])
    for p, it in zip(hist, g["iterations"]):
        assert rel_close(p["λ"], it["lambda"])
        for gname, d in it["pi"].items():
            for i, (m, u) in enumerate(zip(d["m"], d["u"])):
                assert rel_close(p["π"][gname]["prob_dist_match"][f"level_{i}"]["probability"], m), (gname, i)
                assert rel_close(p["π"][gname]["prob_dist_non_match"][f"level_{i}"]["probability"], u), (gname, i)


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
