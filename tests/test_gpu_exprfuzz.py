"""Random comparison columns and residual blocking rules (tests/exprgen.py) on the HIP path against the sqlite
oracle: the filter kernel's classes under every comparator, threshold and level order, the near misses that
must fall to the interpreter, general AND / OR / NOT predicates up to the 16-instruction limit, all packed
into one code word per pair; the same programs as blocking-rule residuals.  tests/test_exprgen_host.py shows
that the compiler, sqlite and a plain emulation of the compiled programs agree on these expressions, so a
mismatch here is in a kernel or in the host-side classification (classify_simple / simple_class /
prepare_tests / equal_level).

A failed cell prints the seed, the mode, the one expression, the two records and the got / want levels."""
import random

import numpy as np
import pandas as pd
import pytest

import exprgen as xg
import oracle as orc

pytestmark = pytest.mark.gpu

OVERFLOW = {5: "jw", 11: "lev", 17: "num"}  # seeds whose job has one S column more than the filter has slots


@pytest.fixture(scope="module")
def amd():
    from splink_amd import AmdSession, _native
    if _native.device_count() == 0:
        pytest.fail("no HIP device visible: the -m gpu tests need an MI355X")
    return AmdSession(0)


def _check(seed, mode, cols, got, want, rec_l, rec_r):
    assert got.shape == want.shape, (seed, mode, got.shape, want.shape)
    bad = np.argwhere(got != want)
    if len(bad):
        i, k = bad[0]
        pytest.fail(f"{len(bad)} cells differ; first: " +
                    xg.describe(seed, mode, cols[k]["expr"], rec_l(i), rec_r(i), got[i, k], want[i, k]))


def _all_modes(seed, job, st, cols, want, rec_l, rec_r, modes):
    """Every filter mode, then every Levenshtein kernel (tests/test_gpu_parity.py _lev_variants_agree), must
    give `want`; the defaults are restored."""
    try:
        for mode in modes:
            job.ctx.gammas_set_simple(mode)
            job.gammas(st)
            _check(seed, f"simple={mode}", cols, job.gammas_host(), want, rec_l, rec_r)
            # spk_gammas_simple_count is taken after layout_image handed the columns past the filter kernel's
            # slots of their class (FJ_MAX 4, FL_MAX 3, FE_MAX 6, FN_MAX 4) back to the interpreter: the S columns,
            # each class cut at its slots -- and none in interpreter mode.  This keeps the test from silently
            # exercising the interpreter alone.
            assert job.ctx.gammas_simple_count() == (0 if mode % 10 == 0 else xg.expected_simple(cols)), (seed, mode)
        job.ctx.gammas_set_simple(1)
        for kern in (0, 1, 2, 3):
            job.ctx.gammas_set_lev_kernel(kern)
            job.gammas(st)
            _check(seed, f"lev_kernel={kern}", cols, job.gammas_host(), want, rec_l, rec_r)
    finally:
        job.ctx.gammas_set_simple(1)
        job.ctx.gammas_set_lev_kernel(2)


def _pair_frame_case(amd, seed, cols, df):
    from splink_amd.gammas import add_gammas
    gf = add_gammas(df, xg.settings(cols), amd)
    want = orc.sql_gammas(df, [c["case_expression"] for c in gf.settings["comparison_columns"]])
    assert (want != -99).all()
    left = [c for c in df.columns if c.endswith("_l")]
    right = [c for c in df.columns if c.endswith("_r")]
    rec_l = lambda i: df.iloc[i][left].to_dict()
    rec_r = lambda i: df.iloc[i][right].to_dict()
    _check(seed, "default", cols, gf.gamma_matrix(), want, rec_l, rec_r)
    _all_modes(seed, gf.job, gf.settings, cols, want, rec_l, rec_r, (1, 0))


@pytest.mark.parametrize("seed", range(24))
def test_random_columns_on_pair_frames(amd, seed):
    """One pair per row (a_l, a_r, ...), 400 pairs with the long, the huge and the code-point-order rows."""
    rng = random.Random(31000 + seed)
    cols = xg.job(rng, overflow=OVERFLOW.get(seed % 24))
    assert {c["family"] for c in cols} == {"G", "S", "N"} and len(cols) <= 12
    _pair_frame_case(amd, seed, cols, xg.make_pair_frame(rng, 400))


def test_fixed_columns_on_pair_frame(amd):
    """exprgen.FIXED_COLUMNS in one job: seven filter columns (three Levenshtein, two JW, equality, numeric),
    one general and one near miss, on the random pair frame."""
    cols = xg.FIXED_COLUMNS
    assert xg.expected_simple(cols) == 7
    _pair_frame_case(amd, "fixed", cols, xg.make_pair_frame(random.Random(31), 400))


def _split(link_type, df):
    """Inputs of a Job and the keyword arguments of oracle.block for one frame of records."""
    if link_type == "dedupe_only":
        return [df], dict(df=df)
    h = len(df) // 2
    df_l, df_r = df.iloc[:h].reset_index(drop=True), df.iloc[h:].reset_index(drop=True)
    if link_type == "link_only":
        return [df_l, df_r], dict(df_l=df_l, df_r=df_r)
    both = pd.concat([df_l.assign(_source_table="left"), df_r.assign(_source_table="right")], ignore_index=True)
    return [both], dict(df_l=df_l, df_r=df_r)


def _device_pairs(job):
    """(unique_id_l, unique_id_r) of the job's pairs, in device order."""
    l, r = job.pair_rows()
    tl, tr = job.tables[0], job.r_table()
    ul, ur = tl["unique_id"].to_numpy()[l], tr["unique_id"].to_numpy()[r]
    return list(zip(ul.tolist(), ur.tolist()))


@pytest.mark.parametrize("seed", range(6))
@pytest.mark.parametrize("link_type", ["dedupe_only", "link_only"])
def test_random_columns_on_blocked_jobs(amd, link_type, seed):
    """300 records blocked on `l.a = r.a` and `l.k = r.k`, in both rule orders: the string S columns compare
    column a, so the pairs of the first of these rules take their level from equal_level (implied_equal; only
    when column a holds no empty string: the even seeds) under random comparators and thresholds, and the
    second rule's pairs run through the rule-view launch when it is forced (mode 21)."""
    from splink_amd.engine import Job
    from splink_amd.settings import complete_settings_dict
    rng = random.Random(52000 + seed)
    cols = xg.job(rng, s_col="a")
    df = xg.make_records(rng, 300, empty_a=seed % 2 == 1, n_keys=16, huge=True)
    inputs, kw = _split(link_type, df)
    by_uid = df.set_index("unique_id").to_dict("index")
    rules = ["l.a = r.a", "l.k = r.k"]
    st = complete_settings_dict(xg.settings(cols, link_type, rules), amd)
    pairs, left, right = orc.block(st, **kw)
    cmp_df = orc.comparison_frame(pairs, left, right)
    g = orc.sql_gammas(cmp_df, [c["case_expression"] for c in st["comparison_columns"]])
    assert (g != -99).all() and 300 < len(g) <= 3500
    want_of = dict(zip(zip(cmp_df["unique_id_l"].tolist(), cmp_df["unique_id_r"].tolist()), g))
    assert len(want_of) == len(g)
    implied = False
    for order in (rules, rules[::-1]):
        job = Job(link_type, inputs, "unique_id", 0)
        job.block(order)
        ids = _device_pairs(job)
        assert sorted(ids) == sorted(want_of), (seed, order)
        want = np.stack([want_of[p] for p in ids])
        rec_l, rec_r = (lambda i: by_uid[ids[i][0]]), (lambda i: by_uid[ids[i][1]])
        _all_modes(seed, job, st, cols, want, rec_l, rec_r, (1, 21, 0))
        job.gammas(st)
        imp = job.ctx.gammas_implied_pairs(len(cols))
        str_s = [k for k, c in enumerate(cols) if c["family"] == "S" and c["cls"] != "num"]
        if seed % 2 == 0:
            assert (str_s or seed >= 6) and all(imp[k] > 0 for k in str_s), (seed, imp)
            implied = True
        else:
            assert not any(imp), (seed, imp)  # column a holds '': equality of keys does not fix the level
    assert implied == (seed % 2 == 0)


@pytest.mark.parametrize("seed", range(4))
@pytest.mark.parametrize("link_type", ["dedupe_only", "link_only", "link_and_dedupe"])
def test_random_residual_rules(amd, link_type, seed):
    """2-8 rules `l.k = r.k and (<predicate>)` over 150 records: the emitted pair set is oracle.block's (sqlite
    evaluates each whole rule, with the ifnull(earlier rule, false) exclusions), and each pair sits in the range
    of the rule that emits it -- the first rule that is TRUE for it, rule ranges following in rule order."""
    from splink_amd.engine import Job
    rng = random.Random(73000 + seed)
    n_rules = [2, 8, 5, 3][seed % 4]
    rules = xg.residual_rules(rng, n_rules, xg.make_pair_frame(rng, 200))
    df = xg.make_records(rng, 150, n_keys=6, huge=True)
    inputs, kw = _split(link_type, df)
    by_uid = df.set_index("unique_id").to_dict("index")
    st = {"link_type": link_type, "blocking_rules": rules, "unique_id_column_name": "unique_id"}
    pairs, left, right = orc.block(st, **kw)
    cmp_df = orc.comparison_frame(pairs, left, right)
    truth = orc.sql_gammas(cmp_df, [xg.rule_as_case(r) for r in rules])
    assert (truth.max(axis=1) == 1).all()  # every emitted pair satisfies a rule
    first = truth.argmax(axis=1)
    want_rule = dict(zip(zip(cmp_df["unique_id_l"].tolist(), cmp_df["unique_id_r"].tolist()), first.tolist()))
    assert len(want_rule) == len(pairs) <= 3500
    job = Job(link_type, inputs, "unique_id", 0)
    job.block(rules)
    ids = _device_pairs(job)
    missing = sorted(set(want_rule) - set(ids))
    extra = sorted(set(ids) - set(want_rule))
    for what, ps in (("missing", missing), ("extra", extra)):
        if ps:
            l, r = ps[0]
            row = {**{f"{c}_l": v for c, v in by_uid[l].items()}, **{f"{c}_r": v for c, v in by_uid[r].items()}}
            vals = orc.sql_gammas(pd.DataFrame([row]).astype({c: np.float64 for c in ("x_l", "x_r", "y_l", "y_r")}),
                                  [xg.rule_as_case(q) for q in rules])[0].tolist()
            k = want_rule.get((l, r), next((j for j, v in enumerate(vals) if v == 1), 0))
            pytest.fail(f"{len(ps)} pairs {what}; first: " + xg.describe(
                seed, link_type, rules[k], by_uid[l], by_uid[r], what, f"rule values {vals}"))
    assert len(ids) == len(set(ids)) == len(want_rule)
    seq = [want_rule[p] for p in ids]
    down = [i for i in range(1, len(seq)) if seq[i] < seq[i - 1]]
    assert not down, xg.describe(seed, link_type, rules[seq[down[0]]], by_uid[ids[down[0]][0]], by_uid[ids[down[0]][1]],
                                 f"in the range of a later rule than {seq[down[0]]}", seq[down[0]])
