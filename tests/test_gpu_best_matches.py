"""filtered.best_matches(per, ties) on the device (spk_select_best): the best pair per record.

The oracle is numpy / pandas, below: from the filtered parent's rows in ordinal order, a stable sort by (score
descending, position ascending) and the first row per group -- or score == group maximum for ties="all" -- combined
per mode.  Every comparison is exact (ordinals, rows, levels, and scores with ==), and every value the device returns
is one the parent frame returns too."""
import copy
import warnings

import numpy as np
import pandas as pd
import pytest

from conftest import load_golden

pytestmark = pytest.mark.gpu
warnings.filterwarnings("ignore")

MP, TF = "match_probability", "tf_adjusted_match_prob"
PERS = ["l", "r", "either", "mutual"]
TIES = ["first", "all"]
# m / u of the hand-made contexts (levels [2, 3]): twelve patterns with distinct probabilities
M = np.array([0.2, 0.8, 0.1, 0.3, 0.6])
U = np.array([0.7, 0.3, 0.5, 0.3, 0.2])
LAM = 0.3
LEVELS = [2, 3]


@pytest.fixture(scope="module")
def amd():
    from splink_amd import AmdSession, _native
    if _native.device_count() == 0:
        pytest.fail("no HIP device visible: the -m gpu tests need an MI355X")
    return AmdSession(0)


# ---- the oracle ---------------------------------------------------------------------------------------------
def winners(ids, score, ties):
    """{(group, position)}: the best positions of every group.  ids: one array of group ids per side that counts."""
    pos = np.arange(len(score))
    x = np.concatenate(ids)
    p = np.concatenate([pos] * len(ids))
    s = np.concatenate([score] * len(ids))
    ok = ~np.isnan(s)  # a NULL score is never kept and never beats anything
    x, p, s = x[ok], p[ok], s[ok]
    if ties == "all":
        d = pd.DataFrame({"x": x, "p": p, "s": s})
        d = d[d["s"] == d.groupby("x")["s"].transform("max")]
    else:
        order = np.lexsort((p, -s))  # score descending, then position ascending
        d = pd.DataFrame({"x": x[order], "p": p[order]}).drop_duplicates("x", keep="first")
    return set(zip(d["x"].tolist(), d["p"].tolist()))


def oracle_mask(gl, gr, score, per, ties):
    """The kept rows of a frame whose rows are in ordinal order: gl / gr the records of the two sides (one id space:
    equal ids are one record), score with NaN = NULL."""
    gl, gr, score = np.asarray(gl), np.asarray(gr), np.asarray(score, dtype=np.float64)
    sides = {"l": [gl], "r": [gr]}.get(per, [gl, gr])
    w = winners(sides, score, ties)
    n = len(score)
    bl = np.array([(g, i) in w for i, g in enumerate(gl.tolist())], dtype=bool).reshape(n)
    br = np.array([(g, i) in w for i, g in enumerate(gr.tolist())], dtype=bool).reshape(n)
    return {"l": bl, "r": br, "either": bl | br, "mutual": bl & br}[per]


def frame_records(job, settings, pdf):
    """Integer record ids of the two sides of a pair frame (link_only: a left and a right record never coincide)."""
    uid = settings["unique_id_column_name"]
    if job.link_type == "link_only":
        l = [("left", x) for x in pdf[uid + "_l"]]
        r = [("right", x) for x in pdf[uid + "_r"]]
    elif job.link_type == "link_and_dedupe":
        l = list(zip(pdf["_source_table_l"], pdf[uid + "_l"]))
        r = list(zip(pdf["_source_table_r"], pdf[uid + "_r"]))
    else:
        l = [("", x) for x in pdf[uid + "_l"]]
        r = [("", x) for x in pdf[uid + "_r"]]
    code = {k: i for i, k in enumerate(dict.fromkeys(l + r))}
    return np.array([code[k] for k in l], dtype=np.int64), np.array([code[k] for k in r], dtype=np.int64)


def check_frame(best, filtered, by, per, ties):
    """best.toPandas() == the oracle's rows of filtered.toPandas(): columns, order, dtypes, values."""
    from splink_amd import BestMatchFrame
    assert isinstance(best, BestMatchFrame)
    kept = filtered.toPandas()
    gl, gr = frame_records(filtered.job, filtered.settings, kept)
    mask = oracle_mask(gl, gr, kept[by].to_numpy(dtype=np.float64), per, ties)
    exp = kept[mask].reset_index(drop=True)
    got = best.toPandas()
    pd.testing.assert_frame_equal(got, exp, check_exact=True)
    assert list(got.dtypes) == list(exp.dtypes) and list(got.columns) == best.columns == filtered.columns
    assert best.count() == len(best) == len(exp)
    return got


# ---- hand-made contexts -------------------------------------------------------------------------------------
def make_ctx(rows_l, rows_r, g, n0, n1=None):
    """A context with loaded pairs and levels, as test_gpu_components.py::test_abi_states makes one; n1: link_only."""
    from splink_amd import _native as N
    c = N.Context(0)
    if n1 is not None:
        c.set_link_type(N.LINK_TYPES["link_only"])
        c.table_create(1, n1, 1)
    c.table_create(0, n0, 1)
    c.pairs_load(rows_l.astype(np.int32), rows_r.astype(np.int32))
    c.gammas_load(LEVELS, g.astype(np.int8))
    return c


def select_all(c, terms=(), m=M, u=U):
    return c.select(LAM, 1 - LAM, m, u, list(terms))


def copy_sel(c, k):
    """(ordinal, l, r, gammas, mp) of the context's k selected pairs."""
    if k == 0:
        return (np.empty(0, np.int64), np.empty(0, np.int32), np.empty(0, np.int32), np.empty((0, 2), np.int8),
                np.empty(0, np.float64))
    return c.select_copy(0, k, len(LEVELS))


def check_ctx(c, terms, mode_name, ties, r_base=0, m=M, u=U):
    """select, narrow, and compare everything select_copy returns with the oracle's rows of the selection."""
    from splink_amd import _native as N
    from splink_amd.select import best_match_args
    field, mode, keep = best_match_args(mode_name, ties)
    k = select_all(c, terms, m, u)
    before = copy_sel(c, k)
    _, l, r, _, mp = before
    mask = oracle_mask(l.astype(np.int64), r.astype(np.int64) + r_base, mp, mode_name, ties)
    kept = c.select_best(field, mode, keep)
    assert kept == int(mask.sum()) and c.select_info()[0] == kept and c.select_best_info()[:2] == (k, kept)
    after = copy_sel(c, kept)
    for a, b in zip(before, after):
        assert a.dtype == b.dtype and np.array_equal(a[mask], b, equal_nan=True)
    assert (np.diff(after[0]) > 0).all()  # ascending pair ordinal
    return before, after, mask


def random_pairs(seed, n, n0, n1=None):
    rng = np.random.Generator(np.random.PCG64(seed))
    g = np.stack([rng.integers(-1, L, n) for L in LEVELS], axis=1).astype(np.int8)
    l = rng.integers(0, n0, n).astype(np.int32)
    r = rng.integers(0, n0 if n1 is None else n1, n).astype(np.int32)
    l[n // 2:n // 2 + 300] = l[:300]  # repeated pairs ...
    r[n // 2:n // 2 + 300] = r[:300]
    if n1 is None:
        r[100:140] = l[100:140]       # ... and self pairs
    return l, r, g


# ---- 1. random, every mode ----------------------------------------------------------------------------------
@pytest.mark.parametrize("two", [False, True], ids=["one_table", "link_only"])
def test_random_every_mode(two, amd):
    from splink_amd import _native as N
    from splink_amd.select import best_match_args
    n0, n1 = 300, (200 if two else None)
    l, r, g = random_pairs(1, 5000, n0, n1)
    c = make_ctx(l, r, g, n0, n1)
    r_base = n0 if two else 0
    half = [(N.SEL_GAMMA, 1, N.SEL_OP[">="], 1.0)]  # keeps about half the pairs (levels -1, 0, 1, 2)
    for terms in ([], half):
        for per in PERS:
            for ties in TIES:
                before, after, mask = check_ctx(c, terms, per, ties, r_base)
                assert len(before[0]) == (int((g[:, 1] >= 1).sum()) if terms else 5000) and 2000 < len(before[0])
                assert mask.any()  # a non-empty S: every mode keeps at least one pair
                assert len(np.unique(before[4])) <= 12  # at most 12 patterns: nearly every group has ties
                # again, byte for byte
                _, again, _ = check_ctx(c, terms, per, ties, r_base)
                for a, b in zip(after, again):
                    assert a.tobytes() == b.tobytes()
                # the same mode on the narrowed selection keeps everything
                field, mode, keep = best_match_args(per, ties)
                assert c.select_best(field, mode, keep) == len(after[0])
                for a, b in zip(after, copy_sel(c, len(after[0]))):
                    assert a.tobytes() == b.tobytes()
                if per == "mutual" and ties == "first":  # no record occurs in two kept pairs
                    ids = np.concatenate([after[1].astype(np.int64), after[2].astype(np.int64) + r_base])
                    self_pair = (after[1].astype(np.int64) == after[2].astype(np.int64) + r_base)
                    assert len(np.unique(ids)) == 2 * len(after[0]) - int(self_pair.sum())


# ---- 2. lane, wave and chunk edges --------------------------------------------------------------------------
def _edge_counts():
    from splink_amd import _native as N
    C = N.SELECT_CHUNK
    return [1, 63, 64, 65, 255, 256, 257, C - 1, C, C + 1, 3 * C + 17]


@pytest.mark.parametrize("n", _edge_counts())
def test_lane_wave_and_chunk_edges(n, amd):
    from splink_amd import _native as N
    C = N.SELECT_CHUNK
    rng = np.random.Generator(np.random.PCG64(2000 + n))
    lengths, total = [], 0
    cycle = [1, 2, 63, 64, 65, 130]
    while total < n:  # runs of equal left rows, the last one cut at n
        lengths.append(min(cycle[len(lengths) % len(cycle)], n - total))
        total += lengths[-1]
    starts = np.concatenate([[0], np.cumsum(lengths)[:-1]])
    l = np.repeat(np.arange(len(lengths)), lengths).astype(np.int32)
    n0 = len(lengths) + 40
    r = rng.integers(0, n0, n).astype(np.int32)
    # the pattern (1, 2) has the largest probability under M / U; every other pair gets a smaller one
    g = np.stack([rng.integers(-1, 1, n), rng.integers(-1, 3, n)], axis=1).astype(np.int8)
    for i, (s, k) in enumerate(zip(starts, lengths)):
        g[s + k - 1 if i % 2 == 0 else s] = (1, 2)  # the maximum in the last pair of the run, or in the first
    c = make_ctx(l, r, g, n0)
    if n == 3 * C + 17:
        ends = starts + np.array(lengths)
        assert any(s < b < e for s, e in zip(starts, ends) for b in (C, 2 * C, 3 * C))  # a run spans two chunks
        assert any(e - s >= 127 for s, e in zip(starts, ends))                          # and one covers a whole wave
    for per in ("l", "mutual"):
        for ties in TIES:
            before, after, mask = check_ctx(c, [], per, ties)
            assert len(before[0]) == n
            if per == "l" and ties == "first":
                want = np.array([s + k - 1 if i % 2 == 0 else s for i, (s, k) in enumerate(zip(starts, lengths))])
                mp = before[4]
                assert (mp[want] == mp.max()).all() and (np.delete(mp, want) < mp.max()).all()
                assert np.array_equal(after[0], want)


# ---- 3. hub -------------------------------------------------------------------------------------------------
def test_hub(amd):
    hub_pairs = 20000
    spokes = np.arange(1, hub_pairs + 1)
    l = np.concatenate([spokes, spokes, spokes[::2] + 2 * hub_pairs])
    r = np.concatenate([np.zeros(hub_pairs, dtype=np.int64), spokes + hub_pairs, spokes[::2]])
    n0 = 3 * hub_pairs + 1
    rng = np.random.Generator(np.random.PCG64(3))
    order = rng.permutation(len(l))
    l, r = l[order], r[order]
    hub = np.nonzero(r == 0)[0]
    assert len(hub) == hub_pairs and not (l == 0).any()
    g = np.zeros((len(l), 2), dtype=np.int8)  # one pattern: all scores equal
    c = make_ctx(l, r, g, n0)
    for per in ("r", "either", "mutual"):
        before, after, mask = check_ctx(c, [], per, "first")
        assert len(np.unique(before[4])) == 1
        kept_hub = after[0][after[2] == 0]
        if per == "mutual":  # the hub's first pair is its spoke's best only if the spoke has no earlier pair
            spoke = l[hub[0]]
            first_of_spoke = np.nonzero((l == spoke) | (r == spoke))[0][0]
            assert kept_hub.tolist() == ([hub[0]] if first_of_spoke == hub[0] else [])
        else:
            assert kept_hub.tolist()[:1] == [hub[0]]  # the smallest ordinal wins
            assert per == "either" or kept_hub.tolist() == [hub[0]]
    g[hub[-1]] = (1, 2)  # one strictly larger score on the hub's last pair: that pair wins
    c = make_ctx(l, r, g, n0)
    for per in ("r", "either", "mutual"):
        before, after, mask = check_ctx(c, [], per, "first")
        assert before[4][hub[-1]] > before[4][hub[0]]
        assert hub[-1] in after[0].tolist()
        if per == "r":
            assert after[0][after[2] == 0].tolist() == [hub[-1]]
    for per in ("r", "mutual"):
        check_ctx(c, [], per, "all")


# ---- 4. NULL scores -----------------------------------------------------------------------------------------
def test_null_scores(amd):
    n0 = 300
    l, r, g = random_pairs(4, 5000, n0)
    m, u = M.copy(), U.copy()
    m[3] = u[3] = 0.0  # level 1 of column 1: that pattern's denominator is 0, its probability NULL
    all_null = 20      # records 0..19: every pair that touches them is NULL
    g[(l < all_null) | (r < all_null), 1] = 1
    c = make_ctx(l, r, g, n0)
    for per in PERS:
        for ties in TIES:
            before, after, mask = check_ctx(c, [], per, ties, m=m, u=u)
            mp = before[4]
            null = np.isnan(mp)
            assert np.array_equal(null, g[:, 1] == 1) and 0 < null.sum() < len(mp)
            assert not np.isnan(after[4]).any()  # never kept, under ties="all" either
            touched = np.concatenate([after[1], after[2]])
            assert not (touched < all_null).any()  # a record whose every pair is NULL has no kept pair
            if per == "l":  # every left record with a non-NULL pair keeps one: a NULL sibling never wins
                assert set(after[1].tolist()) == set(l[~null].tolist())


# ---- 5. pipelines -------------------------------------------------------------------------------------------
def frame(d):
    return pd.DataFrame(d) if d else None


def scored(g, amd):
    from splink_amd import Splink
    linker = Splink(copy.deepcopy(g["settings_in"]), amd if g["jaro"] else "supress_warnings", df=frame(g.get("df")),
                    df_l=frame(g.get("df_l")), df_r=frame(g.get("df_r")))
    return linker, linker.get_scored_comparisons()


def golden_case(name):
    return load_golden("link_options")[name[len("link_options/"):]] if name.startswith("link_options/") else load_golden(name)


def union_find(n_nodes, u, v):
    parent = list(range(n_nodes))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for a, b in zip(np.asarray(u).tolist(), np.asarray(v).tolist()):
        a, b = find(a), find(b)
        if a != b:
            parent[max(a, b)] = min(a, b)
    return np.array([find(x) for x in range(n_nodes)], dtype=np.int64)


def input_positions(job, settings, pdf):
    """Input positions (the cluster frame's node ids) of the two sides of a pair frame."""
    uid = settings["unique_id_column_name"]
    if job.link_type == "link_only":
        ids = [("left", x) for x in job.inputs[0][uid]] + [("right", x) for x in job.inputs[1][uid]]
        l = [("left", x) for x in pdf[uid + "_l"]]
        r = [("right", x) for x in pdf[uid + "_r"]]
    elif job.link_type == "link_and_dedupe":
        ids = list(zip(job.inputs[0]["_source_table"], job.inputs[0][uid]))
        l = list(zip(pdf["_source_table_l"], pdf[uid + "_l"]))
        r = list(zip(pdf["_source_table_r"], pdf[uid + "_r"]))
    else:
        ids = [("", x) for x in job.inputs[0][uid]]
        l = [("", x) for x in pdf[uid + "_l"]]
        r = [("", x) for x in pdf[uid + "_r"]]
    pos = {k: i for i, k in enumerate(ids)}
    return len(ids), [pos[k] for k in l], [pos[k] for k in r]


@pytest.mark.parametrize("name", ["synthetic_cfg1", "link_options/link_only_plain_rules",
                                  "link_options/link_and_dedupe_repeat_rules"])
def test_pipeline_best_matches_match_pandas(name, amd):
    g = golden_case(name)
    _, df_e = scored(g, amd)
    pdf = df_e.toPandas()
    t = float(pdf[MP].median())
    from splink_amd.frames import FilteredFrame
    from splink_amd.select import Predicate
    for thr in (t, None):
        # the filtered parent whose rows the oracle reads: the pairs above the threshold, or every pair
        parent = df_e.filter(f"{MP} > {t!r}") if thr is not None else FilteredFrame(df_e, Predicate())
        if thr is None:
            pd.testing.assert_frame_equal(parent.toPandas(), pdf, check_exact=True)
        else:
            assert 0 < parent.count() < len(pdf)
        for per in PERS:
            check_frame(df_e.best_matches(thr, per=per), parent, MP, per, "first")
            for ties in TIES:
                inner = df_e.filter(f"{MP} > {t!r}") if thr is not None else FilteredFrame(df_e, Predicate())
                got = check_frame(inner.best_matches(per=per, ties=ties), parent, MP, per, ties)
                assert 0 < len(got) <= parent.count()
        # clusters() of the mutual frame: the union-find over its pairs, a matching
        best = df_e.best_matches(thr, per="mutual")
        kept = best.toPandas()
        n_nodes, u, v = input_positions(df_e.job, df_e.settings, kept)
        cf = best.clusters().toPandas()
        assert np.array_equal(cf["cluster_id"].to_numpy(), union_find(n_nodes, u, v))
        assert np.bincount(cf["cluster_id"].to_numpy()).max() <= 2 and len(cf) == n_nodes


# ---- 6. tf --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("retain", [False, True])
def test_tf_best_matches(retain, amd):
    from splink_amd.term_frequencies import make_adjustment_for_term_frequencies
    g = load_golden("link_tf")
    linker, df_e = scored(g, amd)
    tf = make_adjustment_for_term_frequencies(df_e, linker.params, linker.settings, amd, retain_adjustment_columns=retain)
    pdf = tf.toPandas()
    assert ("surname_adj" in pdf.columns) == retain
    t = float(pdf[TF].median())
    cond = f"{TF} > {t!r}"
    parent = tf.filter(cond)
    assert 0 < parent.count() < len(pdf)
    for per in PERS:
        for ties in TIES:
            got = check_frame(tf.filter(cond).best_matches(per=per, ties=ties), parent, TF, per, ties)
            assert ("surname_adj" in got.columns) == retain and list(got.columns)[:2] == [TF, MP]
            check_frame(tf.filter(cond).best_matches(per=per, ties=ties, by=MP), parent, MP, per, ties)
    check_frame(tf.best_matches(t, per="mutual"), parent, TF, "mutual", "first")
    from splink_amd.select import Predicate
    from splink_amd.term_frequencies import TfFilteredFrame
    check_frame(tf.best_matches(per="r"), TfFilteredFrame(tf, Predicate()), TF, "r", "first")
    with pytest.raises(ValueError, match="legal values"):
        tf.filter(cond).best_matches(by="surname_adj")
    with pytest.raises(ValueError, match="legal values"):
        df_e.filter(f"{MP} > 0.5").best_matches(by=TF)


# ---- 7. frames ----------------------------------------------------------------------------------------------
def synthetic_tables(n, seed):
    from splink_amd.synthetic import make_records
    return make_records(n, seed=seed, surname_vocab=120, first_vocab=80, city_vocab=20)[
        ["unique_id", "first_name", "surname", "dob", "city", "email"]]


def scored_job(amd, link_type, tables, shard=(0, 1)):
    from splink_amd.engine import Job
    from splink_amd.frames import ExpectationFrame, GammaFrame
    from splink_amd.params import Params
    from splink_amd.synthetic import cfg_settings
    s = cfg_settings(2)
    s["link_type"] = link_type
    params = Params(s, amd)
    st = params.settings
    job = Job(link_type, tables, "unique_id", 0, shard=shard)
    job.block(st["blocking_rules"])
    return params, ExpectationFrame(GammaFrame(job, st), st, params.params["λ"], params._level_probabilities())


def test_frames(amd):
    from splink_amd.expectation_step import run_expectation_step
    from splink_amd.iterate import iterate
    from splink_amd.maximisation_step import run_maximisation_step
    from splink_amd.params import Params
    from splink_amd.term_frequencies import make_adjustment_for_term_frequencies
    df = synthetic_tables(1500, seed=7)
    params, df_e = scored_job(amd, "dedupe_only", [df])
    pdf = df_e.toPandas()
    t = float(np.quantile(pdf[MP], 0.5))
    inner = df_e.filter(f"{MP} > {t!r}")
    all_kept = inner.toPandas()
    assert 0 < len(all_kept) < len(pdf)
    a, b = inner.best_matches(per="l"), inner.best_matches(per="mutual")
    got_a = check_frame(a, inner, MP, "l", "first")
    # after a best-match frame materialised, the inner frame still returns all of its survivors
    fresh_inner = df_e.filter(f"{MP} > {t!r}")
    a2 = fresh_inner.best_matches(per="l")
    assert a2.count() == len(got_a)
    pd.testing.assert_frame_equal(fresh_inner.toPandas(), all_kept, check_exact=True)
    assert fresh_inner.count() == len(all_kept)
    # two best-match frames with different `per`, used alternately
    got_b = check_frame(b, inner, MP, "mutual", "first")
    assert len(got_b) < len(got_a)
    ctx = df_e.job.ctx
    for f, want in ((a, got_a), (b, got_b), (a, got_a), (b, got_b)):
        f._pdf = None  # copy from the device again: the context's selection is the other frame's by now
        pd.testing.assert_frame_equal(f.toPandas(), want, check_exact=True)
        assert ctx.select_info()[0] == len(want) and df_e.job.selection_owner is f
    # no filter or best_matches after the narrowing
    for method in (a.filter, a.where, a.best_matches):
        with pytest.raises(ValueError, match="filter first"):
            method(f"{MP} > 0.5")
    # the stage functions refuse the frame
    with pytest.raises(ValueError, match="best-match frame"):
        run_expectation_step(a, params, params.settings, amd)
    with pytest.raises(ValueError, match="best-match frame"):
        iterate(a, params, params.settings, amd)
    with pytest.raises(ValueError, match="best-match frame"):
        run_maximisation_step(a, params, amd)
    with pytest.raises(ValueError, match="best-match frame"):
        make_adjustment_for_term_frequencies(a, params, params.settings, amd)
    # a sharded job, a gamma-table job, an unscored frame
    _, sharded = scored_job(amd, "dedupe_only", [df], shard=(0, 2))
    with pytest.raises(ValueError, match="shards"):
        sharded.best_matches(0.5)
    with pytest.raises(ValueError, match="shards"):
        sharded.filter(f"{MP} > 0.5").best_matches()
    data = {"unique_id_l": np.arange(50), "unique_id_r": np.arange(50) + 1, "gamma_c0": np.arange(50) % 3 - 1}
    settings = {"link_type": "dedupe_only", "blocking_rules": [], "comparison_columns": [{"col_name": "c0", "num_levels": 2}]}
    p2 = Params(settings, "supress_warnings")
    table_e = run_expectation_step(pd.DataFrame(data), p2, p2.settings, amd)
    with pytest.raises(ValueError, match="gamma table"):
        table_e.best_matches(0.5)
    with pytest.raises(ValueError, match="gamma table"):
        table_e.filter("gamma_c0 = 1").best_matches()
    with pytest.raises(ValueError, match="no score"):
        df_e.gammas.filter(f"{df_e.gammas.meta[0][0]} >= 0").best_matches()
    with pytest.raises(ValueError, match="legal values"):
        inner.best_matches(per="both")
    with pytest.raises(ValueError, match="legal values"):
        inner.best_matches(ties="none")


# ---- 8. ABI states ------------------------------------------------------------------------------------------
def test_abi_states(amd):
    from splink_amd import _native as N
    n0 = 300
    l, r, g = random_pairs(8, 5000, n0)
    c = N.Context(0)
    with pytest.raises(RuntimeError, match="no selection"):
        c.select_best(N.SEL_MP, N.BEST_L, 0)
    assert c.select_best_info() == (-1, -1, -1.0)
    c.gammas_load(LEVELS, g)  # codes without pairs: a selection without rows
    select_all(c)
    with pytest.raises(RuntimeError, match="pair rows"):
        c.select_best(N.SEL_MP, N.BEST_L, 0)
    assert c.select_info()[0] == -1  # a failing call leaves no selection
    c = make_ctx(l, r, g, n0)
    eq1 = (N.SEL_GAMMA, 1, N.SEL_OP["="], 1.0)
    c.select(0.0, 0.0, None, None, [eq1])  # made without m / u: no match_probability
    with pytest.raises(RuntimeError, match="no match_probability"):
        c.select_best(N.SEL_MP, N.BEST_L, 0)
    assert c.select_info()[0] == -1
    select_all(c)
    with pytest.raises(RuntimeError, match="no tf_adjusted_match_prob"):
        c.select_best(N.SEL_TF_MP, N.BEST_L, 0)
    assert c.select_info()[0] == -1
    select_all(c)
    c.gammas_load(LEVELS, g)  # new codes: the selection is stale
    with pytest.raises(RuntimeError, match="changed since spk_select"):
        c.select_best(N.SEL_MP, N.BEST_L, 0)
    assert c.select_info()[0] == -1
    for bad in ((7, N.BEST_L, 0), (N.SEL_GAMMA, N.BEST_L, 0), (N.SEL_MP, 4, 0), (N.SEL_MP, -1, 0), (N.SEL_MP, N.BEST_L, 2),
                (N.SEL_MP, N.BEST_L, -1)):
        assert select_all(c) == 5000
        with pytest.raises(ValueError):
            c.select_best(*bad)
        assert c.select_info()[0] == -1 and c.select_best_info()[:2] == (-1, -1)
    # success: the bookkeeping, the memory, the timing
    k = select_all(c)
    before = c.memory()
    kept = c.select_best(N.SEL_MP, N.BEST_MUTUAL, 0)
    after = c.memory()
    assert 0 < kept < k and c.select_info()[0] == kept
    assert c.select_best_info() == (k, kept, -1.0)  # timing off
    assert after["em_score_tf"] <= before["em_score_tf"]
    assert before["em_score_tf"] - after["em_score_tf"] >= 20 * (k - kept)  # ordinal, rows and code of the dropped pairs
    for mem in (before, after):
        assert mem["total"] == sum(v for key, v in mem.items() if key != "total")
    c.enable_timing(True)
    select_all(c)
    sel_ms = c.select_info()[1]
    assert c.select_best(N.SEL_MP, N.BEST_MUTUAL, 0) == kept
    b, kk, ms = c.select_best_info()
    assert (b, kk) == (k, kept) and ms >= 0.0 and c.select_info() == (kept, sel_ms)
    c.enable_timing(False)
    # an empty selection keeps 0
    assert c.select(LAM, 1 - LAM, M, U, [(N.SEL_MP, 0, N.SEL_OP[">"], 2.0)]) == 0
    assert c.select_best(N.SEL_MP, N.BEST_EITHER, 1) == 0
    assert c.select_info()[0] == 0 and c.select_best_info() == (0, 0, -1.0)
    # the narrowed selection feeds spk_components
    select_all(c)
    kept = c.select_best(N.SEL_MP, N.BEST_MUTUAL, 0)
    n_nodes, n_clusters, _ = c.components()
    _, kl, kr, _, _ = copy_sel(c, kept)
    assert n_nodes == n0 and n_clusters == n0 - int((kl != kr).sum())  # a matching: every kept pair joins two records


# ---- 9. leaves the rest alone -------------------------------------------------------------------------------
def test_best_matches_leave_scores_tf_em_and_labels_alone(amd):
    g = load_golden("link_tf")
    linker, df_e = scored(g, amd)
    job = df_e.job
    pdf = df_e.toPandas()
    t = float(pdf[MP].median())
    tf_col = next(c["col_name"] for c in df_e.settings["comparison_columns"] if c["term_frequency_adjustments"])

    def state(with_best):
        """Select and label, optionally narrow, then everything a best_matches call must not have touched."""
        f = df_e.filter(f"{MP} >= {t!r}")
        k = f.count()
        assert 0 < k < len(pdf)
        n_nodes, n_clusters, _ = job.ctx.components()
        labels = job.ctx.components_copy(0, n_nodes)
        if with_best:
            b = f.best_matches(per="mutual")
            assert 0 < b.count() < k and job.ctx.select_info()[0] == b.count()
        labels_after = job.ctx.components_copy(0, n_nodes)  # still copyable
        col = job._col_index[(tf_col, "str")]
        nv = job.ctx.tf_column_values(col)
        scale = job.ctx.tf_scales_column(col, nv)
        limbs, counts = job.ctx.tf_accumulate_column_exact(col, nv, scale)
        tf = linker.make_term_frequency_adjustments(df_e).toPandas()
        stats = job.em_stats(df_e.lam, df_e.level_probs)
        mp = job.score(df_e.lam, df_e.level_probs)
        return [labels, labels_after, scale.copy(), limbs.copy(), counts.copy(), stats.copy(), mp.copy()], tf
    job.score(df_e.lam, df_e.level_probs, want_host=False)
    plain, tf0 = state(False)
    job.score(df_e.lam, df_e.level_probs, want_host=False)
    job.selection_owner = None  # select again, as the first time
    narrowed, tf1 = state(True)
    assert np.array_equal(narrowed[0], narrowed[1])
    for a, b in zip(plain, narrowed):
        assert np.array_equal(a, b, equal_nan=True)
    pd.testing.assert_frame_equal(tf0, tf1, check_exact=True)
