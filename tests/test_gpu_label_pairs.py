"""Pairs against a table of labelled pairs on the device (spk_label_pairs_histogram) and the frames above it.

Hand-made contexts compare the counts with a Python dict of the labelled pairs and np.bincount(state * n_patterns +
code) (label_pairs_common.expected); the pipelines compare truth_table_from_pairs() / labelled_pairs() /
prediction_errors() / estimate_from_pair_labels() with the merge of df_e.toPandas() and the labels table on the unique
ids, the only route there was before.  Every comparison is exact."""
import ctypes
import socket
import warnings

import numpy as np
import pandas as pd
import pytest

from label_pairs_common import (canonical, capacity_of, codes_of, distinct_pairs, expected, home_slot, m_u, make_ctx,
                                mixed_labels, n_patterns, random_case)

pytestmark = pytest.mark.gpu
warnings.filterwarnings("ignore")

MP = "match_probability"
LAM = 0.3
STEP = 512 * 8  # pairs one workgroup takes per step (LH_THREADS x LH_PAIRS in csrc/spk_labels.hip)
NONE = (-1, -1.0, -1, -1)  # label_pairs_info() before a call and after a failing one


@pytest.fixture(scope="module")
def amd():
    from splink_amd import AmdSession, _native
    if _native.device_count() == 0:
        pytest.fail("no HIP device visible: the -m gpu tests need an MI355X")
    return AmdSession(0)


def em_histogram(c):
    import torch
    hist = torch.zeros(c.n_patterns(), dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    c.em_histogram(hist.data_ptr())
    return hist.cpu().numpy()


def check_counts(c, rows_l, rows_r, g, levels, lab_l, lab_r, y, one_table, **scored):
    want, want_code = expected(rows_l, rows_r, g, levels, lab_l, lab_r, y, one_table)
    counts, mp, code = c.label_pairs_histogram(lab_l, lab_r, y, **scored)
    assert counts.dtype == np.int64 and counts.shape == want.shape and code.dtype == np.int32
    assert np.array_equal(counts, want)
    assert np.array_equal(code, want_code)
    info = c.label_pairs_info()
    assert info[0] == len(rows_l) == counts.sum() and info[2] == capacity_of(len(lab_l))
    return counts, mp, code


# ---- 1. pair counts: tail, vector path, partial wave, several workgroups, the grid-stride loop ---------------------
def sparse_pair_set(rng, P, n0):
    """Random pairs of n0 records, none with (l + r) % 4 == 0: however large P is, pairs that are no candidates remain
    for the labels to name."""
    rows_l, rows_r = rng.integers(0, n0, P), rng.integers(0, n0, P)
    hit = (rows_l + rows_r) % 4 == 0
    rows_r = np.where(hit, np.where(rows_r < n0 - 1, rows_r + 1, rows_r - 1), rows_r)
    assert not ((rows_l + rows_r) % 4 == 0).any()
    return rows_l, rows_r


@pytest.mark.parametrize("n_labels", [0, 1, 64, 1000])
@pytest.mark.parametrize("P", [0, 1, 63, 64, 65, 8 * 64 + 5, 3 * STEP, 8 * (1024 * 512 + 37) + 5])
def test_pair_counts_against_bincount(P, n_labels, amd):
    levels = [2, 3]
    rng = np.random.Generator(np.random.PCG64([P, n_labels]))
    rows_l, rows_r = sparse_pair_set(rng, P, 97)
    g = np.stack([rng.integers(-1, L, P) for L in levels], axis=1) if P else np.zeros((0, 2), np.int64)
    c = make_ctx(rows_l, rows_r, g, levels, 97)
    assert c.label_pairs_info() == NONE
    lab_l, lab_r, y, n_cand = mixed_labels(rng, n_labels, rows_l, rows_r, 97)
    assert len(lab_l) == n_labels and (n_labels < 2 or P < 64 or 0 < n_cand < n_labels)  # candidates and others
    counts, mp, code = check_counts(c, rows_l, rows_r, g, levels, lab_l, lab_r, y, True)
    assert mp is None and counts.shape == (3, 12)
    assert P == 0 or np.array_equal(counts.sum(axis=0), em_histogram(c))
    assert (code >= 0).sum() == n_cand and c.label_pairs_info()[1] == -1.0
    c.close()


# ---- 2. pattern spaces: LDS counters, global counters, 32-bit codes; link_only and one table -----------------------
@pytest.mark.parametrize("two", [False, True], ids=["one_table", "link_only"])
@pytest.mark.parametrize("levels,lds", [([2, 3], True), ([5] * 4, True), ([3] * 7, False), ([4] * 7, False)],
                         ids=["12", "1296", "16384", "78125"])
def test_pattern_spaces_and_link_types(levels, lds, two, amd):
    from splink_amd import _native as N
    rng = np.random.Generator(np.random.PCG64(len(levels) * 10 + two))
    P, n0, n1 = 8 * 700 + 3, 211, (157 if two else None)
    rows_l, rows_r, g, _, _ = random_case(rng, P, levels, n0, n1)
    c = make_ctx(rows_l, rows_r, g, levels, n0, n1)
    n_pat = n_patterns(levels)
    assert c.n_patterns() == n_pat and (3 * n_pat * 4 <= min(N.LABEL_LDS_BYTES, c.lds_per_block())) == lds
    lab_l, lab_r, y, n_cand = mixed_labels(rng, 900, rows_l, rows_r, n0, n1)
    assert n_cand == 450
    m, u = m_u(levels, rng)
    if len(levels) == 2:
        u[0] = 0.0
        m[0] = 0.0  # patterns whose only non-null level is this one: 0 / 0, a NULL score
    c.enable_timing(True)
    counts, mp, code = check_counts(c, rows_l, rows_r, g, levels, lab_l, lab_r, y, not two,
                                    lam=LAM, one_minus=1 - LAM, m=m, u=u)
    assert c.label_pairs_info()[1] > 0.0 and counts[:2].sum() >= n_cand
    assert np.array_equal(counts.sum(axis=0), em_histogram(c))
    # mp per pattern is spk_score's value of every pair, bit for bit (NaN with NaN)
    score = c.score(LAM, 1 - LAM, m, u, 0, P)
    assert np.array_equal(mp[codes_of(g, levels)], score, equal_nan=True)
    assert len(levels) != 2 or np.isnan(score).any()
    # without m / u: the same counts and codes, no scores
    again, none, code2 = c.label_pairs_histogram(lab_l, lab_r, y)
    assert none is None and np.array_equal(again, counts) and np.array_equal(code2, code)
    c.close()


# ---- 3. orientation ------------------------------------------------------------------------------------------
def test_orientation_one_table(amd):
    levels = [2, 3]
    rng = np.random.Generator(np.random.PCG64(31))
    P, n0 = 8 * 90 + 3, 60
    rows_l, rows_r, g, _, _ = random_case(rng, P, levels, n0)
    keep = rows_l != rows_r
    rows_l, rows_r, g = rows_l[keep], rows_r[keep], g[keep]
    assert (rows_l > rows_r).any() and (rows_l < rows_r).any()
    c = make_ctx(rows_l, rows_r, g, levels, n0)
    # every distinct candidate pair labelled once, given as (r, l)
    seen, lab = set(), []
    for a, b in zip(rows_l.tolist(), rows_r.tolist()):
        if canonical(a, b, True) not in seen:
            seen.add(canonical(a, b, True))
            lab.append((b, a))
    lab_l, lab_r = np.array([p[0] for p in lab]), np.array([p[1] for p in lab])
    y = rng.integers(0, 2, len(lab)).astype(np.uint8)
    counts, _, code = check_counts(c, rows_l, rows_r, g, levels, lab_l, lab_r, y, True)
    assert counts[2].sum() == 0 and (code >= 0).all()
    # the same labels as (l, r): the same result
    again, _, code2 = c.label_pairs_histogram(lab_r, lab_l, y)
    assert np.array_equal(again, counts) and np.array_equal(code2, code)
    c.close()


def test_orientation_link_only(amd):
    levels = [2, 3]
    n0 = n1 = 40
    # candidates (a, b) with a < b only; (b, a) names valid rows of both tables and is another pair
    rows_l, rows_r = np.triu_indices(n0, k=1)
    rng = np.random.Generator(np.random.PCG64(32))
    g = np.stack([rng.integers(-1, L, len(rows_l)) for L in levels], axis=1)
    c = make_ctx(rows_l, rows_r, g, levels, n0, n1)
    pick = rng.permutation(len(rows_l))[:100]
    y = rng.integers(0, 2, 100).astype(np.uint8)
    counts, _, code = check_counts(c, rows_l, rows_r, g, levels, rows_l[pick], rows_r[pick], y, False)
    assert counts[:2].sum() == 100 and (code >= 0).all()
    counts, _, code = check_counts(c, rows_l, rows_r, g, levels, rows_r[pick], rows_l[pick], y, False)
    assert counts[:2].sum() == 0 and (code == -1).all()
    # both orders of one pair are two labels, not one given twice
    both_l = np.concatenate([rows_l[pick], rows_r[pick]])
    both_r = np.concatenate([rows_r[pick], rows_l[pick]])
    counts, _, code = check_counts(c, rows_l, rows_r, g, levels, both_l, both_r, np.concatenate([y, 1 - y]), False)
    assert counts[:2].sum() == 100 and (code[:100] >= 0).all() and (code[100:] == -1).all()
    c.close()


# ---- 4. probe chains -------------------------------------------------------------------------------------------
def test_load_one_half(amd):
    """1024 labels: capacity 2048, the largest load the capacity rule allows."""
    levels = [2, 3]
    rng = np.random.Generator(np.random.PCG64(41))
    P, n0 = 8 * 500 + 1, 300
    rows_l, rows_r, g, _, _ = random_case(rng, P, levels, n0)
    c = make_ctx(rows_l, rows_r, g, levels, n0)
    lab_l, lab_r, y, n_cand = mixed_labels(rng, 1024, rows_l, rows_r, n0)
    assert n_cand == 512
    check_counts(c, rows_l, rows_r, g, levels, lab_l, lab_r, y, True)
    pairs, _, cap, probe = c.label_pairs_info()
    assert cap == 2048 and 1 <= probe <= 2048
    c.close()


def test_constructed_collisions_wrap_around(amd):
    """Keys whose home slot is the last one of a 64-slot table, found with the documented hash: the longest insert
    probe shows that the chain wrapped and that the documented hash is the device's."""
    levels = [2, 3]
    n0, cap = 97, 64
    last = [(a, b) for a in range(n0) for b in range(a + 1, n0) if home_slot(a, b, cap) == cap - 1][:5]
    assert len(last) >= 4
    rng = np.random.Generator(np.random.PCG64(42))
    others = distinct_pairs(rng, 20, n0, avoid=last)
    lab = last + others
    assert capacity_of(len(lab)) == cap
    lab = [lab[i] for i in rng.permutation(len(lab))]
    lab_l, lab_r = np.array([p[0] for p in lab]), np.array([p[1] for p in lab])
    y = rng.integers(0, 2, len(lab)).astype(np.uint8)
    # candidates: every colliding key (twice, in both orders), half of the others, and pairs without a label
    extra = distinct_pairs(rng, 300, n0, avoid=lab)
    cand = last + [(b, a) for a, b in last] + others[::2] + extra
    cand = [cand[i] for i in rng.permutation(len(cand))]
    rows_l, rows_r = np.array([p[0] for p in cand]), np.array([p[1] for p in cand])
    g = np.stack([rng.integers(-1, L, len(cand)) for L in levels], axis=1)
    c = make_ctx(rows_l, rows_r, g, levels, n0)
    counts, _, code = check_counts(c, rows_l, rows_r, g, levels, lab_l, lab_r, y, True)
    assert counts[:2].sum() == 2 * len(last) + 10 and (code >= 0).sum() == len(last) + 10
    assert c.label_pairs_info()[3] >= 4
    c.close()


@pytest.mark.parametrize("labelled", ["all", "none"])
def test_every_pair_labelled_and_none(labelled, amd):
    levels = [2, 3]
    rng = np.random.Generator(np.random.PCG64(43))
    n0 = 80
    cand = distinct_pairs(rng, 8 * 150 + 5, n0)
    rows_l, rows_r = np.array([p[0] for p in cand]), np.array([p[1] for p in cand])
    g = np.stack([rng.integers(-1, L, len(cand)) for L in levels], axis=1)
    c = make_ctx(rows_l, rows_r, g, levels, n0)
    lab = cand if labelled == "all" else distinct_pairs(rng, 700, n0, avoid=cand)
    lab = [lab[i] for i in rng.permutation(len(lab))]
    lab_l, lab_r = np.array([p[1] for p in lab]), np.array([p[0] for p in lab])
    y = rng.integers(0, 2, len(lab)).astype(np.uint8)
    counts, _, code = check_counts(c, rows_l, rows_r, g, levels, lab_l, lab_r, y, True)
    if labelled == "all":
        assert counts[2].sum() == 0 and (code >= 0).all()
    else:
        assert counts[:2].sum() == 0 and (code == -1).all()
    c.close()


# ---- 5. agreement with the column route ---------------------------------------------------------------------
@pytest.mark.parametrize("two", [False, True], ids=["one_table", "link_only"])
def test_agrees_with_label_column(two, amd):
    levels = [2, 3]
    rng = np.random.Generator(np.random.PCG64(51 + two))
    P, n0, n1 = 8 * 400 + 7, 90, (70 if two else None)
    rows_l, rows_r, g, ids0, ids1 = random_case(rng, P, levels, n0, n1)
    if not two:  # a record with itself is no pair a labels table can hold
        keep = rows_l != rows_r
        rows_l, rows_r, g = rows_l[keep], rows_r[keep], g[keep]
    c = make_ctx(rows_l, rows_r, g, levels, n0, n1)
    a, b = ids0[rows_l], (ids0 if ids1 is None else ids1)[rows_r]
    seen, lab = set(), []
    for l, r, x, z in zip(rows_l.tolist(), rows_r.tolist(), a.tolist(), b.tolist()):
        if x >= 0 and z >= 0 and canonical(l, r, not two) not in seen:  # a repeated candidate pair: labelled once
            seen.add(canonical(l, r, not two))
            lab.append((l, r, int(x == z)))
    assert len(lab) < len(rows_l)
    lab_l, lab_r, y = (np.array([t[k] for t in lab]) for k in range(3))
    by_column, _ = c.label_histogram(ids0, ids1)
    counts, _, _ = c.label_pairs_histogram(lab_l, lab_r, y.astype(np.uint8))
    assert np.array_equal(counts, by_column) and (counts.sum(axis=1) > 0).all()
    c.close()


# ---- 6. a hand-loaded pair set that repeats a pair -------------------------------------------------------------
def test_duplicated_candidate_pair(amd):
    levels = [2, 3]
    rows_l = np.array([3, 5, 9, 5, 1, 9, 9])
    rows_r = np.array([4, 9, 5, 9, 2, 5, 8])  # (5, 9) four times, in both orders
    g = np.array([[0, 0], [1, 2], [-1, 0], [0, 1], [1, 1], [1, -1], [0, 0]])
    c = make_ctx(rows_l, rows_r, g, levels, 12)
    lab_l, lab_r, y = np.array([9, 1, 7]), np.array([5, 2, 8]), np.array([1, 0, 1], dtype=np.uint8)
    counts, _, code = check_counts(c, rows_l, rows_r, g, levels, lab_l, lab_r, y, True)
    four = codes_of(g[[1, 2, 3, 5]], levels)
    assert counts[1].sum() == 4 and counts[0].sum() == 1 and counts[2].sum() == 2
    assert code.tolist() == [int(four.max()), int(codes_of(g[[4]], levels)[0]), -1] and len(set(four.tolist())) == 4
    c.close()


# ---- 7. errors and state ---------------------------------------------------------------------------------------
def raw_call(c, n, lab_l, lab_r, y, out, mp=None, m=None, u=None):
    from splink_amd import _native as N
    N.check(c._lib.spk_label_pairs_histogram(c._h, ctypes.c_int64(n), N._ptr(lab_l), N._ptr(lab_r), N._ptr(y),
                                             ctypes.c_double(0.5), ctypes.c_double(0.5), N._ptr(m), N._ptr(u),
                                             N._ptr(out), N._ptr(mp), N._ptr(None)), "spk_label_pairs_histogram")


def test_invalid_labels(amd):
    levels = [2, 3]
    rows = np.arange(8)
    i32, u8 = (lambda *x: np.array(x, dtype=np.int32)), (lambda *x: np.array(x, dtype=np.uint8))
    c = make_ctx(rows, rows[::-1], np.zeros((8, 2)), levels, 8)
    out = np.zeros(3 * 12, dtype=np.uint64)
    bad = [
        ("outside its table", i32(1, 8), i32(2, 3), u8(0, 1)),
        ("outside its table", i32(1, 2), i32(2, -1), u8(0, 1)),
        ("with itself", i32(1, 4), i32(2, 4), u8(0, 1)),
        ("given twice", i32(1, 4, 1), i32(2, 5, 2), u8(0, 1, 0)),
        ("given twice", i32(1, 4, 2), i32(2, 5, 1), u8(0, 1, 1)),  # the other order, the other label
        ("other than 0 or 1", i32(1, 4), i32(2, 5), u8(0, 2)),
    ]
    for text, lab_l, lab_r, y in bad:
        with pytest.raises(ValueError, match=text):
            c.label_pairs_histogram(lab_l, lab_r, y)
        assert c.label_pairs_info() == NONE
    ok = (i32(1, 4), i32(2, 5), u8(0, 1))
    with pytest.raises(ValueError, match="null rows_l"):  # NULL arrays with labels
        raw_call(c, 2, None, ok[1], ok[2], out)
    with pytest.raises(ValueError, match="null rows_l"):
        raw_call(c, 2, ok[0], ok[1], None, out)
    with pytest.raises(ValueError, match="null out_counts"):
        raw_call(c, 2, *ok, None)
    with pytest.raises(ValueError, match="needs m and u"):
        raw_call(c, 2, *ok, out, mp=np.zeros(12))
    with pytest.raises(ValueError, match="come together"):
        raw_call(c, 2, *ok, out, m=np.full(5, 0.5))
    with pytest.raises(ValueError, match="2\\^27"):  # SPK_E_LIMIT, before a label is read
        raw_call(c, (1 << 27) + 1, *ok, out)
    assert c.label_pairs_info() == NONE
    # a good call after the failing ones
    c.enable_timing(True)
    counts, _, code = c.label_pairs_histogram(*ok)
    assert counts.sum() == 8 and c.label_pairs_info()[0] == 8 and c.label_pairs_info()[1] > 0.0
    c.close()
    # link_only: l == r is two records, and a row is checked against its own table
    c = make_ctx(rows, rows[::-1], np.zeros((8, 2)), levels, 8, 5 + 8)
    counts, _, code = c.label_pairs_histogram(i32(4, 7), i32(4, 12), u8(1, 0))
    assert counts.sum() == 8 and code.tolist() == [-1, -1]
    with pytest.raises(ValueError, match="outside its table"):
        c.label_pairs_histogram(i32(4, 12), i32(4, 7), u8(1, 0))
    c.close()


def test_states_and_limits(amd):
    from splink_amd import _native as N
    levels = [2, 3]
    lab = (np.array([1], dtype=np.int32), np.array([2], dtype=np.int32), np.array([1], dtype=np.uint8))
    c = N.Context(0)
    c.table_create(0, 8, 1)
    with pytest.raises(RuntimeError, match="no gammas"):  # SPK_E_STATE: no codes
        c.label_pairs_histogram(*lab)
    c.pairs_load(np.arange(4, dtype=np.int32), np.arange(4, dtype=np.int32))
    with pytest.raises(RuntimeError, match="no gammas"):
        c.label_pairs_histogram(*lab)
    c.close()
    c = N.Context(0)
    c.table_create(0, 8, 1)
    c.gammas_load(levels, np.zeros((4, 2), dtype=np.int8))  # a gamma table: codes without pair rows
    with pytest.raises(RuntimeError, match="no pair rows"):
        c.label_pairs_histogram(*lab)
    assert c.label_pairs_info() == NONE
    c.close()
    # 3 x n_patterns > 2^30 (straight at the ABI: nothing of that size is allocated on either side)
    big = [19] * 7
    c = make_ctx([0], [1], np.zeros((1, 7)), big, 8)
    assert 3 * c.n_patterns() > 1 << 30
    with pytest.raises(ValueError, match="2\\^30"):
        raw_call(c, 1, *lab, np.zeros(1, dtype=np.uint64))
    c.close()


def test_bystanders_untouched(amd):
    from splink_amd import _native as N
    levels = [2, 3]
    rng = np.random.Generator(np.random.PCG64(75))
    P, n0 = 8 * 200 + 3, 120
    rows_l, rows_r, g, _, _ = random_case(rng, P, levels, n0)
    c = make_ctx(rows_l, rows_r, g, levels, n0)
    m, u = m_u(levels, rng)
    c.score(LAM, 1 - LAM, m, u, 0, P, want_host=False)
    k = c.select(LAM, 1 - LAM, m, u, [(N.SEL_MP, 0, N.SEL_OP[">"], 0.4)])
    assert 0 < k < P
    nodes, clusters, _ = c.components()
    tf_ids = rng.integers(0, 7, n0).astype(np.int64)

    def snapshot():
        return (c.select_copy(0, k, 2), c.components_copy(0, nodes), c.tf_accumulate(7, tf_ids, tf_ids),
                c.select_info()[0], c.components_info()[:2])

    before = snapshot()
    mem = c.memory()
    lab_l, lab_r, y, _ = mixed_labels(rng, 300, rows_l, rows_r, n0)
    m2, u2 = m_u(levels, rng)  # other parameters than the selection's and the scores'
    check_counts(c, rows_l, rows_r, g, levels, lab_l, lab_r, y, True, lam=0.6, one_minus=0.4, m=m2, u=u2)
    assert c.memory() == mem  # the call's buffers are gone
    with pytest.raises(ValueError):  # and after a failing call too
        c.label_pairs_histogram(lab_l[:1], lab_l[:1], y[:1])
    assert c.memory() == mem
    after = snapshot()  # the selection made before the calls is still valid
    for x, z in zip(before[:3], after[:3]):
        for a, b in zip(x, z) if isinstance(x, tuple) else ((x, z),):
            assert np.array_equal(a, b, equal_nan=True)
    assert before[3:] == after[3:]
    c.close()


# ---- 8. end to end -----------------------------------------------------------------------------------------------
def records(n, seed):
    from splink_amd.synthetic import make_records
    return make_records(n, seed=seed, surname_vocab=120, first_vocab=80, city_vocab=20)[
        ["unique_id", "first_name", "surname", "dob", "city", "email", "cluster"]]


def scored_frames(amd, link_type, tables):
    from splink_amd import Params, add_gammas, block_using_rules, run_expectation_step
    from splink_amd.synthetic import cfg_settings
    s = cfg_settings(2)
    s["link_type"] = link_type
    s["additional_columns_to_retain"] = ["cluster"]
    params = Params(s, amd)
    st = params.settings
    kw = {"df": tables[0]} if link_type == "dedupe_only" else {"df_l": tables[0], "df_r": tables[1]}
    gf = add_gammas(block_using_rules(st, amd, **kw), st, amd)
    return params, gf, run_expectation_step(gf, params, st, amd)


def pair_key(link_type, a, b, sa=None, sb=None):
    """One hashable key per pair of records: order-free unless the job is link_only."""
    if link_type == "link_only":
        return (a, b)
    if link_type == "dedupe_only":
        return (min(a, b), max(a, b))
    return tuple(sorted([(sa, a), (sb, b)]))


def record_keys(df, link_type):
    """pair_key of every row of a frame with unique_id_l / _r (and, link_and_dedupe, _source_table_l / _r)."""
    l, r = df["unique_id_l"].tolist(), df["unique_id_r"].tolist()
    if link_type != "link_and_dedupe":
        return [pair_key(link_type, a, b) for a, b in zip(l, r)]
    return [pair_key(link_type, a, b, x, z)
            for a, b, x, z in zip(l, r, df["_source_table_l"].tolist(), df["_source_table_r"].tolist())]


def make_labels(rng, link_type, tables, pdf, n_cand=1500, n_other=300):
    """A clerical sample: candidate pairs, plus same-cluster and different-cluster pairs blocking did not produce;
    the score follows the truth except for the 5 % the reviewer got wrong; one-table pairs in either order."""
    sourced = link_type == "link_and_dedupe"
    cols = ["unique_id_l", "unique_id_r"] + (["_source_table_l", "_source_table_r"] if sourced else [])
    part = pdf.iloc[rng.permutation(len(pdf))[:n_cand]]
    data = {c: part[c].tolist() for c in cols}
    truth = (part["cluster_l"] == part["cluster_r"]).tolist()
    # the records the two sides of a pair come from
    if link_type == "link_only":
        left, right = tables
    elif sourced:
        left = right = pd.concat([tables[0].assign(_source_table="left"), tables[1].assign(_source_table="right")],
                                 ignore_index=True)
    else:
        left = right = tables[0]
    uid_l, uid_r = left["unique_id"].tolist(), right["unique_id"].tolist()
    src_l = left["_source_table"].tolist() if sourced else [None] * len(left)
    src_r = right["_source_table"].tolist() if sourced else [None] * len(right)
    cl_l, cl_r = left["cluster"].tolist(), right["cluster"].tolist()
    have = set(record_keys(pdf, link_type))
    want = {True: n_other // 2, False: n_other - n_other // 2}

    def add(i, j):
        same = cl_l[i] == cl_r[j]
        key = pair_key(link_type, uid_l[i], uid_r[j], src_l[i], src_r[j])
        if (left is right and i == j) or want[same] == 0 or key in have:
            return
        have.add(key)
        want[same] -= 1
        for c, v in zip(cols, (uid_l[i], uid_r[j], src_l[i], src_r[j])):
            data[c].append(v)
        truth.append(same)

    mates = right.groupby("cluster").indices
    for i in rng.permutation(len(left)).tolist():  # same cluster: rare among random pairs, so drawn per record
        if cl_l[i] in mates:
            add(i, int(rng.choice(mates[cl_l[i]])))
    while want[False]:
        add(int(rng.integers(0, len(left))), int(rng.integers(0, len(right))))
    assert want[True] < n_other // 2
    lab = pd.DataFrame(data)
    truth = np.array(truth, dtype=bool)
    lab["clerical_match_score"] = np.where(truth ^ (rng.random(len(lab)) < 0.05), 0.9, 0.2)
    if link_type != "link_only":  # either order
        flip = rng.random(len(lab)) < 0.5
        for x, z in [(c, c[:-2] + "_r") for c in cols if c.endswith("_l")]:
            lab.loc[flip, [x, z]] = lab.loc[flip, [z, x]].to_numpy()
    return lab.iloc[rng.permutation(len(lab))].reset_index(drop=True)


def check_pipeline(amd, link_type, tables):
    from splink_amd import LabelCounts, PairLabelCounts, Params, estimate_from_pair_labels
    params, gf, df_e = scored_frames(amd, link_type, tables)
    names, levels = gf.meta
    pdf = df_e.toPandas()
    rng = np.random.Generator(np.random.PCG64(len(pdf)))
    labels = make_labels(rng, link_type, tables, pdf)
    y = (labels["clerical_match_score"] >= 0.5).to_numpy()
    # ---- the merge the device replaces
    at = {k: i for i, k in enumerate(record_keys(pdf, link_type))}
    assert len(at) == len(pdf)
    row = np.array([at.get(k, -1) for k in record_keys(labels, link_type)])
    found = row >= 0
    assert found.sum() >= 1000 and (~found & y).any() and (~found & ~y).any()
    state = np.full(len(pdf), 2)
    state[row[found]] = y[found]
    mp = pdf[MP].to_numpy()
    lab_mp = np.where(found, mp[np.maximum(row, 0)], np.nan)
    # ---- counts
    pc = df_e.label_counts_from_pairs(labels)
    assert isinstance(pc, PairLabelCounts) and pc.link_type == link_type and pc.counts.sum() == len(pdf)
    code = codes_of(pdf[names].to_numpy(), levels)
    n_pat = n_patterns(levels)
    host_counts = np.bincount(state * n_pat + code, minlength=3 * n_pat).reshape(3, n_pat)
    assert np.array_equal(pc.counts, host_counts)
    assert pc.true_pairs_total == y.sum() and pc.missed_by_blocking == (y & ~found).sum()
    assert pc.non_matches_missed_by_blocking == (~y & ~found).sum()
    plain = gf.label_counts_from_pairs(labels)
    assert plain.mp is None and np.array_equal(plain.counts, pc.counts)
    assert np.array_equal(plain.label_code, pc.label_code)
    # ---- truth table, every row
    tt = df_e.truth_table_from_pairs(labels)
    assert len(tt) > 10 and (np.diff(tt["threshold"]) > 0).all()
    picked = df_e.truth_table_from_pairs(labels, [0.5, 0.9, 0.99])
    for table in (tt, picked):
        for r in table.itertuples():
            above = lab_mp > r.threshold  # NaN: not among the candidates, or a NULL score
            assert (r.tp, r.fp) == ((above & y).sum(), (above & ~y).sum())
            assert (r.fn, r.tn) == ((found & ~above & y).sum(), (found & ~above & ~y).sum())
            assert r.n_unlabelled_above == ((state == 2) & (mp > r.threshold)).sum()
            assert r.recall_of_all_true_pairs == r.tp / y.sum()
    # ---- the labelled pairs and the errors
    lp = pc.labelled_pairs()
    assert list(lp.columns) == list(labels.columns) + ["found_by_blocking"] + names + [MP]
    assert lp[list(labels.columns)].equals(labels) and np.array_equal(lp["found_by_blocking"].to_numpy(), found)
    assert np.array_equal(lp[MP].to_numpy(), lab_mp, equal_nan=True)
    for name in names:
        got = lp[name]
        assert np.array_equal(got.isna().to_numpy(), ~found)
        assert np.array_equal(got[found].to_numpy(dtype=np.int64), pdf[name].to_numpy()[row[found]])
    err = pc.prediction_errors(0.9)
    above = lab_mp > 0.9
    fp, fn = above & ~y, ~above & y
    assert (fp.sum() > 0) and (fn & found).sum() > 0 and (fn & ~found).sum() > 0
    assert np.array_equal(err.index.to_numpy(), np.flatnonzero(fp | fn))
    assert err["error"].tolist() == np.where(fp[fp | fn], "fp", "fn").tolist()
    assert err.drop(columns="error").equals(lp[fp | fn])
    # ---- the supervised estimate: m_step_rows on the merged host counts
    lam, rows = LabelCounts(names, levels, host_counts).m_step()
    want = Params(params.settings, amd)
    want._update_params(lam, rows)
    df_e2 = estimate_from_pair_labels(gf, params, params.settings, amd, labels)
    assert params.params["λ"] == want.params["λ"] and params.params["π"] == want.params["π"]
    assert 0 < params.params["λ"] < 1 and params.iteration == 2
    m, u = gf.job.flat_tables(params._level_probabilities())
    lam = float(params.params["λ"])
    assert np.array_equal(df_e2.toPandas()[MP].to_numpy(), gf.job.ctx.score(lam, float(1 - lam), m, u, 0, len(pdf)),
                          equal_nan=True)
    return gf, df_e, labels


def test_pipeline_dedupe_only(amd):
    check_pipeline(amd, "dedupe_only", [records(3000, seed=3)])


def test_pipeline_link_only(amd):
    df = records(3000, seed=4)
    check_pipeline(amd, "link_only", [df.iloc[::2].reset_index(drop=True), df.iloc[1::2].reset_index(drop=True)])


def test_pipeline_link_and_dedupe_colliding_ids(amd):
    df = records(3000, seed=5)
    left, right = df.iloc[::2].reset_index(drop=True), df.iloc[1::2].reset_index(drop=True)
    left["unique_id"] = np.arange(len(left))
    right["unique_id"] = np.arange(len(right))  # every id occurs in both inputs
    gf, df_e, labels = check_pipeline(amd, "link_and_dedupe", [left, right])
    with pytest.raises(ValueError, match="_source_table_l"):
        df_e.label_counts_from_pairs(labels.drop(columns=["_source_table_l", "_source_table_r"]))


def test_refusals_before_the_device(amd):
    from splink_amd import estimate_from_pair_labels
    _, gf, df_e = scored_frames(amd, "dedupe_only", [records(600, seed=9)])
    pdf = df_e.toPandas()
    labels = pdf[["unique_id_l", "unique_id_r"]].head(20).assign(clerical_match_score=1.0)
    with pytest.raises(ValueError, match="clerical_match_score"):
        df_e.label_counts_from_pairs(labels.drop(columns="clerical_match_score"))
    with pytest.raises(ValueError, match="filtered frame"):
        estimate_from_pair_labels(df_e.filter(f"{MP} > 0.5"), None, {}, amd, labels)
    have = set(record_keys(pdf, "dedupe_only"))
    a = int(pdf["unique_id_l"].iloc[0])
    b = next(int(x) for x in pdf["unique_id_r"] if x != a and pair_key("dedupe_only", a, int(x)) not in have)
    far = pd.DataFrame({"unique_id_l": [a], "unique_id_r": [b], "clerical_match_score": [1.0]})
    with pytest.raises(ValueError, match="no labelled pair"):
        estimate_from_pair_labels(gf, None, {}, amd, far)
    assert df_e.label_counts_from_pairs(labels).counts[1].sum() == 20


# ---- 9. the sharded path at one rank ---------------------------------------------------------------------------
@pytest.fixture
def nccl_group():
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


def test_sharded_path_at_one_rank(amd, nccl_group):
    """force_reduce, as tests/test_gpu_dist.py sets it for the EM histogram: the counts (summed) and the labels' codes
    (their maximum) go through the host all-reduce and come back the same."""
    _, gf, df_e = scored_frames(amd, "dedupe_only", [records(1500, seed=5)])
    pdf = df_e.toPandas()
    rng = np.random.Generator(np.random.PCG64(9))
    labels = make_labels(rng, "dedupe_only", [records(1500, seed=5)], pdf, n_cand=600, n_other=60)
    local = df_e.label_counts_from_pairs(labels)
    gf.job.force_reduce = True
    reduced = df_e.label_counts_from_pairs(labels)
    gf.job.force_reduce = False
    assert np.array_equal(local.counts, reduced.counts) and np.array_equal(local.mp, reduced.mp, equal_nan=True)
    assert np.array_equal(local.label_code, reduced.label_code) and (local.label_code >= 0).sum() == 600
    assert local.true_pairs_total == reduced.true_pairs_total and local.counts[1].sum() > 0
