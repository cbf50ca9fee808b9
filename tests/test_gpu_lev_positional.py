"""The positional Levenshtein sketch in the filter pass (spk_gammas_set_lev_bound, spk_filter.hip): a pair table of
email-shaped strings that share a surname, adversarial strings (short and odd lengths, saturated buckets, Latin-1,
front insertions, swapped halves, rows without a sketch) and pairs whose distance sits exactly on a ratio cut and
one past it, under the levenshtein_3 / levenshtein_4 templates and a plain `levenshtein <= 2` chain.  Every level
equals the oracle's; the codes are the same with the whole-string field (mode 0), in every exact-pass kernel mode
and on one and two streams; the positional field lists fewer cells for the exact pass; and a free-text column of
the same job keeps its character-bag decisions (k_compact_lev)."""
import os
import sys

import numpy as np
import pandas as pd
import pytest

import oracle as orc

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import positional_common as pc  # noqa: E402

pytestmark = pytest.mark.gpu

N_FREE = 240  # rows whose free-text column is filled


@pytest.fixture(scope="module")
def amd():
    from splink_amd import AmdSession, _native
    if _native.device_count() == 0:
        pytest.fail("no HIP device visible: the -m gpu tests need an MI355X")
    return AmdSession(0)


def _clip(s, n_bytes=64):
    while len(s.encode("utf-8")) > n_bytes:
        s = s[:-1]
    return s


def _pairs():
    rng = np.random.Generator(np.random.PCG64(31))
    ps = pc.email_pairs(rng, 1500) + pc.adversarial_pairs(rng, 1200)
    for t in (0.2, 0.3, 0.4):  # the cuts of levenshtein_3 / levenshtein_4
        ps += pc.threshold_pairs(rng, 45, t)
    ps += [(p[0], p[0]) for p in ps[:40]] + [("", ""), ("", "a"), ("ab", "ba"), ("abc", "abd")]
    # the right side stays within 64 UTF-8 bytes, so the column has no free-text rows (long rows on one side only)
    left = [a if len(a) >= len(b) else b for a, b in ps]
    right = [_clip(b if len(a) >= len(b) else a) for a, b in ps]
    left += [None, "x", None]
    right += ["x", None, None]
    return left, right


def _free_text(rng, n):
    alpha = list("abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789 ,.-")
    left, right = [], []
    for i in range(n):
        k = int(rng.integers(66, 120))
        a = "".join(alpha[int(j)] for j in rng.integers(0, len(alpha), k))
        if i % 4 == 0:  # a near copy: scanned
            b = list(a)
            for _ in range(int(rng.integers(1, 12))):
                b[int(rng.integers(len(b)))] = alpha[int(rng.integers(len(alpha)))]
            b = "".join(b)
        else:  # unrelated: mostly decided by the bags
            b = "".join(alpha[int(j)] for j in rng.integers(0, len(alpha), int(rng.integers(66, 120))))
        left.append(a)
        right.append(b)
    return left, right


def _ratio_level(a, b, d, cuts):
    """Level of the levenshtein_3 / _4 template: len(cuts) + 1 for equal strings, then one per cut passed."""
    if a == b:
        return len(cuts) + 1
    den = (len(a) + len(b)) / 2.0
    for i, t in enumerate(cuts):
        if d / den <= t:
            return len(cuts) - i
    return 0


@pytest.fixture(scope="module")
def frames(amd):
    """Two jobs over the same pairs (the filter kernel takes three Levenshtein columns): the two ratio templates with
    a free-text column, and the plain chain."""
    from splink_amd import case_statements as cs
    from splink_amd.gammas import add_gammas
    left, right = _pairs()
    fl, fr = _free_text(np.random.Generator(np.random.PCG64(32)), N_FREE)
    pad = [None] * (len(left) - N_FREE)
    df = pd.DataFrame({"a_l": left, "a_r": right, "t_l": fl + pad, "t_r": fr + pad})
    chain = ("case when a_l is null or a_r is null then -1 when a_l = a_r then 2 "
             "when levenshtein(a_l, a_r) <= 2 then 1 else 0 end")
    st = {"link_type": "dedupe_only", "comparison_columns": [
        {"custom_name": "l3", "custom_columns_used": ["a"], "num_levels": 3,
         "case_expression": cs.sql_gen_case_stmt_levenshtein_3("a")},
        {"custom_name": "l4", "custom_columns_used": ["a"], "num_levels": 4,
         "case_expression": cs.sql_gen_case_stmt_levenshtein_4("a")},
        {"custom_name": "ft", "custom_columns_used": ["t"], "num_levels": 4,
         "case_expression": cs.sql_gen_case_stmt_levenshtein_4("t")}]}
    st_chain = {"link_type": "dedupe_only", "comparison_columns": [
        {"custom_name": "lc", "custom_columns_used": ["a"], "num_levels": 3, "case_expression": chain}]}
    want = np.full((len(left), 3), -1, dtype=np.int64)
    want_chain = np.full((len(left), 1), -1, dtype=np.int64)
    for i, (a, b) in enumerate(zip(left, right)):
        if a is not None and b is not None:
            d = orc.levenshtein(a, b)
            want[i, 0] = _ratio_level(a, b, d, [0.3])
            want[i, 1] = _ratio_level(a, b, d, [0.2, 0.4])
            want_chain[i, 0] = 2 if a == b else (1 if d <= 2 else 0)
        if i < N_FREE:
            want[i, 2] = _ratio_level(fl[i], fr[i], orc.levenshtein(fl[i], fr[i]), [0.2, 0.4])
    return [(add_gammas(df, st, amd), want), (add_gammas(df[["a_l", "a_r"]], st_chain, amd), want_chain)]


def _run(gf, bound, kern=2, streams=1):
    ctx = gf.job.ctx
    ctx.gammas_set_lev_bound(bound)
    ctx.gammas_set_lev_kernel(kern)
    if streams == 2:
        ctx.gammas_set_streams(2, 0)
    else:
        ctx.gammas_set_streams(1)
    try:
        gf.job.gammas(gf.settings)
        codes = gf.job.gammas_host()
        exact = [int(x) for x in ctx.gammas_exact_counts(codes.shape[1])]
    finally:
        ctx.gammas_set_lev_bound(1)
        ctx.gammas_set_lev_kernel(2)
        ctx.gammas_set_streams(2)
    return codes, exact


def test_levels_equal_the_oracle(frames):
    for gf, want in frames:
        got = gf.gamma_matrix()
        bad = np.nonzero((got != want).any(axis=1))[0]
        assert len(bad) == 0, (bad[:10], got[bad[:10]], want[bad[:10]])


def test_both_fields_give_the_same_codes_and_the_positional_one_lists_fewer_cells(frames):
    for j, (gf, want) in enumerate(frames):
        c1, e1 = _run(gf, 1)
        c0, e0 = _run(gf, 0)
        print(f"job {j}: cells listed for the exact pass per column: whole-string field {e0}, positional {e1}")
        assert (c1 == want).all() and (c0 == want).all()
        if j == 0:
            assert e1[0] < e0[0] and e1[1] < e0[1]
            assert e1[2] == e0[2]  # the free-text column keeps its field
        again, e1b = _run(gf, 1)  # and back: the image is laid out again on every change of mode
        assert (again == want).all() and e1b == e1


@pytest.mark.parametrize("streams", [1, 2])
@pytest.mark.parametrize("kern", [0, 1, 2, 3])
def test_kernel_modes_and_streams_agree(frames, kern, streams):
    for gf, want in frames:
        for bound in (1, 0):
            codes, _ = _run(gf, bound, kern, streams)
            assert (codes == want).all(), (bound, kern, streams, np.nonzero((codes != want).any(axis=1))[0][:10])


def test_free_text_column_keeps_its_bag_decisions(frames):
    gf, want = frames[0]
    ctx = gf.job.ctx
    ctx.gammas_set_streams(1)
    try:
        gf.job.gammas(gf.settings)
        assert (gf.job.gammas_host() == want).all()
        n = int(ctx.gammas_exact_counts(3)[2])
        items = ctx.gammas_exact_list(2, n)
    finally:
        ctx.gammas_set_streams(2)
    assert n > 0 and (items < 0).sum() > 0, "no free-text cell was decided from its character bag"
