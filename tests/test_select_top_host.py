"""orderBy / limit without a device: the argument validation, asc / desc, the key mapping, and the emulated passes of
spk_select_top / spk_select_top_of (tools/emulate_select_top.py) against the definition (a stable sort, NULL lowest)."""
import numpy as np
import pytest

import splink_amd
from splink_amd import select as S
from select_top_common import definition_order, emulator

MP = ("match_probability",)
TF = ("tf_adjusted_match_prob", "match_probability")


def test_top_args_accepts():
    assert S.top_args("match_probability", True, 5, MP) == (S.FIELD_MP, S.TOP_ASC, 5)
    assert S.top_args("match_probability", False, 0, MP) == (S.FIELD_MP, S.TOP_DESC, 0)
    assert S.top_args("tf_adjusted_match_prob", False, 7, TF) == (S.FIELD_TF, S.TOP_DESC, 7)
    assert S.top_args("match_probability", np.bool_(True), np.int64(3), TF) == (S.FIELD_MP, S.TOP_ASC, 3)
    assert S.top_args(None, True, 9, ()) == (None, S.TOP_FIRST, 9)          # limit alone needs no score
    field, order, k = S.top_args("match_probability", True, None, MP)        # orderBy without limit: every pair
    assert (field, order) == (S.FIELD_MP, S.TOP_ASC) and k >= (1 << 62)
    assert S.top_args(None, True, 1 << 70, ())[2] == (1 << 63) - 1          # clamped to the ABI's int64


@pytest.mark.parametrize("k", [-1, True, False, 1.0, "3", [1]])
def test_top_args_rejects_k(k):
    with pytest.raises(ValueError, match="limit"):
        S.top_args(None, True, k, MP)
    with pytest.raises(ValueError, match="limit"):
        S.top_args("match_probability", True, k, MP)


@pytest.mark.parametrize("column,allowed", [("gamma_surname", MP), ("tf_adjusted_match_prob", MP), ("surname_l", TF),
                                            (3, MP), (("match_probability", "gamma_x"), MP), ("match_probability", ())])
def test_top_args_rejects_column(column, allowed):
    with pytest.raises(ValueError, match="orderBy") as e:
        S.top_args(column, True, 5, allowed)
    for name in allowed:
        assert name in str(e.value)  # names the supported ones


def test_top_args_rejects_ascending():
    with pytest.raises(ValueError, match="ascending"):
        S.top_args("match_probability", "no", 5, MP)
    with pytest.raises(ValueError, match="ascending"):
        S.top_args("match_probability", 0, 5, MP)


def test_asc_desc_behave_as_ascending():
    assert splink_amd.asc is S.asc and splink_amd.desc is S.desc
    for ascending in (True, False):
        assert S.top_args(S.asc("match_probability"), ascending, 4, MP) == S.top_args("match_probability", True, 4, MP)
        assert S.top_args(S.desc("match_probability"), ascending, 4, MP) == S.top_args("match_probability", False, 4, MP)
    with pytest.raises(ValueError, match="orderBy"):
        S.top_args(S.desc("gamma_city"), True, 4, MP)


def test_key_mapping_is_monotone():
    emu = emulator()
    denormal = np.float64(5e-324)
    ladder = [np.nan, -np.inf, -1.0, -0.0, 0.0, denormal, 1.0, np.nextafter(1.0, 2.0), np.inf]
    asc = emu.key(ladder, emu.ASC).tolist()
    desc = emu.key(ladder, emu.DESC).tolist()
    assert asc[3] == asc[4] and desc[3] == desc[4]           # -0.0 and +0.0 share a key
    distinct = [0, 1, 2, 3, 5, 6, 7, 8]
    assert all(asc[a] < asc[b] for a, b in zip(distinct, distinct[1:]))
    assert all(desc[a] > desc[b] for a, b in zip(distinct, distinct[1:]))
    assert asc[0] == 0 and desc[0] == (1 << 64) - 1          # NULL: first ascending, last descending
    for x in ladder[1:]:
        for order in (emu.ASC, emu.DESC):
            back = emu.key_score(emu.key([x], order)[0], order)
            assert back == x                                  # the cut score read back from the key
    assert np.isnan(emu.key_score(emu.key([np.nan], emu.DESC)[0], emu.DESC))


def test_top_order_equals_definition():
    rng = np.random.Generator(np.random.PCG64(5))
    values = np.concatenate([rng.random(7), [np.nan, -0.0, 0.0, -np.inf, np.inf]])
    score = values[rng.integers(0, len(values), 500)]
    assert np.array_equal(S.top_order(score, S.TOP_ASC), definition_order(score, True))
    assert np.array_equal(S.top_order(score, S.TOP_DESC), definition_order(score, False))
    assert np.array_equal(S.top_order(score, S.TOP_FIRST), np.arange(500))


def _figures(score, eligible, order, k, emu):
    """(kept mask, (eligible, kept, cut score, tied, tied_kept)) by the definition, written out here."""
    idx = np.nonzero(eligible)[0]
    if order != emu.FIRST:
        idx = idx[definition_order(score[idx], order == emu.ASC)]
    kk = min(k, len(idx))
    kept = np.zeros(len(score), dtype=bool)
    kept[idx[:kk]] = True
    fig = (len(idx), kk, None, 0, 0)
    if order != emu.FIRST and 0 < k < len(idx):
        s = score[idx[kk - 1]]
        same = eligible & (np.isnan(score) if s != s else (score == s))
        fig = (len(idx), kk, None if s != s else float(s), int(same.sum()), int((same & kept).sum()))
    return kept, fig


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 4097])
@pytest.mark.parametrize("distinct", [3, 600])
def test_emulated_passes_equal_the_definition(n, distinct):
    emu = emulator()
    rng = np.random.Generator(np.random.PCG64(100 * n + distinct))
    values = np.concatenate([rng.random(distinct), [np.nan, -0.0, 0.0]])
    weight = np.ones(len(values))
    weight[0] = len(values)            # one large tie class
    weight[distinct] = len(values) / 4  # and many NULLs
    code = rng.choice(len(values), size=n, p=weight / weight.sum())
    score = values[code]
    pat_eligible = rng.random(len(values)) < 0.85
    pat_eligible[[0, distinct, distinct + 1, distinct + 2]] = True
    every = np.ones(n, dtype=bool)
    largest = int((code == 0).sum())
    for order in (emu.FIRST, emu.ASC, emu.DESC):
        # a k inside the largest tie class: past what sorts before value 0 under the order, plus half of the class
        before = int((np.isnan(score) | (score < values[0])).sum()) if order == emu.ASC else int((score > values[0]).sum())
        inside = before + max(largest // 2, 1) if largest else n // 2
        for k in (0, 1, inside, n, n + 5):
            exp = _figures(score, every, order, k, emu)
            for got in (emu.top_of_by_passes(score, order, k, chunk=64), emu.top_by_definition(score, every, order, k)):
                assert np.array_equal(got[0], exp[0]) and got[1] == exp[1], (order, k, got[1], exp[1])
            if order != emu.FIRST and k == inside and largest > 1 and 0 < k < n:
                assert exp[1][3] >= largest and 0 < exp[1][4] < exp[1][3]  # the cut does split the class
            el = pat_eligible[code]
            k_el = min(k, max(int(el.sum()) - 1, 0)) if k == inside else k
            exp = _figures(score, el, order, k_el, emu)
            for got in (emu.top_by_passes(code, values, pat_eligible, order, k_el, chunk=64),
                        emu.top_by_definition(score, el, order, k_el)):
                assert np.array_equal(got[0], exp[0]) and got[1] == exp[1], (order, k_el, got[1], exp[1])


def test_emit_rule_spans_chunks():
    """One class at the cut across many chunks: a chunk's output starts at above-before + min(at-before, r)."""
    emu = emulator()
    cls = np.array([emu.AT, emu.ABOVE, emu.OUT] * 100)
    for r in (0, 1, 33, 34, 100, 150):
        kept, where = emu.emit(cls, r, chunk=7)
        exp = (cls == emu.ABOVE) | ((cls == emu.AT) & (np.cumsum(cls == emu.AT) <= r))
        assert np.array_equal(kept, exp)
        assert np.array_equal(where[kept], np.arange(kept.sum()))  # dense, in ordinal order
