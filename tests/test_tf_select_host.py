"""tf.filter(condition): tf_adjusted_match_prob in the predicate compiler, the SPK_SEL_TF_MP constant and the
term-frequency frame's surface (no GPU)."""
import os
import re

import pytest

from conftest import ROOT

from splink_amd import _native as N
from splink_amd.select import FIELD_GAMMA, FIELD_MP, FIELD_TF, MAX_TERMS, OP, Term, compile_condition

GAMMAS = ["gamma_first_name", "gamma_surname", "gamma_dob"]


def tf_terms(cond):
    p = compile_condition(cond, GAMMAS, allow_mp=True, allow_tf=True)
    assert not p.never
    return list(p.terms)


def test_default_still_rejects_the_tf_column():
    for kwargs in ({}, {"allow_mp": True}, {"allow_mp": False}, {"allow_tf": False}):
        with pytest.raises(ValueError, match="column 'tf_adjusted_match_prob'") as e:
            compile_condition("tf_adjusted_match_prob > 0.5", GAMMAS, **kwargs)
        assert "supported:" in str(e.value) and "tf_adjusted_match_prob (the term-frequency frame)" not in str(e.value)


def test_tf_term_forms():
    assert tf_terms("tf_adjusted_match_prob > 0.99") == [Term(FIELD_TF, 0, OP[">"], 0.99)]
    assert tf_terms("TF_ADJUSTED_MATCH_PROB >= 1") == [Term(FIELD_TF, 0, OP[">="], 1.0)]
    for text, op in (("<", "<"), ("<=", "<="), (">", ">"), (">=", ">="), ("=", "="), ("==", "="), ("!=", "!="),
                     ("<>", "!=")):
        assert tf_terms(f"tf_adjusted_match_prob {text} 0.25") == [Term(FIELD_TF, 0, OP[op], 0.25)], text
    assert tf_terms("tf_adjusted_match_prob < 1e-3") == [Term(FIELD_TF, 0, OP["<"], 1e-3)]


def test_literal_on_the_left_flips_the_operator():
    assert tf_terms("0.9 < tf_adjusted_match_prob") == [Term(FIELD_TF, 0, OP[">"], 0.9)]
    assert tf_terms("0.9 >= tf_adjusted_match_prob") == [Term(FIELD_TF, 0, OP["<="], 0.9)]
    assert tf_terms("0.5 = tf_adjusted_match_prob") == [Term(FIELD_TF, 0, OP["="], 0.5)]
    assert tf_terms("0.5 <> tf_adjusted_match_prob") == [Term(FIELD_TF, 0, OP["!="], 0.5)]


def test_is_null_on_the_tf_column_goes_to_the_device():
    assert tf_terms("tf_adjusted_match_prob is null") == [Term(FIELD_TF, 0, OP["is null"], 0.0)]
    assert tf_terms("tf_adjusted_match_prob IS NOT NULL") == [Term(FIELD_TF, 0, OP["is not null"], 0.0)]


def test_mixed_fields_keep_order_and_needs_tf():
    p = compile_condition("tf_adjusted_match_prob > 0.9 and match_probability >= 0.5 and gamma_surname >= 1",
                          GAMMAS, allow_tf=True)
    assert list(p.terms) == [Term(FIELD_TF, 0, OP[">"], 0.9), Term(FIELD_MP, 0, OP[">="], 0.5),
                             Term(FIELD_GAMMA, 1, OP[">="], 1.0)]
    assert p.native_terms() == [(N.SEL_TF_MP, 0, OP[">"], 0.9), (N.SEL_MP, 0, OP[">="], 0.5),
                                (N.SEL_GAMMA, 1, OP[">="], 1.0)]
    assert p.needs_tf and p.needs_mp
    q = compile_condition("match_probability >= 0.5 and gamma_dob = -1", GAMMAS, allow_tf=True)
    assert not q.needs_tf and q.needs_mp
    assert q.and_(p).needs_tf
    r = compile_condition("gamma_dob is null and tf_adjusted_match_prob > 0.5", GAMMAS, allow_tf=True)
    assert r.never and r.needs_tf and r.native_terms() == [(FIELD_GAMMA, 0, OP["is null"], 0.0)]


def test_eight_term_limit_across_mixed_fields():
    three = compile_condition("tf_adjusted_match_prob > 0.1 and match_probability > 0.1 and gamma_dob >= 0", GAMMAS,
                              allow_tf=True)
    five = compile_condition(" and ".join(["tf_adjusted_match_prob < 0.9", "gamma_surname >= 0"] * 2 +
                                          ["match_probability < 0.9"]), GAMMAS, allow_tf=True)
    assert len(three.and_(five).terms) == MAX_TERMS == 8
    with pytest.raises(ValueError, match="more than 8 terms"):
        three.and_(five).and_(compile_condition("tf_adjusted_match_prob is not null", GAMMAS, allow_tf=True))
    with pytest.raises(ValueError, match="more than 8 terms"):
        compile_condition(" and ".join(["tf_adjusted_match_prob > 0.1"] * 9), GAMMAS, allow_tf=True)


@pytest.mark.parametrize("cond,named", [
    ("tf_adjusted_match_prob > 0.9 or gamma_dob = 1", "OR"),
    ("surname_adj > 0.5", "column 'surname_adj'"),
    ("l.tf_adjusted_match_prob > 0.5", r"column 'l\.tf_adjusted_match_prob'"),
    ("tf_adjusted_match_prob > 'x'", "string literal 'x'"),
    ("tf_adjusted_match_prob > match_probability", "column 'match_probability'"),
])
def test_rejections_on_a_tf_frame_name_the_tf_column_as_supported(cond, named):
    with pytest.raises(ValueError, match=named) as e:
        compile_condition(cond, GAMMAS, allow_tf=True)
    assert "supported:" in str(e.value) and "tf_adjusted_match_prob (the term-frequency frame)" in str(e.value)


def test_header_constant_matches_the_binding():
    text = open(os.path.join(ROOT, "include", "splink_hip.h")).read()
    consts = dict(re.findall(r"#define (SPK_SEL[A-Z_]*) (\d+)", text))
    assert int(consts["SPK_SEL_TF_MP"]) == N.SEL_TF_MP == FIELD_TF == 2
    assert len({N.SEL_MP, N.SEL_GAMMA, N.SEL_TF_MP}) == 3
    for name in ("spk_select_tf", "spk_select_tf_columns", "spk_select_copy_tf"):
        assert name in N.EXPORTS and re.search(r"\b%s\s*\(" % name, text)
    for name in ("select_tf", "select_tf_columns", "select_copy_tf"):
        assert callable(getattr(N.Context, name))


def test_tf_frame_offers_filter_where_and_clusters():
    from splink_amd.frames import FilteredFrame
    from splink_amd.term_frequencies import TermFrequencyFrame, TfFilteredFrame
    assert callable(TermFrequencyFrame.filter) and TermFrequencyFrame.where is TermFrequencyFrame.filter
    assert callable(TermFrequencyFrame.clusters)
    assert issubclass(TfFilteredFrame, FilteredFrame) and TfFilteredFrame.where is TfFilteredFrame.filter


def test_stage_functions_reject_a_tf_filtered_frame():
    from splink_amd.frames import reject_filtered
    from splink_amd.term_frequencies import TfFilteredFrame
    f = TfFilteredFrame.__new__(TfFilteredFrame)
    for what in ("iterate", "make_adjustment_for_term_frequencies"):
        with pytest.raises(ValueError, match="filtered frame"):
            reject_filtered(f, what)
