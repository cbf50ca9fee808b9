"""filtered.best_matches(): the constants, the argument check and the header (no GPU)."""
import os
import re

import pytest

from conftest import ROOT

from splink_amd import _native as N
from splink_amd import select as SEL

SYMBOLS = ["spk_select_best", "spk_select_best_info"]


def header():
    return open(os.path.join(ROOT, "include", "splink_hip.h")).read()


def test_constants_equal_the_header_defines():
    mine = {"SPK_BEST_L": N.BEST_L, "SPK_BEST_R": N.BEST_R, "SPK_BEST_EITHER": N.BEST_EITHER,
            "SPK_BEST_MUTUAL": N.BEST_MUTUAL}
    text = header()
    for name, value in mine.items():
        m = re.search(r"^#define %s (\d+)\b" % name, text, flags=re.M)
        assert m, name
        assert int(m.group(1)) == value, name
    assert sorted(mine.values()) == [0, 1, 2, 3]
    # the fields best_matches ranks by are the selection's
    for name, value in (("SPK_SEL_MP", N.SEL_MP), ("SPK_SEL_TF_MP", N.SEL_TF_MP)):
        assert int(re.search(r"^#define %s (\d+)\b" % name, text, flags=re.M).group(1)) == value


def test_arguments_map_to_the_native_values():
    f = SEL.best_match_args
    assert f() == (N.SEL_MP, N.BEST_L, 0)
    both = ("tf_adjusted_match_prob", "match_probability")
    for per, mode in (("l", N.BEST_L), ("r", N.BEST_R), ("either", N.BEST_EITHER), ("mutual", N.BEST_MUTUAL)):
        for ties, keep in (("first", 0), ("all", 1)):
            assert f(per, ties, "match_probability") == (N.SEL_MP, mode, keep)
            assert f(per=per, ties=ties, by="tf_adjusted_match_prob", allowed_by=both) == (N.SEL_TF_MP, mode, keep)
            assert f(per=per, ties=ties, by="match_probability", allowed_by=both) == (N.SEL_MP, mode, keep)


@pytest.mark.parametrize("kwargs, legal", [
    ({"per": "left"}, ["'l'", "'r'", "'either'", "'mutual'"]),
    ({"per": None}, ["'l'", "'r'", "'either'", "'mutual'"]),
    ({"per": 0}, ["'l'", "'r'", "'either'", "'mutual'"]),
    ({"ties": "any"}, ["'first'", "'all'"]),
    ({"ties": True}, ["'first'", "'all'"]),
    ({"by": "gamma_surname"}, ["'match_probability'"]),
    ({"by": "tf_adjusted_match_prob"}, ["'match_probability'"]),  # a frame without the tf score
    ({"by": "score", "allowed_by": ("tf_adjusted_match_prob", "match_probability")},
     ["'match_probability'", "'tf_adjusted_match_prob'"]),
])
def test_illegal_arguments_name_the_legal_values(kwargs, legal):
    with pytest.raises(ValueError) as e:
        SEL.best_match_args(**kwargs)
    msg = str(e.value)
    bad = next(k for k in ("per", "ties", "by") if k in kwargs)
    assert msg.startswith("best_matches: %s=" % bad)
    for word in legal:
        assert word in msg, (word, msg)
    if kwargs.get("by") == "tf_adjusted_match_prob":
        assert "'tf_adjusted_match_prob'" not in msg.split("legal values:")[1]


def test_header_declares_both_functions():
    lib = N.load_library()
    for name in SYMBOLS:
        getattr(lib, name)
    assert set(SYMBOLS) <= set(N.EXPORTS)
    text = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    for name in SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(\s*spk_ctx \*ctx" % name, text), name
    assert re.search(r"spk_select_best\(spk_ctx \*ctx,\s*int field\s*,\s*int mode,\s*int keep_ties,\s*int64_t \*out_n_kept\)",
                     text)
    assert re.search(r"spk_select_best_info\(spk_ctx \*ctx,\s*int64_t \*out_n_before,\s*int64_t \*out_n_kept,\s*"
                     r"double \*out_ms\)", text)


def test_frames_have_the_methods_and_the_stage_functions_refuse_the_frame():
    from splink_amd import BestMatchFrame, FilteredFrame
    from splink_amd.frames import ExpectationFrame, reject_filtered
    from splink_amd.term_frequencies import TermFrequencyFrame, TfFilteredFrame
    for cls in (FilteredFrame, TfFilteredFrame, ExpectationFrame, TermFrequencyFrame):
        assert callable(cls.best_matches), cls
    for name in ("select_best", "select_best_info"):
        assert callable(getattr(N.Context, name)), name
    assert issubclass(BestMatchFrame, FilteredFrame)
    b = BestMatchFrame.__new__(BestMatchFrame)
    with pytest.raises(ValueError, match="best-match frame"):
        reject_filtered(b, "run_expectation_step")
    for method in (b.filter, b.where, b.best_matches):
        with pytest.raises(ValueError, match="filter first"):
            method("match_probability > 0.5")
