"""Host restatement (positional_common.py) of the positional sketch and the Levenshtein lower bound the filter
derives from it, checked against the oracle's Levenshtein over code points: the bound never exceeds the
distance, its closed form is the minimum of the two-segment expression over every split point, and on
email-shaped pairs that share a surname it decides more cells than the whole-string sketch does."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import oracle as orc  # noqa: E402
import positional_common as pc  # noqa: E402


@pytest.fixture(scope="module")
def pairs():
    rng = np.random.Generator(np.random.PCG64(11))
    return pc.adversarial_pairs(rng, 2400) + pc.email_pairs(rng, 600) + pc.threshold_pairs(rng, 120)


def test_rows():
    assert pc.pos_row(None) == pc.LEN_NULL
    assert pc.pos_row("") == 0
    assert pc.pos_row("a" * 253) & 255 == 253
    assert pc.pos_row("a" * 254) == pc.LEN_NONE and pc.pos_row("ab\U0001F600") == pc.LEN_NONE
    n, h1, h2 = pc.row_counts(pc.pos_row("Aaab.b7"))  # halves "Aaab" / ".b7"
    assert n == 7 and h1[0] == 3 and h1[1] == 1 and h2[1] == 1 and h2[29] == 1 and h2[27] == 1  # '.' = 46, '7' = 55
    assert h1.sum() == 4 and h2.sum() == 3


def test_bound_never_exceeds_levenshtein(pairs):
    none = decided = 0
    for a, b in pairs:
        bnd = pc.pos_bound(a, b)
        no_sketch = any(len(s) >= 254 or any(ord(c) >= 0x10000 for c in s) for s in (a, b))
        assert (bnd is None) == no_sketch, (a, b)
        if bnd is None:
            none += 1
            continue
        d = orc.levenshtein(a, b)
        assert bnd <= d, (a, b, bnd, d)
        decided += bnd > pc.ratio_cut(a, b)
    assert none > 100 and decided > 500


def test_closed_form_is_the_minimum_over_every_split(pairs):
    for a, b in pairs:
        ra, rb = pc.pos_row(a), pc.pos_row(b)
        if (ra & 255) >= pc.LEN_NONE or (rb & 255) >= pc.LEN_NONE:
            continue
        for x, y in ((ra, rb), (rb, ra)):
            _, _, seg, parts = pc.pos_terms(x, y)
            assert seg == pc.two_segment_brute(*parts), (a, b, parts)


def test_closed_form_on_every_small_case():
    """Every (A1, A2, B1, B2, I1, I2) with halves up to 4 units and I <= min of the halves' lengths."""
    for A1 in range(5):
        for A2 in range(5):
            for B1 in range(5):
                for B2 in range(5):
                    for I1 in range(min(A1, B1) + 1):
                        for I2 in range(min(A2, B2) + 1):
                            p = (A1, A2, B1, B2, I1, I2)
                            assert pc.two_segment_closed(*p) == pc.two_segment_brute(*p), p


def test_threshold_pairs_sit_on_the_cut():
    rng = np.random.Generator(np.random.PCG64(12))
    ps = pc.threshold_pairs(rng, 30)
    for i, (a, b) in enumerate(ps):
        assert orc.levenshtein(a, b) == pc.ratio_cut(a, b) + (i & 1), (a, b)
        assert pc.pos_bound(a, b) <= orc.levenshtein(a, b)


def test_decides_more_email_cells_than_the_whole_string_sketch():
    rng = np.random.Generator(np.random.PCG64(13))
    ps = pc.email_pairs(rng, 2000)
    whole = pos = 0
    for a, b in ps:
        cut = pc.ratio_cut(a, b, 0.3)
        whole += pc.unit_bound(a, b) > cut
        pos += pc.pos_bound(a, b) > cut
    print(f"decided at ratio 0.3: whole-string sketch {whole}, positional sketch {pos} of {len(ps)}")
    assert pos > whole
