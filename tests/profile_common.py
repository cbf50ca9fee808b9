"""A pandas / numpy restatement of spk_block_profile's key-level figures, for rules whose key terms are plain columns
or one substr of a column: group sizes per side, n(n-1)/2 or nL * nR candidates per block, bit-length bins, and the
top-k multiset.  Exact Python integers throughout; shared by tests/test_block_profile_host.py (which checks it
against the reference's fixture) and tests/test_gpu_block_profile.py (which checks the device against it)."""
from collections import Counter

import numpy as np
import pandas as pd

BINS = 64


def _null(v):
    return v is None or (isinstance(v, float) and v != v) or v is pd.NA


def key_tuples(df, exprs):
    """exprs: [(column, None) | (column, (start, length))] -- Spark's 1-based substr on code points.  One key per
    row: a tuple of the terms' values, or None when any of them is NULL."""
    cols = []
    for col, sub in exprs:
        vals = df[col].tolist()
        if sub is not None:
            a, n = sub
            # Python slicing is Spark's substr only there (tests/substr_common.py has the whole function; position 0
            # and negative arguments are pinned by tests/test_substr_host.py and tests/test_gpu_substr.py)
            assert a >= 1 and n >= 0
            vals = [v if _null(v) else str(v)[a - 1:a - 1 + n] for v in vals]
        cols.append(vals)
    out = []
    for row in zip(*cols):
        out.append(None if any(_null(v) for v in row) else tuple(row))
    return out


def group_sizes(keys):
    return Counter(k for k in keys if k is not None)


def bit_length(c):
    return int(c).bit_length()


def figures(keys_l, keys_r=None):
    """keys_l / keys_r: key_tuples of the join's l- and r-side; keys_r None: a symmetric self-join (n(n-1)/2
    candidates per block).  Returns rows_l, rows_r, blocks, candidates, largest_candidates, hist [BINS][2] and
    `per_block`: {key: (rows_l, rows_r, candidates)} over the l-side keys."""
    gl = group_sizes(keys_l)
    tri = keys_r is None
    gr = gl if tri else group_sizes(keys_r)
    per_block = {}
    for k, n in gl.items():
        nr = n if tri else gr.get(k, 0)
        per_block[k] = (n, nr, n * (n - 1) // 2 if tri else n * nr)
    hist = [[0, 0] for _ in range(BINS)]
    for _, _, c in per_block.values():
        hist[bit_length(c)][0] += 1
        hist[bit_length(c)][1] += c
    cands = [c for _, _, c in per_block.values()]
    return dict(rows_l=sum(gl.values()), rows_r=sum(gr.values()), blocks=len(gl), candidates=sum(cands),
                largest_candidates=max(cands, default=0), hist=hist, per_block=per_block)


def top_k(per_block, k, by):
    """The k largest values of `by` ("candidates" or "rows_l") over the blocks, descending: what any tie order
    returns."""
    i = {"rows_l": 0, "candidates": 2}[by]
    return sorted((v[i] for v in per_block.values()), reverse=True)[:k]


def check_rule(rule, hist, largest, want, limit, by, key_of_row):
    """One rule's device figures (a RULE_PROFILE_DTYPE record, its [BINS, 2] histogram, its largest-block entries)
    against `want` = figures(...).  key_of_row(row_l) gives the l-side key tuple of a device row."""
    for f in ("rows_l", "rows_r", "blocks", "candidates", "largest_candidates"):
        assert int(rule[f]) == want[f], (f, int(rule[f]), want[f])
    assert np.asarray(hist).tolist() == want["hist"]
    assert int(np.asarray(hist)[:, 0].sum()) == want["blocks"]
    assert int(np.asarray(hist)[:, 1].sum()) == want["candidates"]
    assert len(largest) == min(limit, want["blocks"])
    metric = "rows_l" if by == "rows_l" else "candidates"
    assert [int(v) for v in largest[metric]] == top_k(want["per_block"], limit, by)
    seen = set()
    for e in largest:
        k = key_of_row(int(e["row_l"]))
        assert k is not None and k not in seen, k
        seen.add(k)
        assert (int(e["rows_l"]), int(e["rows_r"]), int(e["candidates"])) == want["per_block"][k], k
