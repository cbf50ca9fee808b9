"""Shared by the orderBy / limit tests: tools/emulate_select_top.py as a module, and the expected rows of a frame."""
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_emu = None


def emulator():
    """tools/emulate_select_top.py as a module (the key, the definition and the emulated passes)."""
    global _emu
    if _emu is None:
        spec = importlib.util.spec_from_file_location("emulate_select_top",
                                                      os.path.join(ROOT, "tools", "emulate_select_top.py"))
        _emu = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(_emu)
    return _emu


def definition_order(score, ascending):
    """The positions of `score` (given in frame order) under the definition, written without any of the package's or
    the emulation's code: a stable sort, NULL lowest, -0.0 equal to +0.0."""
    score = np.asarray(score, dtype=np.float64)
    rows = [(i, s) for i, s in enumerate(score.tolist())]

    def rank(row):  # NULL lowest: (0, 0) before every (1, value)
        i, s = row
        return (0, 0.0) if s != s else (1, s)  # Python compares -0.0 == 0.0

    if ascending:
        rows.sort(key=rank)  # list.sort is stable: ties stay in frame order
    else:
        rows.sort(key=lambda row: (-rank(row)[0], -rank(row)[1] if row[1] == row[1] else 0.0))
    return np.array([i for i, _ in rows], dtype=np.int64)


def expected_top(pdf, by, ascending, k, mask=None):
    """(expected frame, expected cut()) of `pdf[mask].orderBy(by, ascending).limit(k)`; by None: frame order; k None:
    no limit.  pdf is the parent frame in frame order."""
    inner = pdf if mask is None else pdf[np.asarray(mask, dtype=bool)]
    inner = inner.reset_index(drop=True)
    n = len(inner)
    kk = n if k is None else min(int(k), n)
    cut = {"eligible": n, "kept": kk, "score": None, "tied": 0, "tied_kept": 0}
    if by is None:
        return inner.iloc[:kk].reset_index(drop=True), cut
    score = inner[by].to_numpy(dtype=np.float64)
    order = definition_order(score, ascending)
    exp = inner.iloc[order[:kk]].reset_index(drop=True)
    if 0 < kk < n and k is not None and k < n:
        s = score[order[kk - 1]]
        same = np.isnan(score) if s != s else (score == s)
        cut["score"] = None if s != s else float(s)
        cut["tied"] = int(same.sum())
        cut["tied_kept"] = int(same[order[:kk]].sum())
    return exp, cut


def assert_frames_identical(got, exp):
    """Rows, order, columns, dtypes, and every float bit for bit (NaN equal to NaN)."""
    assert list(got.columns) == list(exp.columns)
    assert len(got) == len(exp), (len(got), len(exp))
    assert list(got.dtypes) == list(exp.dtypes), (got.dtypes, exp.dtypes)
    for c in got.columns:
        a, b = got[c].to_numpy(), exp[c].to_numpy()
        if a.dtype == np.float64:
            null = np.isnan(a)
            assert np.array_equal(null, np.isnan(b)), c
            assert np.array_equal(a[~null].view(np.uint64), b[~null].view(np.uint64)), c
        elif a.dtype == object:
            assert all((x is y) or x == y or (x != x and y != y) for x, y in zip(a.tolist(), b.tolist())), c
        else:
            assert np.array_equal(a, b), c
