"""Jaro-Winkler values pinned to the bit in every comparison path of the device.

The ladders of tests/jw_ladder_common.py put the thresholds on the reference values themselves, so a comparison
column's level reveals the value: a device value one ulp off the oracle's changes a code.  No tolerance anywhere.
Which family reaches which kernel (jw_exact's dispatch, spk_strsim.h), and how the test knows:

  planes32  jw_planes2<uint32_t>   both rows Latin-1, longer row <= 32 units      exact_counts >= the pinned cells
  planes64  jw_planes2<uint64_t>   longer row 33..64, shorter on both sides of 32  exact_counts >= the pinned cells
  mixed     jw_planes<u32 / u64>   a unit >= 256 in the shorter row                exact_counts >= the pinned cells
            jw_small (global)      a unit >= 256 in the longer row                 (a bound cannot decide a test whose
  slow      jw_long, lane words    65..1024 units                                  threshold is the cell's own value)
  huge      jw_long, device scratch  > 1024 units                                  gammas_deferred >= the pinned cells

(The counts leave out equal strings, which the keys decide, and strings without a common unit, whose value 0.0 the
sketches prove; so gammas_deferred is compared with the cells pinned in the call, not with all long pairs.)

Mode 1 runs the filter kernel (ev_jw's fp32 bound, prepare_tests' rounded thresholds) and jw_cell for the first
four columns of a call -- the filter kernel has four Jaro-Winkler slots -- and the interpreter for the others; mode 0
runs the interpreter for all (jw_upper, jw_exact, its slow and huge passes); mode 101 leaves the slow lists to the
settlement.  gammas_simple_count tells which of them ran."""
import copy
import warnings

import numpy as np
import pandas as pd
import pytest

import jw_ladder_common as J
import oracle as orc

pytestmark = pytest.mark.gpu
warnings.filterwarnings("ignore")


@pytest.fixture(scope="module")
def amd():
    from splink_amd import AmdSession, _native
    if _native.device_count() == 0:
        pytest.fail("no HIP device visible: the -m gpu tests need an MI355X")
    return AmdSession(0)


def _completed(call, amd):
    from splink_amd.settings import complete_settings_dict
    return complete_settings_dict(copy.deepcopy(call["settings"]), amd)


def _job(pairs, call, amd):
    """One Job over the pairs as a comparison table (pair i = row i of both sides); later calls reuse it."""
    from splink_amd.gammas import add_gammas
    df = pd.DataFrame({"a_l": pd.Series([a for a, b in pairs], dtype=object),
                       "a_r": pd.Series([b for a, b in pairs], dtype=object)})
    return add_gammas(df, call["settings"], amd).job


def _mismatch(pairs, refs, call, got, want):
    rows = []
    for i, k in zip(*np.nonzero(got != want)):
        a, b = pairs[i]
        rows.append((int(i), int(k), J.kernel_of(a, b), None if a is None else J.ulen(a),
                     None if b is None else J.ulen(b),
                     None if refs[i] is None else refs[i].hex(), call["rungs"][k], int(got[i, k]), int(want[i, k]),
                     None if a is None else a[:70], None if b is None else b[:70]))
        if len(rows) == 6:
            break
    return int((got != want).sum()), rows


def _run_calls(job, pairs, refs, calls, settings, want, positive_pins, mode, all_long):
    """Every call in one mode: the whole code matrix, then the diagnostics that tell which path ran."""
    ctx = job.ctx
    ctx.gammas_set_simple(mode)
    for c, (call, st, w) in enumerate(zip(calls, settings, want)):
        job.gammas(st)
        got = job.gammas_host()
        n_cols = len(call["rungs"])
        simple, exact, deferred = ctx.gammas_simple_count(), ctx.gammas_exact_counts(n_cols), ctx.gammas_deferred()
        print(f"mode {mode} {call['form']} call {c}: {n_cols} columns, {ctx.n_patterns()} patterns, simple {simple}, "
              f"exact {exact}, pinned {positive_pins[c]}, deferred {deferred}")
        assert got.shape == w.shape
        assert (got == w).all(), (mode, call["form"], c) + _mismatch(pairs, refs, call, got, w)
        assert ctx.n_patterns() == 8 ** n_cols  # <= 65536: uint16 codes (the narrow layout), else uint32
        if call["form"] == J.MIXED_EQ or mode % 10 == 0:
            assert simple == 0  # `=` next to Jaro-Winkler tests has no filter class: the interpreter
        else:
            assert simple == min(n_cols, J.FILTER_JW_SLOTS)
        for k in range(n_cols):
            assert exact[k] >= positive_pins[c][k], (mode, c, k, exact, positive_pins[c])
        # every pair of the slow and huge families has a side past the exact pass's 64 units: its cell in its pinning
        # column is on a slow list; no cell of the other families is
        assert deferred >= sum(positive_pins[c]) if all_long else deferred == 0


def _positive_pins(pairs, refs, calls):
    """Per call and column, the unequal pairs pinned there whose value is not 0.0: no bound can decide the test at a
    cell's own value, so each is an exact-pass cell.  (Equal strings are decided by their keys, and strings without
    a common unit by the sketches, which prove the value 0.0 itself.)"""
    out = [[0] * len(call["rungs"]) for call in calls]
    for (a, b), v, pin in zip(pairs, refs, J.pinned(refs, calls)):
        if v is None or a == b or v == 0.0:
            continue
        for c, k, level in pin:
            out[c][k] += 1
    return out


@pytest.mark.parametrize("name", J.FAMILIES)
def test_jw_values_pinned(name, amd):
    """Every ladder call of the family, in the narrow (uint16 codes) and the wide (uint32 codes) layout: the whole
    code matrix equals the expected levels -- every pair against every rung of its call, not only its own -- in
    mode 1 (filter + exact), mode 0 (interpreter) and mode 101 (slow lists settled late), and with an equality test
    mixed into the columns in mode 1."""
    pairs, refs = J.family(name)
    long_pair = [max(J.ulen(a), J.ulen(b)) > 64 for a, b in pairs if a is not None and b is not None]
    assert all(long_pair) if name in ("slow", "huge") else not any(long_pair)
    plans = []
    for form in (J.LADDER, J.MIXED_EQ):
        calls = J.family_calls(name, form)
        plans.append((calls, [_completed(c, amd) for c in calls], [J.expected_levels(pairs, refs, c) for c in calls],
                      _positive_pins(pairs, refs, calls)))
    job = _job(pairs, plans[0][0][0], amd)
    try:
        for mode in (1, 0, 101):
            _run_calls(job, pairs, refs, *plans[0], mode, all(long_pair))
        _run_calls(job, pairs, refs, *plans[1], 1, all(long_pair))
    finally:
        job.ctx.gammas_set_simple(1)


def _view_rows():
    """Rows for the views: a_l of 43..64 units (and a few shorter than the cut), a_r on both sides of the view's 40
    units -- longer (41..64: the view is the shorter side, read through UnitReader next to a_r's planes) and shorter
    (the view is the longer side: jw_small over global memory)."""
    rng = np.random.Generator(np.random.PCG64(4001))
    alpha = J.ALPHA_LATIN1
    base = J.draw(rng, alpha, 64)
    rows = []
    for n in (43, 44, 50, 57, 63, 64):
        a = J.mutate(rng, base[:n], 2, alpha, 64)
        for p in (1, 2, 3, 4):
            view = a[p - 1:p - 1 + 40]
            rows.append((a, J.mutate(rng, view + base[40:40 + 4 + p], 2, alpha, 64)))  # longer than the view
            rows.append((a, J.mutate(rng, view[:20 + 4 * p], 2, alpha, 39)))            # shorter than the view
    rows += [
        ("ab" + J.SURROGATE + base[:50], base[:45]),      # a surrogate pair before the cut: code-point substr
        ("ab" + J.SURROGATE + base[:50], "ab" + base[:30]),
        (base[:39] + "š" + base[40:50], base[:50]),        # a unit >= 256 inside the view
        ("ab", "ab"), ("abc", "c"), ("abcd", "bcd"), ("", "abc"),  # rows shorter than the view's start
        (base, base[:40]), (base, base[1:41]), (base, base[3:43]),  # a view equal to a_r
        (None, "abc"), (base, None),
    ]
    return base, rows


def _view_kernel(x, y, x_row, y_row):
    """kernel_of for operands of which only a whole table row (x_row / y_row) can carry planes: a substr view or a
    literal never does (apply_substr, lit_view)."""
    k = J.kernel_of(x, y)
    if k in ("null", "equal", "slow", "huge"):
        return k
    x_longer = J.ulen(x) > J.ulen(y)
    mx, mn = (x, y) if x_longer else (y, x)
    mx_row, mn_row = (x_row, y_row) if x_longer else (y_row, x_row)
    word = "u32" if J.ulen(mx) <= 32 else "u64"
    if not (mx_row and J.has_planes(mx)):
        return "small_global"
    return f"planes2_{word}" if mn_row and J.has_planes(mn) else f"planes_{word}"


def test_jw_values_on_views(amd):
    """jaro_winkler_sim over substr views and literals (interpreter columns): substr(a_l, p, 40) for the four
    alignment phases p = 1..4 of a view that starts inside an aligned 8-byte word, in either argument position and
    on the shorter and on the longer side; literals of 3, 33 and 70 units (planes + UnitReader over the unpadded
    literal buffer; the slow pass).  Reference: the oracle over Python slices, which count code points as Spark's
    substr does.  Pinned with the same ladders."""
    base, rows = _view_rows()
    lits = [base[20:23], base[5:30] + "xy" + base[30:36], base + "-" + base[:5]]
    assert [J.ulen(s) for s in lits] == [3, 33, 70]
    specs = []
    for p in (1, 2, 3, 4):
        specs.append((f"jaro_winkler_sim(substr(a_l, {p}, 40), a_r)", lambda a, b, p=p: (a[p - 1:p - 1 + 40], b),
                      False, True))
        specs.append((f"jaro_winkler_sim(a_r, substr(a_l, {p}, 40))", lambda a, b, p=p: (b, a[p - 1:p - 1 + 40]),
                      True, False))
    for lit in lits:
        specs.append((f"jaro_winkler_sim(a_l, '{lit}')", lambda a, b, lit=lit: (a, lit), True, False))
    kernels = set()
    plans = []
    for jw, view, x_row, y_row in specs:
        viewed = [(None, None) if a is None or b is None else view(a, b) for a, b in rows]
        refs = [orc.jaro_winkler(x, y) for x, y in viewed]
        kernels |= {_view_kernel(x, y, x_row, y_row) for x, y in viewed}
        for call in J.ladder_calls(refs, J.WIDE_COLS, jw=jw):
            plans.append((call, _completed(call, amd), J.expected_levels(viewed, refs, call), viewed, refs))
    assert {"planes_u32", "planes_u64", "small_global", "slow"} <= kernels, kernels
    job = _job(rows, plans[0][0], amd)
    try:
        for mode in (1, 0):
            job.ctx.gammas_set_simple(mode)
            for call, st, want, viewed, refs in plans:
                job.gammas(st)
                got = job.gammas_host()
                assert (got == want).all(), (mode, st["comparison_columns"][0]["case_expression"][:90]) + \
                    _mismatch(viewed, refs, call, got, want)
                assert job.ctx.gammas_simple_count() == 0  # a view or a literal operand: the interpreter's columns
    finally:
        job.ctx.gammas_set_simple(1)


def test_jw_udf_matches_on_ladder_pairs(amd):
    """The bulk UDF (LDS-staged jw_small, jw_long) over the same pairs: bit-equal to the oracle."""
    from splink_amd import _native as N
    left, right, want = [], [], []
    for name in J.FAMILIES:
        pairs, refs = J.family(name)
        for (a, b), v in zip(pairs, refs):
            if v is not None:
                left.append(a)
                right.append(b)
                want.append(v)
    got = N.Context(0).jaro_winkler_sim(left, right)
    bad = [(a[:70], b[:70], float(g).hex(), w.hex()) for a, b, g, w in zip(left, right, got, want) if g != w]
    assert not bad, (len(bad), bad[:5])
