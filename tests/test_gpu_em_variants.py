"""Every dispatch variant of the E+M launch (splink_amd/csrc/spk_em.hip) on hand-made comparison vectors, against
the exact reference of tests/em_common.py.

Which kernel, template arguments and branches run is decided by the pattern space, the code width, the pair count,
the grid, Σ L_k and the slot count; tests/em_common.py restates that plan (`em_plan`) and holds one case per
variant (`CASES`; tests/test_em_reference_host.py proves the table covers every reachable variant).  Each case here
first asserts that the library's own lane plan (spk_em_lane_copies) is the restated one, so a change of LDS budget
or device moves no case off its variant silently, then checks, on one context:

  pattern counts     spk_em_histogram in modes 1, 0, 2 == np.bincount, into a sentinel-filled buffer
  one launch         spk_em_iteration in modes 1 and 2: bit-identical; row counts equal to the reference's, every
                     sum within sum_bound of the EXACT sum (mode 0, histogram + finalize launches, likewise)
  multi-GPU form     spk_em_histogram + spk_em_finalize: the same bounds
  async form         spk_em_iteration_start / _wait: bit-identical to the blocking call
  repeat             a second spk_em_iteration: bit-identical (ticket and rows were reset)
  scoring            spk_score over odd / even ranges: mp per pair bit-equal to the float64 restatement (NaN = NaN)

Each case prints `EMCASE name P=… seconds=… max_err/bound=…` before it asserts."""
import time

import numpy as np
import pytest

from em_common import (CASES, ENUM_P, em_plan, em_reference, entry_terms, gammas_of, is_count_entry, make_codes,
                       pattern_tables, plan_variants, rel_err, stale_x, sum_bound)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def device():
    """(LDS bytes per workgroup, compute units) of cuda:0, as the library sees them."""
    import torch
    from splink_amd import _native as N
    ctx = N.Context(0)
    lds = ctx.lds_per_block()
    ctx.close()
    return lds, int(torch.cuda.get_device_properties(0).multi_processor_count)


def _same_bits(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def _check_stats(got, ref, terms, what):
    """Counts equal, sums within sum_bound of the exact value; returns the largest error as a share of its bound."""
    assert len(got) == len(ref)
    worst = 0.0
    bad = []
    for i, (x, r, n) in enumerate(zip(got, ref, terms)):
        if is_count_entry(i):
            if float(x) != float(r):
                bad.append((what, i, float(x), int(r)))
            continue
        e, b = rel_err(x, r), sum_bound(n)
        worst = max(worst, e / b)
        if not e <= b:
            bad.append((what, i, float(x), float(r), e, b))
    return worst, bad


def _histogram(ctx, n_pat):
    import torch
    d = torch.full((n_pat,), -1, dtype=torch.int64, device="cuda:0")  # sentinel: every bin must be written
    torch.cuda.synchronize()  # torch's fill runs on its own stream
    ctx.em_histogram(d.data_ptr())
    return d, d.cpu().numpy()


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_em_variant(case, device):
    from splink_amd import _native as N
    t0 = time.perf_counter()
    lds, n_cu = device
    nlev, n_pat = case.nlev, case.n_pat
    P = case.P(n_cu)
    plan = em_plan(n_pat, P, lds, n_cu, nlev)
    variants = plan_variants(plan)
    assert case.want <= variants, f"this device moves the case off its variant: {sorted(case.want - variants)}"
    lam, one_minus, m, u = case.tables()
    n_stats = 5 + 4 * sum(L + 1 for L in nlev)
    ctx = N.Context(0)
    if not isinstance(case.dist, str):
        # a stale uncounted pattern: the first launch on codes dominated by X makes X the hot pattern; codes
        # without any X, same P and space, are then counted with X still uncounted (its bin = P - rest = 0)
        ctx.gammas_load(nlev, gammas_of(make_codes(case, P, dist=case.dist[1]), nlev))
        ctx.em_iteration(lam, one_minus, m, u, n_stats)
    codes = make_codes(case, P)
    g = gammas_of(codes, nlev)
    ctx.gammas_load(nlev, g)
    assert ctx.n_patterns() == n_pat
    assert ctx.em_lane_copies() == plan["R"]
    want_hist = np.bincount(codes, minlength=n_pat)
    ref = em_reference(want_hist, nlev, lam, one_minus, m, u)
    terms = entry_terms(nlev)
    assert ref[1] == P
    if case.null_level:  # the pairs at the zeroed level, and only they, score NULL
        assert ref[1] - ref[2] == int((g[:, -1] == min(1, nlev[-1] - 1)).sum()) > 0
    if not isinstance(case.dist, str):
        assert want_hist[stale_x(case)] == 0
    t_host = time.perf_counter() - t0

    # pattern counts
    hists = {}
    for mode in (1, 0, 2):
        ctx.em_set_lane_histogram(mode)
        assert ctx.em_lane_copies() == (plan["R"] if mode else 0)
        hists[mode] = _histogram(ctx, n_pat)[1]
    # the one-launch iteration with and without the fence, and the histogram + finalize launches (mode 0)
    stats = {}
    for mode in (1, 2, 0):
        ctx.em_set_lane_histogram(mode)
        stats[mode] = ctx.em_iteration(lam, one_minus, m, u, n_stats).copy()
    ctx.em_set_lane_histogram(1)
    again = ctx.em_iteration(lam, one_minus, m, u, n_stats).copy()
    ctx.em_iteration_start(lam, one_minus, m, u, n_stats)
    waited = ctx.em_iteration_wait(n_stats).copy()
    d_hist, _ = _histogram(ctx, n_pat)
    two_step = ctx.em_finalize(d_hist.data_ptr(), lam, one_minus, m, u, n_stats).copy()
    # scoring
    mp_pat = pattern_tables(nlev, lam, one_minus, m, u)[0]
    want_mp = mp_pat[codes]
    n = min(P, ENUM_P)
    ranges = [(0, n), (0, 1), (1, 0), (1, 1), (1, 2), (1, 7), (2, 6), (3, n - 3), (n - 1, 1), (n - 2, 2),
              (P - 1, 1), (P - 3, 3)]
    scored = [(s, c, ctx.score(lam, one_minus, m, u, s, c)) for s, c in ranges if s >= 0 and c >= 0 and s + c <= P]
    ctx.close()

    checks = [_check_stats(stats[1], ref, terms, "iteration"), _check_stats(stats[0], ref, terms, "mode 0"),
              _check_stats(two_step, ref, terms, "histogram + finalize")]
    worst = max(w for w, _ in checks)
    mp_equal = all(bool(((got.view(np.uint64) == want_mp[s:s + c].view(np.uint64)) |
                         (np.isnan(got) & np.isnan(want_mp[s:s + c]))).all()) for s, c, got in scored)
    print(f"EMCASE {case.name} n_pat={n_pat} P={P} R={plan['R']} variants={','.join(sorted(variants))} "
          f"seconds={time.perf_counter() - t0:.2f} host_reference_seconds={t_host:.2f} "
          f"max_err_over_bound={worst:.4f} mp_bit_equal={mp_equal}", flush=True)

    for mode in (1, 0, 2):
        assert np.array_equal(hists[mode], want_hist), f"histogram mode {mode}"
    for _, bad in checks:
        assert not bad, bad[:5]
    assert _same_bits(stats[1], stats[2]), "fenced and unfenced launches differ"
    assert _same_bits(again, stats[1]), "a repeated launch differs: ticket or rows not reset"
    assert _same_bits(waited, stats[1]), "start / wait differs from the blocking call"
    if n_pat <= ENUM_P <= P and isinstance(case.dist, str) and case.dist not in ("mislead", "one"):
        assert (codes[:n_pat] == np.arange(n_pat)).all()  # the scored ranges cover every pattern
    assert mp_equal, "match_probability differs from the float64 restatement"


def test_pattern_space_limit():
    """2^31 patterns do not fit the device's int pattern index: refused at load; 2^30 loads.  Loading only: no EM
    runs on a 2^30-pattern space."""
    from splink_amd import _native as N
    ctx = N.Context(0)
    with pytest.raises(ValueError, match="2\\^31"):
        ctx.gammas_load([1] * 31, np.zeros((1, 31), dtype=np.int8))
    ctx.close()
    ctx = N.Context(0)
    ctx.gammas_load([1] * 30, np.zeros((1, 30), dtype=np.int8))
    assert ctx.n_patterns() == 2 ** 30
    ctx.close()
