"""The E+M tests' own reference and case table (tests/em_common.py), checked on the host: the exact reference against
the per-pair C oracle, and every case of tests/test_gpu_em_variants.py against the dispatch variant it is meant to
reach, so that the table cannot drift off a variant unnoticed."""
import numpy as np
import pytest

import oracle as orc
from em_common import (CASES, HL_LDS_BYTES, HL_STATIC_BYTES, UNREACHABLE, VARIANTS, em_plan, em_reference, gammas_of,
                       make_codes, n_patterns, plan_variants, reference_floats, sampled_vectors, stale_x, strides,
                       sum_bound)


@pytest.mark.parametrize("nlev,null_col", [([2], None), ([3, 3, 2], 1), ([4, 1, 5, 2], 3), ([6, 6], 0), ([1] * 7, None)])
def test_reference_matches_oracle(nlev, null_col):
    """em_reference (per pattern, exact sums) against oracle.em_stats (per pair, compensated sums) on random small
    jobs; one column with m = u = 0 at a level, so some pairs score NULL."""
    rng = np.random.Generator(np.random.PCG64(sum(nlev) * 31 + len(nlev)))
    P = 5000
    g = np.stack([rng.integers(-1, L, P) for L in nlev], axis=1).astype(np.int8)
    lam = float(rng.uniform(0.05, 0.6))
    ms, us = [], []
    for k, L in enumerate(nlev):
        a, b = rng.random(L) + 0.05, rng.random(L) + 0.05
        a, b = a / a.sum(), b / b.sum()
        if k == null_col:
            a[L - 1] = b[L - 1] = 0.0
        ms.append([orc.quantise(x) for x in a])
        us.append([orc.quantise(x) for x in b])
    want = orc.em_stats(g, nlev, lam, ms, us)
    codes = ((g.astype(np.int64) + 1) * np.array(strides(nlev))).sum(axis=1)
    hist = np.bincount(codes, minlength=n_patterns(nlev))
    ref = em_reference(hist, nlev, float(repr(lam)), float(repr(1 - lam)), sum(ms, []), sum(us, []))
    got = reference_floats(ref)
    if null_col is not None:
        assert got[2] < got[1] == P  # the NULL rows are there
    assert got[1] == want[1] and got[2] == want[2]
    assert np.allclose(got[0], want[0], rtol=1e-11, atol=0)
    assert np.array_equal(got[5::4], want[3::4]) and np.array_equal(got[6::4], want[4::4])
    assert np.allclose(got[7::4], want[5::4], rtol=1e-11, atol=1e-300)
    assert np.allclose(got[8::4], want[6::4], rtol=1e-11, atol=1e-300)
    ll = orc.log_likelihood(g, nlev, lam, ms, us)
    assert ll is not None and abs(got[3] - ll) <= 1e-11 * abs(ll)
    assert got[4] == got[2]  # d > 0 exactly where d != 0: m, u >= 0


def test_factorisations():
    """The pattern counts the case names promise."""
    want = {"n640": 640, "n642": 642, "n1280": 1280, "n1281": 1281, "n2560": 2560, "n2562": 2562,
            "n5120": 5120, "n5123": 5123, "n10240": 10240, "n10241": 10241, "R64_632": 632, "R32_635": 635,
            "R32_1264": 1264, "R16_1265": 1265, "R16_2528": 2528, "R8_2530": 2530, "R8_5056": 5056, "R4_5060": 5060,
            "R4_10112": 10112, "R0_10115": 10115, "tab_4096": 4096,
            "tab_4100": 4100, "bins_16384": 16384, "bins_16385": 16385, "u16_65536": 65536, "u32_65540": 65540,
            "tiny_3": 3}
    by_name = {c.name: c for c in CASES}
    assert len(by_name) == len(CASES)
    for name, n in want.items():
        assert by_name[name].n_pat == n, name
    assert sum(by_name["mu_96"].nlev) == 96 and sum(by_name["mu_97"].nlev) == 97
    for n_slots in (28, 29, 31, 32, 33):
        assert sum(L + 1 for L in by_name[f"slots_{n_slots}"].nlev) == n_slots
    # strides that do not divide 32 and strides above 32 both occur in the slot cases
    st = {s for c in CASES if c.name.startswith("slots_") for s in strides(c.nlev)}
    assert {3, 7, 15} <= st and any(s > 32 for s in st)
    for c in CASES:
        assert all(1 <= L <= 126 for L in c.nlev)
        if not c.name.startswith("pipe_"):
            assert c.P() <= 300_000


def test_every_case_reaches_its_variant():
    for c in CASES:
        got = plan_variants(c.plan(HL_LDS_BYTES, 256))
        assert c.want <= got, (c.name, sorted(c.want - got))
        assert c.want <= set(VARIANTS)


def test_every_variant_is_reached():
    """Every dispatch variant is hit by at least one case; the only exceptions are the unreachable ones, by name."""
    hit = set()
    for c in CASES:
        hit |= plan_variants(c.plan(HL_LDS_BYTES, 256))
    assert hit <= set(VARIANTS)
    missing = set(VARIANTS) - hit
    assert missing == set(UNREACHABLE) == {"khist_u32_lds", "score_u32_lds"}, sorted(missing)
    # each distribution runs with the uncounted hot pattern (R < 64) and without it (R = 64)
    for dist in ("dom0", "domlast", "uniform", "mislead", ("no_x", "dom_x"), "one"):
        rs = {c.plan()["R"] for c in CASES if c.dist == dist}
        assert 64 in rs and any(0 < r < 64 for r in rs), dist
    rs = {c.plan()["R"] for c in CASES if c.null_level}
    assert 64 in rs and any(0 < r < 64 for r in rs)


def test_plan_thresholds():
    """em_plan at the thresholds the library's code states, both sides."""
    for n_pat, R in [(632, 64), (633, 32), (1264, 32), (1265, 16), (2528, 16), (2529, 8), (5056, 8), (5057, 4),
                     (10112, 4), (10113, 0)]:
        assert em_plan(n_pat, 1000)["R"] == R
        # counters and the reserve for the kernel's static LDS together stay within the device's 160 KiB
        assert n_pat * R * 4 + HL_STATIC_BYTES <= HL_LDS_BYTES
    assert em_plan(632, 1000, lds_budget=64 * 1024)["R"] == 16  # a smaller device moves the plan
    assert em_plan(640, 2 ** 32 - 1)["R"] == 0                  # uint32 rows: fewer than 2^32 - 1 pairs
    assert em_plan(65536, 10)["code_bytes"] == 2 and em_plan(65537, 10)["code_bytes"] == 4
    assert em_plan(16384, 10)["hist"] == "khist_lds" and em_plan(16385, 10)["hist"] == "khist_global"
    p = em_plan(640, 1024 * 8)
    assert p["grid"] == 1 and not p["pre"] and p["stride"] == 1024
    p = em_plan(640, 1025 * 8)
    assert p["grid"] == 2 and p["pre"] and p["stride"] == 1024
    # the existing hand-made test's P leaves the pipelined loop unrun
    assert em_plan(3125, 1_000_003)["pipe_rounds"] == (0, 0)


def test_make_codes():
    by_name = {c.name: c for c in CASES}
    for name in ("R64_632", "u32_65540", "dom0_R32", "domlast_R32", "uniform_R64", "null_R32"):
        c = by_name[name]
        codes = make_codes(c, c.P())
        assert len(codes) == c.P() and codes.min() >= 0 and codes.max() < c.n_pat
        assert (codes[:c.n_pat] == np.arange(c.n_pat)).all()  # scoring reads every pattern back
        g = gammas_of(codes, c.nlev)
        assert (((g.astype(np.int64) + 1) * np.array(strides(c.nlev))).sum(axis=1) == codes).all()
    c = by_name["dom0_R32"]
    assert np.bincount(make_codes(c, c.P())).argmax() == 0
    c = by_name["domlast_R32"]
    assert np.bincount(make_codes(c, c.P())).argmax() == c.n_pat - 1
    c = by_name["mislead_R32"]  # the sample sees only A = 5; B = n_pat - 2 has the majority
    codes = make_codes(c, c.P())
    n_vec = c.P() // 8
    sv = sampled_vectors(n_vec)
    assert len(sv) == 8192 and (codes.reshape(-1)[:n_vec * 8].reshape(n_vec, 8)[sv] == 5).all()
    assert np.bincount(codes).argmax() == c.n_pat - 2
    c = by_name["stale_R32"]
    assert (make_codes(c, c.P()) != stale_x(c)).all()
    assert np.bincount(make_codes(c, c.P(), dist="dom_x")).argmax() == stale_x(c)
    c = by_name["one_R64"]
    assert len(set(make_codes(c, c.P()).tolist())) == 1
    c = by_name["pipe_7.5"]
    assert c.P() % 8 == 3 and c.plan()["pipe_rounds"] == (1, 2) and c.plan()["grid"] == 256
    assert by_name["pipe_8.5"].plan()["pipe_rounds"] == (2, 2) and by_name["pipe_3.5"].plan()["pipe_rounds"] == (0, 1)


def test_sum_bound_shape():
    assert sum_bound(1) == 27 * 2.0 ** -52 and sum_bound(32) == 27 * 2.0 ** -52 and sum_bound(33) == 28 * 2.0 ** -52
    assert sum_bound(65540) < 1e-12
