"""Host-side reference, launch plan and case table of the E+M launch (splink_amd/csrc/spk_em.hip), shared by
tests/test_em_reference_host.py (CPU) and tests/test_gpu_em_variants.py (GPU).

Three things live here:

* `em_reference`: one E+M pass over a pattern histogram.  Per pattern num, den, d, mp and 1 - mp are float64 in
  `pattern_mp`'s literal left-associative order (the library is built with -ffp-contract=off -fno-fast-math, so these
  are meant to be the device's bits); ln(d) is taken with mpmath from the double d; every total is the EXACT sum of
  count x value over those doubles.
* `sum_bound`: how far a device sum may be from that exact sum, derived from the shape of the device's summation.
* `em_plan` and `CASES`: which kernel, template arguments and branches a (pattern space, pair count) takes, restated
  from lane_plan / lane_grid / launch_em_lanes / enqueue_histogram / em_finalize_block / spk_score, and the table of
  hand-made cases with the variant each is meant to reach.
"""
from __future__ import annotations

import math
from fractions import Fraction

import mpmath
import numpy as np

# ---- constants mirrored from spk_em.hip (only the tests' choice of cases depends on them) -----------------------
HL_THREADS = 1024          # k_em_iter workgroup
HL_LDS_BYTES = 160 * 1024  # its LDS budget (capped by the device attribute) ...
HL_STATIC_BYTES = 2048     # ... of which this much is kept for the kernel's static LDS, the rest holds counters
HL_UNROLL = 4              # vectors in flight per lane in the pipelined loop
EF_THREADS = 1024          # k_em_finalize workgroup (em_finalize_block runs with 16 waves in both kernels)
EF_LDS_PAT = 4096
SC_LDS_PAT = 4096
H_LDS_BINS = 16384
PA_INLINE_MU = 96
HS_SAMPLES = 8192          # vectors k_em_hot_sample reads
# sizeof(PatArgs): K, n_pat, n_slots, tot (4 x int32); lambda, one_minus (2 x double); mu_dev (pointer);
# stride[64] int32; moff[64] int16; nlev[64] uint8; mu[2 * 96] double
PATARGS_BYTES = 16 + 16 + 8 + 64 * 4 + 64 * 2 + 64 + 2 * PA_INLINE_MU * 8
N_HEAD = 5

mpmath.mp.prec = 240  # > 70 digits for ln(d) and the sums over it


# ---- the pattern space ----------------------------------------------------------------------------------------
def n_patterns(nlev):
    return int(np.prod([int(L) + 1 for L in nlev], dtype=object))


def strides(nlev):
    out, s = [], 1
    for L in nlev:
        out.append(s)
        s *= int(L) + 1
    return out


def digits(nlev):
    """int64 [n_pat, K]: gamma level (-1 .. L_k - 1) of every pattern index in every column."""
    idx = np.arange(n_patterns(nlev), dtype=np.int64)
    cols = []
    for L in nlev:
        cols.append(idx % (L + 1) - 1)
        idx = idx // (L + 1)
    return np.stack(cols, axis=1)


def gammas_of(codes, nlev):
    """int8 [P, K]: the comparison vectors whose packed codes are `codes`."""
    codes = np.asarray(codes, dtype=np.int64)
    g = np.empty((len(codes), len(nlev)), dtype=np.int8)
    for k, (L, s) in enumerate(zip(nlev, strides(nlev))):
        g[:, k] = ((codes // s) % (L + 1) - 1).astype(np.int8)
    return g


# ---- the reference -----------------------------------------------------------------------------------------
def pattern_tables(nlev, lam, one_minus, m, u):
    """(mp, 1 - mp, d) per pattern in float64, in pattern_mp's order: num = ((λ·f_1)·f_2)·…, den likewise from
    1 - λ and u, a NULL level (γ = -1) contributing 1.0; d = num + den; mp = NaN where d == 0."""
    m = np.asarray(m, dtype=np.float64)
    u = np.asarray(u, dtype=np.float64)
    dg = digits(nlev)
    n_pat = dg.shape[0]
    num = np.full(n_pat, np.float64(lam))
    den = np.full(n_pat, np.float64(one_minus))
    off = 0
    for k, L in enumerate(nlev):
        g = dg[:, k]
        idx = off + np.maximum(g, 0)
        num = num * np.where(g < 0, 1.0, m[idx])
        den = den * np.where(g < 0, 1.0, u[idx])
        off += L
    d = num + den
    with np.errstate(invalid="ignore", divide="ignore"):
        mp = np.where(d == 0.0, np.nan, num / d)
    return mp, 1.0 - mp, d


def _exact_dot(counts, values, sel):
    """Σ counts[p] · values[p] over p in sel, exactly (values are doubles: n / 2^e)."""
    num, den_log = 0, 0  # running sum num / 2^den_log
    for p in sel:
        n, dd = float(values[p]).as_integer_ratio()
        e = dd.bit_length() - 1
        if e > den_log:
            num <<= e - den_log
            den_log = e
        num += int(counts[p]) * (n << (den_log - e))
    return Fraction(num, 1 << den_log)


def em_reference(hist, nlev, lam, one_minus, m, u):
    """One E+M pass in the library's layout: a list of N_HEAD + 4 · Σ(L_k + 1) exact values,
    [Σmp, rows, non-null rows, Σ ln d, non-null ln rows] then per column k, per level v = -1 .. L_k - 1
    [rows, non-null rows, Σmp, Σ(1 - mp)].  Row counts are ints, the mp sums Fractions, Σ ln d an mpmath number.
    NaN handling as em_finalize_block: a NaN mp drops the pattern from the non-null rows and both mp sums, a NaN
    ln (d <= 0) from the two ln entries; a pattern without pairs contributes nothing."""
    hist = np.asarray(hist).astype(np.int64)
    n_pat = n_patterns(nlev)
    assert hist.shape == (n_pat,)
    mp, omp, d = pattern_tables(nlev, lam, one_minus, m, u)
    dg = digits(nlev)
    live = hist > 0
    ok = live & ~np.isnan(mp)
    # the bound below is relative: it does not hold where a product c · value falls into the subnormals
    for tab in (mp, omp):
        t = np.abs(tab[ok])
        assert not ((t > 0) & (t < 2.0 ** -1000)).any(), "case reaches subnormal terms: sum_bound does not apply"
    out = [None] * N_HEAD
    ok_idx = np.nonzero(ok)[0]
    out[0] = _exact_dot(hist, mp, ok_idx)
    out[1] = int(hist.sum())
    out[2] = int(hist[ok].sum())
    ll_ok = live & (d > 0.0)
    ll_sum = mpmath.mpf(0)
    cache = {}
    for p in np.nonzero(ll_ok)[0]:
        dv = float(d[p])
        if dv not in cache:
            cache[dv] = mpmath.log(mpmath.mpf(dv))
        ll_sum += int(hist[p]) * cache[dv]
    out[3] = ll_sum
    out[4] = int(hist[ll_ok].sum())
    for k, L in enumerate(nlev):
        for v in range(-1, L):
            in_slot = dg[:, k] == v
            sel = np.nonzero(in_slot & ok)[0]
            out += [int(hist[in_slot].sum()), int(hist[in_slot & ok].sum()), _exact_dot(hist, mp, sel),
                    _exact_dot(hist, omp, sel)]
    return out


COUNT_ENTRIES = (1, 2, 4)  # integer entries of the head; per slot entries 0 and 1


def is_count_entry(i):
    return i in COUNT_ENTRIES if i < N_HEAD else (i - N_HEAD) % 4 < 2


def reference_floats(ref):
    """The reference rounded to float64 (for comparisons against another float64 implementation)."""
    return np.array([float(x) for x in ref], dtype=np.float64)


def entry_terms(nlev):
    """Patterns the device walks for each entry: n_pat for the head, n_pat / (L_k + 1) for a slot of column k."""
    n_pat = n_patterns(nlev)
    out = [n_pat] * N_HEAD
    for L in nlev:
        out += [n_pat // (L + 1)] * (4 * (L + 1))
    return out


def rel_err(got, exact):
    """|got - exact| / |exact| as a float (0 when both are zero, inf when only the exact value is)."""
    got = float(got)
    if isinstance(exact, Fraction):
        if exact == 0:
            return 0.0 if got == 0.0 else math.inf
        if math.isnan(got) or math.isinf(got):
            return math.inf
        return float(abs(Fraction(got) - exact) / abs(exact))
    if exact == 0:
        return 0.0 if got == 0.0 else math.inf
    if math.isnan(got) or math.isinf(got):
        return math.inf
    return float(abs(mpmath.mpf(got) - exact) / abs(exact))


def sum_bound(n_terms):
    """Relative tolerance of a device sum over n_terms patterns (terms all >= 0, or all <= 0) against the exact sum.

    Derived from em_finalize_block's summation, with u = 2^-53 the unit roundoff and S = Σ|term| = |exact sum|
    (one sign, so no cancellation); a floating-point sum of j numbers in any fixed order is off by at most
    (j - 1) u S to first order.

    * Terms.  The reference sums the exact products count · value of the same doubles the device holds (count is
      exact in a double, mp and 1 - mp are bit-equal by construction).  The device rounds each product once: u.
      For Σ ln d the device's log is not correctly rounded; OpenCL's conformance limit for double log is 3 ulp,
      i.e. 6 u, so a term carries at most 7 u.
    * Per lane.  A statistics slot is walked by a half-wave, 32 lanes striding the slot's patterns: at most
      n = ceil(n_terms / 32) terms per lane, added one at a time: (n - 1) u.  (The split totals stride 128 or more
      lanes, fewer terms each.)
    * Tree.  Half-wave slots: four DPP steps and one add of two lane reads, 5 levels; the split totals: four DPP
      steps and two levels of lane reads, 6 levels: 6 u.
    * Wave partials.  The split totals add the partials of at most 15 spare waves in wave order: 14 roundings
      (the first lands on 0.0): 14 u.

    First order: (n - 1 + 6 + 14 + 7) u = (n + 26) u.  Doubling it covers the second-order terms (all of relative
    size (n + 26) u below the first-order ones) with room to spare: 2 (n + 26) u = (n + 26) · 2^-52.  (A looser
    (n + 40) · 2^-52 was first proposed for the same shape; the constant here is the derived one.)
    The bound assumes no term is subnormal, which em_reference asserts."""
    return (-(-int(n_terms) // 32) + 26) * 2.0 ** -52


# ---- the launch plan -------------------------------------------------------------------------------------------
def em_plan(n_pat, P, lds_budget=HL_LDS_BYTES, n_cu=256, nlev=None):
    """What the library runs for n_pat patterns and P pairs on a device with lds_budget bytes of LDS per workgroup
    and n_cu compute units (default histogram mode).  With nlev also the slot walk and the m / u transport."""
    plan = {"n_pat": n_pat, "P": P}
    code_bytes = 2 if n_pat <= 65536 else 4
    vec = 16 // code_bytes
    n_vec = P // vec
    plan.update(code_bytes=code_bytes, vec=vec, n_vec=n_vec)
    # lane_plan
    budget = min(HL_LDS_BYTES, lds_budget) - HL_STATIC_BYTES
    R = 64
    while R >= 4 and n_pat * R * 4 > budget:
        R >>= 1
    if R < 4 or P >= 2 ** 32 - 1:
        R = 0
    plan["R"] = R
    if R:
        lds_bytes = max(n_pat * R * 4, PATARGS_BYTES)
        grid = max(1, min(n_cu, -(-n_vec // HL_THREADS)))  # lane_grid
        pre = grid > 1
        stride = (grid - (1 if pre else 0)) * HL_THREADS
        room = ((PATARGS_BYTES + 7) // 8 + 3 * n_pat) * 8 <= lds_bytes
        # pipelined rounds of the lane that starts at vector v0: while v + 3 stride < n_vec, v += 4 stride

        def rounds(v0):
            r, v = 0, v0
            while v + (HL_UNROLL - 1) * stride < n_vec:
                r += 1
                v += HL_UNROLL * stride
            return r
        plan.update(grid=grid, pre=pre, stride=stride, room=room, hist="lanes",
                    pipe_rounds=(rounds(stride - 1), rounds(0)),  # fewest and most over the lanes
                    iter_table="lds" if room and n_pat <= EF_LDS_PAT else "global")
    else:
        plan.update(grid=None, pre=None, stride=None, room=None, pipe_rounds=None, iter_table=None,
                    hist="khist_lds" if n_pat <= H_LDS_BINS else "khist_global")
    plan["finalize_table"] = "lds" if n_pat <= EF_LDS_PAT else "global"  # k_em_finalize
    plan["score_table"] = "lds" if n_pat <= SC_LDS_PAT else "global"
    if nlev is not None:
        assert n_patterns(nlev) == n_pat
        n_slots = sum(L + 1 for L in nlev)
        n_waves = EF_THREADS // 64
        col_waves = (n_slots + 1) // 2
        split = n_waves - col_waves >= 2
        plan.update(n_slots=n_slots, split=split, tot=sum(nlev),
                    slot_rounds=1 if split else -(-(n_slots + 1) // (2 * n_waves)),
                    mu="inline" if sum(nlev) <= PA_INLINE_MU else "upload")
    return plan


# Every dispatch variant, by label.  UNREACHABLE: combinations no input can produce, with the reason.
VARIANTS = [
    "lanes_R64", "lanes_R32", "lanes_R16", "lanes_R8", "lanes_R4",
    "khist_u16_lds", "khist_u16_global", "khist_u32_global", "khist_u32_lds",
    "iter_room_lds", "iter_room_global", "iter_noroom",  # the finalize inside k_em_iter: its pattern table
    "finalize_lds", "finalize_global",                   # k_em_finalize's
    "grid_1", "grid_2", "grid_many",
    "P_0", "n_vec_0", "remainder_only", "pipe_some_lanes", "pipe_all_lanes", "pipe_two_rounds",
    "totals_split", "slots_one_round", "slots_two_rounds", "slots_more_rounds",
    "mu_inline", "mu_upload",
    "score_u16_lds", "score_u16_global", "score_u32_global", "score_u32_lds",
]
UNREACHABLE = {
    "khist_u32_lds": "uint32 codes mean more than 65 536 patterns; the LDS histogram stops at 16 384",
    "score_u32_lds": "uint32 codes mean more than 65 536 patterns; the LDS score table stops at 4096",
}


def plan_variants(plan):
    """The labels of VARIANTS a plan (made with nlev) reaches."""
    v = set()
    cw = "u16" if plan["code_bytes"] == 2 else "u32"
    if plan["R"]:
        v.add(f"lanes_R{plan['R']}")
        v.add("iter_noroom" if not plan["room"] else f"iter_room_{plan['iter_table']}")
        v.add("grid_1" if plan["grid"] == 1 else "grid_2" if plan["grid"] == 2 else "grid_many")
        lo, hi = plan["pipe_rounds"]
        if plan["n_vec"] > 0:
            if hi == 0:
                v.add("remainder_only")
            elif lo == 0:
                v.add("pipe_some_lanes")
            else:
                v.add("pipe_all_lanes")
            if hi >= 2:
                v.add("pipe_two_rounds")
    else:
        v.add(f"khist_{cw}_{'lds' if plan['hist'] == 'khist_lds' else 'global'}")
    if plan["P"] == 0:
        v.add("P_0")
    if plan["n_vec"] == 0:
        v.add("n_vec_0")
    v.add(f"finalize_{plan['finalize_table']}")
    v.add(f"score_{cw}_{plan['score_table']}")
    if plan["split"]:
        v.add("totals_split")
    else:
        v.add({1: "slots_one_round", 2: "slots_two_rounds"}.get(plan["slot_rounds"], "slots_more_rounds"))
    v.add(f"mu_{plan['mu']}")
    return v


# ---- the cases -------------------------------------------------------------------------------------------------
ENUM_P = 100_003  # every pattern once, then filler: odd, past the last 16-byte vector, a grid of 13 / 25 workgroups


class Case:
    """nlev, a rule for P, a distribution and the variants the case is meant to reach.

    P rules: an int; ("vec", a, b) = a · VEC + b codes; ("pipe", tenths, rem) = (tenths / 10 · stride + rem)
    vectors plus 3 codes, stride = (n_cu - 1) · 1024, sized from the device's compute units.
    Distributions: see `make_codes`."""

    def __init__(self, name, nlev, P, dist, want, null_level=False):
        self.name, self.nlev, self.P_rule, self.dist, self.want = name, list(nlev), P, dist, set(want)
        self.null_level = null_level
        self.n_pat = n_patterns(nlev)

    def P(self, n_cu=256):
        vec = 8 if self.n_pat <= 65536 else 4
        r = self.P_rule
        if isinstance(r, int):
            return r
        if r[0] == "vec":
            return r[1] * vec + r[2]
        if r[0] == "pipe":
            stride = (n_cu - 1) * HL_THREADS
            return (r[1] * stride // 10 + r[2]) * vec + 3
        raise ValueError(r)

    def plan(self, lds_budget=HL_LDS_BYTES, n_cu=256):
        return em_plan(self.n_pat, self.P(n_cu), lds_budget, n_cu, self.nlev)

    def tables(self):
        """λ, 1 - λ and flat m / u: per column m rises and u falls over the levels, as the EM's own tables do;
        null_level sets m = u = 0 at level 1 of the last column (its pairs score NULL)."""
        lam, m, u = 0.3, [], []
        for L in self.nlev:
            pm = np.linspace(1.0, 2.0, L)
            m += list(pm / pm.sum())
            u += list(pm[::-1] / pm.sum())
        if self.null_level:
            at = sum(self.nlev[:-1]) + min(1, self.nlev[-1] - 1)
            m[at] = u[at] = 0.0
        return lam, 1.0 - lam, np.array(m), np.array(u)

    def __repr__(self):
        return self.name


def sampled_vectors(n_vec):
    """Indices of the 16-byte vectors k_em_hot_sample reads."""
    S = min(n_vec, HS_SAMPLES)
    return np.arange(S, dtype=np.int64) * n_vec // S if S else np.zeros(0, dtype=np.int64)


def make_codes(case, P, seed=0, dist=None):
    """The packed codes of a case, int64 [P].  Every set starts with each pattern once when P allows ("enum"
    prefix, which scoring reads back), then:
      skew     per column 80 % level 0, else uniform over -1 .. L - 1 (the shape real comparison vectors have)
      dom0     80 % pattern 0, the rest uniform            domlast  80 % pattern n_pat - 1, the rest uniform
      uniform  uniform over the patterns
      mislead  every vector k_em_hot_sample reads carries pattern A = 5 throughout, every other code is
               B = n_pat - 2: the sample votes A, B holds the majority (no enum prefix)
      one      every pair has pattern n_pat // 2 (no enum prefix)
      no_x     uniform over the patterns except X = `stale_x(case)`, which never occurs (no enum prefix)
      dom_x    80 % pattern X (no enum prefix)"""
    rng = np.random.Generator(np.random.PCG64(seed * 1000 + case.n_pat))
    n_pat, nlev = case.n_pat, case.nlev
    if dist is None:
        dist = case.dist if isinstance(case.dist, str) else case.dist[0]
    vec = 8 if n_pat <= 65536 else 4

    def fill(n, dist):
        if dist == "skew":
            c = np.zeros(n, dtype=np.int64)
            for L, s in zip(nlev, strides(nlev)):
                lev = np.where(rng.random(n) < 0.8, 0, rng.integers(-1, L, n))
                c += (lev + 1) * s
            return c
        if dist in ("dom0", "domlast", "dom_x"):
            top = {"dom0": 0, "domlast": n_pat - 1, "dom_x": stale_x(case)}[dist]
            return np.where(rng.random(n) < 0.8, top, rng.integers(0, n_pat, n)).astype(np.int64)
        if dist == "uniform":
            return rng.integers(0, n_pat, n).astype(np.int64)
        if dist == "one":
            return np.full(n, n_pat // 2, dtype=np.int64)
        if dist == "no_x":
            c = rng.integers(0, n_pat - 1, n).astype(np.int64)
            return c + (c >= stale_x(case))
        if dist == "mislead":
            c = np.full(n, n_pat - 2, dtype=np.int64)
            for v in sampled_vectors(n // vec):
                c[v * vec:(v + 1) * vec] = 5
            return c
        raise ValueError(dist)
    if dist in ("mislead", "one", "no_x", "dom_x") or P < n_pat:
        return fill(P, dist)
    return np.concatenate([np.arange(n_pat, dtype=np.int64), fill(P - n_pat, dist)])


def stale_x(case):
    return case.n_pat // 3


def _cases():
    C = []
    add = lambda *a, **k: C.append(Case(*a, **k))  # noqa: E731
    # R boundaries, each side: n_pat · R · 4 <= 160 KiB - 2 KiB, so R = 64 up to 632 patterns, 32 up to 1264,
    # 16 up to 2528, 8 up to 5056, 4 up to 10 112
    add("R64_632", [7, 78], ENUM_P, "skew", ["lanes_R64", "iter_room_lds", "grid_many", "remainder_only"])
    add("R32_635", [4, 126], ENUM_P, "skew", ["lanes_R32", "iter_room_lds"])
    add("R32_1264", [15, 78], ENUM_P, "skew", ["lanes_R32"])
    add("R16_1265", [4, 10, 22], ENUM_P, "skew", ["lanes_R16"])
    add("R16_2528", [31, 78], ENUM_P, "skew", ["lanes_R16"])
    add("R8_2530", [1, 4, 10, 22], ENUM_P, "skew", ["lanes_R8"])
    add("R8_5056", [63, 78], ENUM_P, "skew", ["lanes_R8", "iter_room_global", "finalize_global"])
    add("R4_5060", [3, 4, 10, 22], ENUM_P, "skew", ["lanes_R4", "iter_noroom"])
    add("R4_10112", [1, 63, 78], ENUM_P, "skew", ["lanes_R4", "iter_noroom", "grid_many"])
    add("R0_10115", [4, 6, 16, 16], ENUM_P, "skew", ["khist_u16_lds", "finalize_global"])
    # the counters alone filling the whole 160 KiB (640 · 64, 1280 · 32, ... words) and the first space past each:
    # there the launch was refused until the plan left room for the kernel's static LDS; now one R further down
    add("n640", [9, 7, 7], ENUM_P, "skew", ["lanes_R32", "iter_room_lds"])
    add("n642", [1, 2, 106], ENUM_P, "skew", ["lanes_R32", "iter_room_lds"])
    add("n1280", [9, 7, 15], ENUM_P, "skew", ["lanes_R16"])
    add("n1281", [2, 6, 60], ENUM_P, "skew", ["lanes_R16"])
    add("n2560", [9, 15, 15], ENUM_P, "skew", ["lanes_R8"])
    add("n2562", [1, 2, 6, 60], ENUM_P, "skew", ["lanes_R8"])
    add("n5120", [19, 15, 15], ENUM_P, "skew", ["lanes_R4", "iter_noroom", "finalize_global"])
    add("n5123", [46, 108], ENUM_P, "skew", ["lanes_R4", "iter_noroom", "mu_upload"])
    add("n10240", [19, 31, 15], ENUM_P, "skew", ["khist_u16_lds", "finalize_global"])
    add("n10241", [6, 6, 10, 18], ENUM_P, "skew", ["khist_u16_lds", "finalize_global"])
    # the per-pattern tables at 4096, the LDS histogram at 16 384, the code width at 65 536
    add("tab_4096", [15, 15, 15], ENUM_P, "skew", ["lanes_R8", "iter_room_lds", "finalize_lds", "score_u16_lds"])
    add("tab_4100", [3, 24, 40], ENUM_P, "skew",
        ["lanes_R8", "iter_room_global", "finalize_global", "score_u16_global"])
    add("bins_16384", [15, 31, 31], ENUM_P, "skew", ["khist_u16_lds"])
    add("bins_16385", [4, 28, 112], ENUM_P, "skew", ["khist_u16_global", "mu_upload", "slots_more_rounds"])
    add("u16_65536", [63, 31, 31], ENUM_P, "skew", ["khist_u16_global", "score_u16_global"])
    add("u32_65540", [3, 4, 28, 112], ENUM_P, "skew", ["khist_u32_global", "score_u32_global"])
    add("tiny_3", [2], ENUM_P, "skew", ["lanes_R64", "iter_noroom", "totals_split"])
    # m / u in the kernel arguments up to Σ L_k = 96, uploaded past it
    add("mu_96", [47, 49], ENUM_P, "skew", ["mu_inline", "lanes_R16"])
    add("mu_97", [48, 49], ENUM_P, "skew", ["mu_upload", "lanes_R16"])
    # the slot walk: split totals up to 28 slots, one round up to 31, a second with an idle half-wave at 32
    # (33 slots + the totals = 34 half-waves); strides 7, 49, 343 / 3, 15, 165 / 8, 64, 512
    add("slots_28", [6, 6, 6, 6], ENUM_P, "skew", ["totals_split"])
    add("slots_29", [6, 6, 6, 7], ENUM_P, "skew", ["slots_one_round"])
    add("slots_31", [2, 4, 10, 11], ENUM_P, "skew", ["slots_one_round"])
    add("slots_32", [7, 7, 7, 7], ENUM_P, "skew", ["slots_two_rounds"])
    add("slots_33", [2, 4, 10, 13], ENUM_P, "skew", ["slots_two_rounds"])
    # P on one small pattern space per code width ("vec": a · VEC + b codes)
    for tag, nlev, wide in (("u16", [1, 2, 106], False), ("u32", [3, 4, 28, 112], True)):
        kern = ["khist_u32_global"] if wide else ["lanes_R32"]
        one = [] if wide else ["grid_1"]  # the grid is k_em_iter's: the uint32 space takes k_hist
        add(f"P0_{tag}", nlev, 0, "skew", kern + one + ["P_0", "n_vec_0"])
        add(f"P1_{tag}", nlev, 1, "skew", kern + one + ["n_vec_0"])
        add(f"Pvec-1_{tag}", nlev, ("vec", 1, -1), "skew", kern + one + ["n_vec_0"])
        add(f"Pvec_{tag}", nlev, ("vec", 1, 0), "skew", kern + one + ([] if wide else ["remainder_only"]))
        add(f"Pvec+1_{tag}", nlev, ("vec", 1, 1), "skew", kern + one + ([] if wide else ["remainder_only"]))
        add(f"P1024vec_{tag}", nlev, ("vec", 1024, 0), "skew", kern + one)
        add(f"P1025vec_{tag}", nlev, ("vec", 1025, 0), "skew", kern + ([] if wide else ["grid_2"]))
    # the software-pipelined loop of k_em_iter: n_vec = 8.5 / 7.5 / 3.5 strides plus an odd remainder.  At 8.5
    # every lane takes two pipelined rounds and one remainder step; at 7.5 the lanes below half a stride take two
    # rounds and no remainder step, the others one round and three steps; at 3.5 the lower half takes one round,
    # the upper half only the remainder loop.
    add("pipe_8.5", [1, 2, 106], ("pipe", 85, 77), "skew", ["lanes_R32", "pipe_all_lanes", "pipe_two_rounds"])
    add("pipe_7.5", [1, 2, 106], ("pipe", 75, 77), "skew", ["lanes_R32", "pipe_all_lanes", "pipe_two_rounds"])
    add("pipe_3.5", [1, 2, 106], ("pipe", 35, 77), "skew", ["lanes_R32", "pipe_some_lanes"])
    # distributions, on an R = 32 space (the uncounted hot pattern) and an R = 64 space
    for tag, nlev, R in (("R32", [1, 2, 106], "lanes_R32"), ("R64", [3, 3, 2, 2, 3], "lanes_R64")):
        add(f"dom0_{tag}", nlev, ENUM_P, "dom0", [R])
        add(f"domlast_{tag}", nlev, ENUM_P, "domlast", [R])
        add(f"uniform_{tag}", nlev, ENUM_P, "uniform", [R])
        add(f"mislead_{tag}", nlev, 262_149, "mislead", [R])
        add(f"stale_{tag}", nlev, ENUM_P, ("no_x", "dom_x"), [R])  # dom_x is loaded and run first
        add(f"one_{tag}", nlev, ENUM_P, "one", [R])
        add(f"null_{tag}", nlev, ENUM_P, "skew", [R], null_level=True)
    return C


CASES = _cases()
