"""jaccard_sim, cosine_distance and the q-gram tokenisers on the device, against the pure-Python restatement of
tests/setsim_common.py: the bulk functions' values bit for bit, the levels of every pair of a small job in every
filter mode and window split, a mixed program, and a blocking rule with a jaccard_sim residual."""
import copy
import math
import random
import warnings

import numpy as np
import pandas as pd
import pytest

import residual_common as rc
import setsim_common as S

pytestmark = pytest.mark.gpu
warnings.filterwarnings("ignore")


@pytest.fixture(scope="module")
def amd():
    from splink_amd import AmdSession, _native
    if _native.device_count() == 0:
        pytest.fail("no HIP device visible: the -m gpu tests need an MI355X")
    return AmdSession(0)


def _hex(v):
    return None if v is None else float(v).hex()


# ---- 1. values, bit for bit ----------------------------------------------------------------------------------
def test_bulk_values_bit_for_bit(amd):
    from splink_amd import _native as N
    pairs = S.value_pairs()
    assert len(pairs) == 400
    lens = {(S.ulen(a), S.ulen(b)) for a, b in pairs}
    for n in S.LENGTH_EDGES:  # either side and both
        assert any(x == n and y < 64 for x, y in lens) and any(y == n and x < 64 for x, y in lens) and (n, n) in lens
    left, right = [a for a, b in pairs], [b for a, b in pairs]
    ctx = N.Context(0)
    got_j, got_c = ctx.jaccard_sim(left, right), ctx.cosine_distance(left, right)
    want_j = [S.jaccard_sim(a, b) for a, b in pairs]
    want_c = [S.cosine_distance(a, b) for a, b in pairs]
    bad = [(i, a[:40], b[:40], _hex(g), _hex(w)) for i, ((a, b), g, w) in enumerate(zip(pairs, got_j, want_j)) if g != w]
    assert not bad, ("jaccard_sim", len(bad), bad[:6])
    bad = [(i, a[:40], b[:40], _hex(g), _hex(w)) for i, ((a, b), g, w) in enumerate(zip(pairs, got_c, want_c))
           if (not math.isnan(g) if w is None else g != w)]  # NaN where an operand is blank
    assert not bad, ("cosine_distance", len(bad), bad[:6])
    # the list holds what it should
    assert sum(w is None for w in want_c) >= 8 and {0.0, 1.0, 0.13, 0.38, 0.63, 0.88, 0.01} <= set(want_j)
    assert any(w is not None and w < 0 for w in want_c) and any(w is not None and 0 < w < 1e-15 for w in want_c)
    # identical multi-token strings: the restatement's +-2.2e-16, not 0
    same = ["john smith", "a b c", "ab cd ef gh", "x y", "one two three four five"]
    got = ctx.cosine_distance(same, same)
    want = [S.cosine_distance(s, s) for s in same]
    assert [float(g).hex() for g in got] == [w.hex() for w in want]
    assert want[0] == 2.220446049250313e-16 and want[1] == -2.220446049250313e-16


# ---- 2. levels per pair through the public API ---------------------------------------------------------------------
JAC = "jaccard_sim(name_l, name_r)"
COSQ = "cosine_distance(QgramTokeniser(lower(surname_l)), QgramTokeniser(lower(surname_r)))"
COSA = "cosine_distance(addr_l, addr_r)"
COLUMNS = [
    {"custom_name": "jac", "custom_columns_used": ["name"], "num_levels": 3,
     "case_expression": f"case when name_l is null or name_r is null then -1 when {JAC} >= 0.43 then 2 "
                        f"when {JAC} > 0.13 then 1 else 0 end"},
    {"custom_name": "cosq", "custom_columns_used": ["surname"], "num_levels": 3,
     "case_expression": f"case when {COSQ} <= 0.5 then 2 when {COSQ} < 0.5917517095361371 then 1 else 0 end"},
    {"custom_name": "cosa", "custom_columns_used": ["addr"], "num_levels": 3,
     "case_expression": f"case when addr_l is null or addr_r is null then -1 when {COSA} = 0.5000000000000001 then 2 "
                        f"when {COSA} < 0.5 then 1 else 0 end"},
]


def _null(v):
    return v is None or (isinstance(v, float) and math.isnan(v))


class Levels:
    """The three columns' levels of a record pair, from the restatement (values cached per string pair)."""

    def __init__(self):
        self.cache = {}

    def value(self, fn, a, b):
        key = (fn.__name__, a, b)
        if key not in self.cache:
            self.cache[key] = fn(a, b)
        return self.cache[key]

    def jac(self, a, b):
        if _null(a) or _null(b):
            return -1
        v = self.value(S.jaccard_sim, a, b)
        return S.case_level([(S.value_test(v, ">=", 0.43), 2), (S.value_test(v, ">", 0.13), 1)], 0)

    def cosq(self, a, b):  # no null guard: a NULL operand makes both tests NULL
        v = None if _null(a) or _null(b) else self.value(S.cosine_distance, S.qgram(a.lower(), 2), S.qgram(b.lower(), 2))
        return S.case_level([(S.value_test(v, "<=", 0.5), 2), (S.value_test(v, "<", 0.5917517095361371), 1)], 0)

    def cosa(self, a, b):
        if _null(a) or _null(b):
            return -1
        v = self.value(S.cosine_distance, a, b)  # None for a blank text: both tests NULL, the ELSE level
        return S.case_level([(S.value_test(v, "=", 0.5000000000000001), 2), (S.value_test(v, "<", 0.5), 1)], 0)


def _records():
    """300 records: the first 60 carry the edge values (NULLs, blanks, anchors, the lengths around the exact pass's 64
    units and the slow pass's 1024) and share one city with 30 ordinary ones, so every edge meets every other."""
    rng = random.Random(77)
    names = ["night", "nacht", "abcdefgh", "a", "abc", "aaa", "xyz", None, "", S.SURROGATE + "ab", "NIGHT"]
    # (the long texts have long words: cosine_distance walks both texts once per distinct token)
    names += [S.words(rng, n, longest=24) for n in S.LENGTH_EDGES] + [S.distinct(1025), S.distinct(1500, 0x300)]
    # QgramTokeniser of n units has 3n - 4: 22 / 23 units straddle 64, 342 / 343 straddle 1024
    surnames = ["john", "jon", "JOHN", "abcde", "abcxy", None, "", " ", "a", "ab", "smith", "smyth", "Smith"]
    surnames += ["".join(rng.choice("abcdef") for _ in range(n)) for n in (22, 23, 22, 23, 342, 343)]
    addrs = ["john smith", "john smyth", "a a b", "a b b", "jo oh hn", "jo on", None, "", "  ", "\t", "\u3000", "!!!",
             "smith john", "john  smith", "John Smith"]
    addrs += [S.words(rng, n, longest=24) for n in S.LENGTH_EDGES] + [S.words(rng, 1500, longest=24)]
    vocab_n = ["night", "nacht", "knight", "abcdefgh", "abcd", "efgh", "hgfedcba", "light", "abc"]
    vocab_s = ["john", "jon", "johnson", "smith", "smyth", "abcde", "abcxy", "Jones", "jones"]
    vocab_a = ["john smith", "john smyth", "mary jones", "jones mary", "a b c", "a b", "12 high st", "12 high street"]
    rows = []
    for i in range(300):
        edge = i < 60
        rows.append({"unique_id": i, "city": "c0" if i < 90 else f"c{1 + i % 4}",
                     "name": names[i % len(names)] if edge else rng.choice(vocab_n),
                     "surname": surnames[(i * 7) % len(surnames)] if edge else rng.choice(vocab_s),
                     "addr": addrs[(i * 5) % len(addrs)] if edge else rng.choice(vocab_a)})
    df = pd.DataFrame(rows)
    for c in ("city", "name", "surname", "addr"):
        df[c] = df[c].astype(object)
    return df


def _settings(link_type, columns, rules):
    return {"link_type": link_type, "proportion_of_matches": 0.01, "max_iterations": 2, "em_convergence": 1e-12,
            "blocking_rules": rules, "comparison_columns": copy.deepcopy(columns)}


def _frames(link_type, df):
    if link_type == "dedupe_only":
        return dict(df=df)
    return dict(df_l=df.iloc[0::2].reset_index(drop=True), df_r=df.iloc[1::2].reset_index(drop=True))


@pytest.fixture(scope="module")
def levels():
    return Levels()


@pytest.mark.parametrize("link_type", ["dedupe_only", "link_only"])
def test_levels_of_every_pair(amd, levels, link_type):
    from splink_amd.blocking import block_using_rules
    from splink_amd.gammas import add_gammas
    from splink_amd.settings import complete_settings_dict
    df = _records()
    st = complete_settings_dict(_settings(link_type, COLUMNS, ["l.city = r.city"]), amd)
    gf = add_gammas(block_using_rules(st, amd, **_frames(link_type, df)), st, amd)
    job = gf.job
    l, r = job.pair_rows()
    tl, tr = job.tables[0], job.tables[job.r_side()]
    P = job.n_pairs
    assert P == len(l) and P > (2000 if link_type == "link_only" else 4000)
    cols = {c: (tl[c].to_numpy(dtype=object)[l], tr[c].to_numpy(dtype=object)[r]) for c in ("name", "surname", "addr")}
    want = np.array([[levels.jac(a, b) for a, b in zip(*cols["name"])],
                     [levels.cosq(a, b) for a, b in zip(*cols["surname"])],
                     [levels.cosa(a, b) for a, b in zip(*cols["addr"])]], dtype=np.int8).T
    for k in range(3):  # every level of every column occurs
        assert set(want[:, k].tolist()) >= {0, 1, 2}, (k, set(want[:, k].tolist()))
    assert -1 in want[:, 0] and -1 in want[:, 2] and -1 not in want[:, 1]
    # the frame the public API hands out, then every filter mode, whole and in two windows
    out = gf.toPandas()
    got = out[["gamma_jac", "gamma_cosq", "gamma_cosa"]].to_numpy()
    assert (got == want).all(), np.nonzero((got != want).any(axis=1))[0][:10]
    ctx = job.ctx
    try:
        for mode in (1, 0, 11, 21, 101):
            for window in (0, P // 2 + 1):
                ctx.gammas_set_simple(mode)
                ctx.gammas_set_window(window)
                job.gammas(st)
                got = job.gammas_host()
                bad = np.nonzero((got != want).any(axis=1))[0]
                assert got.shape == want.shape and not len(bad), (mode, window, len(bad), [
                    (int(p), got[p].tolist(), want[p].tolist(), [str(cols[c][0][p])[:30] for c in cols],
                     [str(cols[c][1][p])[:30] for c in cols]) for p in bad[:5]])
                assert ctx.gammas_windows() == (2 if window else 1)
                assert ctx.gammas_simple_count() == 0  # the new tests have no filter class: the interpreter's columns
    finally:
        ctx.gammas_set_simple(1)
        ctx.gammas_set_window(0)


# ---- 3. mixed program -----------------------------------------------------------------------------------------------
def test_jaccard_column_beside_template_columns(amd, levels):
    from splink_amd.engine import Job
    from splink_amd.settings import complete_settings_dict
    from splink_amd.synthetic import cfg_settings, make_records
    df = make_records(300, seed=3, surname_vocab=30, first_vocab=50, city_vocab=20)[
        ["unique_id", "first_name", "surname", "dob", "city", "email"]]
    base = cfg_settings(1, max_iterations=2)
    plus = copy.deepcopy(base)
    expr = ("case when first_name_l is null or first_name_r is null then -1 "
            "when jaccard_sim(first_name_l, first_name_r) >= 0.5 then 1 else 0 end")
    plus["comparison_columns"].insert(2, {"custom_name": "fj", "custom_columns_used": ["first_name"], "num_levels": 2,
                                          "case_expression": expr})
    base, plus = complete_settings_dict(base, amd), complete_settings_dict(plus, amd)
    job = Job("dedupe_only", [df], "unique_id", 0)
    job.block(base["blocking_rules"])
    assert job.n_pairs > 500
    job.gammas(base)
    want = job.gammas_host()
    job.gammas(plus)
    got = job.gammas_host()
    assert job.ctx.gammas_simple_count() == want.shape[1]  # the template columns stay with the filter kernel
    assert got.shape == (want.shape[0], want.shape[1] + 1)
    assert (np.delete(got, 2, axis=1) == want).all()
    l, r = job.pair_rows()
    fn = job.tables[0]["first_name"].to_numpy(dtype=object)
    fj = [-1 if _null(a) or _null(b) else int(S.jaccard_sim(a, b) >= 0.5) for a, b in zip(fn[l], fn[r])]
    assert (got[:, 2] == np.array(fj)).all() and {0, 1} <= set(fj)


# ---- 4. a residual rule ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("link_type", ["dedupe_only", "link_only"])
def test_jaccard_residual_rule(amd, link_type):
    from splink_amd.engine import Job
    rng = random.Random(5)
    vocab = ["smith", "smyth", "smithe", "jones", "jonas", "johnson", "abc", "xyz", "", None, "night", "nacht"]
    df = pd.DataFrame({"unique_id": range(120),
                       "city": pd.Series([rng.choice(["a", "b", "c", None]) for _ in range(120)], dtype=object),
                       "surname": pd.Series([rng.choice(vocab) for _ in range(120)], dtype=object),
                       "dob": pd.Series([rng.choice(["1990", "1991", "1992"]) for _ in range(120)], dtype=object)})
    rules = ["l.city = r.city and jaccard_sim(l.surname, r.surname) >= 0.5", "l.dob = r.dob"]

    def residual(l, r):
        a, b = l["surname"], r["surname"]
        return None if _null(a) or _null(b) else S.jaccard_sim(a, b) >= 0.5

    fns = [(rc.eq("city"), residual), (rc.eq("dob"), None)]
    frames = _frames(link_type, df)
    inputs = [frames["df"]] if link_type == "dedupe_only" else [frames["df_l"], frames["df_r"]]
    rows = [[dict(zip(t.columns, v)) for v in t.itertuples(index=False, name=None)] for t in inputs]
    L = rows[0]
    R = rows[-1] if link_type == "link_only" else L
    emitted, stats = rc.brute_force(link_type, L, R, fns)
    assert stats[0]["emitted"] > 0 and stats[0]["rejected"] > 0 and stats[0]["null_residual"] > 0
    assert stats[1]["emitted"] > 0 and stats[1]["after_untrue_earlier"] > 0
    job = Job(link_type, inputs, "unique_id", 0)
    job.block(rules)
    l, r = job.pair_rows()
    rs = job.r_side()
    pl = job.perm[0] if job.perm[0] is not None else np.arange(len(inputs[0]))
    pr = job.perm[rs] if job.perm[rs] is not None else np.arange(len(inputs[rs]))
    got = sorted(zip(pl[l].tolist(), pr[r].tolist()))
    assert job.n_pairs == len(emitted)
    assert got == sorted((i, j) for _, i, j in emitted)
