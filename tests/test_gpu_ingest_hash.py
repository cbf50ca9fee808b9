"""hashed_ids' collision handling (spk_ingest.hip): the dense ids behind the blocking keys and behind every string
comparison column's dictionary come from a 63-bit hash, verified byte for byte against the run predecessor
(k_heads_verify); a collision re-hashes under the next of four seeds, four collisions are an error.  A 63-bit hash
never collides on test data, so Context.ingest_set_hash_bits narrows it: tests/ingest_hash_common.py's port of the
hash finds, for the 250 values used here, the widths at which exactly the wanted seeds collide.  If the verification
were broken, two different values would share an id: they would block together and compare equal."""
import random
import warnings

import numpy as np
import pandas as pd
import pytest

import exprgen as xg
import ingest_hash_common as hc
import oracle as orc

pytestmark = pytest.mark.gpu
warnings.filterwarnings("ignore")

VALUES = [f"{'v' if i % 2 else 'name'}27-{i}" for i in range(250)]
INTS = [(i * 2654435761 + 27 * 97) % (2 ** 40) - 2 ** 39 for i in range(250)]
# seeds that must (True) / must not (False) collide; None: either
PATTERNS = {"seed0-collides-seed1-free": [True, False, None, None], "only-seed3-free": [True, True, True, False]}
ALL_COLLIDE = [True, True, True, True]


@pytest.fixture(scope="module")
def amd():
    from splink_amd import AmdSession, _native
    if _native.device_count() == 0:
        pytest.fail("no HIP device visible: the -m gpu tests need an MI355X")
    return AmdSession(0)


def _tables(values, groups, col):
    """Left and right records {unique_id, <col>, c}: every value once over the two tables, 130 repeats, 20 NULLs, and
    each value of the colliding `groups` in both tables with c = 'c0' -- so that a collision taken for equality
    would add pairs under every link type and under the two-term rule."""
    rng = random.Random(99)
    vals = list(values) + [rng.choice(values) for _ in range(130)] + [None] * 20
    rng.shuffle(vals)
    rows = [{col: v, "c": rng.choice(["c0", "c1"])} for v in vals]
    half = len(rows) // 2
    sides = [rows[:half], rows[half:]]
    for g in groups:
        for v in g:
            for side in sides:
                side.append({col: v, "c": "c0"})
    out, uid = [], 0
    for side in sides:
        df = pd.DataFrame(side)
        df.insert(0, "unique_id", range(uid, uid + len(df)))
        uid += len(df)
        if col == "n":
            df["n"] = pd.array([None if v is None or v != v else int(v) for v in df["n"].tolist()], dtype="Int64")
        else:
            df[col] = df[col].astype(object).where(df[col].notna(), None)
        df["c"] = df["c"].astype(object)
        out.append(df)
    return out


def _job_and_kw(link_type, df_l, df_r):
    from splink_amd.engine import Job
    if link_type == "dedupe_only":
        both = pd.concat([df_l, df_r], ignore_index=True)
        return Job(link_type, [both], "unique_id", 0), dict(df=both)
    if link_type == "link_and_dedupe":
        both = pd.concat([df_l.assign(_source_table="left"), df_r.assign(_source_table="right")], ignore_index=True)
        return Job(link_type, [both], "unique_id", 0), dict(df_l=df_l, df_r=df_r)
    return Job(link_type, [df_l, df_r], "unique_id", 0), dict(df_l=df_l, df_r=df_r)


def _device_pairs(job):
    l, r = job.pair_rows()
    ul, ur = job.tables[0]["unique_id"].to_numpy()[l], job.r_table()["unique_id"].to_numpy()[r]
    return sorted(zip(ul.tolist(), ur.tolist()))


def _oracle_pairs(link_type, kw, rules):
    st = {"link_type": link_type, "blocking_rules": list(rules), "unique_id_column_name": "unique_id"}
    pairs, left, right = orc.block(st, **kw)
    ul = left["unique_id"].to_numpy()[pairs["row_l"].to_numpy(dtype=np.int64)]
    ur = right["unique_id"].to_numpy()[pairs["row_r"].to_numpy(dtype=np.int64)]
    return sorted(zip(ul.tolist(), ur.tolist()))


def _false_pairs(link_type, df_l, df_r, col, bits):
    """Pairs of rows with different values and one seed-0 key at `bits` bits, that the link type would emit."""
    key = lambda v: None if v is None or v is pd.NA else hc.key_of(v, hc.SEEDS[0], bits)  # noqa: E731
    l = [(v, key(v)) for v in df_l[col].tolist()]
    r = [(v, key(v)) for v in df_r[col].tolist()]
    both = l + r
    if link_type == "link_only":
        return sum(1 for a, ka in l for b, kb in r if ka is not None and ka == kb and a != b)
    return sum(1 for i, (a, ka) in enumerate(both) for b, kb in both[i + 1:] if ka is not None and ka == kb and a != b)


def _check_blocking(link_type, values, col, bits, rule_sets):
    groups = hc.colliding_values(values, bits)
    assert groups
    df_l, df_r = _tables(values, groups, col)
    assert set(values) == {v for t in (df_l, df_r) for v in t[col].tolist() if v is not None and v is not pd.NA}
    assert _false_pairs(link_type, df_l, df_r, col, bits) >= len(groups)
    for rules in rule_sets:
        job, kw = _job_and_kw(link_type, df_l, df_r)
        want = _oracle_pairs(link_type, kw, rules)
        assert len(want) >= 20
        job.ctx.ingest_set_hash_bits(bits)
        job.block(list(rules))
        got = _device_pairs(job)
        assert got == want, (rules, bits, sorted(set(got) - set(want))[:3], sorted(set(want) - set(got))[:3])


def test_the_search_finds_every_width():
    """The widths the tests below run at (the search's answers for VALUES and INTS), and the port on fixed points."""
    widths = {k: hc.find_bits(VALUES, p) for k, p in PATTERNS.items()}
    widths["all-four"] = hc.find_bits(VALUES, ALL_COLLIDE)
    widths["int64"] = hc.find_bits(INTS, PATTERNS["seed0-collides-seed1-free"])
    print(widths)
    assert all(b is not None and 8 <= b < 40 for b in widths.values()), widths
    assert widths["seed0-collides-seed1-free"] > widths["only-seed3-free"] > widths["all-four"]
    assert hc.colliding_seeds(VALUES, 63) == [False] * 4 and hc.colliding_seeds(INTS, 63) == [False] * 4
    assert hc.mix64(0) == 0 and hc.mix64(1) == 0xB456BCFC34C2CB2C  # MurmurHash3's fmix64


@pytest.mark.parametrize("link_type", ["dedupe_only", "link_only", "link_and_dedupe"])
@pytest.mark.parametrize("pattern", list(PATTERNS))
def test_blocking_keys_survive_collisions(amd, pattern, link_type):
    """`l.a = r.a` and the two-term `l.a = r.a and l.c = r.c` at a width where seed 0 collides and seed 1 does
    not, and at one where only seed 3 is collision-free: the pairs are the oracle's."""
    bits = hc.find_bits(VALUES, PATTERNS[pattern])
    assert bits is not None
    assert not all(hc.colliding_seeds(["c0", "c1"], bits))  # the second term's column finds a seed too
    _check_blocking(link_type, VALUES, "a", bits, (["l.a = r.a"], ["l.a = r.a and l.c = r.c"]))


@pytest.mark.parametrize("link_type", ["dedupe_only", "link_only"])
def test_int64_keys_survive_collisions(amd, link_type):
    """A numeric rule `l.n = r.n` on an int64 column (k_hash's mix64 branch, same_value's integer compare)."""
    bits = hc.find_bits(INTS, PATTERNS["seed0-collides-seed1-free"])
    assert bits is not None
    _check_blocking(link_type, INTS, "n", bits, (["l.n = r.n"],))


@pytest.mark.parametrize("pattern", list(PATTERNS))
def test_dictionary_ids_survive_collisions(amd, pattern):
    """A string comparison column compares dictionary ids (spk_table_add_raw_utf8): on a pair frame that holds the
    colliding pairs, `a_l = a_r` is the oracle's, plain and in the filter's guarded shape."""
    from splink_amd.engine import Job
    from splink_amd.settings import complete_settings_dict
    bits = hc.find_bits(VALUES, PATTERNS[pattern])
    groups = hc.colliding_values(VALUES, bits)
    assert bits is not None and groups
    rng = random.Random(17)
    rows = [(v, v if rng.random() < 0.4 else rng.choice(VALUES)) for v in VALUES]
    rows += [(g[i], g[j]) for g in groups for i in range(len(g)) for j in range(len(g)) if i != j]
    rows += [(None, VALUES[0]), (VALUES[1], None), (None, None)]
    rng.shuffle(rows)
    df = pd.DataFrame({"a_l": pd.Series([a for a, _ in rows], dtype=object),
                       "a_r": pd.Series([b for _, b in rows], dtype=object)})
    cols = [dict(name="c0", L=2, expr="case when a_l = a_r then 1 else 0 end"),
            dict(name="c1", L=2, expr="case when a_l is null or a_r is null then -1 when a_l = a_r then 1 else 0 end"),
            dict(name="c2", L=2, expr="case when a_l != a_r then 1 else 0 end")]
    want = orc.sql_gammas(df, [c["expr"] for c in cols])
    assert (want != -99).all() and 50 <= int((want[:, 0] == 1).sum()) <= len(df) - 50
    job = Job("link_only", [pd.DataFrame({"a": df["a_l"]}), pd.DataFrame({"a": df["a_r"]})], "", 0)
    job.ctx.ingest_set_hash_bits(bits)
    idx = np.arange(len(df), dtype=np.int32)
    job.load_pairs(idx, idx)
    st = complete_settings_dict(xg.settings(cols), amd)
    try:
        for mode in (1, 0):
            job.ctx.gammas_set_simple(mode)
            job.gammas(st)
            got = job.gammas_host()
            bad = np.argwhere(got != want)
            assert not len(bad), (mode, bits, [(df.iloc[i].tolist(), cols[k]["expr"]) for i, k in bad[:3]])
    finally:
        job.ctx.gammas_set_simple(1)


def test_four_collisions_are_an_error_and_the_context_recovers(amd):
    """At a width where all four seeds collide the call returns the library's error (no device fault); at 63 bits the
    same context then blocks to the oracle's pairs."""
    bits = hc.find_bits(VALUES, ALL_COLLIDE)
    assert bits is not None
    df_l, df_r = _tables(VALUES, hc.colliding_values(VALUES, bits), "a")
    job, kw = _job_and_kw("dedupe_only", df_l, df_r)
    job.ctx.ingest_set_hash_bits(bits)
    with pytest.raises(RuntimeError, match=f"{bits}-bit hash collisions under four seeds"):
        job.block(["l.a = r.a"])
    for bad in (0, 64, -1):
        with pytest.raises(ValueError, match="1 .. 63"):
            job.ctx.ingest_set_hash_bits(bad)
    job.ctx.ingest_set_hash_bits(63)
    job.block(["l.a = r.a"])
    assert _device_pairs(job) == _oracle_pairs("dedupe_only", kw, ["l.a = r.a"])
