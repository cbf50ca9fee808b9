"""Random-pair sampling on the host: properties of the definition (tests/sample_common.py restates it from
include/splink_hip.h), Params.fix_u_probabilities, and the u arithmetic of estimate_u_using_random_sampling."""
import copy
import itertools
import json

import numpy as np
import pytest

import sample_common as sc


def ranks(n, kind, seed=0):
    rng = np.random.Generator(np.random.PCG64(seed))
    if kind == "distinct":
        return rng.permutation(n).astype(np.int64), 0
    if kind == "duplicated":
        return rng.integers(0, max(n // 2, 1), n).astype(np.int64), 0
    # NULL unique ids: rank = source * div + r, r == div - 1 for a NULL id; two sources
    div = n + 1
    r = rng.permutation(n).astype(np.int64)
    r[rng.random(n) < 0.2] = div - 1
    return (np.arange(n) >= n // 2).astype(np.int64) * div + r, div


@pytest.mark.parametrize("kind", ["distinct", "duplicated", "null"])
@pytest.mark.parametrize("n0,total", [(40, 17), (40, 40), (40, 1500), (2, 50), (3, 7)])
def test_dedupe_draws_are_ordered_pairs_of_the_cartesian_block(kind, n0, total):
    rank, div = ranks(n0, kind, seed=n0 + total)
    l, r = sc.sample(3, total, 0, total, n0, rank=rank, null_div=div)
    assert len(l) == len(r) <= total
    assert (l != r).all() and (rank[l] < rank[r]).all()
    if div:
        same = rank[l] // div == rank[r] // div
        assert not (same & ((rank[l] % div == div - 1) | (rank[r] % div == div - 1))).any()
    if kind == "distinct":
        assert len(l) == total  # nothing to drop


def test_anchors_are_stratified_and_non_decreasing():
    for n0, total in [(97, 10), (97, 97), (97, 1000), (5, 64)]:
        a = [sc.anchor(9, i, total, n0) for i in range(total)]
        assert all(x <= y for x, y in zip(a, a[1:]))
        assert all((i * n0) // total <= x < max(((i + 1) * n0) // total, (i * n0) // total + 1)
                   for i, x in enumerate(a))
        if total >= n0:  # every row is the anchor of floor(total / n0) or one more draws
            cnt = np.bincount(a, minlength=n0)
            assert cnt.min() >= total // n0 and cnt.max() <= total // n0 + 1


def test_ranges_concatenate_to_the_whole_sample():
    rank, _ = ranks(40, "duplicated", seed=1)
    whole = sc.sample(5, 1000, 0, 1000, 40, rank=rank)
    cuts = [0, 1, 333, 334, 900, 1000]
    parts = [sc.sample(5, 1000, a, b - a, 40, rank=rank) for a, b in zip(cuts, cuts[1:])]
    assert np.array_equal(np.concatenate([p[0] for p in parts]), whole[0])
    assert np.array_equal(np.concatenate([p[1] for p in parts]), whole[1])
    wl = sc.sample(5, 1000, 0, 1000, 40, n1=23)
    pl = [sc.sample(5, 1000, a, b - a, 40, n1=23) for a, b in zip(cuts, cuts[1:])]
    assert np.array_equal(np.concatenate([p[1] for p in pl]), wl[1]) and len(wl[0]) == 1000
    assert wl[1].min() >= 0 and wl[1].max() < 23


def test_every_dedupe_pair_is_in_the_set_of_all_pairs():
    n0 = 40
    uid = np.random.Generator(np.random.PCG64(2)).permutation(n0).astype(np.int64)  # rank = unique id order
    allowed = {(i, j) for i in range(n0) for j in range(n0) if uid[i] < uid[j]}
    l, r = sc.sample(1, 5000, 0, 5000, n0, rank=uid)
    assert set(zip(l.tolist(), r.tolist())) <= allowed and len(allowed) == n0 * (n0 - 1) // 2


def test_every_unordered_pair_occurs():
    n0, total = 12, 66 * 400
    l, r = sc.sample(0, total, 0, total, n0, rank=np.arange(n0, dtype=np.int64))
    assert set(zip(l.tolist(), r.tolist())) == set(itertools.combinations(range(n0), 2))


def test_degenerate_tables_have_no_pairs():
    assert len(sc.sample(0, 10, 0, 10, 1, rank=np.zeros(1, np.int64))[0]) == 0
    assert len(sc.sample(0, 10, 0, 10, 0, rank=np.zeros(0, np.int64))[0]) == 0
    assert len(sc.sample(0, 10, 0, 10, 5, n1=0)[0]) == 0
    assert len(sc.sample(0, 0, 0, 0, 5, n1=3)[0]) == 0


# ---- Params.fix_u_probabilities ----------------------------------------------------------------------------
def _params():
    from splink_amd.params import Params
    return Params(copy.deepcopy(sc.settings(["l.city = r.city"])), None)


def _pi_rows(scale):
    rows = []
    for name, L in zip(sc.NAMES, sc.LEVELS):
        for v in range(-1, L):
            rows.append({"gamma_col": name, "gamma_value": v, "new_probability_match": scale * (v + 2) / 16,
                         "new_probability_non_match": scale * (L - v) / 16})
    return rows


def _u(params_dict):
    return {(g, k): lv["probability"] for g, d in params_dict["π"].items()
            for k, lv in d["prob_dist_non_match"].items()}


def _m(params_dict):
    return {(g, k): lv["probability"] for g, d in params_dict["π"].items() for k, lv in d["prob_dist_match"].items()}


def test_fix_u_probabilities_holds_u_and_moves_m_and_lambda():
    p = _params()
    assert p.fix_u_probabilities is False
    u0, m0, lam0 = _u(p.params), _m(p.params), p.params["λ"]
    p.fix_u_probabilities = True
    p._update_params(0.25, _pi_rows(1.0))
    assert _u(p.params) == u0 and _u(p.param_history[-1]) == u0
    assert _m(p.params) != m0 and p.params["λ"] == 0.25 != lam0
    assert _m(p.params)[("gamma_city", "level_1")] == 3 / 16 and p.iteration == 2
    p._update_params(0.5, _pi_rows(0.5))
    assert _u(p.params) == u0 and p.params["λ"] == 0.5 and len(p.param_history) == 2
    # is_converged sees no movement in u: an M-step with the same m and another u has converged
    other_u = [dict(r, new_probability_non_match=r["new_probability_non_match"] / 2) for r in _pi_rows(0.5)]
    p._update_params(0.5, other_u)
    assert p.is_converged() and _u(p.params) == u0
    # without the flag the same updates move u, and the last one has not converged
    q = _params()
    q._update_params(0.25, _pi_rows(1.0))
    assert _u(q.params) != u0 and _u(q.params)[("gamma_city", "level_0")] == 2 / 16
    q._update_params(0.5, _pi_rows(0.5))
    q._update_params(0.5, other_u)
    assert _m(q.params) == _m(p.params) and not q.is_converged()


def test_fix_u_probabilities_json(tmp_path):
    from splink_amd.params import load_params_from_dict, load_params_from_json
    p = _params()
    p._update_params(0.25, _pi_rows(1.0))
    assert set(p._to_dict()) == {"current_params", "historical_params", "settings"}  # the parent's keys exactly
    plain = json.dumps(p._to_dict(), indent=4)
    p.fix_u_probabilities = True
    assert set(p._to_dict()) == {"current_params", "historical_params", "settings", "fix_u_probabilities"}
    path = str(tmp_path / "model.json")
    p.save_params_to_json_file(path)
    back = load_params_from_json(path)
    assert back.fix_u_probabilities is True and back.params == p.params and back.param_history == p.param_history
    u0 = _u(back.params)
    back._update_params(0.4, _pi_rows(0.5))
    assert _u(back.params) == u0
    old = load_params_from_dict(json.loads(plain))
    assert old.fix_u_probabilities is False
    # a model saved without the flag is written back with the parent's keys (the settings are completed again on
    # load, as before, so only the parameters are compared)
    again = json.loads(json.dumps(old._to_dict(), indent=4))
    assert list(again) == list(json.loads(plain)) == ["current_params", "historical_params", "settings"]
    assert all(again[k] == json.loads(plain)[k] for k in ("current_params", "historical_params"))
    with pytest.raises(ValueError):
        load_params_from_dict({**json.loads(plain), "other": 1})


# ---- the u arithmetic ----------------------------------------------------------------------------------------
def test_u_from_a_hand_made_histogram():
    from splink_amd.labels import LabelCounts
    from splink_amd.sampling import u_rows_from_histogram
    names, levels = ["gamma_a", "gamma_b", "gamma_c"], [3, 2, 2]
    # gamma_a: levels -1, 0, 2 observed (1 never); gamma_b: all observed; gamma_c: NULL only
    vectors = [((-1, 0, -1), 5), ((0, 0, -1), 7), ((0, 1, -1), 11), ((2, 1, -1), 3), ((2, -1, -1), 2), ((2, 0, -1), 1)]
    hist = np.zeros(4 * 3 * 3, dtype=np.int64)
    for (a, b, c), n in vectors:
        hist[(a + 1) + 4 * (b + 1) + 12 * (c + 1)] += n
    lam, rows = LabelCounts(names, levels, np.stack([hist, 0 * hist, 0 * hist])).m_step()
    got = {(r["gamma_col"], r["gamma_value"]): r["new_probability_non_match"] for r in rows}
    f32 = lambda x: float(np.float32(x))  # noqa: E731
    assert got[("gamma_a", 0)] == f32(18 / 24) and got[("gamma_a", 2)] == f32(6 / 24)
    assert ("gamma_a", 1) not in got  # never observed: no row, _populate_params leaves it at 0
    assert got[("gamma_b", 0)] == f32(13 / 27) and got[("gamma_b", 1)] == f32(14 / 27)
    assert got[("gamma_c", -1)] is None and [k for k in got if k[0] == "gamma_c"] == [("gamma_c", -1)]
    assert all(r["new_probability_match"] is None for r in rows)  # no matches: m has no estimate
    table = {(r["gamma_col"], r["gamma_value"]): (r["count"], r["u_probability"])
             for r in u_rows_from_histogram(names, levels, hist)}
    assert table[("gamma_a", -1)] == (5, None) and table[("gamma_a", 0)] == (18, f32(18 / 24))
    assert table[("gamma_a", 1)] == (0, 0) and table[("gamma_a", 2)] == (6, f32(6 / 24))
    assert table[("gamma_b", -1)] == (2, None) and table[("gamma_b", 1)] == (14, f32(14 / 27))
    assert table[("gamma_c", -1)] == (29, None) and table[("gamma_c", 0)] == (0, 0) and table[("gamma_c", 1)] == (0, 0)
    assert len(table) == 4 + 3 + 3
    # the shared host restatement agrees
    g = np.concatenate([np.tile(np.array(v, dtype=np.int8), (n, 1)) for v, n in vectors])
    us, counts = sc.host_u(g[:, :2], levels[:2])
    assert us[0] == [table[("gamma_a", v)][1] for v in range(3)]
    assert us[1] == [table[("gamma_b", v)][1] for v in range(2)]
    assert counts[0].tolist() == [table[("gamma_a", v)][0] for v in range(-1, 3)]
