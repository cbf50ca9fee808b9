"""Blocking rules with residual predicates: a brute-force restatement of the reference's semantics
(blocking.py:59-68, 133-158) in plain Python over all row pairs with SQL three-valued logic (None = NULL),
shared by tests/test_residual_rules_host.py and tests/test_gpu_residual.py.

For rules R_0 .. R_{n-1} and the link-type predicate T, rule r emits (l, r) iff T is TRUE, R_r is TRUE and
ifnull(R_j, false) is FALSE for every j < r.
"""
import math

GOLDEN_RULES = [
    "l.city = r.city and abs(l.age - r.age) < 5",
    "l.surname = r.surname and levenshtein(l.first_name, r.first_name) <= 1",
    "l.city = r.city",
    "l.surname = r.surname and l.age < r.age",
]


def null(v):
    return v is None or (isinstance(v, float) and math.isnan(v))


def levenshtein(a, b):
    prev = list(range(len(b) + 1))
    for i, ca in enumerate(a, 1):
        cur = [i]
        for j, cb in enumerate(b, 1):
            cur.append(min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (ca != cb)))
        prev = cur
    return prev[-1]


def k_and(*xs):
    """Kleene AND: FALSE if any is FALSE, else NULL if any is NULL, else TRUE."""
    if any(x is False for x in xs):
        return False
    if any(x is None for x in xs):
        return None
    return True


def cmp(op, a, b):
    if null(a) or null(b):
        return None
    return {"=": a == b, "!=": a != b, "<": a < b, "<=": a <= b}[op]


def eq(col):
    return lambda l, r: cmp("=", l[col], r[col])


def _abs_age_lt5(l, r):
    return None if null(l["age"]) or null(r["age"]) else abs(l["age"] - r["age"]) < 5


def _lev_first_le1(l, r):
    a, b = l["first_name"], r["first_name"]
    return None if null(a) or null(b) else levenshtein(a, b) <= 1


# (key part, residual part or None) of GOLDEN_RULES; the whole rule is their Kleene AND
GOLDEN_RULE_FNS = [
    (eq("city"), _abs_age_lt5),
    (eq("surname"), _lev_first_le1),
    (eq("city"), None),
    (eq("surname"), lambda l, r: cmp("<", l["age"], r["age"])),
]


def rule_value(fn, l, r):
    key, res = fn
    return key(l, r) if res is None else k_and(key(l, r), res(l, r))


def records(d):
    """Column dict (golden JSON) -> list of row dicts."""
    names = list(d)
    return [dict(zip(names, vals)) for vals in zip(*(d[c] for c in names))]


def sides(link_type, df=None, df_l=None, df_r=None, uid="unique_id"):
    """(l rows, r rows) of the join; each row gets `_id`, what identifies it in the output: (source, unique id)."""
    if link_type == "dedupe_only":
        rows = [dict(r, _id=(None, r[uid])) for r in df]
        return rows, rows
    if link_type == "link_only":
        return [dict(r, _id=(None, r[uid])) for r in df_l], [dict(r, _id=(None, r[uid])) for r in df_r]
    rows = [dict(r, _source_table="left", _id=("left", r[uid])) for r in df_l] + \
           [dict(r, _source_table="right", _id=("right", r[uid])) for r in df_r]
    return rows, rows


def link_predicate(link_type, l, r, uid="unique_id"):
    if link_type == "link_only":
        return True
    lt = cmp("<", l[uid], r[uid])
    if link_type == "dedupe_only":
        return lt
    if l["_source_table"] < r["_source_table"]:
        return True
    return k_and(lt, l["_source_table"] == r["_source_table"])


def brute_force(link_type, L, R, rule_fns, uid="unique_id"):
    """Every (rule, l row index, r row index) the rules emit, in rule order, and per-rule statistics:
    `candidates` (T TRUE and the key part TRUE), `rejected` (of those, rule not TRUE), `null_residual` (of those,
    rule NULL), `emitted`, `after_untrue_earlier` (emitted pairs that key-match an earlier rule with a residual
    whose whole value is not TRUE: what an exclusion on the key alone would lose)."""
    out = []
    stats = [dict(candidates=0, rejected=0, null_residual=0, emitted=0, after_untrue_earlier=0) for _ in rule_fns]
    same = L is R
    for i, l in enumerate(L):
        for j, r in enumerate(R):
            if same and i == j:
                continue  # T is never TRUE for a row with itself
            if link_predicate(link_type, l, r, uid) is not True:
                continue
            keys = [fn[0](l, r) for fn in rule_fns]
            vals = [rule_value(fn, l, r) for fn in rule_fns]
            for k, fn in enumerate(rule_fns):
                if keys[k] is True:
                    stats[k]["candidates"] += 1
                    stats[k]["rejected"] += vals[k] is not True
                    stats[k]["null_residual"] += vals[k] is None
            first = next((k for k, v in enumerate(vals) if v is True), None)
            if first is None:
                continue
            stats[first]["emitted"] += 1
            if any(keys[k] is True and rule_fns[k][1] is not None for k in range(first)):
                stats[first]["after_untrue_earlier"] += 1
            out.append((first, i, j))
    out.sort(key=lambda t: t[0])
    return out, stats


def golden_pair_ids(g):
    e = g["df_e"]
    n = len(e["unique_id_l"])
    sl = e.get("_source_table_l", [None] * n)
    sr = e.get("_source_table_r", [None] * n)
    return sorted(zip(sl, e["unique_id_l"], sr, e["unique_id_r"]), key=repr)
