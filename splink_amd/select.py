"""Predicates of `frame.filter(condition)`: SQL text to the terms of a device selection (spk_select).

The reference's users filter the scored frame with Spark SQL, `df_e.filter("match_probability > 0.9")` or a
condition on `gamma_*` columns.  Both are functions of a pair's comparison pattern, so a conjunction over them is
decided once per pattern on the device.  The frame of the term-frequency stage is filtered on
`tf_adjusted_match_prob` as well, which the device decides per pair (spk_select_tf).  This module parses the
condition (sqlexpr) and turns it into at most `MAX_TERMS` terms `(field, col, op, value)`; anything else raises
ValueError naming what it met.
"""
from __future__ import annotations

import math
import numbers
from dataclasses import dataclass
from typing import Sequence, Tuple

import numpy as np

from . import _native as N
from . import sqlexpr as S

MAX_TERMS = N.SELECT_MAX_TERMS
FIELD_MP, FIELD_GAMMA, FIELD_TF = N.SEL_MP, N.SEL_GAMMA, N.SEL_TF_MP
OP = N.SEL_OP
_FLIP = {"<": ">", "<=": ">=", ">": "<", ">=": "<=", "=": "=", "!=": "!="}

SUPPORTED = ("supported: a conjunction (AND) of at most %d terms, each `<column> <op> <number>` (or the number on "
             "the left) with <op> one of < <= > >= = != <>, or `<column> is [not] null`, where <column> is "
             "match_probability (scored frames) or one of the frame's gamma_* columns" % MAX_TERMS)
SUPPORTED_TF = SUPPORTED.replace("match_probability (scored frames)",
                                 "tf_adjusted_match_prob (the term-frequency frame), match_probability (scored frames)")


BEST_PER = {"l": N.BEST_L, "r": N.BEST_R, "either": N.BEST_EITHER, "mutual": N.BEST_MUTUAL}
BEST_TIES = {"first": 0, "all": 1}
BEST_BY = {"match_probability": FIELD_MP, "tf_adjusted_match_prob": FIELD_TF}


def best_match_args(per="l", ties="first", by="match_probability", allowed_by=("match_probability",)):
    """(field, mode, keep_ties) of spk_select_best for best_matches(per=, ties=, by=); `allowed_by`: the scores the
    frame carries.  Anything else raises ValueError naming the legal values."""
    def pick(what, value, table, legal):
        if not isinstance(value, str) or value not in legal:
            raise ValueError(f"best_matches: {what}={value!r}; legal values: " + ", ".join(repr(v) for v in legal))
        return table[value]
    mode = pick("per", per, BEST_PER, tuple(BEST_PER))
    keep_ties = pick("ties", ties, BEST_TIES, tuple(BEST_TIES))
    field = pick("by", by, BEST_BY, tuple(b for b in BEST_BY if b in allowed_by))
    return field, mode, keep_ties


SAMPLE_MAX_STRATA = N.SAMPLE_MAX_STRATA


def _plain_int(x):
    return isinstance(x, numbers.Integral) and not isinstance(x, bool)


def sample_args(per_stratum=200, strata=10, seed=0):
    """(edges, quota, seed) of spk_select_sample for sample_pairs(per_stratum=, strata=, seed=): `strata` is a number
    of equal-width bins over [0, 1] or a sequence of finite, strictly ascending edges (1 to SAMPLE_MAX_STRATA
    strata), `per_stratum` one non-negative int or one per stratum, `seed` an int in [0, 2**64).  Anything else raises
    ValueError."""
    if _plain_int(strata):
        if not 1 <= strata <= SAMPLE_MAX_STRATA:
            raise ValueError(f"sample_pairs: strata={strata!r}; 1 to {SAMPLE_MAX_STRATA} strata")
        edges = [i / int(strata) for i in range(int(strata) + 1)]
    else:
        try:
            edges = [float(e) for e in strata]
        except (TypeError, ValueError):
            raise ValueError(f"sample_pairs: strata={strata!r}; an int (equal-width bins over [0, 1]) or a sequence "
                             "of edges") from None
        if not 2 <= len(edges) <= SAMPLE_MAX_STRATA + 1:
            raise ValueError(f"sample_pairs: {len(edges)} edges; 2 to {SAMPLE_MAX_STRATA + 1} edges (1 to "
                             f"{SAMPLE_MAX_STRATA} strata)")
        if not all(math.isfinite(e) for e in edges):
            raise ValueError(f"sample_pairs: the edges must be finite, got {edges!r}")
        if any(a >= b for a, b in zip(edges, edges[1:])):
            raise ValueError(f"sample_pairs: the edges must be strictly ascending, got {edges!r}")
    n = len(edges) - 1
    if _plain_int(per_stratum):
        quota = [int(per_stratum)] * n
    else:
        try:
            quota = list(per_stratum)
        except TypeError:
            raise ValueError(f"sample_pairs: per_stratum={per_stratum!r}; an int or one int per stratum") from None
        if not all(_plain_int(q) for q in quota):
            raise ValueError(f"sample_pairs: per_stratum={per_stratum!r}; an int or one int per stratum")
        if len(quota) != n:
            raise ValueError(f"sample_pairs: {len(quota)} quotas for {n} strata")
        quota = [int(q) for q in quota]
    if any(q < 0 or q >= 1 << 63 for q in quota):
        raise ValueError(f"sample_pairs: a quota is negative or too large, got {per_stratum!r}")
    if not _plain_int(seed) or not 0 <= seed < 1 << 64:
        raise ValueError(f"sample_pairs: seed={seed!r}; an int in [0, 2**64)")
    return edges, quota, int(seed)


def sample_strata(mp, edges):
    """The stratum of every sampled pair's match_probability under the call's edges, as the device decides it: the
    number of inner edges <= x (left-closed strata, the last one closed on the right as well).  Sampled pairs lie
    inside the edges, so there is no "none" here."""
    return np.searchsorted(np.asarray(edges[1:-1], dtype=np.float64), np.asarray(mp, dtype=np.float64), side="right")


TOP_FIRST, TOP_ASC, TOP_DESC = N.TOP_FIRST, N.TOP_ASC, N.TOP_DESC


@dataclass(frozen=True)
class SortColumn:
    """What `asc(name)` / `desc(name)` return: a column name with its direction, for `frame.orderBy(...)`."""
    name: str
    ascending: bool = True


def asc(name):
    """`frame.orderBy(asc("match_probability"))`, as in Spark: NULLs first, ties by the pair's ordinal."""
    return SortColumn(name, True)


def desc(name):
    """`frame.orderBy(desc("match_probability"))`, as in Spark: NULLs last, ties by the pair's ordinal."""
    return SortColumn(name, False)


def top_args(column, ascending, k, allowed):
    """(field, order, k) of spk_select_top / spk_select_top_of for orderBy(column, ascending).limit(k) on a frame whose
    score columns are `allowed`.  column None: frame order (limit alone), field is then None; k None: every eligible
    pair (an orderBy without limit).  `column` is a name or asc(name) / desc(name), which carries its own direction.
    Anything else raises ValueError naming what is supported."""
    if k is None:
        k = (1 << 63) - 1
    elif not _plain_int(k) or k < 0:
        raise ValueError(f"limit: k={k!r}; an int >= 0")
    k = min(int(k), (1 << 63) - 1)
    if column is None:
        return None, TOP_FIRST, k
    if isinstance(column, SortColumn):
        column, ascending = column.name, column.ascending
    if not isinstance(ascending, (bool, np.bool_)):
        raise ValueError(f"orderBy: ascending={ascending!r}; True or False")
    if not isinstance(column, str) or column not in BEST_BY or column not in allowed:
        legal = ", ".join(repr(b) for b in BEST_BY if b in allowed) or "none (the frame is not scored)"
        raise ValueError(f"orderBy: column {column!r}; supported: one score column of the frame ({legal}); ordering "
                         "by several columns or by gamma columns is not offered")
    return BEST_BY[column], (TOP_ASC if ascending else TOP_DESC), k


def top_order(score, order):
    """The positions of `score`'s elements (given in ascending ordinal) in the order of spk_select_top: NULL (NaN)
    lowest, -0.0 equal to +0.0, ties by position.  TOP_FIRST: the positions as they are."""
    score = np.asarray(score, dtype=np.float64)
    n = len(score)
    if order == TOP_FIRST:
        return np.arange(n, dtype=np.int64)
    null = np.isnan(score)
    val = np.where(null, -np.inf, score) + 0.0  # -0.0 + 0.0 = +0.0
    pos = np.arange(n, dtype=np.int64)
    if order == TOP_ASC:
        return np.lexsort((pos, val, ~null))        # NULLs first, then by value, then by position
    return np.lexsort((pos, -val, null))            # by value descending, NULLs last


@dataclass(frozen=True)
class Term:
    field: int    # FIELD_MP / FIELD_GAMMA / FIELD_TF
    col: int      # comparison column of a FIELD_GAMMA term (0 otherwise)
    op: int       # OP[...]
    value: float  # the literal (0.0 for is [not] null)

    def native(self):
        return (self.field, self.col, self.op, self.value)


@dataclass(frozen=True)
class Predicate:
    """A conjunction of terms.  `never`: a term folded on the host is FALSE for every pair (`gamma_x is null`)."""
    terms: Tuple[Term, ...] = ()
    never: bool = False

    def and_(self, other: "Predicate") -> "Predicate":
        return _checked(self.terms + other.terms, self.never or other.never)

    def native_terms(self):
        """The terms handed to spk_select.  A predicate that is never TRUE goes down as one term the device
        evaluates to FALSE for every pattern (a gamma is never NULL), so every path stays the same."""
        if self.never:
            return [(FIELD_GAMMA, 0, OP["is null"], 0.0)]
        return [t.native() for t in self.terms]

    @property
    def needs_mp(self) -> bool:
        return any(t.field == FIELD_MP for t in self.terms)

    @property
    def needs_tf(self) -> bool:
        """Some term reads tf_adjusted_match_prob: the selection is decided per pair, not per pattern."""
        return any(t.field == FIELD_TF for t in self.terms)


def _checked(terms, never) -> Predicate:
    if len(terms) > MAX_TERMS:
        raise ValueError(f"filter: more than {MAX_TERMS} terms ({len(terms)}) in the condition; {SUPPORTED}")
    return Predicate(tuple(terms), bool(never))


def _describe(node) -> str:
    if isinstance(node, S.Bin) and node.op == "or":
        return "OR"
    if isinstance(node, S.Un) and node.op == "not":
        return "NOT"
    if isinstance(node, S.Func):
        return f"function {node.name}(...)"
    if isinstance(node, S.Case):
        return "CASE expression"
    if isinstance(node, S.Lit):
        if isinstance(node.value, str):
            return f"string literal {node.value!r}"
        if node.value is None:
            return "NULL literal"
        return f"literal {node.value!r}"
    if isinstance(node, S.Col):
        name = f"{node.qualifier}.{node.name}" if node.qualifier else node.name
        return f"column {name!r}"
    if isinstance(node, S.Bin):
        return f"expression with operator {node.op!r}"
    if isinstance(node, S.Un):
        return f"unary {node.op!r}"
    return type(node).__name__


def _reject(node, text, supported=SUPPORTED):
    raise ValueError(f"filter: unsupported {_describe(node)} in condition {text!r}; {supported}")


def _number(node):
    return isinstance(node, S.Lit) and isinstance(node.value, (int, float)) and not isinstance(node.value, bool)


def _column(node, gamma_index, allow_mp, text, allow_tf=False):
    """(field, col) of a column node the frame can filter on."""
    supported = SUPPORTED_TF if allow_tf else SUPPORTED
    if not isinstance(node, S.Col) or node.qualifier:
        _reject(node, text, supported)
    if node.name == "tf_adjusted_match_prob" and allow_tf:
        return FIELD_TF, 0
    if node.name == "match_probability":
        if not allow_mp:
            raise ValueError(f"filter: column 'match_probability' in condition {text!r}: this frame is not scored "
                             f"(filter the frame run_expectation_step returns); {SUPPORTED}")
        return FIELD_MP, 0
    if node.name in gamma_index:
        return FIELD_GAMMA, gamma_index[node.name]
    _reject(node, text, supported)


def compile_condition(condition: str, gamma_names: Sequence[str], allow_mp: bool = True,
                      allow_tf: bool = False) -> Predicate:
    """The terms of `condition` over a frame whose gamma columns are `gamma_names` (in comparison-column order).
    allow_tf: the frame carries tf_adjusted_match_prob (the term-frequency frame)."""
    supported = SUPPORTED_TF if allow_tf else SUPPORTED
    if not isinstance(condition, str):
        raise TypeError(f"filter: the condition must be a SQL string, got {type(condition).__name__}")
    gamma_index = {g.lower(): i for i, g in enumerate(gamma_names)}
    terms, never = [], False
    for node in S.conjuncts(S.parse(condition)):
        if isinstance(node, S.IsNull):
            field, col = _column(node.a, gamma_index, allow_mp, condition, allow_tf)
            if field == FIELD_GAMMA:  # a gamma is never NULL (-1 is a level): folded here
                never = never or not node.negated
                continue
            terms.append(Term(field, col, OP["is not null" if node.negated else "is null"], 0.0))
            continue
        if not (isinstance(node, S.Bin) and node.op in _FLIP):
            _reject(node, condition, supported)
        a, b, op = node.a, node.b, node.op
        if _number(a) and not _number(b):
            a, b, op = b, a, _FLIP[op]
        if not _number(b):
            _reject(b if isinstance(a, S.Col) else a, condition, supported)
        field, col = _column(a, gamma_index, allow_mp, condition, allow_tf)
        value = float(b.value)
        if field == FIELD_GAMMA and value != int(value):
            raise ValueError(f"filter: non-integral literal {b.value!r} compared with a gamma column in condition "
                             f"{condition!r} (levels are integers); {SUPPORTED}")
        terms.append(Term(field, col, OP[op], value))
    return _checked(tuple(terms), never)
