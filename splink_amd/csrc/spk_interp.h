// The comparison programs' interpreter (device functions only): a column is a sequence of WHEN branches, each an
// RPN predicate over SQL three-valued logic plus UNDECIDED.  eval_column<MODE> runs one column for one pair in the
// filter pass (bounds), the exact pass (registers), the slow pass (global memory) or the huge pass (device scratch).
#pragma once

#include "spk_gamma.h"

namespace spk {

// Spark UTF8String.substringSQL(pos, len) on a code-point range, mapped to UTF-16 units.
__device__ inline void apply_substr(StrView &s, int pos, int len) {
    int nc = s.ncp;
    int start = pos > 0 ? pos - 1 : (pos < 0 ? nc + pos : 0);
    long end = (long)start + len;
    if (start < 0) start = 0;
    if (end > nc) end = nc;
    s.has_meta = 0;
    s.planes = nullptr;
    if (start >= end) {
        s.n = 0;
        s.ncp = 0;
        return;
    }
    if (s.ncp == s.n) {  // BMP only: units == code points
        s.p += start;
        s.n = (int)(end - start);
        s.ncp = s.n;
        return;
    }
    int u = 0, c = 0, ub = 0;
    while (u < s.n && c < end) {
        if (c == start) ub = u;
        uint16_t w = s.p[u];
        u += (w >= 0xD800 && w < 0xDC00 && u + 1 < s.n) ? 2 : 1;
        ++c;
    }
    s.p += ub;
    s.n = u - ub;
    s.ncp = (int)(end - start);
}

__device__ inline StrView lit_view(const GammaArgs &A, int lit) {
    return plain_view(A.lit_units + A.lit_off[lit], A.lit_len[lit], A.lit_cplen[lit]);
}

// A row's string view from its metadata record.
__device__ inline StrView row_view(const ColDesc &c, const RecMeta &m, int64_t row, int col) {
    StrView s = plain_view(c.units + meta_off(m), m.len16, meta_cplen(m));
    s.planes = (m.cpf & CPF_PLANES) ? c.planes + row * N_PLANES : nullptr;
    s.has_meta = 1;
    s.exact_key = (m.cpf & CPF_ID) ? col + 1 : 0;  // ids are per column (both sides share)
    s.key = m.key;
    s.sketch = m.sketch;
    return s;
}

__device__ inline StrView get_str(const GammaArgs &A, const spk_operand &op, int32_t x, int32_t y) {
    StrView s;
    if (op.kind == 0) {
        const ColDesc &c = (op.side ? A.cols1 : A.cols0)[op.col];
        const int32_t row = op.side ? y : x;
        const RecMeta m = c.meta[row];
        if (m.len16 >= 0) {
            s = row_view(c, m, row, op.col);
        } else if (op.lit >= 0) {
            s = lit_view(A, op.lit);
        }
    } else if (op.kind == 1) {
        s = lit_view(A, op.lit);
    }
    if (!s.null && op.substr_start != 0) apply_substr(s, op.substr_start, op.substr_len);
    return s;
}

__device__ inline bool get_num(const GammaArgs &A, const spk_operand &op, int32_t x, int32_t y, double &v) {
    if (op.kind == 2) {
        v = op.num;
        return true;
    }
    const ColDesc &c = (op.side ? A.cols1 : A.cols0)[op.col];
    const int32_t row = op.side ? y : x;
    if (c.valid[row]) {
        v = c.val[row];
        return true;
    }
    if (op.has_num_default) {
        v = op.num;
        return true;
    }
    return false;
}

// code-point order (= Spark's UTF-8 byte order) for <, <=, >, >=
__device__ inline int str_order(const StrView &a, const StrView &b) {
    int i = 0, j = 0;
    while (i < a.n && j < b.n) {
        uint32_t ca = a.p[i], cb = b.p[j];
        int la = 1, lb = 1;
        if (ca >= 0xD800 && ca < 0xDC00 && i + 1 < a.n) { ca = 0x10000 + ((ca - 0xD800) << 10) + (a.p[i + 1] - 0xDC00); la = 2; }
        if (cb >= 0xD800 && cb < 0xDC00 && j + 1 < b.n) { cb = 0x10000 + ((cb - 0xD800) << 10) + (b.p[j + 1] - 0xDC00); lb = 2; }
        if (ca != cb) return ca < cb ? -1 : 1;
        i += la;
        j += lb;
    }
    if (i < a.n) return 1;
    if (j < b.n) return -1;
    return 0;
}

// The last fp64 value (jaro_winkler_sim, jaccard_sim or cosine_distance: the key carries the function above
// the operand pair) and the last Levenshtein distance of a column, so several WHENs over one operand pair
// compute each once.
struct Memo {
    int jw_key, lev_key;
    double jw;
    int lev;
};

// jaccard_sim(a, b) / cosine_distance(a, b) of two non-NULL strings in global memory (NaN: a blank text under
// cosine_distance).  S: the huge pass's scratch (two presence bitmaps for jaccard_sim), unused otherwise.
template <int MODE>
__device__ inline double setsim_value(int op, const StrView &a, const StrView &b, const Scratch &S) {
    const GlbAcc ga{a.p}, gb{b.p};
    if (op == SPK_OP_COSINE) return cosine_tokens(ga, a.n, gb, b.n);
    if (MODE == M_HUGE)
        return jaccard_bitmap(ga, a.n, gb, b.n, S.at<uint64_t>(0), S.at<uint64_t>(JACCARD_WORDS));
    return jaccard_units(ga, a.n, gb, b.n);
}

// One WHEN predicate.  Sets *slow when the exact pass needs the global-memory pass.
// SET: the instantiation evaluates jaccard_sim / cosine_distance.  The exact, slow and huge kernels exist in
// both forms, and a column whose program names neither function (GammaCols.setsim) runs the form without, which
// keeps the register and private-segment budget it had before these functions existed (profiles/ab_setsim.log);
// there the opcodes are an error like any unknown one.  The filter pass has one form: it only bounds them.
template <int MODE, bool SET = MODE == M_FILTER>
__device__ int eval_pred(const GammaArgs &A, int first, int count, int32_t x, int32_t y, Memo &mm,
                         bool *slow, const Scratch &S) {
    uint32_t st = 0;  // stack of truth values, 2 bits per entry
    for (int k = 0; k < count; ++k) {
        const spk_instr in = A.instr[first + k];
        int r = KN;
        switch (in.op) {
            case SPK_OP_AND: {
                int b = st & 3; st >>= 2; int a = st & 3; st >>= 2;
                r = k_and(a, b);
                break;
            }
            case SPK_OP_OR: {
                int b = st & 3; st >>= 2; int a = st & 3; st >>= 2;
                r = k_or(a, b);
                break;
            }
            case SPK_OP_NOT: {
                int a = st & 3; st >>= 2;
                r = k_not(a);
                break;
            }
            case SPK_OP_CONST: r = in.i0; break;
            case SPK_OP_ISNULL:
            case SPK_OP_NOTNULL: {
                const spk_operand &o = A.ops[in.a];
                bool isnull;
                if (o.kind == 2 || (o.kind == 0 && (o.side ? A.cols1 : A.cols0)[o.col].kind == COL_NUM)) {
                    double v;
                    isnull = !get_num(A, o, x, y, v);
                } else {
                    isnull = get_str(A, o, x, y).null != 0;
                }
                r = (isnull == (in.op == SPK_OP_ISNULL)) ? KT : KF;
                break;
            }
            case SPK_OP_NUM_CMP:
            case SPK_OP_ABSDIFF:
            case SPK_OP_PERCDIFF: {
                double a, b;
                if (!get_num(A, A.ops[in.a], x, y, a) || !get_num(A, A.ops[in.b], x, y, b)) { r = KN; break; }
                if (in.op == SPK_OP_NUM_CMP) {
                    r = cmpd(a, b, in.cmp);
                } else if (in.op == SPK_OP_ABSDIFF) {
                    r = cmpd(fabs(a - b), in.t, in.cmp);
                } else {
                    double d = fabs(a > b ? a : b);
                    r = d == 0.0 ? KN : cmpd(fabs(a - b) / d, in.t, in.cmp);
                }
                break;
            }
            case SPK_OP_STR_CMP: {
                StrView a = get_str(A, A.ops[in.a], x, y), b = get_str(A, A.ops[in.b], x, y);
                if (a.null || b.null) { r = KN; break; }
                if (in.cmp == SPK_CMP_EQ || in.cmp == SPK_CMP_NE) {
                    r = (units_equal(a, b) == (in.cmp == SPK_CMP_EQ)) ? KT : KF;
                } else {
                    r = cmpd((double)str_order(a, b), 0.0, in.cmp);
                }
                break;
            }
            case SPK_OP_LEN: {
                StrView a = get_str(A, A.ops[in.a], x, y);
                r = a.null ? KN : cmpd((double)a.ncp, in.t, in.cmp);
                break;
            }
            case SPK_OP_JW: {
                StrView a = get_str(A, A.ops[in.a], x, y), b = get_str(A, A.ops[in.b], x, y);
                if (a.null || b.null) { r = KN; break; }
                const int key = in.a * 4096 + in.b;
                if (mm.jw_key != key) {
                    double v;
                    if (a.n == b.n && units_equal(a, b)) {
                        v = a.n > 0 ? 1.0 : 0.0;  // identical strings: m = n, t = 0 -> exactly 1.0
                    } else if (MODE == M_FILTER) {
                        const double hi = jw_upper(a, b);
                        if (hi < 0.0) {
                            v = 0.0;  // no common unit: m = 0
                        } else {
                            r = decide(0.0, hi + 1e-12, in.cmp, in.t);  // margin >> rounding of either side
                            break;
                        }
                    } else if (MODE == M_HUGE) {
                        v = jw_long(GlbAcc{a.p}, a.n, GlbAcc{b.p}, b.n, S.at<uint64_t>(0), S.at<uint64_t>(S.words));
                    } else if (MODE == M_SLOW) {
                        if (a.n > SLOW_LIMIT || b.n > SLOW_LIMIT) { *slow = true; return KN; }  // huge pass
                        else if (a.n <= 64 && b.n <= 64) v = jw_small(GlbAcc{a.p}, a.n, GlbAcc{b.p}, b.n);
                        else v = jw_long(GlbAcc{a.p}, a.n, GlbAcc{b.p}, b.n);
                    } else {
                        if (a.n > 64 || b.n > 64) { *slow = true; return KN; }
                        v = jw_exact(a, b);
                    }
                    mm.jw = v;
                    mm.jw_key = key;
                }
                r = cmpd(mm.jw, in.t, in.cmp);
                break;
            }
            case SPK_OP_JACCARD:
            case SPK_OP_COSINE: {
                if (!SET) { atomicOr(A.err, 2); r = KN; break; }
                StrView a = get_str(A, A.ops[in.a], x, y), b = get_str(A, A.ops[in.b], x, y);
                if (a.null || b.null) { r = KN; break; }
                const int key = ((in.op - SPK_OP_JACCARD + 1) << 24) + in.a * 4096 + in.b;
                if (mm.jw_key != key) {
                    double v;
                    if (in.op == SPK_OP_JACCARD && a.n == b.n && units_equal(a, b)) {
                        v = a.n > 0 ? 1.0 : 0.0;  // A = B: Math.round(1.0 * 100.0) / 100.0; two empty strings: 0.0
                    } else if (MODE == M_FILTER) {
                        // the function's range alone: jaccard_sim in [0, 1]; cosine_distance = 1 - cos with cos in
                        // [0, 1] up to rounding, once a first unit that is no whitespace shows neither text is blank
                        if (in.op == SPK_OP_JACCARD) r = decide(0.0, 1.0, in.cmp, in.t);
                        else if (a.n > 0 && b.n > 0 && !whitespace_unit(a.p[0]) && !whitespace_unit(b.p[0]))
                            r = decide(-1e-9, 1.0 + 1e-9, in.cmp, in.t);
                        else r = KU;
                        break;
                    } else {
                        const int lim = MODE == M_SLOW ? SLOW_LIMIT : MAXU;
                        if (MODE != M_HUGE && (a.n > lim || b.n > lim)) { *slow = true; return KN; }
                        v = setsim_value<MODE>(in.op, a, b, S);
                    }
                    mm.jw = v;
                    mm.jw_key = key;
                }
                r = mm.jw != mm.jw ? KN : cmpd(mm.jw, in.t, in.cmp);
                break;
            }
            case SPK_OP_LEV:
            case SPK_OP_LEVRATIO: {
                StrView a = get_str(A, A.ops[in.a], x, y), b = get_str(A, A.ops[in.b], x, y);
                if (a.null || b.null) { r = KN; break; }
                const double den = (double)(a.ncp + b.ncp) / 2.0;
                if (in.op == SPK_OP_LEVRATIO && den == 0.0) { r = KN; break; }
                const int key = in.a * 4096 + in.b;
                if (mm.lev_key != key) {
                    int v;
                    if (a.n == b.n && units_equal(a, b)) {
                        v = 0;
                    } else if (MODE == M_FILTER) {
                        const int lo = lev_lower(a, b);
                        const int hi = a.ncp > b.ncp ? a.ncp : b.ncp;
                        if (in.op == SPK_OP_LEV) r = decide((double)lo, (double)hi, in.cmp, in.t);
                        else r = decide((double)lo / den, (double)hi / den, in.cmp, in.t);
                        break;
                    } else if (MODE == M_HUGE) {
                        v = lev_long(a, b, S.at<uint32_t>(0), S.at<int32_t>(S.units));
                    } else if (MODE == M_SLOW) {
                        if (a.n > SLOW_LIMIT || b.n > SLOW_LIMIT) { *slow = true; return KN; }  // huge pass
                        else v = lev_long(a, b);
                    } else {
                        if (a.n > 64 || b.n > 64 || a.ncp != a.n || b.ncp != b.n) { *slow = true; return KN; }
                        v = lev_exact(a, b);
                    }
                    mm.lev = v;
                    mm.lev_key = key;
                }
                r = in.op == SPK_OP_LEV ? cmpd((double)mm.lev, in.t, in.cmp) : cmpd((double)mm.lev / den, in.t, in.cmp);
                break;
            }
            default: atomicOr(A.err, 2); r = KN; break;
        }
        st = (st << 2) | (uint32_t)r;
    }
    return (int)(st & 3);
}

template <int MODE, bool SET = MODE == M_FILTER>
__device__ int eval_column(const GammaArgs &A, int k, int32_t x, int32_t y, int &level,
                           const Scratch &S = Scratch{}) {
    const spk_column_program prog = A.progs[k];
    Memo mm{-1, -1, 0.0, 0};
    for (int w = 0; w < prog.n_when; ++w) {
        const int wi = prog.first_when + w;
        bool slow = false;
        const int r = eval_pred<MODE, SET>(A, A.when_first[wi], A.when_n[wi], x, y, mm, &slow, S);
        if (slow) return ST_NEEDS_SLOW;
        if (r == KU) return ST_UNDECIDED;
        if (r == KT) {
            level = A.when_level[wi];
            return ST_DONE;
        }
    }
    level = prog.else_level;
    return ST_DONE;
}

}  // namespace spk
