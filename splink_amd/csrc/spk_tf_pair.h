// tf_adjusted_match_prob of one pair (term_frequencies.py:98-117), shared by k_tf_apply (spk_tf.hip) and the
// selection on the tf-adjusted score (k_select_tf_count / k_select_tf_emit, spk_select.hip): the arithmetic has
// one definition, so the value a selection compares and returns is the value spk_tf_apply* gives for the pair,
// bit for bit.  Contraction is off in these functions whatever the translation unit is built with: b * (1 - v)
// followed by a + b must stay a multiply and an add in every caller.
#pragma once

#include <cmath>

#include "spk_internal.h"

namespace spk {

struct TfApply {
    int n;
    const int64_t *ids0[8];
    const int64_t *ids1[8];
    const double *tab[8];
    int64_t tab_n[8];
};

// The adjustment of one column for a pair whose rows carry the value ids a and b: the table's entry for equal,
// non-NULL ids inside the table, 0.5 otherwise and for a NaN entry (:68-95).
__device__ inline double tf_adj(int64_t a, int64_t b, const double *__restrict__ tab, int64_t tab_n) {
    double v = 0.5;
    if (a >= 0 && a == b && a < tab_n) {
        const double x = tab[a];
        if (!isnan(x)) v = x;
    }
    return v;
}

// bayes(mp, adj...) = Πp / (Πp + Π(1-p)) (:21-46): start with a = mp, b = 1 - mp, fold every column's adjustment
// in column order, finish.
__device__ inline void tf_begin(double m, double &a, double &b) {
    a = m;
    b = 1.0 - m;
}

__device__ inline void tf_fold(double &a, double &b, double v) {
#pragma clang fp contract(off)
    a = a * v;
    b = b * (1.0 - v);
}

__device__ inline double tf_finish(double m, double a, double b) {
#pragma clang fp contract(off)
    if (isnan(m)) return NAN;
    const double d = a + b;
    return d == 0.0 ? NAN : a / d;
}

// One pair with rows l (side 0) and r (side 1) and match probability m; out_adj [T.n] gets the adjustments, or null.
__device__ inline double tf_pair(const TfApply &T, double m, int32_t l, int32_t r, double *__restrict__ out_adj) {
#pragma clang fp contract(off)
    double a, b;
    tf_begin(m, a, b);
    for (int c = 0; c < T.n; ++c) {
        const double v = tf_adj(T.ids0[c][l], T.ids1[c][r], T.tab[c], T.tab_n[c]);
        if (out_adj) out_adj[c] = v;
        tf_fold(a, b, v);
    }
    return tf_finish(m, a, b);
}

// The value ids of every tf column for both sides and the adjustment tables, staged on the device for one call
// (spk_tf_apply*, spk_select_tf*): they live as long as this object.
struct TfStage {
    DevBuf<int64_t> d0[8], d1[8];
    DevBuf<double> dt[8];
    TfApply T{};
};
// Host value ids per row (ids_side0[c] has table 0's rows, ids_side1[c] the other side's).
int tf_stage_host_ids(spk_ctx *ctx, int n_tf_cols, const int64_t *const *ids_side0, const int64_t *const *ids_side1,
                      TfStage &S);
// The dictionary ids of string columns decoded on the device (spk_table_add_raw_utf8).
int tf_stage_column_ids(spk_ctx *ctx, int n_tf_cols, const int32_t *cols, TfStage &S);
int tf_stage_tables(spk_ctx *ctx, const double *const *adj_tables, const int64_t *table_sizes, TfStage &S);

}  // namespace spk
